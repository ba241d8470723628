function [X, error_hist, residual_hist, niters, status] = gmres_bounds_mismatch( ...
    A, B0, E, coefs, b, x_true, tol, maxit, side, lambdas)
% One {AB,BA}gmres_{hybrid,nonhybrid}_bounds solver (side = 'ab' / 'ba'; hybrid when lambdas is given
% and non-empty) of ONE right-hand side b for every back-projector B0 + coefs(j)*E in ONE lockstep
% sweep on the device (hgm_gmres_bounds_mismatch): the loop over the mismatch levels of
% plot_error_vs_mismatch_norm.m:23-61 in one call.  No B_pert = B0 + c*E is formed or uploaded: B0 and
% E (size(B0); the same sparsity pattern, or one of its own) are read once per group of up to 8 running
% levels and iteration.  Column j of X and of the maxit x numel(coefs) histories is the solve with
% coefs(j) and lambdas(j) (NaN past niters(j)); x_true is n x 1 or [] (error_hist stays NaN).
% status(j) ~= 0: x of column j was never assigned (breakdown at k = 1; X(:,j) is NaN), the other
% columns are complete.  At most 64 levels per call.
if nargin < 10 || isempty(lambdas)
    [X, error_hist, residual_hist, niters, status] = hgmres_mex('gmres_bounds_mismatch', side, 0, A, B0, E, coefs, b, x_true, tol, maxit);
else
    [X, error_hist, residual_hist, niters, status] = hgmres_mex('gmres_bounds_mismatch', side, 1, A, B0, E, coefs, b, x_true, tol, maxit, lambdas);
end
end
