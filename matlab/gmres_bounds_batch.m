function [X, error_hist, residual_hist, niters, status] = gmres_bounds_batch( ...
    A, B, Bm, x_true, tol, maxit, side, lambdas)
% One {AB,BA}gmres_{hybrid,nonhybrid}_bounds solver (side = 'ab' / 'ba'; hybrid when lambdas is given
% and non-empty) for every column of Bm in ONE lockstep batch on the device (hgm_gmres_bounds_batch):
% the loop over the noise levels of plot_error_vs_noise_level.m:28-54 in one call, the operators read
% once per group of up to 8 running columns and iteration.  Column j of X and of the maxit x nrhs
% histories is the solve of Bm(:,j) with lambdas(j) (NaN past niters(j)); x_true is n x 1 (shared by
% every column), n x nrhs, or [] (error_hist stays NaN).  status(j) ~= 0: x of column j was never
% assigned (breakdown at k = 1; X(:,j) is NaN), the other columns are complete.
if nargin < 8 || isempty(lambdas)
    [X, error_hist, residual_hist, niters, status] = hgmres_mex('gmres_bounds_batch', side, 0, A, B, Bm, x_true, tol, maxit);
else
    [X, error_hist, residual_hist, niters, status] = hgmres_mex('gmres_bounds_batch', side, 1, A, B, Bm, x_true, tol, maxit, lambdas);
end
end
