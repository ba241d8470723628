function [X, error_hist, residual_hist, ar_hist, niters] = gk_batch(A, Bm, x_true, tol, maxit, kind, lambdas)
% One Golub-Kahan solver (kind = 'lsqr', 'lsmr', 'hybrid_lsqr' or 'hybrid_lsmr': lsqr_solver.m, lsmr_solver.m,
% hybrid_lsqr_solver.m, hybrid_lsmr_solver.m) for every column of Bm in ONE lockstep batch on the device
% (hgm_gk_batch): the loop over the noise levels of plot_error_vs_noise_level.m:28-54 over the solvers that
% run_equivalence_plots.m:12-22 sets beside the GMRES ones, the operator read once per group of up to 8 running
% columns and pass.  Column j of X and of the maxit x nrhs histories is the solve of Bm(:,j) with lambdas(j) (NaN
% past niters(j)); the hybrid kinds need lambdas, and an m x 1 Bm with several lambdas is one b shared by every
% column (a lambda sweep).  x_true is n x 1 (shared by every column), n x nrhs, or [] (error_hist stays NaN).
% ar_hist is filled for 'lsmr' only.
if nargin < 7 || isempty(lambdas)
    [X, error_hist, residual_hist, ar_hist, niters] = hgmres_mex('gk_batch', kind, A, Bm, x_true, tol, maxit);
else
    [X, error_hist, residual_hist, ar_hist, niters] = hgmres_mex('gk_batch', kind, A, Bm, x_true, tol, maxit, lambdas);
end
end
