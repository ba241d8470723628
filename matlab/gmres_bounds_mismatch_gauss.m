function [X, error_hist, residual_hist, niters, status] = gmres_bounds_mismatch_gauss( ...
    A, B0, seed, scale, coefs, b, x_true, tol, maxit, side, lambdas)
% gmres_bounds_mismatch with the dense Gaussian perturbation of plot_error_vs_mismatch_norm.m:16
% (E = randn(size(A'))) generated on the device: column j is the solve of b with the back-projector
% B0 + coefs(j)*scale*G, where G = randn(size(B0)) is a pure function of (seed, row, column)
% (hgm_gauss_create) that is regenerated inside every product and never stored or uploaded.
% seed is a non-negative integer (below 2^53); scale multiplies the coefficients on the host
% (scale = 1/norm(G,'fro') is :17's normalisation).  Every other argument and output is
% gmres_bounds_mismatch's: side = 'ab' / 'ba'; hybrid when lambdas is given and non-empty.
if nargin < 11 || isempty(lambdas)
    [X, error_hist, residual_hist, niters, status] = hgmres_mex('gmres_bounds_mismatch_gauss', side, 0, A, B0, seed, scale, coefs, b, x_true, tol, maxit);
else
    [X, error_hist, residual_hist, niters, status] = hgmres_mex('gmres_bounds_mismatch_gauss', side, 1, A, B0, seed, scale, coefs, b, x_true, tol, maxit, lambdas);
end
end
