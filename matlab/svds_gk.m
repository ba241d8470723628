function [sigma, resid, utb, steps_done, VtX, U, V] = svds_gk(A, b, steps, nsv, X)
% Leading singular triplets of A by Golub-Kahan-Lanczos bidiagonalisation started at b with full
% reorthogonalisation, on the device (hgm_svds): what [U,S,V] = svd(A,'econ') of plot_filter_factors.m:30 gives,
% restricted to the modes that b excites -- a mode with u_i'*b = 0 is not found, and an exactly repeated singular
% value comes back once, as the projection of b on its singular subspace.  sigma (descending), resid
% (= norm(A'*u_i - sigma_i*v_i); norm(A*v_i - sigma_i*u_i) is at rounding level) and utb (= u_i'*b >= 0) are
% nsv x 1, NaN past min(nsv, steps_done); VtX = V'*X for an n x nx X (nx <= 64; [] without X); U (m x nsv) and V
% (n x nsv) are formed only when asked for.  b = [] starts from a fixed vector.  steps is clipped to min(size(A)); a
% breakdown ends the run early (steps_done < steps) and is not an error.
if nargin < 5, X = []; end
if nargout <= 5
    [sigma, resid, utb, steps_done, VtX] = hgmres_mex('svds_gk', A, b, steps, nsv, X);
else
    [sigma, resid, utb, steps_done, VtX, Phi_, nconv_, U, V] = hgmres_mex('svds_gk', A, b, steps, nsv, X);
end
end
