function [sigma, Phi, resid, nconv] = empirical_filter_factors(A, b, X, steps, nsv)
% Empirical filter factors of the solutions X (n x nx) on the leading singular triplets of A that b excites:
% Phi(i,r) = sigma_i * (v_i'*X(:,r)) / d_i with d = U'*b and the guard d(abs(d) < 1e-12) = 1
% (plot_filter_factors.m:31-40), the triplets from svds_gk (hgm_svds) in place of the dense svd(A,'econ') of :30.
% Phi is nsv x nx (NaN past the triplets found); resid_i = norm(A'*u_i - sigma_i*v_i); nconv counts the leading
% triplets with resid <= 1e-10 * sigma(1): compare rows 1:nconv with phi_final of the *_bounds solvers.
[sigma, resid, utb_, steps_done_, VtX_, Phi, nconv] = hgmres_mex('svds_gk', A, b, steps, nsv, X);
end
