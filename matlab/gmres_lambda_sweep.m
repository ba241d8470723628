function [error_surf, residual_surf, solnorm_surf, niters, X] = gmres_lambda_sweep( ...
    A, B, b, x_true, tol, maxit, lambdas, side)
% ABgmres_hybrid_bounds (side = 'ab') / BAgmres_hybrid_bounds (side = 'ba') for every lambda of
% lambdas from ONE Arnoldi on the device (hgm_gmres_bounds_sweep): the loops of
% analyze_regularization.m:22-33 and plot_error_surface.m:28-42 in one call.  Column l of the
% maxit x numel(lambdas) surfaces is the history of the single solve at lambdas(l), NaN past
% niters(l) (the padding of plot_error_surface.m:32,36); solnorm_surf is norm(x_k); X(:,l) is that
% solve's x (formed only when asked for).  x_true may be [] (error_surf stays NaN).
if nargout <= 4
    [error_surf, residual_surf, solnorm_surf, niters] = hgmres_mex('gmres_lambda_sweep', side, A, B, b, x_true, tol, maxit, lambdas);
    return
end
[error_surf, residual_surf, solnorm_surf, niters, X] = hgmres_mex('gmres_lambda_sweep', side, A, B, b, x_true, tol, maxit, lambdas);
end
