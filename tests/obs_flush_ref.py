"""CPU helpers of tests/test_gpu_obs_skip.py: the observation kernel's values in fp64, the fp64
oracle of the observation map in the device's association on flushed kernel values, and
host_image.h obs_cutoff_tau restated in numpy.  Self-checks: tests/test_obs_flush_ref.py."""
import numpy as np

import extended_ref as E


def kernel_values(p, xs):
    """exp(-|x* - X_i|^2 / l^2), N x n, fp64 (values below the smallest subnormal are 0)."""
    return E.rbf(p["X"], np.asarray(xs, dtype=np.float64), p["y_log_lengthscales"]).astype(np.float64)


def oracle_obs_triangular_flushed(om, xs, tau=None):
    """extended_ref.oracle_obs_triangular with the kernel values below ``tau`` flushed to 0 first
    (gp_tile.h's filter launch): R = U^-1 from the reference's Cholesky recipe, quadratic form
    |R^T k|^2, mean k^T (R R^T Y).  Returns (mu[n, D], vc[n])."""
    from oracle import gpmdm_oracle as O
    Ky = O.rbf_kernel(om.X, om.X, om.y_log_lengthscales, om.y_log_sigma_n, om.sigma_n_num_Y, noise=True)
    R = np.linalg.inv(np.linalg.cholesky(Ky).T)
    beta = (R @ R.T) @ om.Y
    Ks = O.rbf_kernel(om.X, xs, om.y_log_lengthscales)
    if tau:
        Ks = np.where(Ks < tau, 0.0, Ks)
    V = Ks.T @ R
    return Ks.T @ beta, 1.0 - np.sum(V * V, axis=1)


def tau_numpy(N, sigma2, M, y_absmax):
    """host_image.h obs_cutoff_tau: min(tau_q, tau_mu), the column sums in row order."""
    vc_min = sigma2 / (N + sigma2)
    h = 0.5 * (np.nextafter(vc_min, 1.0) - vc_min)
    tau = np.sqrt(sigma2) * h / (2.001 * np.sqrt(float(N)))
    for j in range(M.shape[1]):
        m1 = 0.0
        for v in np.abs(M[:, j]):
            m1 += v
        y = y_absmax[j]
        if m1 > 0.0 and y > 0.0:
            tau = min(tau, 0.5 * (np.nextafter(y, 1e308) - y) / m1)
    return tau
