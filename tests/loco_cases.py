"""Synthetic configurations shared by tests/test_gpu_loco.py and tests/loco_dist_worker.py: rows in units (configurations)
of given sizes, labels of the reference's fitsnap_dict, and brute-force leave-one-unit-out predictions by downdated
solves (G - X_c^T X_c + alpha I) beta = c - X_c^T y_c, which is the refit without the unit's rows."""
import numpy as np


def config_rows(seed, K, sizes, testing_frac=0.0):
    rng = np.random.default_rng(seed)
    m = int(sum(sizes))
    A = rng.standard_normal((m, K)) * rng.uniform(0.5, 2.0, K)
    b = A @ rng.standard_normal(K) + 0.05 * rng.standard_normal(m)
    w = rng.uniform(0.5, 2.0, m)
    cfg = np.repeat(np.arange(len(sizes)), sizes)
    testing = rng.random(m) < testing_frac
    labels = {
        "Configs": [f"cfg{c}" for c in cfg],
        "Groups": [f"g{c % 3}" for c in cfg],
        "Testing": testing.tolist(),
        "Row_Type": [("Energy", "Force", "Stress")[i % 3] for i in range(m)],
    }
    return A, b, w, labels


def downdated(A, b, w_eff, rows, alpha, G=None, c=None):
    """Prediction of the rows ``rows`` by the fit without them (ridge alpha; alpha = 0 is the least-squares fit)."""
    Aw, bw = A * w_eff[:, None], b * w_eff
    if G is None:
        G, c = Aw.T @ Aw, Aw.T @ bw
    Xc, yc = Aw[rows], bw[rows]
    beta = np.linalg.solve(G - Xc.T @ Xc + alpha * np.eye(A.shape[1]), c - Xc.T @ yc)
    return A[rows] @ beta
