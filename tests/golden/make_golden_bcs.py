"""Generate tests/golden/bcs_reference.npz by RUNNING THE REFERENCE'S OWN ``bcs()`` (fitsnap3lib/solvers/bcs.py).

Run in the build container only (needs the reference checkout):

    python tests/golden/make_golden_bcs.py

The reference's solver factory does not import its BCS module, and the module's class statement needs a global ``pt`` that
nothing defines; the module is therefore loaded from its file with a stand-in ``pt`` whose ``sub_rank_zero`` is the identity,
and ``bcs()`` is called the way the reference's ``BCS.perform_fit`` calls it (``bcs(aw, bw, eta=1.e-18)``).  ``numpy.delete``
is counted while it runs: ``bcs()`` calls it in its deletion branch only, six times per deletion.

Cases (tags in ``tags``):
  ta            the Ta rows of tests/golden/ta_abw.npz, aw = w A, bw = w b
  ta_testing    the same with every fourth row from the second held out as testing
  ta_transpose  the reference's substitution aw <- aw.T aw, bw <- aw.T bw
  k1, k2, k7, k33, k144     synthetic rows without a deletion
  k7_del, k33_del           synthetic rows on which the reference goes through a deletion
Synthetic rows (``synthetic`` below; tests/bcs_cases.py rebuilds them from the recorded arguments and checks them against the
stored rows): Gaussian columns mixed by I + c N / sqrt(K), a sparse truth of ``nnz`` entries and Gaussian noise.

Per case: ``<tag>_A`` / ``<tag>_y`` (the synthetic rows; the Ta cases store ``<tag>_testing`` instead), ``<tag>_weights``,
``_errbars``, ``_used``, ``_sigma2``, ``_Sig`` (as bcs() returns them: Sig clipped at 0), ``_deletions`` and ``_own_error``:
the largest relative difference (weights, errbars, Sig: to their largest entry; sigma2) between this float64 run and the same
``bcs()`` run on ``numpy.longdouble`` copies of the rows -- the reference's own rounding error, which bounds how closely anything
can be asked to agree with it.  On all Ta rows it is 9e-9 (the condition number of the rows is 3e5); the testing mask is the
first of 2::5, 1::4 for which it is below 1e-9 (2::5: 3e-8), and ``main`` asserts that.

Only data is written: no reference source text is copied.
"""
from __future__ import annotations

import importlib.util
import os
import sys
import types
import warnings

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import REF, import_reference  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
ETA = 1.0e-18
# tag: (m, K, c, nnz, noise, seed)
SYNTHETIC = {
    "k1": (40, 1, 0.0, 1, 0.3, 0),
    "k2": (60, 2, 0.5, 1, 0.3, 0),
    "k7": (96, 7, 1.0, 3, 0.5, 0),
    "k33": (200, 33, 1.0, 5, 0.4, 0),
    "k144": (300, 144, 1.0, 6, 0.3, 0),
    "k7_del": (96, 7, 1.0, 3, 0.3, 32),
    "k33_del": (200, 33, 1.0, 5, 0.3, 16),
}


def synthetic(m, K, c, nnz, noise, seed):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((m, K))
    A = X @ (np.eye(K) + c * rng.standard_normal((K, K)) / np.sqrt(K))
    truth = np.zeros(K)
    sup = rng.choice(K, size=min(nnz, K), replace=False)
    truth[sup] = rng.standard_normal(len(sup)) * 2.0
    y = A @ truth + noise * rng.standard_normal(m)
    return A, y


def import_reference_bcs():
    import_reference()
    path = os.path.join(REF, "fitsnap3lib", "solvers", "bcs.py")
    spec = importlib.util.spec_from_file_location("fitsnap3lib.solvers.bcs", path)
    mod = importlib.util.module_from_spec(spec)
    mod.pt = types.SimpleNamespace(sub_rank_zero=lambda f: f)
    spec.loader.exec_module(mod)
    return mod.bcs


def own_error(bcs, A, y, weights, errbars, used, sigma2, Sig):
    """The float64 results against the same function on long-double rows (its determinant check, which numpy cannot take in
    long double, is stood in for while it runs)."""
    LD = np.longdouble
    det = np.linalg.det
    np.linalg.det = lambda x: 1.0
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            wl, el, ul, sl, _, Sl = bcs(np.asarray(A, dtype=LD), np.asarray(y, dtype=LD), eta=ETA)
    finally:
        np.linalg.det = det
    if list(ul) != list(used):
        return np.inf

    def rel(x, ref):
        return float(np.max(np.abs(np.asarray(x, dtype=LD) - ref)) / np.max(np.abs(ref)))

    s64, s80 = np.asarray(sigma2, dtype=LD).reshape(-1)[0], np.asarray(sl, dtype=LD).reshape(-1)[0]
    return max(rel(weights, wl), rel(errbars, el), rel(Sig, Sl), float(abs(s64 - s80) / s80))


def run(bcs, A, y):
    calls = [0]
    real = np.delete

    def counting(*a, **k):
        calls[0] += 1
        return real(*a, **k)

    np.delete = counting
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            weights, errbars, used, sigma2, _, Sig = bcs(A, y, eta=ETA)
    finally:
        np.delete = real
    assert calls[0] % 6 == 0
    own = own_error(bcs, A, y, weights, errbars, used, sigma2, Sig)
    return {"own_error": np.float64(own),"weights": np.asarray(weights, dtype=np.float64), "errbars": np.asarray(errbars, dtype=np.float64),
            "used": np.asarray(used, dtype=np.int64), "sigma2": np.float64(np.asarray(sigma2).reshape(-1)[0]),
            "Sig": np.asarray(Sig, dtype=np.float64), "deletions": np.int64(calls[0] // 6)}


def main():
    bcs = import_reference_bcs()
    z = np.load(os.path.join(HERE, "ta_abw.npz"))
    A, b, w = z["A"], z["b"], z["w"]
    aw, bw = w[:, None] * A, w * b
    testing = np.zeros(A.shape[0], dtype=bool)
    testing[1::4] = True
    out = {"eta": np.float64(ETA)}
    tags = []

    def store(tag, res, **extra):
        tags.append(tag)
        for k, v in {**res, **extra}.items():
            out[f"{tag}_{k}"] = v
        print(f"{tag}: used {res['used'].tolist()}, deletions {int(res['deletions'])}, sigma2 {float(res['sigma2']):.6e}, "
              f"own error {float(res['own_error']):.1e}", flush=True)

    store("ta", run(bcs, aw, bw), testing=np.zeros(A.shape[0], dtype=bool))
    store("ta_testing", run(bcs, aw[~testing], bw[~testing]), testing=testing)
    assert out["ta_testing_own_error"] < 1e-9
    store("ta_transpose", run(bcs, aw.T @ aw, aw.T @ bw), testing=np.zeros(A.shape[0], dtype=bool))
    for tag, args in SYNTHETIC.items():
        As, ys = synthetic(*args)
        store(tag, run(bcs, As, ys), A=As, y=ys, args=np.array(args, dtype=np.float64))
    out["tags"] = np.array(tags)
    np.savez_compressed(os.path.join(HERE, "bcs_reference.npz"), **out)


if __name__ == "__main__":
    main()
