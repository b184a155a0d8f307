"""Worker of test_host_finish_cpu.py / test_gpu_host_finish.py: solves a fixed list of cases and prints one line per
case, `<name> <sha256 of (status, beta bytes, rank, rcond bytes)>`, then `digest <sha256 over all lines>`.

FSNAP_CHOL_VARIANT is read once per process, so the tests run this file twice -- with FSNAP_CHOL_VARIANT=3 (scale/build,
register-blocked factorisation and two sweeps as separate steps) and without (the fused left-looking pass where it
applies) -- and compare the output.

    python host_finish_worker.py cpu     the host solve alone, through _capi.solve (no GPU)
    python host_finish_worker.py gpu     whole fits, through fit_resident / solve_device
"""
import hashlib
import os
import struct
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from fitsnap_amd import _capi  # noqa: E402

GOOD_K = (48, 49, 63, 64, 65, 96, 110, 127, 128, 129, 142, 144, 145, 200, 231, 255, 256, 47, 257, 300)
KINDS = (("ridge", _capi.SOLVE_RIDGE, 1e-8), ("chol", _capi.SOLVE_CHOL, 0.0), ("lstsq", _capi.SOLVE_LSTSQ, 1e-13),
         ("ridge_inv", _capi.SOLVE_RIDGE_INV, 1e-6))

_lines = []


def record(name, status, beta=None, rank=0, rcond=0.0):
    h = hashlib.sha256()
    h.update(str(status).encode())
    if beta is not None:
        h.update(np.ascontiguousarray(beta, dtype=np.float64).tobytes())
    h.update(struct.pack("<q", int(rank)))
    h.update(struct.pack("<d", float(rcond)))
    _lines.append(f"{name} {h.hexdigest()}")


def host_solve(name, kind, param, G, c):
    try:
        beta, rank, rcond = _capi.solve(kind, param, G, c)
    except Exception as e:          # the status, as the exception it maps to
        record(name, f"{type(e).__name__}: {e}")
        return None
    record(name, "ok", beta, rank, rcond)
    return beta


def statistics(K, seed, decades):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((3 * K + 7, K)) * (10.0 ** rng.uniform(-decades, decades, size=K))
    y = rng.standard_normal(3 * K + 7)
    return X, y


def cpu_cases():
    for K in GOOD_K:
        # column scales 10^U(-3, 3), and one family whose entries of G span 30 decades (the Ta golden set's range)
        for fam, decades in (("s3", 3.0), ("s30", 7.5)):
            X, y = statistics(K, 1000 + K, decades)
            G, c = X.T @ X, X.T @ y
            for kname, kind, param in KINDS:
                host_solve(f"good K={K} {fam} {kname}", kind, param, G, c)
    for K in (128, 142):
        X, y = statistics(K, 2000 + K, 3.0)
        # a duplicated column, no ridge shift
        Xd = X.copy()
        Xd[:, K - 9] = Xd[:, 5]
        G, c = Xd.T @ Xd, Xd.T @ y
        for kname, kind, _ in KINDS:
            host_solve(f"dup K={K} {kname}", kind, 1e-13 if kind == _capi.SOLVE_LSTSQ else 0.0, G, c)
        G0, c0 = X.T @ X, X.T @ y
        # a NaN above the diagonal in a late row
        G = G0.copy()
        G[K - 5, K - 2] = np.nan
        for kname, kind, param in KINDS:
            host_solve(f"nan K={K} {kname}", kind, param, G, c0)
        # an Inf in the right-hand side
        c = c0.copy()
        c[K // 3] = np.inf
        for kname, kind, param in KINDS:
            host_solve(f"infc K={K} {kname}", kind, param, G0, c)
        # an exactly-zero column, least squares
        Xz = X.copy()
        Xz[:, 77] = 0.0
        host_solve(f"zerocol K={K} lstsq", _capi.SOLVE_LSTSQ, 1e-13, Xz.T @ Xz, Xz.T @ y)
        # a pivot that falls below 1e-3 halfway: column K/2 is almost a combination of two earlier ones
        Xp = X.copy()
        s = np.linalg.norm(Xp, axis=0)
        Xp[:, K // 2] = s[K // 2] * (Xp[:, 3] / s[3] + Xp[:, 11] / s[11] + 1e-3 * Xp[:, K // 2] / s[K // 2])
        G, c = Xp.T @ Xp, Xp.T @ y
        for kname, kind, param in KINDS:
            host_solve(f"smallpivot K={K} {kname}", kind, param, G, c)


def gpu_cases():
    ctx = _capi.HipContext(0)

    def fit(name, m, K, kind, param, mask_frac=0.0, rhs_pair=False):
        rng = np.random.default_rng(m + K)
        A = rng.standard_normal((m, K)) * (10.0 ** rng.uniform(-3, 3, size=K))
        b = rng.standard_normal(m)
        w = rng.uniform(0.5, 2.0, size=m)
        mask = (rng.uniform(size=m) >= mask_frac).astype(np.uint8) if mask_frac > 0 else None     # 1 = training row
        ctx.upload_rows(A, b)
        ctx.set_weights(w, mask)
        beta, rank, rcond, d_packed = ctx.fit_resident(kind, param)
        record(name, "ok", beta, rank, rcond)
        # the same coefficients, bit for bit, from the host solve on the statistics the fit left on the device
        G, c = ctx.download_packed(d_packed, K)[:2]
        beta_host = host_solve(name + " host", kind, param, G, c)
        assert beta_host is not None and beta_host.tobytes() == np.asarray(beta).tobytes(), name
        if rhs_pair:
            r = rng.standard_normal(K)
            delta = ctx.solve_device(kind, param, K, d_packed, rhs=r)
            record(name + " rhs", "ok", delta[0], delta[1], delta[2])

    for kname, kind, param in (("ridge", _capi.SOLVE_RIDGE, 1e-8), ("lstsq_probe", _capi.SOLVE_LSTSQ_PROBE, 1e-13),
                               ("ridge_inv", _capi.SOLVE_RIDGE_INV, 1e-6)):
        fit(f"4096x128 masked {kname}", 4096, 128, kind, param, mask_frac=0.1)
        fit(f"1303x142 {kname}", 1303, 142, kind, param)
        fit(f"2000x96 {kname}", 2000, 96, kind, param)
        fit(f"3000x200 {kname}", 3000, 200, kind, param)
    fit("4096x128 lstsq_probe + rhs", 4096, 128, _capi.SOLVE_LSTSQ_PROBE, 1e-13, rhs_pair=True)
    ctx.close()


if __name__ == "__main__":
    (cpu_cases if sys.argv[1] == "cpu" else gpu_cases)()
    for line in _lines:
        print(line)
    print("digest", hashlib.sha256("\n".join(_lines).encode()).hexdigest())
