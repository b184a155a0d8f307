"""Per-iteration times of the robust (IRLS) step on the GPU (csrc/fsnap_robust.hip) next to the composed route it replaces,
in one process and run, at 10^6 x 128 in three classes and at 15 213 x 31:

  new route       R1 fsnap_robust_residuals | R2 fsnap_robust_scale | R3 fsnap_robust_reweight | fit fsnap_fit_resident,
                  and the fused R1 + R3 launch fsnap_robust_step of an iteration whose scales are known
  composed route  fsnap_predict (predictions downloaded) -> numpy medians and weights -> fsnap_set_weights -> fsnap_fit_resident

Every entry is synchronous; a time is the median over --reps warm calls of a host clock around the call.  Kernel times come
from the device events the library brackets its row passes with (fsnap_timing, slot "predict_ms"): R1, the fused launch,
R3 (with its fold) and fsnap_predict's kernel, so that R1 can be read against the HBM-bound pass it is modelled on.

    python scripts/robust_timing.py [--reps N] [--out FILE]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from fitsnap_amd import _capi  # noqa: E402
from fitsnap_amd.solvers import robust  # noqa: E402


def timed(fn, reps, ctx=None):
    """(median host ms, median event ms of the row pass the call bracketed) over ``reps`` warm calls."""
    fn()
    fn()
    ts, ks = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
        if ctx is not None:
            ks.append(ctx.timing()["predict_ms"])
    return 1e3 * float(np.median(ts)), (float(np.median(ks)) if ks else float("nan"))


def problem(m, K, seed):
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((m, K))
    cat = rng.choice(3, size=m, p=(0.15, 0.55, 0.30)).astype(np.int32)
    sigma = np.array([1e-3, 5e-2, 2.0])[cat]
    b = A @ rng.standard_normal(K) + sigma * rng.standard_normal(m)
    out = rng.choice(m, m // 20, replace=False)
    b[out] += rng.uniform(20, 200, len(out)) * sigma[out]
    w = np.array([100.0, 1.0, 1e-2])[cat]
    return A, b, w, cat


def measure(m, K, reps):
    A, b, w, cat = problem(m, K, K)
    c = robust.DEFAULT_TUNE["huber"]
    ctx = _capi.HipContext(0)
    ctx.upload_rows(A, b)
    ctx.set_weights(w)
    beta = ctx.fit_resident(_capi.SOLVE_RIDGE, 1e-8)[0]
    t_fit0, _ = timed(lambda: ctx.fit_resident(_capi.SOLVE_RIDGE, 1e-8), reps)
    t_pk, k_pk = timed(lambda: ctx.predict(beta, want_preds=False, want_sse=True), reps, ctx)
    # the composed route, step by step and as a whole
    part = w > 0
    state = {}

    def host_step():
        e = w * (b - state["preds"])
        s, _ = robust.class_scales(e, cat, 3, part)
        r, _ = robust.robust_weight("huber", c, s[cat], e)
        state["wr"] = w * r

    def composed():
        state["preds"] = ctx.predict(beta)[0]
        host_step()
        ctx.set_weights(state["wr"])
        ctx.fit_resident(_capi.SOLVE_RIDGE, 1e-8)

    t_pred, _ = timed(lambda: state.__setitem__("preds", ctx.predict(beta)[0]), reps)
    t_host, _ = timed(host_step, reps)
    t_setw, _ = timed(lambda: (ctx.set_weights(state["wr"]), ctx.sync()), reps)
    t_comp, _ = timed(composed, reps)
    ctx.set_weights(w)
    # the new route
    ctx.robust_begin(cat, 3)
    t_r1, k_r1 = timed(lambda: ctx.robust_residuals(beta), reps, ctx)
    t_r2, _ = timed(ctx.robust_scale, reps)
    t_r3, k_r3 = timed(lambda: ctx.robust_reweight("huber", c), reps, ctx)
    t_fit, _ = timed(lambda: ctx.fit_resident(_capi.SOLVE_RIDGE, 1e-8), reps)
    t_fused, k_fused = timed(lambda: ctx.robust_step(beta, "huber", c), reps, ctx)

    def new_iter():
        ctx.robust_residuals(beta)
        ctx.robust_scale()
        ctx.robust_reweight("huber", c)
        ctx.fit_resident(_capi.SOLVE_RIDGE, 1e-8)

    def fused_iter():
        ctx.robust_step(beta, "huber", c)
        ctx.fit_resident(_capi.SOLVE_RIDGE, 1e-8)

    t_new, _ = timed(new_iter, reps)
    t_newf, _ = timed(fused_iter, reps)
    wr_dev = ctx.robust_download(e=False, wr=True)["wr"]
    ctx.robust_end()
    ctx.close()
    state["preds"] = A @ beta
    host_step()
    gb = m * K * 8 / 1e9
    return [
        f"m = {m}, K = {K}, 3 classes, huber; median of {reps} warm synchronous calls (host clock, ms); kernel = device events",
        f"  new route      R1 residuals {t_r1:.3f} (kernel {k_r1:.3f}, {gb / k_r1 * 1e3:.0f} GB/s of A)   R2 scale {t_r2:.3f}   "
        f"R3 reweight {t_r3:.3f} (kernels {k_r3:.3f})   fit {t_fit:.3f}   iteration {t_new:.3f}",
        f"  fused R1 + R3  step {t_fused:.3f} (kernels {k_fused:.3f})   iteration with known scales {t_newf:.3f}",
        f"  fsnap_predict  kernel with SSE, nothing downloaded: call {t_pk:.3f} (kernel {k_pk:.3f}, {gb / k_pk * 1e3:.0f} GB/s of A); "
        f"R1 kernel / predict kernel = {k_r1 / k_pk:.2f}",
        f"  composed route predict + download {t_pred:.3f}   numpy medians and weights {t_host:.3f}   set_weights {t_setw:.3f}   "
        f"fit (base weights) {t_fit0:.3f}   iteration {t_comp:.3f}",
        f"  iteration: composed / new = {t_comp / t_new:.1f}, composed / fused = {t_comp / t_newf:.1f}; the fit reading w r costs "
        f"{t_fit / t_fit0:.2f} x the fit reading the context's own weights; max |w r (device) - w r (numpy)| / w = "
        f"{np.max(np.abs(wr_dev - state['wr']) / w):.1e}",
    ]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if _capi.device_count() < 1:
        raise SystemExit("robust_timing.py needs a gfx950 GPU: nothing is measured without one")
    lines = []
    for m, K in ((1_000_000, 128), (15_213, 31)):
        lines += measure(m, K, args.reps)
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
