"""GPU: fsnap_sse_batch (kernels S1 / S1G of csrc/fsnap_mcmc.hip) against extended precision, its batch invariance, and
the MCMC solver against the reference's own runs (tests/golden/ta_mcmc_reference.npz): accept pattern, samples, mode,
speculation, residency, scale, predictive variance, the CLI and two ranks."""
import os
import subprocess
import sys

import numpy as np
import pytest

from fitsnap_amd import _capi
from fitsnap_amd.config import Config
from fitsnap_amd.parallel_tools import ParallelTools
from fitsnap_amd.solvers import solver_factory
from fitsnap_amd.solvers import mcmc as mcmc_mod
from fitsnap_amd.solvers.mcmc import chain_samples, run_chain

from mcmc_cases import case_rows, load_golden, numpy_evaluator, relmax

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
G = load_golden()
TAGS = [str(t) for t in G["tags"]]


def _problem(m, K, seed, nan_test_rows=False, zero_w=False):
    r = np.random.default_rng(seed)
    A = r.standard_normal((m, K)) * (1.0 + r.random(K))
    b = A @ r.standard_normal(K) + 0.3 * r.standard_normal(m)
    w = 0.5 + r.random(m)
    mask = (r.random(m) < 0.85).astype(np.uint8)
    mask[0] = 1
    if zero_w:
        w[r.random(m) < 0.2] = 0.0
    if nan_test_rows:
        t = np.flatnonzero(mask == 0)
        A[t[: len(t) // 2], 0] = np.nan
        b[t[len(t) // 2:]] = np.inf
        w[t[::3]] = np.nan
    return A, b, w, mask


def _ctx_for(A, b, w, mask, lda=None):
    ctx = _capi.HipContext(0)
    m, K = A.shape
    keep = None
    if lda is None:
        ctx.upload_rows(A, b)
    else:
        import torch
        dev = torch.zeros((m + 1) * lda, dtype=torch.float64, device="cuda:0")
        dev[: m * lda].view(m, lda)[:, :K] = torch.from_numpy(A).to("cuda:0")
        db = torch.from_numpy(b.copy()).to("cuda:0")
        ctx.bind_rows(dev.data_ptr(), m, K, lda, db.data_ptr())
        keep = (dev, db)
    ctx.set_weights(w, mask.astype(bool))
    return ctx, keep


def np_sse(A, b, w, mask, U):
    """(sse[P] in long double, the scale sum (w (|a| . |u| + |b|))^2 of each)."""
    L = np.longdouble
    k = mask.astype(bool)
    Ak, bk, wk = A[k].astype(L), b[k].astype(L), w[k].astype(L)
    r = wk[:, None] * (Ak @ U.T.astype(L) - bk[:, None])
    scale = (np.abs(wk)[:, None] * (np.abs(Ak) @ np.abs(U.T).astype(L) + np.abs(bk)[:, None])) ** 2
    return np.sum(r * r, axis=0), np.sum(scale, axis=0)


KERNEL_CASES = [  # (m, K, lda, extras)
    (1, 1, None, {}), (15, 3, None, {"zero_w": True}), (17, 31, 37, {"nan_test_rows": True}),
    (1000, 128, None, {"nan_test_rows": True}), (15213, 31, None, {"zero_w": True}), (1000, 142, 149, {}),
    (17, 288, None, {"nan_test_rows": True}), (1000, 288, 293, {"zero_w": True}), (1, 1595, None, {}),
    (1000, 1595, 1601, {"nan_test_rows": True, "zero_w": True}), (15213, 128, None, {}),
]


@pytest.mark.parametrize("P", [1, 7, 16])
@pytest.mark.parametrize("m,K,lda,extra", KERNEL_CASES)
def test_sse_batch_matches_extended_precision(m, K, lda, extra, P):
    A, b, w, mask = _problem(m, K, m + K + P, **extra)
    r = np.random.default_rng(P)
    U = r.standard_normal((P, K))
    ctx, keep = _ctx_for(A, b, w, mask, lda)
    sse, n = ctx.sse_batch(U)
    ref, scale = np_sse(A, b, w, mask, U)
    assert n == int(mask.sum())
    assert np.all(np.isfinite(sse))
    err = np.abs(sse.astype(np.longdouble) - ref) / np.maximum(scale, np.longdouble(1e-300))
    assert float(err.max()) <= 1e-13, (float(err.max()), sse, ref)
    ctx.close()


@pytest.mark.parametrize("K", [31, 128, 200])
def test_sse_batch_is_batch_invariant_and_deterministic(K):
    A, b, w, mask = _problem(20_011, K, K, nan_test_rows=True)
    ctx, _ = _ctx_for(A, b, w, mask)
    r = np.random.default_rng(3)
    v = r.standard_normal(K)
    one, _ = ctx.sse_batch(v[None, :])
    U = r.standard_normal((16, K))
    U[13] = v
    many, _ = ctx.sse_batch(U)
    again, _ = ctx.sse_batch(U)
    assert one[0] == many[13]
    assert np.array_equal(many, again)
    singles = np.array([ctx.sse_batch(U[p:p + 1])[0][0] for p in range(16)])
    assert np.array_equal(singles, many)
    ctx.close()


def test_sse_batch_errors_and_empty_context():
    A, b, w, mask = _problem(100, 8, 1)
    ctx, _ = _ctx_for(A, b, w, mask)
    with pytest.raises(ValueError):
        ctx.sse_batch(np.zeros((17, 8)))
    with pytest.raises(ValueError, match="resident rows have 8 columns"):
        ctx.sse_batch(np.zeros((2, 9)))             # K is not the resident width
    lib = _capi.load_library()
    assert lib.fsnap_sse_batch(ctx._h, 8, _capi._ptr(np.zeros(8)), 0, _capi._ptr(np.zeros(1)), None) == _capi.E_ARG
    ctx.close()
    empty = _capi.HipContext(0)
    sse, n = empty.sse_batch(np.ones((3, 5)))
    assert n == 0 and np.array_equal(sse, np.zeros(3))
    empty.close()


def test_sse_batch_keeps_rows_and_category_layout():
    A, b, w, mask = _problem(5000, 31, 2)
    ctx, _ = _ctx_for(A, b, w, mask)
    cat = (np.arange(5000) % 7).astype(np.int32)
    tag = ctx.cat_prepare(cat, 7)
    for _ in range(3):
        ctx.sse_batch(np.random.default_rng(0).standard_normal((16, 31)))
    assert ctx.cat_info()["layout"] == tag
    ctx.cat_normal_eq(tag)                          # the layout is still accepted
    a2, b2, w2 = ctx.download_rows()
    assert np.array_equal(a2, A) and np.array_equal(b2, b)
    ctx.close()


# -- the solver ---------------------------------------------------------------------------------------------------------
def _ta():
    z = np.load(os.path.join(GOLDEN, "ta_abw.npz"))
    return np.ascontiguousarray(z["A"]), np.ascontiguousarray(z["b"]), np.ascontiguousarray(z["w"])


def _mcmc_solver(nmcmc, gamma, sigma, transpose=False, nsam=None):
    pt = ParallelTools()
    sol = {"solver": "MCMC", "mcmc_num": nmcmc, "mcmc_gamma": gamma, "mcmc_sigma": sigma}
    if nsam is not None:
        sol["nsam"] = nsam
    raw = {"SOLVER": sol}
    if transpose:
        raw["EXTRAS"] = {"apply_transpose": 1}
    s = solver_factory.solver("MCMC", pt, Config(pt, raw))
    return pt, s


def _golden_fit(tag, shared=False, own_start=False):
    """The golden case's fit; the chain starts at the reference's own start unless ``own_start`` (the proposals after the
    first adaptation depend on the last bits of the start, see MCMC.cini)."""
    A, b, w = _ta()
    testing = G[f"{tag}_testing"]
    pt, s = _mcmc_solver(int(G["nmcmc"]), float(G[f"{tag}_gamma"]), float(G[f"{tag}_sigma"]),
                         bool(int(G[f"{tag}_transpose"])))
    if not own_start:
        s.cini = G[f"{tag}_samples"][0]
    np.random.seed(int(G["seed"]))
    if shared:
        m, K = A.shape
        pt.create_shared_array("a", m, K)
        pt.create_shared_array("b", m)
        pt.create_shared_array("w", m)
        pt.shared_arrays["a"].array[:] = A
        pt.shared_arrays["b"].array[:] = b
        pt.shared_arrays["w"].array[:] = w
        pt.fitsnap_dict["Testing"] = testing.tolist()
        s.perform_fit()
    else:
        s.perform_fit(A, b, w, fs_dict={"Testing": testing.tolist()})    # full-length w, indexed like the rows
    return pt, s


@pytest.mark.parametrize("tag", TAGS)
def test_mcmc_class_matches_the_reference(tag, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    pt, s = _golden_fit(tag, shared=(tag == "train"))      # "testing": a full-length w with testing rows, indexed
    assert np.array_equal(s.accepted, G[f"{tag}_accepted"])
    assert relmax(s.samples[::int(G["stride"])], G[f"{tag}_samples"]) <= 1e-10
    assert relmax(s.cmode, G[f"{tag}_cmode"]) <= 1e-10 and relmax(s.fit, G[f"{tag}_fit"]) <= 1e-10
    assert relmax(s.fit_sam, G[f"{tag}_fit_sam"]) <= 1e-10
    assert abs(s.pmode - float(G[f"{tag}_pmode"])) <= 1e-9 * abs(float(G[f"{tag}_pmode"]))
    assert np.random.random_sample() == float(G[f"{tag}_next_uniform"])
    for name in ("chn.txt", "chn_sam.txt", "mean.npy", "unique_chn.npy", "unique_chn_weights.npy"):
        assert (tmp_path / name).exists()
    assert np.array_equal(np.load(tmp_path / "unique_chn_weights.npy"), G[f"{tag}_weights"])
    # the class's own start is the reference's lstsq solution up to rounding (on (G, c), cond(G) ~ 7e10 amplifies the
    # rounding of G itself)
    assert relmax(s.start, G[f"{tag}_samples"][0]) <= (1e-5 if int(G[f"{tag}_transpose"]) else 1e-9)
    pt.free()


def test_mcmc_class_own_start_runs_the_chain(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    pt, s = _golden_fit("train", own_start=True)
    assert np.array_equal(s.samples[0], s.start)
    assert np.array_equal(s.accepted[:199], G["train_accepted"][:199])      # the warm-up accepts every step
    assert 0.02 < s.acc_rate < 0.5 and np.all(np.isfinite(s.samples))
    assert abs(s.pmode - float(G["train_pmode"])) <= 1e-3 * abs(float(G["train_pmode"]))
    pt.free()


def test_speculation_changes_passes_not_the_chain(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    runs = {}
    for spec in (1, 16):
        monkeypatch.setattr(mcmc_mod, "SPECULATE", spec)
        pt, s = _golden_fit("train")
        runs[spec] = (s.samples.copy(), s.accepted.copy(), s.fit.copy(), s.passes)
        pt.free()
    assert np.array_equal(runs[1][0], runs[16][0]) and np.array_equal(runs[1][1], runs[16][1])
    assert np.array_equal(runs[1][2], runs[16][2])
    assert runs[16][3] < runs[1][3] / 3, (runs[16][3], runs[1][3])


def test_mcmc_at_scale_matches_the_numpy_chain(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    r = np.random.default_rng(32)
    m, K = 1_000_000, 32
    A = r.standard_normal((m, K))
    b = A @ r.standard_normal(K) + 0.1 * r.standard_normal(m)
    w = np.full(m, 0.01)
    pt, s = _mcmc_solver(400, 0.01, 0.1, nsam=10)
    s.save_files = False
    np.random.seed(4)
    s.perform_fit(A, b, w, trainall=True)
    aw, bw = w[:, None] * A, w * b
    np.random.seed(4)
    ref = run_chain(s.samples[0], 400, 0.01, numpy_evaluator(aw, bw, 0.1))
    assert np.array_equal(s.accepted, ref.accepted)
    assert np.array_equal(s.samples, ref.samples)
    assert s.accepted[200:].any()                    # the chain moved after the warm-up
    pt.free()


def test_sam_variance_on_mcmc_samples(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    pt, s = _golden_fit("train")
    A, _, _ = _ta()
    rows = A[:500]
    sd = s._compute_stdev(rows, method="sam")      # the reference's sam: the std of the predictions over fit_sam
    ref = np.std(rows @ s.fit_sam.T, axis=1)
    assert sd.shape == (500,)
    assert np.max(np.abs(sd - ref)) <= 1e-9 * np.max(ref)
    pv = s.prediction_variance(rows, method="sam")
    assert np.max(np.abs(pv["var"] - ref ** 2)) <= 1e-9 * np.max(ref ** 2)
    assert np.max(np.abs(pv["preds"] - rows @ s.fit)) <= 1e-12 * np.max(np.abs(rows @ s.fit))
    pt.free()


def test_python_m_fitsnap3_runs_mcmc(tmp_path, monkeypatch):
    import runpy

    import pandas as pd

    from fitsnap_amd.io.outputs.snap import parse_snapcoeff

    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_cli_cpu import TA_IN

    A, b, w = _ta()
    np.save(tmp_path / "Descriptors.npy", A)
    np.save(tmp_path / "Truth-Ref.npy", b)
    np.save(tmp_path / "Weights.npy", w)
    m = len(b)
    df = pd.DataFrame({"Row_Type": ["Energy"] * 363 + ["Force"] * 12672 + ["Stress"] * 2178, "Groups": ["Ta"] * m,
                       "Configs": ["c"] * m, "Testing": [False] * m, "Atom_I": [0] * m, "Atom_Type": [0] * m})
    df.to_pickle(tmp_path / "FitSNAP.df")
    text = TA_IN.replace("dump_descriptors = 1", "dump_descriptors = 0")
    text = text.replace("solver = SVD", "solver = MCMC\nmcmc_num = 600\nmcmc_gamma = 0.01\nmcmc_sigma = 0.1\nnsam = 20")
    (tmp_path / "Ta.in").write_text(text)
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(sys, "argv", ["fitsnap3", "Ta.in", "--descriptors", str(tmp_path), "--overwrite"])
    np.random.seed(0)
    with pytest.raises(SystemExit) as e:
        runpy.run_module("fitsnap3", run_name="__main__", alter_sys=True)
    assert e.value.code == 0
    for name in ("chn.txt", "chn_sam.txt", "mean.npy", "unique_chn.npy", "unique_chn_weights.npy"):
        assert (tmp_path / name).exists(), name
    mean = np.load(tmp_path / "mean.npy")
    assert np.loadtxt(tmp_path / "chn.txt").shape == (600, 31) and np.loadtxt(tmp_path / "chn_sam.txt").shape == (20, 31)
    coeffs = parse_snapcoeff(tmp_path / "Ta_pot.snapcoeff")
    assert np.max(np.abs(coeffs - mean)) <= 1e-10 * np.max(np.abs(mean))


def test_mcmc_two_ranks_p2p_match_one_rank(tmp_path, monkeypatch):
    world = 2
    procs = []
    for rank in range(world):
        env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "LOCAL_WORLD_SIZE")}
        env.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), LOCAL_WORLD_SIZE=str(world),
                   FSNAP_COMM_FILE=str(tmp_path / "comm_id"), FSNAP_COMM_TOKEN="mcmc two ranks",
                   HSA_ENABLE_IPC_MODE_LEGACY="0", FSNAP_COMM_TIMEOUT="120", FSNAP_DIST_TRANSPORT="p2p")
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "mcmc_dist_worker.py"), str(tmp_path)],
                                      env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, cwd=tmp_path))
    logs = []
    for p in procs:
        try:
            logs.append(p.communicate(timeout=600)[0])
        except subprocess.TimeoutExpired:
            p.kill()
            logs.append(p.communicate()[0] + "\n[killed after 600 s]")
    assert all(p.returncode == 0 for p in procs), "\n".join(logs)[-4000:]
    r0, r1 = (dict(np.load(tmp_path / f"mcmc_rank{r}.npz")) for r in range(world))
    assert np.array_equal(r0["fit"], r1["fit"]) and np.array_equal(r0["fit_sam"], r1["fit_sam"])
    assert (tmp_path / "chn.txt").exists()
    monkeypatch.chdir(tmp_path)
    pt, s = _golden_fit("train")
    assert np.array_equal(r0["accepted"], s.accepted)
    assert np.array_equal(r0["samples"], s.samples)
    assert relmax(r0["start"], s.start) <= 1e-9        # the lstsq start of two ranks' rows
    pt.free()
