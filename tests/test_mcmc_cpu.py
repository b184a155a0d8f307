"""CPU: the MCMC chain driver (fitsnap_amd/solvers/mcmc.py run_chain) reproduces the reference's own MCMC runs
(tests/golden/ta_mcmc_reference.npz) when it is driven by a numpy restatement of the reference's log-posterior, whatever
the speculation depth; the solver is registered and configured like the reference's."""
import os

import numpy as np
import pytest

from fitsnap_amd.config import Config
from fitsnap_amd.parallel_tools import ParallelTools
from fitsnap_amd.solvers import MCMC, solver_factory
from fitsnap_amd.solvers import mcmc as mcmc_mod
from fitsnap_amd.solvers.mcmc import chain_samples, neg_logpost, run_chain, save_chain_files

from mcmc_cases import case_rows, load_golden, numpy_evaluator, relmax

G = load_golden()
TAGS = [str(t) for t in G["tags"]]


def golden_chain(tag, speculate=None):
    aw, bw = case_rows(G, tag)
    n = int(G["nmcmc"])
    np.random.seed(int(G["seed"]))
    res = run_chain(G[f"{tag}_samples"][0], n, float(G[f"{tag}_gamma"]), numpy_evaluator(aw, bw, float(G[f"{tag}_sigma"])),
                    speculate=speculate)
    return res, np.random.random_sample()


@pytest.mark.parametrize("tag", TAGS)
def test_chain_matches_the_reference(tag):
    res, nxt = golden_chain(tag)
    n = int(G["nmcmc"])
    assert np.array_equal(res.accepted, G[f"{tag}_accepted"])
    stride = int(G["stride"])
    assert relmax(res.samples[::stride], G[f"{tag}_samples"]) <= 1e-10
    assert relmax(res.samples[-1], G[f"{tag}_last"]) <= 1e-10
    assert relmax(res.cmode, G[f"{tag}_cmode"]) <= 1e-10
    assert abs(res.pmode - float(G[f"{tag}_pmode"])) <= 1e-10 * abs(float(G[f"{tag}_pmode"]))
    fs = chain_samples(res.samples, n, 133)
    assert fs.shape == G[f"{tag}_fit_sam"].shape
    assert relmax(fs, G[f"{tag}_fit_sam"]) <= 1e-10
    assert np.array_equal(res.sample_weights, G[f"{tag}_weights"])
    assert res.acc_rate == float(G[f"{tag}_acc_rate"])
    assert nxt == float(G[f"{tag}_next_uniform"])          # the global generator is where the reference leaves it


def test_speculation_depth_does_not_change_the_chain():
    runs = {spec: golden_chain("train", spec)[0] for spec in (1, 4, 16)}
    for spec in (4, 16):
        assert np.array_equal(runs[spec].samples, runs[1].samples)
        assert np.array_equal(runs[spec].accepted, runs[1].accepted)
        assert runs[spec].pmode == runs[1].pmode
    assert runs[16].passes < runs[4].passes < runs[1].passes


def test_module_constant_sets_the_default_depth(monkeypatch):
    calls = []
    aw, bw = case_rows(G, "train")
    monkeypatch.setattr(mcmc_mod, "SPECULATE", 3)
    np.random.seed(0)
    run_chain(G["train_samples"][0], 400, 0.01, numpy_evaluator(aw, bw, 0.1, calls))
    assert max(calls) == 3


def test_warm_up_takes_no_evaluation():
    aw, bw = case_rows(G, "train")
    calls = []
    np.random.seed(1)
    res = run_chain(G["train_samples"][0], 201, 0.01, numpy_evaluator(aw, bw, 0.1, calls))
    assert calls == [1] and res.passes == 1                # only the start: steps 0 ... 199 use the zero covariance
    assert res.accepted.all()
    calls.clear()
    np.random.seed(1)
    res = run_chain(G["train_samples"][0], 202, 0.01, numpy_evaluator(aw, bw, 0.1, calls))
    assert calls == [1, 1] and res.passes == 2             # step 200 adapts: one proposal


def test_neg_logpost_from_sums():
    r = np.random.default_rng(0)
    aw, bw = r.standard_normal((50, 4)), r.standard_normal(50)
    x = r.standard_normal(4)
    sse = float(np.sum((aw @ x - bw) ** 2))
    ref = numpy_evaluator(aw, bw, 0.3)(x[None, :])[0]
    assert abs(neg_logpost(sse, 50, 0.3) - ref) <= 1e-12 * abs(ref)


def test_search_finds_mcmc():
    assert type(solver_factory.search("MCMC")) is MCMC
    assert type(solver_factory.search("mcmc")) is MCMC


def test_config_mcmc_defaults_and_values():
    sec = Config(None, {"SOLVER": {"solver": "MCMC"}}).sections["SOLVER"]
    assert sec.mcmc_num == 10000 and sec.mcmc_gamma == 0.01 and sec.mcmc_sigma == 0.1 and sec.nsam == 133
    sec = Config(None, {"SOLVER": {"solver": "MCMC", "mcmc_num": "500", "mcmc_gamma": "0.2", "mcmc_sigma": "3",
                                   "nsam": "7"}}).sections["SOLVER"]
    assert sec.mcmc_num == 500 and sec.mcmc_gamma == 0.2 and sec.mcmc_sigma == 3.0 and sec.nsam == 7
    assert Config(None, {"SOLVER": {"solver": "mcmc"}}).sections["SOLVER"].nsam == 0      # case-sensitive, as the reference
    assert Config(None, {"SOLVER": {"solver": "SVD"}}).sections["SOLVER"].nsam == 0


@pytest.mark.parametrize("settings", [{"mcmc_num": "1"}, {"mcmc_num": "100", "nsam": "51"}, {"nsam": "0"}])
def test_bad_chain_settings_raise_value_error(settings):
    pt = ParallelTools()
    cfg = Config(pt, {"SOLVER": dict({"solver": "MCMC"}, **settings)})
    s = solver_factory.solver("MCMC", pt, cfg)
    with pytest.raises(ValueError):
        s.perform_fit(np.ones((4, 2)), np.ones(4), np.ones(4), trainall=True)


def test_chain_files(tmp_path):
    res, _ = golden_chain("train")
    fs = chain_samples(res.samples, int(G["nmcmc"]), 133)
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        save_chain_files(res, fs)
    finally:
        os.chdir(cwd)
    assert np.array_equal(np.loadtxt(tmp_path / "chn.txt"), res.samples)
    assert np.array_equal(np.loadtxt(tmp_path / "chn_sam.txt"), fs)
    assert np.array_equal(np.load(tmp_path / "mean.npy"), res.cmode)
    uw = np.load(tmp_path / "unique_chn_weights.npy")
    assert np.array_equal(uw, G["train_weights"]) and uw.sum() == int(G["nmcmc"])
    uc = np.load(tmp_path / "unique_chn.npy")
    assert uc.shape == (len(uw), res.samples.shape[1])
    assert np.array_equal(uc[0], res.samples[0]) and np.array_equal(uc[-1], res.samples[-1])
