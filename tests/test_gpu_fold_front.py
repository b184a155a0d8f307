"""GPU: the front that fsnap_lasso_path, fsnap_ard_path and fsnap_omp_path share (fold_check / fold_stage / fold_finish in
csrc/fsnap_capi.cpp) -- one context and its one fold buffer serve the three entry points in turn, and a shared refusal leaves
the context as it was.  The kernels' own acceptance is tests/test_gpu_{lasso,ard,omp}_path.py's; here every figure is compared
bit for bit with the same call on a fresh context."""
import os
import sys

import numpy as np
import pytest

from fitsnap_amd import _capi
from fitsnap_amd.solvers import ard_path as ap
from fitsnap_amd.solvers import lasso_path as lp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lasso_path_cases as cs  # noqa: E402

F, Q, S = 2, 2, 2
SHAPES = [(3, 1), (65, 2), (3, 2), (65, 1)]       # (K, nsub): one and two columns per lane; without and with a fold buffer
GRID = [{"logcut": 1.0, "scap": 1e-3, "scai": 1e-3}, {"logcut": 2.0, "scap": 1e-3, "scai": 1e-3}]


class Stats:
    """F * nsub packed blocks of about 3 K + 10 rows each, left in device memory by a context of their own (``owner``: the
    contexts under test hold no rows and no statistics), and the arguments of the three entry points."""

    def __init__(self, K, nsub):
        ncat = F * nsub
        A, b, w, cat, _ = cs.fold_rows(9100 + 10 * K + nsub, K, [3 * K + 10 + i for i in range(ncat)])
        self.K, self.nsub = K, nsub
        self.owner = _capi.HipContext(0)
        self.owner.upload_rows(A, b)
        self.owner.set_weights(w, None)
        self.ptr = self.owner.cat_normal_eq(self.owner.cat_prepare(cat.astype(np.int32), ncat))
        blocks = lp.download_blocks(self.owner, self.ptr, ncat, K)      # waits for the statistics pass
        self.alphas = cs.alpha_grid(blocks, K, [0.05, 1e-3], nsub)
        self.hyper, run = ap.fold_hypers(*lp.sum_blocks(blocks, nsub), K, GRID, False)
        assert run.all()

    def call(self, ctx, entry):
        if entry == "lasso":
            return ctx.lasso_path(self.ptr, self.K, F, self.nsub, self.alphas, 1000, 1e-6)
        if entry == "ard":
            return ctx.ard_path(self.ptr, self.K, F, self.nsub, self.hyper, 50, 1e-3)
        return ctx.omp_path(self.ptr, self.K, F, self.nsub, "ols", (), S, [1, 2])

    def fresh(self, entry):
        ctx = _capi.HipContext(0)
        try:
            return self.call(ctx, entry)
        finally:
            ctx.close()


def same_bits(got, want):
    return len(got) == len(want) and all(x.dtype == y.dtype and x.tobytes() == y.tobytes() for x, y in zip(got, want))


@pytest.mark.gpu
def test_one_context_serves_the_three_entry_points_and_survives_their_shared_refusals():
    stats = [Stats(K, nsub) for K, nsub in SHAPES]
    # the fold buffer: absent in use (total of K = 3 alone), grown (K = 65, folds and total), shrunk in use (K = 3, folds and
    # total), folds dropped again (total of K = 65 alone)
    order = ["lasso", "omp", "ard", "lasso"]
    ctx = _capi.HipContext(0)
    try:
        for st, entry in zip(stats, order):
            assert same_bits(st.call(ctx, entry), st.fresh(entry)), (entry, st.K, st.nsub)
        # a refusal that the three entry points share: the same exception from each, whatever else is valid
        ok = stats[2]
        for change in (dict(F=0), dict(nsub=0), dict(Q=0), dict(ptr=None), dict(K=145)):
            kinds = set()
            for entry in ("lasso", "ard", "omp"):
                kinds.add(type(refusal(ctx, ok, entry, **change)))
            assert kinds == {ValueError}, (change, kinds)
        for entry in ("omp", "ard", "lasso"):
            assert same_bits(ok.call(ctx, entry), ok.fresh(entry)), ("after the refusals", entry)
    finally:
        ctx.close()
        for st in stats:
            st.owner.close()


def refusal(ctx, st, entry, F=F, nsub=None, Q=Q, ptr=0, K=None):
    """The exception of one call with one shared argument changed (None: none was raised)."""
    K = st.K if K is None else K
    nsub = st.nsub if nsub is None else nsub
    ptr = st.ptr if ptr == 0 else ptr
    try:
        if entry == "lasso":
            ctx.lasso_path(ptr, K, F, nsub, st.alphas[:Q], 1000, 1e-6)
        elif entry == "ard":
            ctx.ard_path(ptr, K, F, nsub, np.ones((max(F, 0) + 1, Q, 6)), 50, 1e-3)
        else:
            ctx.omp_path(ptr, K, F, nsub, "ols", (), S, [1, 2][:Q])
    except Exception as e:                                   # noqa: BLE001 -- the kind is what the test compares
        return e
    return None
