"""MCMC behind the reference's plugin API (fitsnap3lib/solvers/mcmc.py): an adaptive Metropolis chain over the coefficients
with the Gaussian log-posterior ``logpost(x) = sum_rows log N(aw . x; bw, sigma^2)``, started at ``lstsq(aw, bw, 1e-13)``.

The chain is the reference's ``amcmc`` step for step -- the same draws from numpy's global generator in the same order, the
same proposal expression, the same running mean / covariance recurrence and acceptance test -- so that its samples have the
reference's bits whenever the accept decisions agree.  What differs is how the log-posteriors are obtained:

* one GPU pass over the resident rows (``fsnap_sse_batch``) evaluates up to ``SPECULATE`` proposals.  Step k's random draws
  do not depend on the chain, so the proposals of steps k, k + 1, ... ASSUMING every step before them is rejected
  (``samples[k] + z_j F``) are known in advance; the host then walks the uniforms to the first accept ("prefetching"
  MCMC in its simplest form).  A batch never crosses an adaptation step, where the proposal covariance changes.  Since a
  proposal's value does not depend on the batch it was evaluated in, the chain is the sequential one.
* while the proposal covariance is exactly zero (the steps before the first adaptation) the proposal IS the current sample:
  those steps accept without an evaluation.
* the reference's O(steps^2) bookkeeping (sample weights rebuilt every step, unique samples concatenated on every accept) is
  done once at the end.

Several ranks: the rows are split, so every pass is collective.  Rank 0 runs the chain, broadcasts each batch, every rank
adds its rows' sums (``pt.allreduce_host``) and rank 0 decides; at the end the results are broadcast, so every rank has the
same ``fit`` and ``fit_sam`` bits.  Files are written on rank 0."""
from __future__ import annotations

import numpy as np

from .anl import transpose_trick_ok
from .merr import _TransposedRows
from .solver import Solver
from .svd import rows_lstsq

SPECULATE = 16        # proposals per GPU pass (1 ... 16; 1 = the sequential chain)
T0 = 100              # mcmc.py:124-125: t0, tadapt
TADAPT = 100


class ChainResult:
    """Everything ``amcmc`` returns (mcmc.py:77), plus ``accepted`` (bool per step), ``passes`` (evaluator calls) and
    ``cmode_step`` (index of ``cmode`` in ``samples``)."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def neg_logpost(sse, n, sigma):
    """-logpost from the pass's sums: -(n c0 - sse / (2 sigma^2)), c0 = -log(2 pi sigma^2) / 2 (mcmc.py:80-88)."""
    s2 = sigma * sigma
    c0 = -0.5 * np.log(2 * np.pi * s2)
    return -(n * c0 - 0.5 * np.asarray(sse, dtype=np.float64) / s2)


def run_chain(cini, nmcmc, gamma, evaluate, speculate=None, t0=T0, tadapt=TADAPT):
    """The reference's ``amcmc`` (mcmc.py:13-77) with covini = 0.  ``evaluate(U)`` returns -logpost of every row of
    U (P x K, P <= ``speculate``, default the module's ``SPECULATE``); the value of a row must not depend on the others.
    Draws exactly nmcmc - 1 (standard_normal(K), random_sample()) pairs from numpy's global generator."""
    spec = SPECULATE if speculate is None else speculate
    if not 1 <= spec <= 16:
        raise ValueError(f"speculate = {spec}: expected 1 ... 16")
    cini = np.array(cini, dtype=np.float64)
    cdim = cini.shape[0]
    cov = np.zeros((cdim, cdim))
    samples = np.zeros((nmcmc, cdim))
    sigcv = gamma * 2.4**2 / cdim
    samples[0] = cini
    passes = 1
    p1 = float(evaluate(samples[0:1].copy())[0])
    pmode = p1
    cmode_step = 0
    accepted = np.zeros(max(nmcmc - 1, 0), dtype=bool)
    F = np.zeros((cdim, cdim))          # factor of the proposal covariance: propcov = covini = 0 at first
    zero_F = True
    draws = {}                          # step -> (z, u), drawn ahead of the decisions, in the reference's order
    drawn = 0
    Xm = None

    def draw_through(last):
        nonlocal drawn
        while drawn <= last:
            z = np.random.standard_normal([cdim])
            draws[drawn] = (z, np.random.random_sample())
            drawn += 1

    def begin_step(k):
        # mcmc.py:35-47: running mean and covariance with samples[k]; a new proposal covariance at adaptation steps
        nonlocal Xm, cov, F, zero_F
        if k == 0:
            Xm = samples[0]
        else:
            Xm = (k * Xm + samples[k]) / (k + 1.0)
            rt = (k - 1.0) / k
            st = (k + 1.0) / k**2
            cov = rt * cov + st * np.dot(np.reshape(samples[k] - Xm, (cdim, 1)), np.reshape(samples[k] - Xm, (1, cdim)))
            if (k > t0) and (k % tadapt == 0):
                propcov = sigcv * (cov + 10**(-8) * np.identity(cdim))
                # numpy's legacy multivariate_normal: x = dot(z, sqrt(s)[:, None] * v) + mean with (u, s, v) = svd(cov)
                (_, s, v) = np.linalg.svd(propcov.astype(np.double))
                F = np.sqrt(s)[:, None] * v
                zero_F = not F.any()

    def is_adapt(k):
        return k > t0 and k % tadapt == 0

    k = 0
    while k < nmcmc - 1:
        begin_step(k)
        P = 1
        while P < spec and k + P < nmcmc - 1 and not is_adapt(k + P):
            P += 1
        if zero_F:
            P = 1                       # nothing to evaluate: the proposal is samples[k] itself
        draw_through(k + P - 1)
        mean = samples[k]
        props = np.empty((P, cdim))
        for i in range(P):
            x = np.dot(draws[k + i][0].reshape(-1, cdim), F)
            x += mean
            props[i] = x[0]
        if zero_F:
            p2 = np.array([p1])         # the same point: the same value, exp(0) = 1 accepts
        else:
            p2 = np.asarray(evaluate(props), dtype=np.float64)
            passes += 1
        nxt = k + P
        for i in range(P):
            s = k + i
            if i > 0:
                begin_step(s)
            _, u = draws.pop(s)
            pr = np.exp(p1 - p2[i])
            if u <= pr:
                samples[s + 1] = props[i]
                accepted[s] = True
                p1 = float(p2[i])
                if p1 <= pmode:
                    pmode = p1
                    cmode_step = s + 1
                nxt = s + 1
                break
            samples[s + 1] = samples[s]
        k = nxt                         # draws past the first accept stay for the next batch

    na = int(np.count_nonzero(accepted))
    change = np.concatenate([[0], np.flatnonzero(accepted) + 1]).astype(np.int64)
    weights = np.diff(np.concatenate([change, [nmcmc]])).astype(np.float64)
    return ChainResult(samples=samples, cmode=samples[cmode_step].copy(), pmode=pmode,
                       acc_rate=float(na) / max(nmcmc - 1, 1), accepted=accepted, sample_weights=weights,
                       unique_samples=samples[change].copy(), passes=passes, cmode_step=cmode_step)


def chain_samples(samples, nmcmc, nsam):
    """mcmc.py:126-128: every (nmcmc // 2) // nsam-th sample of the second half, the last nsam of them."""
    nevery = (nmcmc // 2) // nsam
    return samples[nmcmc // 2:nmcmc:nevery, :][-nsam:, :]


def save_chain_files(res, fit_sam):
    """mcmc.py:130-134: the chain, the kept samples, the mode, the unique samples and their weights, in the cwd."""
    np.savetxt("chn.txt", res.samples)
    np.savetxt("chn_sam.txt", fit_sam)
    np.save("mean.npy", res.cmode)
    np.save("unique_chn.npy", res.unique_samples)
    np.save("unique_chn_weights.npy", res.sample_weights)


class MCMC(Solver):

    def __init__(self, name, pt, config):
        super().__init__(name, pt, config)
        self.refine_steps = 2       # the start is SVD's lstsq (svd.py:54 / mcmc.py:122)
        self.row_space = True
        self.save_files = True      # the reference writes chn.txt, chn_sam.txt, mean.npy, unique_chn*.npy (mcmc.py:130-134)
        self.samples = None
        self.accepted = None
        self.acc_rate = None
        self.cmode = None
        self.pmode = None
        self.passes = 0
        # chain start: None = lstsq(aw, bw, 1e-13) of the rows (mcmc.py:122); an array = start there instead.  From the first
        # adaptation on, the proposals depend on the last bits of the start (the SVD of sigcv (cov + 1e-8 I) with cov ~ 0 is
        # degenerate), so only a start with the reference's bits gives the reference's chain
        self.cini = None

    def perform_fit(self, a=None, b=None, w=None, fs_dict=None, trainall=False):
        pt, config = self.pt, self.config
        sec = config.sections["SOLVER"]
        nmcmc, gamma, sigma, nsam = int(sec.mcmc_num), float(sec.mcmc_gamma), float(sec.mcmc_sigma), int(sec.nsam)
        if nmcmc < 2:
            raise ValueError(f"MCMC: mcmc_num = {nmcmc}, the chain needs at least 2 steps")
        if not 1 <= nsam <= nmcmc // 2:
            raise ValueError(f"MCMC: nsam = {nsam}, expected 1 ... mcmc_num // 2 = {nmcmc // 2} samples from the "
                             "second half of the chain")
        if not (a is None and b is None and w is None):
            # mcmc.py:111 multiplies a full-length w into a[training]; here w is indexed like the rows (one weight per row,
            # or already one per training row)
            w = np.asarray(w, dtype=np.float64)
            training = self._training_mask(a, fs_dict, trainall)
            if w.ndim == 1 and w.shape[0] == np.shape(a)[0] and w.shape[0] != int(np.count_nonzero(training)):
                w = w[training]
        transposed = False
        if "EXTRAS" in config.sections and config.sections["EXTRAS"].apply_transpose:
            G, c, _ = self._fit_statistics(a, b, w, fs_dict, trainall)
            transposed = transpose_trick_ok(G)          # mcmc.py:113-118
        if transposed:
            from scipy.linalg import lstsq
            start = lstsq(G, c, 1.0e-13)[0]             # mcmc.py:122 on (G, c)
        else:
            start = rows_lstsq(self, a, b, w, fs_dict, trainall)
        self.start = np.array(start, dtype=np.float64)
        if self.cini is not None:
            start = np.array(self.cini, dtype=np.float64).reshape(-1)
            if start.shape != self.start.shape:
                raise ValueError(f"MCMC: cini has {start.shape[0]} entries, the fit has {self.start.shape[0]} columns")
        if pt.multi:
            start = np.array(pt.bcast_object(np.asarray(start, dtype=np.float64), 0), dtype=np.float64)

        collective = pt.multi and not transposed       # (transposed: rank 0 holds all of (G, c))
        rows = None
        if transposed and pt._rank == 0:
            rows = _TransposedRows(pt, G, c)
        ctx = rows.ctx if rows is not None else pt.hip()
        K = len(start)

        def local_sums(U):
            sse, n = ctx.sse_batch(U)
            if collective:
                sums = pt.allreduce_host(np.concatenate([sse, [float(n)]]), 0)
                sse, n = sums[:-1], sums[-1]
            return sse, n

        def evaluate(U):
            if collective:
                pt.bcast_object(U, 0)
            sse, n = local_sums(U)
            return neg_logpost(sse, n, sigma)

        try:
            if pt._rank == 0:
                res = run_chain(start, nmcmc, gamma, evaluate)
                if collective:
                    pt.bcast_object(None, 0)            # the chain is done
            else:
                if collective:
                    while True:
                        U = pt.bcast_object(None, 0)
                        if U is None:
                            break
                        local_sums(U)
                res = None
        finally:
            if rows is not None:
                rows.close()
        if pt.multi:
            res = pt.bcast_object(res, 0)
        self.chain = res
        self.samples, self.accepted, self.acc_rate = res.samples, res.accepted, res.acc_rate
        self.cmode, self.pmode, self.passes = res.cmode, res.pmode, res.passes
        self.fit = res.cmode
        self.fit_sam = chain_samples(res.samples, nmcmc, nsam)
        if pt._rank == 0 and self.save_files:
            save_chain_files(res, self.fit_sam)
