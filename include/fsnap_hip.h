/* fsnap_hip.h — C ABI of libfsnap_hip.so: the MI355X (gfx950) linear-fit hot path for
 * FitSNAP, callable from the reference's Python over ctypes.
 *
 * Boundary rules: extern "C"; plain pointers and sizes only (no torch / numpy types);
 * every function returns an int status — 0 = ok, negative = argument / runtime error
 * (text via fsnap_last_error), positive = numerical failure (e.g. non-SPD normal
 * matrix); no C++ exception ever crosses the boundary.  The caller owns every buffer it
 * passes.  Matrices are row-major fp64; sizes are int64_t; the training mask is uint8_t
 * with 1 = training row (the negation of the reference's fitsnap_dict['Testing']).
 * A context is bound to ONE GPU (one process per GPU; a multi-GPU job gives every rank's
 * context a native RCCL communicator, fsnap_comm_*, and all-reduces the packed statistics).
 * Calls on one context must not be made concurrently from several threads; the ctypes
 * shim releases the GIL for the duration of each call.
 *
 * Each entry point names the reference code it replaces (file:line in FitSNAP/FitSNAP
 * at the surveyed revision).
 */
#ifndef FSNAP_HIP_H
#define FSNAP_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct fsnap_ctx fsnap_ctx;

/* status codes */
#define FSNAP_OK 0
#define FSNAP_E_ARG (-1)      /* bad argument (null pointer, size, unsupported K ...) */
#define FSNAP_E_HIP (-2)      /* HIP runtime error; text in fsnap_last_error          */
#define FSNAP_E_STATE (-3)    /* call order (no rows uploaded, no weights ...)        */
#define FSNAP_E_NOMEM (-4)    /* device / host allocation failed -> MemoryError       */
#define FSNAP_NUM_NOT_SPD 1   /* normal matrix not positive definite -> LinAlgError   */
#define FSNAP_NUM_SINGULAR 2  /* exactly singular system -> LinAlgError               */
#define FSNAP_NUM_NONFINITE 3 /* NaN/Inf in the statistics -> ValueError              */

/* solve kinds for fsnap_solve */
#define FSNAP_SOLVE_CHOL 0       /* G beta = c, SPD required                                        */
#define FSNAP_SOLVE_LSTSQ 1      /* min-norm least squares, param = rcond  (svd.py:54 lstsq(aw,bw,1e-13)) */
#define FSNAP_SOLVE_RIDGE 2      /* (G + alpha I) beta = c, param = alpha (ridge.py:47-57, sklearn Ridge) */
#define FSNAP_SOLVE_RIDGE_INV 3  /* beta = inv(G + alpha I) c             (regressor.py:10-16 Local_Ridge) */
/* LSTSQ / RIDGE / RIDGE_INV without the fallback behind the Cholesky factorisations: when no Cholesky factorisation resolves the system the call returns
 * FSNAP_OK at once with *rank = -1 and beta = 0 (and *rcond_est as described at fsnap_solve) instead of running the
 * cyclic-Jacobi eigendecomposition -- O(K^3) per sweep on one core: 58 s at K = 1595.  For callers that have something
 * better to fall back on: the rows (fsnap_lstsq_rows) or a LAPACK eigensolver. */
#define FSNAP_SOLVE_LSTSQ_PROBE 4
#define FSNAP_SOLVE_RIDGE_PROBE 5
#define FSNAP_SOLVE_RIDGE_INV_PROBE 6 /* ... instead of the scalar LU with partial pivoting (np.linalg.inv semantics) */

/* packed statistics buffer: [ G (K*K row-major) | c (K) | bTb, sum(w*b), n_train ] */
#define FSNAP_PACKED_LEN(K) ((int64_t)(K) * (K) + (K) + 3)

/* ---- library / context ------------------------------------------------------------ */

/* ABI version (major*100 + minor). */
int fsnap_version(void);

/* Number of visible HIP devices. */
int fsnap_device_count(int* count);

/* Create a context on HIP device `device` (own non-blocking stream, timing events).
 * Replaces nothing in the reference: the reference's solvers are rank-0 numpy. */
int fsnap_ctx_create(int device, fsnap_ctx** ctx);
int fsnap_ctx_destroy(fsnap_ctx* ctx);

/* Run all subsequent work of this context on the caller's hipStream_t (e.g.
 * torch.cuda.current_stream().cuda_stream) so that RCCL collectives issued by the host
 * layer order after the kernels without a host sync.  NULL = the HIP default stream. */
int fsnap_ctx_set_stream(fsnap_ctx* ctx, void* hip_stream);

/* Go back to the context's own non-blocking stream. */
int fsnap_ctx_use_own_stream(fsnap_ctx* ctx);

/* Options (all optional; defaults in brackets).  Every key steers a path a default configuration can take -- the A/B forms
 * of rounds 1-5 that lost their measurements (kernels 1 / 1L / 1T2, Cholesky forms 0-4, reduce-to-root fits, ...) are gone,
 * their records are in profiles/ and HISTORY.md:
 * "nblocks" [0 = auto] workgroups of the SYRK kernels 1A / 1P / 1Q (clusters of 1QC, row chunks of 1S);
 * "nsplit" [0 = a scheduling model] row splits of the tiled kernel 1T;
 * "tiled" [0] 1 = the general-K tiled kernel 1T at every width (what short systems of 145 ... 512 columns, K > 512 and the
 *   row-space passes at K > 144 run on by default);
 * "short" [-1 = systems of 81 ... 144 columns with at most three staging phases of rows per pair of CUs (a phase: 128 rows, 112 at
 *   129 ... 144 columns -- 43 008 ... 49 152 rows on 256 CUs) take kernel 1S, which deals the tile triangle over 16 waves per row chunk
 *   instead of giving every wave the whole triangle (13 035 x 142, examples/Ta_PACE_RIDGE)] 0 = never (kernel 1A), 1 = at
 *   every row count (chunks longer than a phase are staged in several);
 * "quad_min_rows" [-1 = 8 192 rows for 145 ... 288 columns (kernel 1Q), 300 000 for 289 ... 512 (kernel 1QC)] fewest rows for
 *   the accumulator-resident kernels at those widths; shorter systems take the tiled kernel;
 * "fused_pack" [1] kernels 1A / 1S / 1P / 1Q / 1QC form the per-row pairs (mask * w, mask * w * b) of their rows in LDS inside the
 *   SYRK launch whenever a workgroup's rows fit; 0 = always the separate packing kernel (the form of larger shards and of the
 *   row-space passes);
 * "repack" [0] 1 = recompute the per-row pairs and the b-only scalars on EVERY fit even when b, w and the mask are
 *   context-owned and unchanged (what a step of bench.py does);
 * "timing_every" [1] HIP events bracket every N-th SYRK launch only -- an event record between two dependent kernels idles
 *   the stream for ~5.6 us; 0 = no events; the first launch after the option is set is a sampled one (fsnap_timing /
 *   fsnap_timing_history see the sampled ones);
 * "device_solve" [0 = K >= 232 is factorised on the GPU by the blocked kernels] 1 = from 129 columns on, 2 = never (host);
 * "chol_reuse" [1] fsnap_solve_device_rhs with a right-hand side of its own -- the refinement steps of a fit, the sweeps of the
 *   condition estimate -- runs a forward and a backward sweep with the factor the last solve of the context's own statistics
 *   left on the device (0.2 instead of 0.54 ms at K = 1595); 0 = factorise again;
 * "fused_residual" [1] fsnap_residual_rhs for K <= 288 in one pass over the rows; 0 = the two-kernel form of wider systems;
 * "rowspace_reuse_stats" [0; one-shot, cleared by the next fsnap_lstsq_rows] 1 = the caller states that the fit from the
 *   statistics which just ran -- fsnap_fit_resident on this context -- saw the rows, weights and mask as they are now; a
 *   single-rank fsnap_lstsq_rows on a system the host factorises then starts its first pass from that fit's statistics, still
 *   in the page-locked mirror, instead of computing them again: 0.35 ms of a 10^6 x 128 call;
 * "reduce_triangle" [-1 = systems of >= 256 columns all-reduce [upper triangle | c | scalars], K (K + 1) / 2 + K + 3 doubles,
 *   between a pack and an unpack kernel] 0 = always the full K^2 + K + 3, 1 = always the triangle -- every rank of a job must
 *   use the same setting;
 * "comm_timeout" [0 = the FSNAP_COMM_TIMEOUT environment default] seconds: bound of every wait behind a collective of this
 *   context and of fsnap_comm_init;
 * "staged_upload" [0 = the runtime's pageable copy: it pins the caller's pages and reads them in place, 27 ms for 1.03 GB
 *   where pinning is cheap] fsnap_upload_rows: 2 = a page-locked double buffer filled by FSNAP_UPLOAD_THREADS (default 4)
 *   host threads while the DMA drains the other slot -- for hosts with free cores and slow pinning; 1 = double buffer, handing
 *   the rest to the pageable copy when the host fills its first two 16 MiB slots at less than 20 GB/s.
 * Unknown key -> FSNAP_E_ARG. */
int fsnap_set_option(fsnap_ctx* ctx, const char* key, int64_t value);

/* Last error text of this context (or of the library when ctx is NULL).  Never NULL. */
const char* fsnap_last_error(const fsnap_ctx* ctx);

/* ---- rows: the A matrix and truth vector ----------------------------------------- */

/* Copy the m x K row-major fp64 matrix A (leading dimension lda doubles) and b[m] from
 * host memory into HBM; they stay resident for any number of re-weightings / fits.
 * Device-side counterpart of pt.shared_arrays['a'|'b'].array
 * (fitsnap3lib/parallel_tools.py:352-389, 944-1077; calculator.py:287-288). */
int fsnap_upload_rows(fsnap_ctx* ctx, const double* A, int64_t m, int64_t K, int64_t lda, const double* b);

/* Same, but A and b already live in device memory (not copied, not owned; the A
 * allocation must be readable for 16 bytes past its last element). */
int fsnap_bind_rows(fsnap_ctx* ctx, const double* dA, int64_t m, int64_t K, int64_t lda, const double* db);

/* This context holds no rows any more (context-owned copies are freed, bound ones forgotten): what a rank of a
 * multi-GPU job calls when the configurations dealt to it for the NEXT fit are none (config i -> rank i % nranks,
 * fitsnap3lib/parallel_tools.py:612-651, with fewer configurations than ranks) -- fsnap_fit_dist / fsnap_lstsq_rows
 * then contribute zeros instead of the rows of an earlier fit. */
int fsnap_drop_rows(fsnap_ctx* ctx);

/* Allocate resident, zero-filled A (m x K), b[m], w[m] in HBM without a host copy: the
 * device-side counterpart of Calculator.create_a -> pt.create_shared_array('a'|'b'|'w')
 * (fitsnap3lib/calculators/calculator.py:261-289), to be filled by fsnap_assemble. */
int fsnap_rows_alloc(fsnap_ctx* ctx, int64_t m, int64_t K);

/* Post-LAMMPS assembly of a batch of configurations straight into the resident rows
 * [row0, row0 + nrows): the `_collect_lammps` transform
 * (fitsnap3lib/calculators/lammps_snap.py:391-556, lammps_pace.py:369-509; single-config
 * form lammps_snap.py:224-389) without the host copy of A.
 *   raw[raw_rows * raw_ld]  the LAMMPS `compute snap|pace` global arrays of the batch, stacked
 *                           (what _extract_compute_np views, lammps_base.py:280-307);
 *                           raw_ld >= ncoeff*ntypes + 1, column ncoeff*ntypes = reference potential
 *   per output row r: src_row[r] (row of raw), kind[r] (0 energy: A = x/d, b = (truth-ref)/d;
 *     1 force: A = x, b = truth-ref; 2 virial: A = (1.6021765e6 x)/d, b = truth-ref;
 *     3 extra per-atom energy row: A = x/d, b = 0, w = 0), d[r] (atoms or cell volume),
 *     truth[r], weight[r], frac[r] (row of `fractions`, or -1)
 *   fractions[nfrac * ntypes]  per-configuration atom-type fractions (offset column of energy rows)
 *   blank2J[K]; offcol = 1 when bzeroflag = 0 (K = ntypes*(ncoeff+1)), else 0.
 * All pointers are host memory; synchronous. */
int fsnap_assemble(fsnap_ctx* ctx, const double* raw, int64_t raw_rows, int64_t raw_ld, int64_t nrows, int64_t row0,
                   const int64_t* src_row, const int32_t* kind, const int32_t* frac, const double* d,
                   const double* truth, const double* weight, const double* fractions, int64_t nfrac,
                   const double* blank2J, int32_t ntypes, int32_t ncoeff, int32_t offcol);

/* Copy the resident rows back to host arrays (any pointer may be NULL): fills the host
 * view of pt.shared_arrays['a'|'b'|'w'] after device-side assembly, and serves
 * Calculator.extras' Descriptors.npy / Truth-Ref.npy / Weights.npy dumps
 * (calculator.py:329-348). */
int fsnap_download_rows(fsnap_ctx* ctx, double* A, int64_t lda, double* b, double* w);

/* Row weights w[m] and training mask[m] (1 = train; NULL = all rows train) from host
 * memory.  pt.shared_arrays['w'].array and `training = [not elem for elem in
 * fitsnap_dict['Testing']]` (svd.py:35-44, ridge.py:28-37, ard.py:18-19). */
int fsnap_set_weights(fsnap_ctx* ctx, const double* w, const uint8_t* mask);
/* (fsnap_set_weights* copy the host arrays into page-locked staging before returning -- the caller may reuse them at
 * once -- and hand the DMA to the context's stream without waiting for it.) */

/* Re-weighting form of the reference's explicit-array call (svd.py:46, ridge.py:39: `w` multiplies `a[training]`
 * without being masked, i.e. the caller hands ONE WEIGHT PER TRAINING ROW): w_train[ntrain] in row order.  mask[m]
 * (1 = train) and rank[m] (rank[i] = number of training rows before row i) are host arrays, or both NULL to keep
 * the mask of the previous call (the genetic-algorithm loop of examples/library/genetic_algorithm/libmod_optimize.py:
 * 461-488 re-weights the same training set hundreds of times).  The per-row weights are expanded on the GPU. */
int fsnap_set_weights_train(fsnap_ctx* ctx, const double* w_train, int64_t ntrain, const uint8_t* mask, const int32_t* rank);

/* Same with device pointers (not copied, not owned). */
int fsnap_bind_weights(fsnap_ctx* ctx, const double* dw, const uint8_t* dmask);

/* ---- hot path --------------------------------------------------------------------- */

/* Fused mask x weight x normal equations on the resident rows:
 *   aw = w[:,None]*A[training]; bw = w*b[training]          (svd.py:44-46, ridge.py:37-39)
 *   G = aw.T @ aw; c = aw.T @ bw                            (svd.py:50-51, ridge.py:42-43,
 *                                                            regressor.py:11-12,
 *                                                            transpose_trick/example.py:234-240)
 * without materialising aw.  Outputs (host, any may be NULL): G[K*K], c[K],
 * scalars[3] = { bw.bw, sum(bw), n_train }.  Synchronous. */
int fsnap_normal_eq(fsnap_ctx* ctx, double* G, double* c, double* scalars);

/* Asynchronous form: launches on the context's stream and leaves the packed statistics
 * (FSNAP_PACKED_LEN(K) doubles) in DEVICE memory at d_packed — the buffer the host
 * layer all-reduces with RCCL (the reference's comm.Allreduce of c and d,
 * examples/library/transpose_trick/example.py:245-246). */
int fsnap_normal_eq_async(fsnap_ctx* ctx, double* d_packed);

/* Streaming form: d_packed (device, FSNAP_PACKED_LEN(K) doubles, zeroed by the caller before the first batch)
 * += statistics of the resident rows.  The reference's per-configuration accumulation `c += cm; d += dm`
 * (examples/library/transpose_trick/example.py:230-237): batches of rows are uploaded (or assembled), accumulated
 * and dropped, so A never has to be resident as a whole.  Asynchronous. */
int fsnap_normal_eq_accumulate(fsnap_ctx* ctx, double* d_packed);

/* The same loop with the assembly fused in -- `a, b, w = process_single(configuration)`, `c += aw.T @ aw`,
 * `d += aw.T @ bw` of examples/library/transpose_trick/example.py:230-237 in ONE pass: the rows of the batch are formed
 * in registers from the raw LAMMPS arrays (the transform of fsnap_assemble: lammps_snap.py:391-556, lammps_pace.py:
 * 369-509), weighted and fed to the matrix pipe; A is never written to (or read from) device memory, the context needs
 * no resident rows and the ones it holds are left alone.  Arguments as fsnap_assemble (no row0: nothing is stored);
 * every row of the batch is a training row with weight[r] (rows of kind 3 carry weight 0, as there).
 * d_packed (device, FSNAP_PACKED_LEN(K) doubles, K = ntypes * (ncoeff + offcol), zeroed by the caller before the
 * first batch) += [G | c | b.W^2.b, sum(w b), rows].  Bit-identical to fsnap_assemble into resident rows followed by
 * fsnap_normal_eq_accumulate with the tiled kernel (option "tiled" = 1; the default for K > 128).  Synchronous (the
 * host arrays may be reused on return). */
int fsnap_assemble_accumulate(fsnap_ctx* ctx, const double* raw, int64_t raw_rows, int64_t raw_ld, int64_t nrows,
                              const int64_t* src_row, const int32_t* kind, const int32_t* frac, const double* d,
                              const double* truth, const double* weight, const double* fractions, int64_t nfrac,
                              const double* blank2J, int32_t ntypes, int32_t ncoeff, int32_t offcol, double* d_packed);

/* Same as fsnap_normal_eq_async into a context-owned device buffer whose address is
 * returned in *d_packed (valid until the next call on this context); asynchronous.
 * For K <= 128 the reduction kernel also writes the statistics into a page-locked host mirror
 * which fsnap_solve_device uses instead of a D2H copy when it is
 * handed this same pointer: read-only for the caller -- to modify the buffer (e.g. all-reduce it)
 * use fsnap_normal_eq_async with a buffer of your own. */
int fsnap_normal_eq_resident(fsnap_ctx* ctx, double** d_packed);

/* Mirror packed statistics that live in device memory (e.g. the buffer a RCCL all-reduce just summed over the ranks,
 * the reference's comm.Allreduce(c), comm.Allreduce(d) in examples/library/transpose_trick/example.py:245-246) into
 * the context's page-locked host mirror; asynchronous (a small copy kernel + an event on the context's stream).  A
 * following fsnap_solve_device on the same pointer then needs no D2H copy.  No-op for K >= 232 (those are factorised
 * on the GPU).  The caller must not modify the buffer between this call and the solve. */
int fsnap_mirror_packed(fsnap_ctx* ctx, const double* d_packed, int64_t K);

/* Copy packed statistics from device memory to host arrays (any may be NULL); synchronous. */
int fsnap_download_packed(fsnap_ctx* ctx, const double* d_packed, int64_t K, double* G, double* c, double* scalars);

/* Stand-alone wavefront row weighting: aw = w[:,None]*A, bw = w*b for ALL m rows
 * (masked rows are written as zeros); host outputs, leading dimension ldaw.
 * svd.py:46 / ridge.py:39 / solver.py:75 for callers that need aw, bw themselves. */
int fsnap_weight_rows(fsnap_ctx* ctx, double* aw, int64_t ldaw, double* bw);

/* Same with device outputs, asynchronous on the context's stream. */
int fsnap_weight_rows_device(fsnap_ctx* ctx, double* d_aw, int64_t ldaw, double* d_bw);

/* preds = A @ beta (solver.py:377) for all m rows; host in/out.  preds may be NULL.
 * If sse is not NULL it receives sum over training rows of (w*(b - A beta))^2 using
 * the current weights (sklearn ARDRegression's per-iteration `rmse_`). */
int fsnap_predict(fsnap_ctx* ctx, const double* beta, double* preds, double* sse);

/* Right-hand side of one step of iterative refinement of the least-squares solution:
 *   s[K] = (wA)^T (wb - wA beta)   over the training rows, with the current weights / mask
 * (two streaming passes over the resident A).  Solving G delta = s and setting beta += delta
 * ("corrected semi-normal equations") brings the normal-equation error (~kappa^2 eps) back
 * to ~kappa eps, i.e. to what the reference's lstsq on A_w delivers (svd.py:54).
 * beta, s: host; *sse (optional) receives sum (w (b - A beta))^2. */
int fsnap_residual_rhs(fsnap_ctx* ctx, const double* beta, double* s, double* sse);

/* Model-error (MERR) log-posterior of the resident training rows and its exact gradient, one pass over A
 * (fitsnap3lib/solvers/lreg.py logpost_emb; kernel M1, or kernels M2 + M3 above 288 columns).  With x_i = w_i a_i,
 * e_i = x_i . c - w_i b_i and v_i = sum_j x_ij^2 q_j + d over the rows of the current mask (weight zero included):
 *   *val = sum_i l(e_i, v_i),  g[K] = sum_i dl/de x_i,  h[K] = sum_i dl/dv x_i o x_i
 * with  iid / full: l = -e^2 / (2 v) - log(v) / 2;  abc: l = -(|e| - sqrt(v))^2 / (2 0.01).  The constants of the density
 * (-n log(2 pi) / 2, or -log(2 pi) / 2 - log(0.1) once for abc) are the caller's, so that the sums of several ranks add.
 * method: FSNAP_MERR_*; K must equal the resident rows' width; c, q (q_j = sigma_j^2, 0 outside the embedded columns):
 * host in; val, g, h: host out.  The workspace stays on the context.  Bit-identical run to run. */
#define FSNAP_MERR_IID 0
#define FSNAP_MERR_ABC 1
#define FSNAP_MERR_FULL 2
int fsnap_merr_eval(fsnap_ctx* ctx, int method, int64_t K, const double* c, const double* q, double d, double* val,
                    double* g, double* h);

/* Weighted residual sums of P coefficient vectors over the resident training rows, one pass over A (the log-posterior of
 * the MCMC solver, fitsnap3lib/solvers/mcmc.py logpost, for a batch of proposals; kernels S1 / S1G of csrc/fsnap_mcmc.hip,
 * fp64 MFMA).  U: host, P x K row-major, 1 <= P <= 16.  Over the rows of the current mask (weight zero included):
 *   sse[p] = sum_i (w_i (a_i . u_p - b_i))^2,   *n_train = number of rows in the mask   (n_train may be NULL)
 * K must equal the resident rows' width, else FSNAP_E_ARG; P outside 1 ... 16: FSNAP_E_ARG.  With no rows (m = 0) the
 * sums and the count are zero.  sse[p] depends only on u_p and the rows: bit-identical in any slot, for any P, whatever
 * the other vectors, and run to run.  Test rows are dropped by selects (NaN / Inf in them reach nothing).  No atomics.
 * The rows, weights and any category layout are left as they are.  Host in and out, synchronous. */
int fsnap_sse_batch(fsnap_ctx* ctx, int64_t K, const double* U, int P, double* sse, int64_t* n_train);

/* Predictive variance of the resident rows under a posterior covariance (Solver._compute_stdev, solver.py:440-472; the
 * ranking pass of the Bayesian active-learning loop, bayesian_active_learning.py:826-828), one pass over the rows (kernels
 * U1 / U1G of csrc/fsnap_uq.hip, fp64 MFMA).  M (host, K x J row-major) is copied to the device on every call; per row a_i:
 *   mode FSNAP_UQ_QUAD (J = K):  var_i = a_i^T M a_i           (fullcov / loop with M = cov)
 *   mode FSNAP_UQ_NORM (J >= 1): var_i = ||a_i M||^2            (chol / choleye / svd with M = L, shifted L, U sqrt(S);
 *                                                               sam with M = centred samples^T / sqrt(nsam))
 * preds_i = a_i . beta from the same read (beta: host, K; needed only for preds).  var is NOT scaled.  With cat[m] (host,
 * int32, id in [0, ncat), negative = the row takes no part; rows of a category need not be adjacent) kernels U2 + U3 give
 * cat_sum[c] = sum of scale_i var_i over the rows of category c in stable-sorted row order (fsnap_cat_chunks), cat_max[c]
 * their max and cat_count[c] their number (scale: m doubles, NULL = 1; an empty category: sum 0, max -inf, count 0).
 * Every output may be NULL; category outputs need cat.  K must equal the resident rows' width, J = K in QUAD mode, every
 * id must be < ncat: else FSNAP_E_ARG.  m = 0 is a no-op (category outputs are those of empty categories).  A row's result
 * depends only on a_i, M, beta (and s_i): bit-identical run to run and under any row subset, order, m or lda.  No atomics.
 * Host in and out, synchronous. */
#define FSNAP_UQ_QUAD 0
#define FSNAP_UQ_NORM 1
int fsnap_row_variance(fsnap_ctx* ctx, int mode, int64_t K, int64_t J, const double* M, const double* beta, const double* scale,
                       const int32_t* cat, int ncat, double* var, double* preds, double* cat_sum, double* cat_max,
                       int64_t* cat_count);

/* Same with device outputs (d_var, d_preds: m doubles; d_cat_sum, d_cat_max: ncat doubles; d_cat_count: ncat int64) and a
 * device d_scale, queued on the context's stream; M, beta and cat stay host arrays.  Returns once the work is queued. */
int fsnap_row_variance_device(fsnap_ctx* ctx, int mode, int64_t K, int64_t J, const double* M, const double* beta,
                              const double* d_scale, const int32_t* cat, int ncat, double* d_var, double* d_preds,
                              double* d_cat_sum, double* d_cat_max, int64_t* d_cat_count);

/* Greedy batch selection for active learning on the resident rows (kernels B1 ... B4 of csrc/fsnap_select.hip; the host
 * algebra is solvers/select.py).  A session keeps var_i = a_i^T C_t a_i of every row, and per category c the sum / max /
 * count of scale_i var_i, on the context; picking a unit changes the posterior to C_t - V V^T, which costs one pass over
 * the rows, and nothing but one (category, score) pair per pick comes back to the host.
 *   fsnap_select_begin     mode, K, J, M, scale, cat, ncat as in fsnap_row_variance (cat is required, ncat >= 1): the initial
 *                          variances and category sums ARE those of fsnap_row_variance (same kernels, same bits), left on the
 *                          device.  objective: the score of a category, FSNAP_SELECT_SUM (cat_sum), _MAX (cat_max) or _MEAN
 *                          (cat_sum / cat_count).  Every category with at least one row starts alive.  A running session is
 *                          replaced.
 *   fsnap_select_pick      *category = the live category of the largest score (ties: the lowest id; a NaN score ranks
 *                          lowest), *score = its score; -1 (score 0) when no category is alive.  The arg-max runs on the
 *                          device.  retire != 0 takes the winner out of the session (it is never returned again);
 *                          retire = 0 only looks (several ranks: the ranks compare their winners first).
 *   fsnap_select_retire    takes a live category out of the session (FSNAP_E_ARG when it is not alive).
 *   fsnap_select_downdate  V (host, K x J row-major, any J >= 1; copied padded to 16-multiples): var_i <- var_i - ||a_i V||^2
 *                          for every row (kernel B1, fp64 MFMA, K <= 144; B1G, untuned, beyond), then the sums / maxima of
 *                          the live categories again (retired categories keep the values they were retired with).  The
 *                          subtracted value has the bits of fsnap_row_variance(FSNAP_UQ_NORM, V); a row's new variance
 *                          depends on a_i, its old variance and V alone: bit-identical run to run and under any row
 *                          subset, order, m or lda; category sums in stable-sorted row order.  No atomics.
 *   fsnap_select_state     downloads var (m doubles), cat_sum, cat_max (ncat doubles), cat_count (ncat int64) and alive
 *                          (ncat int32, 1 / 0); every output may be NULL.
 *   fsnap_select_end       drops the session.
 * Anything that replaces the resident rows or prepares a category layout (fsnap_upload_rows, fsnap_bind_rows,
 * fsnap_rows_alloc, fsnap_drop_rows, fsnap_assemble, fsnap_cat_prepare) ends the session: pick, retire, downdate and state
 * then return FSNAP_E_ARG, as they do without a session.  fsnap_row_variance and the fits leave it alone.  With no rows
 * (m = 0) a session has no live category.  Host in and out, synchronous. */
#define FSNAP_SELECT_SUM 0
#define FSNAP_SELECT_MAX 1
#define FSNAP_SELECT_MEAN 2
int fsnap_select_begin(fsnap_ctx* ctx, int mode, int64_t K, int64_t J, const double* M, const double* scale, const int32_t* cat,
                       int ncat, int objective);
int fsnap_select_pick(fsnap_ctx* ctx, int retire, int32_t* category, double* score);
int fsnap_select_retire(fsnap_ctx* ctx, int32_t category);
int fsnap_select_downdate(fsnap_ctx* ctx, int64_t K, int64_t J, const double* V);
int fsnap_select_state(fsnap_ctx* ctx, double* var, double* cat_sum, double* cat_max, int64_t* cat_count, int32_t* alive);
int fsnap_select_end(fsnap_ctx* ctx);

/* Exact leave-one-configuration-out (LOCO) predictions of a linear smoother from the resident training rows (kernels L1, L2 of
 * csrc/fsnap_loco.hip, fp64 MFMA; no refit).  M (host, K x J row-major) is any factor of C = (G + alpha I)^-1 = M M^T of the
 * fit (RIDGE: its alpha; ANL: pinv with cov_nugget; SVD: alpha = 0, or V_r Lambda_r^-1/2 of the kept directions), beta
 * (host, K) the fit.  sorted_rows[cfg_offsets[ncfg]] (host, int32) lists the rows of configuration c at positions
 * cfg_offsets[c] ... cfg_offsets[c + 1] - 1 (host, int64, cfg_offsets[0] = 0, non-decreasing; every row at most once).
 * With zeta_i = a_i M, z_i = w_i zeta_i, e_i = w_i b_i - w_i (a_i . beta) (w_i = 0 off the mask) and S_c = Z_c^T Z_c:
 *     v_c = (I_J - S_c)^-1 Z_c^T e_c  (solved in J space, or in n space as Z_c^T (I_n - Z_c Z_c^T)^-1 e_c when n_c <= J)
 *     pred_out[i] = a_i . beta - zeta_i . v_c = a_i . beta_{-c}     for every row i of c
 * pred_out: m doubles (NaN for rows that are not listed, and for every row of a configuration that is not identifiable);
 * cfg_info_out: ncfg x 4 doubles (d_c = min(n_c, J), smallest Cholesky pivot of I - S_c, identifiable 1 / 0, n space 1 / 0).
 * A configuration is not identifiable when a pivot is <= 1e-10 (lambda_max(S_c) -> 1; it is never divided through).
 * d_c <= 128 is solved in LDS, larger d_c through global scratch.  K must equal the resident rows' width.  A row's result is
 * bit-identical run to run and under any permutation of the configurations; no atomics.  Host in and out, synchronous. */
int fsnap_loco_rows(fsnap_ctx* ctx, int64_t K, int64_t J, const double* M, const double* beta, const int32_t* sorted_rows,
                    const int64_t* cfg_offsets, int64_t ncfg, double* pred_out, double* cfg_info_out);

/* Leave-one-configuration-out predictive variances next to the predictions (kernel L1 of csrc/fsnap_loco.hip, kernel L3 of
 * csrc/fsnap_loco_uq.hip, fp64 MFMA; no refit).  Arguments, checks and error codes are those of fsnap_loco_rows, and pred_out
 * is what fsnap_loco_rows writes for the same inputs, bit for bit.  With H_c = I - Z_c Z_c^T (n space, n_c <= J) or
 * I - Z_c^T Z_c (J space) = L L^T, the matrix whose inverse is the predictive covariance of the configuration's weighted
 * rows under the fit without c, in units of the noise:
 *     lev_out[i] = q_i = a_i (G - X_c^T X_c + alpha I)^-1 a_i^T      for every row i of c (also where w_i = 0)
 *                = |L^-1 zeta_i^T|^2  (J space)  =  |zeta_i|^2 + |L^-1 Z_c zeta_i^T|^2  (n space)
 *     Var(w_i b_i - w_i pred_i) = sigma^2 (1 + w_i^2 q_i)            with sigma^2 the noise variance of a unit-weight row
 * lev_out: m doubles (NaN for rows that are not listed, and for every row of a configuration that is not identifiable);
 * cfg_info_out: ncfg x 6 doubles (d_c = min(n_c, J), smallest Cholesky pivot, identifiable 1 / 0, n space 1 / 0,
 * l_c = log det H_c = 2 sum log L_kk, D_c = e_c^T H_c^-1 e_c; l_c and D_c are NaN for a configuration that is not
 * identifiable; a configuration without rows gets (0, inf, 1, 1, 0, 0)).  The joint log density of the configuration's
 * weighted targets is -1/2 [n' log(2 pi sigma^2) - l_c + D_c / sigma^2], n' the rows with w_i > 0.  Every sum runs in an order
 * that depends on the configuration's own rows alone: bit-identical run to run and under any permutation or subset of the
 * configurations; no atomics.  Host in and out, synchronous. */
int fsnap_loco_rows_uq(fsnap_ctx* ctx, int64_t K, int64_t J, const double* M, const double* beta, const int32_t* sorted_rows,
                       const int64_t* cfg_offsets, int64_t ncfg, double* pred_out, double* lev_out, double* cfg_info_out);

/* Per-configuration influence on the coefficients and the outer-product sums of the cluster-robust coefficient covariances
 * (kernel L1 of csrc/fsnap_loco.hip, kernels I0 / I1 / I2 of csrc/fsnap_influence.hip, fp64 MFMA; no refit).  M, beta,
 * sorted_rows, cfg_offsets, ncfg, their checks and error codes are those of fsnap_loco_rows.  With its notation, per
 * configuration c:
 *     s_c = Z_c^T e_c                         (J)  the score of the configuration in M space; needs no solve
 *     v_c = (I_J - S_c)^-1 s_c                (J)  fsnap_loco_rows' v: the refit without c is beta_{-c} = beta - M v_c
 *     W_s = sum_c s_c s_c^T,   W_v = sum_{c identifiable} v_c v_c^T        (J x J)
 * so that M W_s M^T is the cluster-robust (CR0) covariance of beta and (U' - 1) / U' M W_v M^T its delete-one-configuration
 * jackknife (CR3), U' the identifiable configurations.
 * mode FSNAP_INFL_FULL (kernels L1, I1, I2): pred_out (m doubles, may be NULL) and cfg_info_out (ncfg x 4) are what
 * fsnap_loco_rows writes for the same inputs, bit for bit; V_out (ncfg x J, may be NULL): v_c, zeros for a configuration that
 * is not identifiable; S_out (ncfg x J, may be NULL): s_c, always; unit_out (ncfg x 3): (|v_c|^2, |s_c|^2, s_c . v_c), the
 * first and third NaN for a configuration that is not identifiable; Ws_out, Wv_out (J x J each, may be NULL).
 * mode FSNAP_INFL_SCORES (kernels L1, I0, I2; no factorisation): S_out, Ws_out as above; cfg_info_out = (d_c, inf, 1, n space)
 * and unit_out = (NaN, |s_c|^2, NaN); V_out, Wv_out or pred_out given return FSNAP_E_ARG, as an unknown mode does.
 * S_out, |s_c|^2 and Ws_out are the same bits in both modes: one loop over the configuration's rows forms s_c everywhere.
 * A configuration without rows gets s = v = 0, info (0, inf, 1, 1) and unit_out zeros; ncfg = 0 or no resident rows give
 * zero matrices and write nothing else.  The per-configuration outputs depend on the configuration's own rows alone:
 * bit-identical run to run and under any permutation or subset of the configurations.  W_s and W_v add the configurations in
 * index order, 4 per MFMA step in chunks of 512 whose partial sums are added in chunk order: bit-identical run to run, but
 * NOT invariant under a permutation of the configurations.  No atomics.  Touches no resident rows, weights or sessions.
 * Host in and out, synchronous. */
#define FSNAP_INFL_SCORES 0   /* s_c, W_s only: kernels L1, I0, I2 */
#define FSNAP_INFL_FULL 1     /* + v_c, W_v, pred: kernels L1, I1, I2 */
int fsnap_influence_rows(fsnap_ctx* ctx, int mode, int64_t K, int64_t J, const double* M, const double* beta,
                         const int32_t* sorted_rows, const int64_t* cfg_offsets, int64_t ncfg, double* pred_out,
                         double* cfg_info_out, double* unit_out, double* S_out, double* V_out, double* Ws_out, double* Wv_out);

/* Exact leave-one-unit-out errors of ridge fits over a grid of alphas from the resident training rows (kernel P1 of
 * csrc/fsnap_path.hip, fp64 MFMA; K <= 144).  G (host, K x K row-major; the lower triangle is read) and c (host, K) are the
 * statistics of the weighted rows x_i = w_i a_i, y_i = w_i b_i (w_i = 0 off the mask), alphas (host, Q doubles, finite, >= 0)
 * the grid.  sorted_rows[unit_offsets[nunits]] (host, int32) lists the rows of unit u at positions unit_offsets[u] ...
 * unit_offsets[u + 1] - 1 (host, int64, unit_offsets[0] = 0, non-decreasing; every row at most once); row_class (host, m bytes
 * by row) the class < nclass <= 8 of every listed row.  For every unit and alpha_q the REFIT without the unit's rows:
 *     B = G - X_u^T X_u + alpha_q I,  D = sqrt(diag B),  beta = D^-1 (D^-1 B D^-1)^-1 D^-1 (c - X_u^T y_u)   (blocked Cholesky)
 *     p_i = a_i . beta,  r_i = b_i - p_i     for every row i of u
 * sums_out: Q x nunits x nclass x 4 doubles (n, sum |r|, sum r^2, sum (w r)^2 over the unit's rows of the class, in position
 * order); info_out: Q x nunits x 2 doubles (smallest pivot of the scaled matrix, identifiable 1 / 0); pred_out (may be NULL):
 * Q x m doubles, NaN for rows that are not listed.  A unit is not identifiable at alpha_q when a diagonal entry of B is <= 0
 * (in floating point: <= 1e-10 (G_jj + alpha_q), the downdate has cancelled) or a pivot is <= 1e-10 (it is never divided
 * through): its predictions are NaN and its sums zero.  A unit without rows has zero sums and info (inf, 1).  Uses the resident rows, b and weights.  FSNAP_E_ARG for K != the resident width, K > 144,
 * Q < 1, a negative or non-finite alpha, nclass outside 1 ... 8, a class >= nclass.  Every sum runs in a fixed order that
 * depends on the unit's own rows only: bit-identical run to run and under any permutation of the units; no atomics.  Host in
 * and out, synchronous. */
int fsnap_ridge_path(fsnap_ctx* ctx, int64_t K, const double* G, const double* c, const double* alphas, int64_t Q,
                     const int32_t* sorted_rows, const int64_t* unit_offsets, int64_t nunits, const uint8_t* row_class,
                     int64_t nclass, double* sums_out, double* info_out, double* pred_out);

/* Grouped K-fold LASSO alpha paths on per-fold statistics (kernels S1, S2 of csrc/fsnap_lasso.hip; what LassoCV with a
 * GroupKFold is to Lasso; the folds, routes and tables are solvers/lasso_path.py).  d_stats (DEVICE) holds F * nsub packed
 * blocks of FSNAP_PACKED_LEN(K) doubles as fsnap_cat_normal_eq / fsnap_cat_normal_eq_dist leave them; fold f is the sum of the
 * blocks f * nsub ... f * nsub + nsub - 1 and the total T the sum of the folds, both added in index order.  Problem (f, q),
 * f < F: the refit without fold f; f = F: the fit on all training rows:
 *     Qm = T.G - G_f,  qv = T.c - c_f,  y2 = T.bb - bb_f,  n = T.n - n_f,  l1_reg = alphas[q] * n       (f = F: T alone)
 * solved as fsnap_lasso_gram solves it, statement for statement, from zeros (every problem starts cold; the sums of the duality
 * gap alone run in another order).  Coordinate j is dead -- skipped, coefficient 0, q_j taken as 0 -- when T.G_jj == 0 or
 * Qm_jj <= 1e-10 T.G_jj (the fold alone touched the column and the subtraction left noise); a problem without a live
 * coordinate (an empty training set) ends after its first sweep.  Outputs (host):
 * coef_out[(F + 1)][Q][K]; info_out[(F + 1)][Q][4] = sweeps run, the last duality gap, l1_reg, n; heldout_out[F][Q][3] = n_f,
 * bb_f - 2 beta . c_f + beta^T G_f beta (the weighted squared error of fold f under its own refit), bb_f.  FSNAP_E_ARG for K
 * outside 1 ... 144, F < 1, nsub < 1, Q < 1, max_iter < 1, a negative or non-finite alpha or tol, a NULL pointer, or F * nsub
 * blocks past FSNAP_CAT_STATS_MAX_BYTES.  No atomics; a problem's result depends on its own (fold, alpha) only: bit-identical
 * run to run and under any permutation or subset of the grid.  The resident rows, weights, mask and category layout are not
 * touched.  Synchronous. */
int fsnap_lasso_path(fsnap_ctx* ctx, int64_t K, int64_t F, int64_t nsub, const double* d_stats, const double* alphas, int64_t Q,
                     int64_t max_iter, double tol, double* coef_out, double* info_out, double* heldout_out);

/* Grouped K-fold ARD threshold paths on per-fold statistics (kernel S1 of csrc/fsnap_lasso.hip, A1 of csrc/fsnap_ard.hip;
 * the grid, the hyper-parameters, the host route and the picks are solvers/ard_path.py).  d_stats (DEVICE), the folds and the
 * total T as for fsnap_lasso_path.  Problem (f, q), f < F: the refit without fold f; f = F: the fit on all training rows:
 *     Qm = T.G - G_f,  qv = T.c - c_f,  y2 = T.bb - bb_f,  n = T.n - n_f                                 (f = F: T alone)
 *     hyper[f][q] = (alpha_1, alpha_2, lambda_1, lambda_2, threshold_lambda, alpha_init)              (host, (F + 1) x Q x 6)
 * Column j is dead -- never kept, coefficient 0 -- when T.G_jj == 0 or Qm_jj <= 1e-10 T.G_jj; d_j = sqrt(Qm_jj) (1 for a dead
 * column).  The iteration is scikit-learn's ARDRegression.fit on the statistics (solvers/ard.py, ARD._ard_loop), from coef = 0,
 * lambda = 1, keep = the live columns, alpha_ = alpha_init; per iteration Sigma = D^-1 W^-1 D^-1 with W = diag(lambda_k / d_k^2)
 * + alpha_ Qm[keep, keep] / (d d^T) = L L^T (a Cholesky factor, inverted in place), coef[keep] = alpha_ Sigma qv[keep], sse =
 * max(y2 - 2 coef . qv + coef^T Qm coef, 0), gamma = 1 - lambda_k Sigma_kk, lambda_k = (gamma + 2 lambda_1) / (coef_k^2 + 2
 * lambda_2), alpha_ = (n - sum gamma + 2 alpha_1) / (sse + 2 alpha_2), keep = lambda < threshold_lambda with the pruned
 * coefficients zeroed; it stops after the second or a later iteration when sum |coef_old - coef| < tol, when keep is empty, or
 * at max_iter, and recomputes Sigma and coef once more when keep is not empty.  A problem without a live column runs no
 * iteration.  A pivot that is not positive or a lambda or alpha_ that is not finite ends the problem with status 1 and NaN
 * coefficients and lambdas; the call still returns FSNAP_OK.  Outputs (host): coef_out, lambda_out[(F + 1)][Q][K];
 * info_out[(F + 1)][Q][6] = iterations, kept columns, final alpha_, the last sum |coef_old - coef| (against zeros in the first
 * iteration; inf before any), the smallest pivot of W over all iterations (inf before any), status (0 converged or emptied,
 * 1 failed, 2 max_iter reached); heldout_out[F][Q][3] = n_f, bb_f - 2 beta . c_f + beta^T G_f beta (the weighted squared error
 * of fold f under its own refit), bb_f.  FSNAP_E_ARG for K outside 1 ... 144, F < 1, nsub < 1, Q < 1, max_iter < 1, a negative
 * or non-finite tol or hyper entry, threshold_lambda <= 0, alpha_init <= 0, a NULL pointer, or F * nsub blocks past
 * FSNAP_CAT_STATS_MAX_BYTES.  fp64, no atomics; every sum runs in an order that depends on the problem alone: bit-identical run
 * to run and under any permutation or subset of the grid.  The resident rows, weights, mask and category layout are not
 * touched.  Synchronous. */
int fsnap_ard_path(fsnap_ctx* ctx, int64_t K, int64_t F, int64_t nsub, const double* d_stats, const double* hyper, int64_t Q,
                   int64_t max_iter, double tol, double* coef_out, double* lambda_out, double* info_out, double* heldout_out);

/* Grouped K-fold greedy forward-selection paths on per-fold statistics (kernel S1 of csrc/fsnap_lasso.hip, O1 of
 * csrc/fsnap_omp.hip; the folds, the host route, the picks and the tables are solvers/omp_path.py).  d_stats (DEVICE), the folds
 * and the total T as for fsnap_lasso_path.  Problem f < F: the refit without fold f; f = F: the fit on all training rows:
 *     Qm = T.G - G_f,  qv = T.c - c_f,  y2 = T.bb - bb_f                                                 (f = F: T alone)
 * run through fsnap_omp_gram's recurrence (below) with diag_ref = T.G_jj for S steps: a Cholesky factorisation of Qm whose pivot
 * is chosen by `criterion` (FSNAP_OMP_OMP / FSNAP_OMP_OLS) after the `forced` columns (host, nforced >= 0 indices in order;
 * may be NULL when nforced = 0), with the right-hand side carried along.  levels (host): Q sparsity levels in ascending order,
 * each in 1 ... S; the coefficients are returned at those only.  Outputs (host): order_out[(F + 1)][S] = the column chosen at
 * step s (-1 once the path has ended); path_out[(F + 1)][S][3] = e_s, the score and the pivot t_j* of the chosen column (the
 * last e_s, 0, 0 once the path has ended); heldout_out[F][S][3] = n_f, h_{f,s} = bb_f - 2 beta . c_f + beta^T G_f beta (the
 * weighted squared error of fold f under its own refit after s steps; the last one once the path has ended, bb_f when it took
 * no step), bb_f; coef_out[(F + 1)][Q][K] = the unshrunk least-squares coefficients on the support after levels[q] steps (the
 * last support's once the path has ended), zero elsewhere.  FSNAP_E_ARG for K outside 1 ... 144, S < 1, S > min(K, 128), F < 1,
 * nsub < 1, Q < 1, levels that decrease or leave 1 ... S, a forced index out of range or repeated, nforced < 0, an unknown
 * criterion, a NULL pointer, or F * nsub blocks past FSNAP_CAT_STATS_MAX_BYTES.  fp64, one wave per problem, no atomics; every
 * sum runs in an order that depends on the problem alone and the argmax compares the fp64 scores exactly (lowest index on
 * equality): bit-identical run to run and under any permutation or subset of the folds; order_out, path_out and coef_out carry
 * the bits of fsnap_omp_gram on the same system.  The resident rows, weights, mask and category layout are not touched.
 * Synchronous. */
#define FSNAP_OMP_OMP 0   /* score_j = r_j^2 / Qm_jj: orthogonal matching pursuit on the column-normalised system */
#define FSNAP_OMP_OLS 1   /* score_j = r_j^2 / t_j:   orthogonal least squares (forward stepwise regression)       */
int fsnap_omp_path(fsnap_ctx* ctx, int64_t K, int64_t F, int64_t nsub, const double* d_stats, int criterion,
                   const int32_t* forced, int64_t nforced, int64_t S, const int32_t* levels, int64_t Q, int32_t* order_out,
                   double* path_out, double* heldout_out, double* coef_out);

/* Grouped K-fold BCS sparsity paths on per-fold statistics (kernel S1 of csrc/fsnap_lasso.hip, B1 of csrc/fsnap_bcs.hip; the
 * grid, the host route, the picks and the tables are solvers/bcs_path.py).  d_stats (DEVICE), the folds and the total T as for
 * fsnap_lasso_path.  Problem (f, q), f < F: the refit of setting q without fold f; f = F: on all training rows:
 *     Qm = T.G - G_f,  qv = T.c - c_f,  y2 = T.bb - bb_f,  sum_y = T.sum wb - sum wb_f,  n = T.n - n_f     (f = F: T alone)
 * run through fsnap_bcs_gram's recurrence (below) with diag_ref = T.G_jj, max_active and deletion, and with
 * hyper[q] = (sigma2 or 0, scale, eta, itermax) (host, Q x 4): a setting with sigma2 = 0 takes sigma2 = max(scale (y2 / n -
 * (sum_y / n)^2), 1e-16) from the problem's OWN downdated scalars.  P = the largest itermax of the settings.  Outputs (host):
 * coef_out[(F + 1)][Q][K]; active_out[(F + 1)][Q][max_active] (int32, the active columns in order, then -1), alpha_out and
 * errbar_out[(F + 1)][Q][max_active] by position (0 past the active set); picks_out[(F + 1)][Q][P][2] (int32: column, action;
 * -1 after the end); info_out[(F + 1)][Q][6] as fsnap_bcs_gram's; heldout_out[F][Q][3] = n_f, bb_f - 2 beta . c_f + beta^T G_f
 * beta (the weighted squared error of fold f under its own refit), bb_f; sig_out[Q][max_active][max_active] = Sig of the f = F
 * problems (unclipped, zero past the active set).  A problem that fails has status 1 and NaN coefficients; the call still
 * returns FSNAP_OK.  FSNAP_E_ARG for K outside 1 ... 144, max_active outside 1 ... min(K, 64), F < 1, nsub < 1, Q < 1, an
 * unknown deletion, a NULL pointer, a hyper row with sigma2 < 0, sigma2 = 0 and scale <= 0, eta < 0, an itermax outside
 * 1 ... 65 536 or not an integer, or any entry not finite, or F * nsub blocks past FSNAP_CAT_STATS_MAX_BYTES.  One workgroup of
 * 256 threads per problem (thread j owns column j); fp64 VALU, no atomics; every sum runs in an order that depends on the
 * problem alone and the argmax compares (ml, index) exactly with the lowest index on equality: bit-identical run to run and
 * under any permutation or subset of the grid or the folds.  The device's log differs from the host's in the last bits, so
 * the results are close to fsnap_bcs_gram's, not identical.  The resident rows, weights, mask and category layout are not
 * touched.  Synchronous. */
int fsnap_bcs_path(fsnap_ctx* ctx, int64_t K, int64_t F, int64_t nsub, const double* d_stats, const double* hyper, int64_t Q,
                   int64_t max_active, int deletion, double* coef_out, int32_t* active_out, double* alpha_out,
                   double* errbar_out, int32_t* picks_out, double* info_out, double* heldout_out, double* sig_out);

/* Grouped K-fold spectral paths on per-fold statistics: every ridge penalty alpha and every singular-value cut rcond from ONE
 * symmetric eigendecomposition per fold (kernel S1 of csrc/fsnap_lasso.hip, E1 and E2 of csrc/fsnap_spectral.hip; the host
 * route, the picks and the tables are solvers/spectral_path.py).  d_stats (DEVICE), the folds and the total T as for
 * fsnap_lasso_path.  Problem f < F is the refit without fold f, f = F the fit on all training rows:
 *     Qm = T.G - G_f,  qv = T.c - c_f,  y2 = T.bb - bb_f                                                (f = F: T alone)
 * run through fsnap_spectral_gram's scheme (below) with diag_ref = T.G_jj.  Settings are the product grid of alphas[Qa] and
 * rconds[Qr] (host), q = ia Qr + ir, Q = Qa Qr.  Outputs (host): eig_out[(F + 1)][K] and z_out[(F + 1)][K], ascending, zero
 * past n_live; info_out[(F + 1)][6] = n_live, sweeps, final off / diag ratio sqrt(sum_{i>j} a_ij^2 / sum_i a_ii^2),
 * lambda_max, smallest lambda, status (0 converged, 2 the cap of 60 sweeps reached: not an error); set_out[(F + 1)][Q][3] =
 * rank, dof, sse; fit_out[Q][K], the coefficients of the f = F problems; coef_out[F][Q][K], the coefficients of the refits
 * (may be NULL: needed only for a row pass); heldout_out[F][Q][nsub][3] = n_{f,s}, bb_{f,s} - 2 beta . c_{f,s} + beta^T G_{f,s}
 * beta (the weighted squared error of row class s of fold f under the fold's own refit), bb_{f,s}, against block f nsub + s.
 * FSNAP_E_ARG for K outside 1 ... 144, F < 1, nsub < 1, Qa < 1 or Qr < 1, a negative or non-finite alpha or rcond, a NULL
 * pointer (coef_out may be NULL), F * nsub blocks or the results past FSNAP_CAT_STATS_MAX_BYTES: nothing is launched then.
 * FSNAP_NUM_NONFINITE for a NaN/Inf among the fits.  Kernel E1: one workgroup of 1024 threads per problem, the working matrix
 * as a packed lower triangle in LDS (83.5 KB at K = 144), the eigenvectors in LDS for K <= 113 and in a per-workgroup scratch
 * that stays in L2 beyond -- the device route serves all of K <= 144.  Kernel E2: one workgroup per (problem, 16 settings).
 * fp64 VALU, no atomics; every sum runs in an order that depends on the problem and the setting alone: bit-identical run to
 * run and under any permutation or subset of the grid or of the folds.  Host and kernel run one text (csrc/
 * fsnap_spectral_body.h) with explicit fmas; the held-out sums of the Python host route are numpy's, in another order.  The
 * resident rows, weights, mask and category layout are not touched.  Synchronous. */
int fsnap_spectral_path(fsnap_ctx* ctx, int64_t K, int64_t F, int64_t nsub, const double* d_stats, const double* alphas,
                        int64_t Qa, const double* rconds, int64_t Qr, double* eig_out, double* z_out, double* info_out,
                        double* set_out, double* fit_out, double* coef_out, double* heldout_out);

/* ms_out[2] = the times of kernel E1 (eigendecompositions) and kernel E2 (settings) of the context's last successful
 * fsnap_spectral_path call, between HIP events on its stream.  FSNAP_E_STATE without such a call. */
int fsnap_spectral_path_times(fsnap_ctx* ctx, double* ms_out);

/* Joint scores of units (normally configurations) of the resident rows for active learning (kernels J1, J2 of
 * csrc/fsnap_joint.hip, fp64 MFMA; the host algebra is solvers/select_joint.py).  With the posterior C = M M^T (M: K x J),
 * the noise variance tau of a unit-weight row, the weighted rows X_u = diag(omega) A_u (n_u x K) of unit u, Z = X_u M and a
 * target T = R^T R given as B = M^T R^T (J x r):
 *     S = I + Z Z^T / tau (n_u <= J, "n space")  or  I + Z^T Z / tau (n_u > J, "J space")  = L L^T
 *     gain_u      = 1/2 logdet(I + X_u C X_u^T / tau) = sum log L_ii           (the information the unit's labels carry)
 *     reduction_u = tr(T C) - tr(T C'_u) = ||L^-1 Z B||_F^2 / tau  (n space)  =  ||B||_F^2 - ||L^-1 B||_F^2  (J space)
 * (C'_u: the posterior with the unit added; no labels, no refit).  A session, like fsnap_select_*:
 *   fsnap_joint_begin    sorted_rows[unit_offsets[nunits]] (host, int32) lists the rows of unit u at positions
 *                        unit_offsets[u] ... unit_offsets[u + 1] - 1 (host, int64, unit_offsets[0] = 0, non-decreasing; every
 *                        row at most once); omega (host, m doubles by row, NULL = 1) the weight of every row.  All of it is
 *                        uploaded once; nothing of size O(m) crosses the bus afterwards.  Every unit with at least one row
 *                        starts alive.  A running session is replaced.
 *   fsnap_joint_score    M (host, K x J row-major), B (host, J x r row-major; NULL / r = 0: no target), tau > 0.  gain,
 *                        reduction (host, nunits doubles; either may be NULL, reduction needs B): the scores of the live
 *                        units, NaN for the others.  info (host, nunits x 4 doubles, may be NULL): dim S = min(n_u, J),
 *                        n space 1 / 0, the smallest Cholesky pivot of S (>= 1 in exact arithmetic), n_u; written for live
 *                        units only.  dim S <= 128 is factorised in LDS, larger ones through global scratch (untuned).
 *   fsnap_joint_retire   takes a live unit out of the session (FSNAP_E_ARG when it is not alive).
 *   fsnap_joint_end      drops the session.
 * Whatever ends a selection session (fsnap_upload_rows, fsnap_bind_rows, fsnap_rows_alloc, fsnap_drop_rows, fsnap_assemble,
 * fsnap_cat_prepare) ends this one: score and retire then return FSNAP_E_ARG, as they do without a session.  K must equal
 * the resident rows' width.  With no rows (m = 0) or no live unit, score writes NaN and does nothing else.  Every sum runs in
 * a fixed order that depends on the unit's own rows only: a unit's scores are bit-identical run to run and under any
 * permutation or subset of the units.  No atomics.  Host in and out, synchronous. */
int fsnap_joint_begin(fsnap_ctx* ctx, const int32_t* sorted_rows, const int64_t* unit_offsets, int64_t nunits,
                      const double* omega);
int fsnap_joint_score(fsnap_ctx* ctx, int64_t K, int64_t J, const double* M, int64_t r, const double* B, double tau,
                      double* gain, double* reduction, double* info);
int fsnap_joint_retire(fsnap_ctx* ctx, int64_t unit);
int fsnap_joint_end(fsnap_ctx* ctx);

/* The step between two fits of a robust M-estimator by iteratively re-weighted least squares (kernels R0 - R3 of
 * csrc/fsnap_robust.hip; the loop is solvers/robust.py).  Participating rows are the training rows with w_i > 0 of the
 * weights and mask the context holds at begin (the BASE weights); no other row reaches a sum, a median or a count.
 * A session, like fsnap_select_*:
 *   fsnap_robust_begin      cat (host, m int32 in [0, ncat), NULL = one class) is uploaded once, the session's vectors
 *                           (e, r, w r: m doubles each) are allocated and the context's weights and mask remembered.
 *                           1 <= ncat <= FSNAP_ROBUST_MAX_CLASSES.  In a communicator a rank without rows opens a session
 *                           of zero rows; without one, no rows is FSNAP_E_STATE.  A running session is ended first.
 *   fsnap_robust_residuals  e_i = w_i (b_i - a_i . beta) with the base weights, one pass over A; stays on the device.
 *   fsnap_robust_scale      s_g = 1.4826 median{|e_i| : class g} by radix selection on the bit pattern of |e| (eight digit
 *                           passes, no host synchronisation between them; both middle order statistics, (lo + hi) * 0.5 for
 *                           an even count; 0 for an empty class).  Collective in a communicator: the digit tables are summed
 *                           over the ranks, every rank gets the same bits.  scale, count (host, ncat; either may be NULL).
 *   fsnap_robust_reweight   r_i = sqrt(omega(e_i / s_g)) for loss = FSNAP_ROBUST_HUBER / _BISQUARE / _CAUCHY with tuning
 *                           constant c > 0, from scale (host, ncat; NULL = the scales of the last fsnap_robust_scale);
 *                           s_g = 0: r = 1.  sums (host, ncat x 6, may be NULL) = n, rows with omega < 1, rows with
 *                           omega = 0, sum omega, sum e^2, sum rho per class, of THIS rank's rows.  From then on the
 *                           context's fits (fsnap_fit_resident, fsnap_fit_dist, fsnap_normal_eq*) read w_i r_i.
 *   fsnap_robust_step       residuals + reweight in one launch: A is read once and no m-vector a second time; the bits of
 *                           the two separate calls.  Needs scales (argument, or an earlier fsnap_robust_scale).
 *   fsnap_robust_download   e, r, wr (host, m doubles; each may be NULL): diagnostics, on demand; also after
 *                           fsnap_robust_end, until the rows change.
 *   fsnap_robust_end        puts the context's weights, mask and packed-weight state back exactly as they were at begin.
 * New rows or new weights (fsnap_upload_rows, fsnap_bind_rows, fsnap_set_weights*, fsnap_bind_weights ...) end a session
 * without restoring anything.  FSNAP_E_ARG: K is not the rows' width, unknown loss, c <= 0, ncat or a class id out of range;
 * FSNAP_E_STATE: no rows, no weights, no session, no residuals or no scales yet.  Every sum is folded in a fixed order and
 * the selection uses integer atomics only: bit-identical run to run.  Host in and out, synchronous. */
#define FSNAP_ROBUST_HUBER 0
#define FSNAP_ROBUST_BISQUARE 1
#define FSNAP_ROBUST_CAUCHY 2
#define FSNAP_ROBUST_MAX_CLASSES 32
int fsnap_robust_begin(fsnap_ctx* ctx, const int32_t* cat, int ncat);
int fsnap_robust_residuals(fsnap_ctx* ctx, const double* beta, int64_t K);
int fsnap_robust_scale(fsnap_ctx* ctx, double* scale, int64_t* count);
int fsnap_robust_reweight(fsnap_ctx* ctx, int loss, double c, const double* scale, double* sums);
int fsnap_robust_step(fsnap_ctx* ctx, const double* beta, int64_t K, int loss, double c, const double* scale, double* sums);
int fsnap_robust_download(fsnap_ctx* ctx, double* e, double* r, double* wr);
int fsnap_robust_end(fsnap_ctx* ctx);

/* ---- K x K solve (host side, no context needed) ----------------------------------- */

/* Solve the K x K system given the statistics.  `kind` is one of FSNAP_SOLVE_*;
 * `param` is rcond (LSTSQ) or alpha (RIDGE, RIDGE_INV), ignored for CHOL.
 * beta[K] out; *rank (may be NULL) receives the numerical rank used; *rcond_est (may be NULL) what the factorisation
 * knows about the conditioning of the Jacobi-scaled matrix S (unit diagonal, so 1 <= lambda_max <= K): for the LSTSQ
 * kinds -- which stand in for an SVD of the rows, svd.py:54 -- min(smallest pivot, lambda_min(S) estimated from the factor
 * by 2 ... 8 Lanczos steps on S^-1, i.e. pairs of triangular sweeps: dpocon's idea, csrc/fsnap_condest.h), an estimate
 * from ABOVE that is within a factor ~1.3 of lambda_min wherever the statistics still resolve it (lambda_min > ~K eps)
 * -- for a factor on the DEVICE (fsnap_solve_device*, K >= 232): the Rayleigh-Ritz value of S^-1 on 31 probe vectors that the
 * factorisation carries in its right-hand-side strip, scaled by 120 / K, within ~[lambda_min / 5, 10 lambda_min], no sweep --;
 * a factor whose estimate falls below 64 K eps counts as unresolved exactly like a failed pivot.  For the other kinds
 * (sklearn's Cholesky, np.linalg.inv: neither looks at the conditioning) the smallest pivot alone, an upper bound of
 * lambda_min that can be off by a factor exponential in K.
 * Replaces scipy.linalg.lstsq (svd.py:54), sklearn Ridge's Cholesky solve
 * (ridge.py:47-57) and np.linalg.inv (regressor.py:15). */
int fsnap_solve(int kind, double param, int64_t K, const double* G, const double* c, double* beta, int* rank,
                double* rcond_est);

/* What the LAST K x K solve of the calling thread (fsnap_solve, fsnap_solve_device*, fsnap_fit_resident, fsnap_fit_dist) learned
 * about the conditioning: info[0] = smallest scaled pivot, info[1] = lambda_min estimate from the factor (0 = none taken or
 * numerically singular), info[2] = applications of S^-1 it took (0 = none: not an LSTSQ kind, or a reused factor),
 * info[3] = 0 host factor / 1 device factor.  Diagnostic: *rcond_est already carries min(info[0], info[1]). */
int fsnap_cond_info(double info[4]);

/* LASSO by cyclic coordinate descent on the statistics: minimises (1/2) w^T Q w - q^T w + l1_reg |w|_1 with Q = A_w^T A_w,
 * q = A_w^T b_w, i.e. scikit-learn's Lasso(alpha, fit_intercept=False, max_iter).fit(aw, bw) of the reference
 * (fitsnap3lib/solvers/lasso.py:23-28) with l1_reg = alpha * n_samples.  Stopping rule as scikit-learn's: duality gap
 * < tol * y_norm2 (y_norm2 = b_w^T b_w), looked at once a sweep's largest update drops below tol x the largest
 * coefficient, or after max_iter sweeps.  w[K]: start vector in (zeros in the reference), coefficients out;
 * *n_iter / *gap (may be NULL): sweeps run and the last duality gap.  Host side, no context needed. */
int fsnap_lasso_gram(int64_t K, const double* Q, const double* q, double y_norm2, double l1_reg, int64_t max_iter, double tol,
                     double* w, int64_t* n_iter, double* gap);

/* Greedy forward selection on the statistics (orthogonal matching pursuit and its orthogonal-least-squares form): the
 * unshrunk least-squares fit on a nested, ordered list of columns, one column more per step.  Q (K x K, row-major, symmetric),
 * q and y2 = |y|^2 are X^T X, X^T y and y^T y of the rows.  Column j is dead -- never chosen, coefficient 0 -- when
 * diag_ref[j] == 0 or Q_jj <= 1e-10 diag_ref[j] (diag_ref = NULL: Q's own diagonal, so only a column with Q_jj <= 0 is).
 * State: t_j = Q_jj, r_j = q_j, e_0 = y2.  Step s = 1 ... S: the candidates are the live columns neither chosen nor struck; a
 * candidate with t_j <= 1e-10 Q_jj is struck for good (it lies in the span of the support).  While `forced` (nforced indices
 * in order; may be NULL when nforced = 0) is not exhausted its next entry is taken if it is a candidate and skipped without a
 * step if not; otherwise j* = argmax score_j, score_j = r_j^2 / Q_jj (FSNAP_OMP_OMP) or r_j^2 / t_j (FSNAP_OMP_OLS), an exact
 * tie going to the lowest index.  Then, for every live column k (dead: w_k = 0),
 *     l = sqrt(t_j*),  w_k = (Q_{j*,k} - sum_{u<s} W_{u,j*} W_{u,k}) / l,  z_s = r_j* / l,
 *     r_k -= w_k z_s,  t_k -= w_k^2,  e_s = e_{s-1} - z_s^2,  row s of W = w
 * (sums with u ascending, one fma per term).  The coefficients after s steps solve L^T beta_S = z_{1..s}, L[v][u] = W_{u,j_v},
 * by column-oriented back substitution from the last row up.  Without a candidate the path ends: later order entries are -1,
 * later path rows (the last e_s, 0, 0) and later coefficient rows repeat the last step's (zeros when no step was taken).
 * Outputs: order[S]; path[S][3] = e_s, the score and the pivot t_j* of the chosen column; coef[S][K].  FSNAP_E_ARG for K < 1,
 * S outside 1 ... K, an unknown criterion, nforced < 0, a forced index out of range or repeated, a NULL pointer;
 * FSNAP_NUM_NONFINITE for a NaN/Inf in the statistics.  Host side, no context needed. */
int fsnap_omp_gram(int64_t K, const double* Q, const double* q, double y2, const double* diag_ref, int criterion,
                   const int32_t* forced, int64_t nforced, int64_t S, int32_t* order, double* path, double* coef);

/* BCS on the statistics: Bayesian compressive sensing by the fast relevance-vector recurrence of Tipping & Faul, the reference's
 * bcs() (fitsnap3lib/solvers/bcs.py) with Q = A^T A (K x K, row-major, symmetric), q = A^T y, y2 = |y|^2, sum_y = sum y and n
 * rows.  sigma2 > 0: the initial noise variance; sigma2 = 0: max(scale (y2 / n - (sum_y / n)^2), 1e-16) (the reference's rule is
 * scale = 0.01).  State: the active columns in order with alpha, mu and Sig by position, S_j and Q_j per column.  Kept from the
 * reference statement for statement: the 1e-16 nugget in its five places; the initial column argmax (q_j^2 + nugget) / (Q_jj
 * + nugget); per iteration ss, qq (rescaled for active columns), theta = qq^2 - ss and the three ml formulas (re-estimate and
 * add for theta > 0, delete for an active column with theta <= 0); argmax ml in numpy's order (a NaN wins; the lowest index on equality); the stop test
 * after the pick, for the third and later iterations only, |ml_t - ml_{t-1}| < |ml_t - ml_0| eta; the re-estimate, add and
 * delete updates (append at the end, compact on deletion); the end when a deletion is asked for and one column is left (before
 * or after it); sigma2_new = rss / (n - n_active + sum alpha_p Sig_pp) with rss = y2 - 2 mu . q_s + mu^T Q_ss mu.
 * deletion = FSNAP_BCS_REFERENCE computes what the reference computes: its deletion reads Sig[:, p] through a view that its
 * own in-place downdate of Sig has zeroed, so mu only loses its entry and S, Q stay stale; FSNAP_BCS_EXACT applies Tipping &
 * Faul's updates of mu, S and Q.  Departures: (1) what the reference forms from rows is formed from Q: comm_j = (sum_a Q[s_a, j]
 * Sig_ap) / sigma2 and comm2_j = (Q[i, j] - sum_a Q[s_a, j] comm1_a) / sigma2, sums with the position a ascending, one fma per
 * term; (2) column j is dead -- never a candidate, not for the initial pick either, coefficient 0 -- when diag_ref[j] == 0 or
 * Q_jj <= 1e-10 diag_ref[j] (diag_ref = NULL: Q's own diagonal); (3) with max_active columns active, inactive columns are not
 * candidates; (4) an iteration without a candidate, or whose pick is an inactive column without theta > 0, ends the problem
 * (the reference would repeat a no-op to itermax); the argmax keeps numpy's order: a NaN ml wins, as it does in the reference
 * after a deletion has left S stale; (5) the reference's assert det(Sig) > -nugget is status 1 (the determinant by
 * symmetric elimination without pivoting), as is a non-finite mu or errbar: such a problem has NaN coefficients and the call
 * still returns FSNAP_OK; (6) itermax is an argument (the reference hard-codes 10).
 * Outputs: coef[K] (mu on the active columns, 0 elsewhere); active[max_active] (int32, in order, then -1); alpha, mu,
 * errbars[max_active] by position (errbars = sqrt(max(Sig_pp, 0)), 0 past the active set); Sig[max_active][max_active]
 * (unclipped, zero past the active set); picks[itermax][2] (int32: column and action 0 re-estimate / 1 add / 2 delete / 3 chosen
 * but stopped; -1 after the end); info[6] = iterations that chose a column, status (0 ended by a stop rule, 1 failed, 2
 * itermax reached), sigma2 as used, sigma2_new, rss, margin = the smallest (ml_best - ml_second) / |ml_best| over the
 * iterations (inf when there never was a second candidate).  FSNAP_E_ARG for K < 1, itermax < 1, max_active outside 1 ... K,
 * an unknown deletion, sigma2 < 0, sigma2 = 0 with scale <= 0, eta < 0, any of them not finite, or a NULL pointer (diag_ref
 * may be NULL); FSNAP_NUM_NONFINITE for a NaN/Inf in the statistics.  Host side, no context needed. */
#define FSNAP_BCS_REFERENCE 0
#define FSNAP_BCS_EXACT 1
int fsnap_bcs_gram(int64_t K, const double* Q, const double* q, double y2, double sum_y, double n, const double* diag_ref,
                   double sigma2, double scale, double eta, int64_t itermax, int64_t max_active, int deletion, double* coef,
                   int32_t* active, double* alpha, double* mu, double* errbars, double* Sig, int32_t* picks, double* info);

/* Spectral path of ONE system on the statistics: the ridge fits (Q + alpha I) beta = q and the truncated least-squares fits of
 * lstsq(rcond) for every setting of a grid from one eigendecomposition (the host route of fsnap_spectral_path above and its
 * check; solvers/spectral_path.py).  Column j is dead -- coefficient 0, no part in the decomposition -- when diag_ref[j] == 0
 * or Q_jj <= 1e-10 diag_ref[j] (diag_ref = NULL: Q's own diagonal); L are the n_live live columns.
 * (1) Q[L, L] = V diag(lambda) V^T by two-sided Jacobi rotations on the unscaled matrix (Jacobi resolves the small eigenvalues
 * of graded matrices to high relative accuracy; alpha and rcond both live in unscaled coordinates): the rotation formula, the
 * skip of |a_pq| <= 1e-18 sqrt(|a_pp| |a_qq|), the stop at off^2 <= 1e-34 diag^2 and the cap of 60 sweeps are the internal
 * eigensolver's behind fsnap_solve; the pairs of a sweep come in the round-robin (circle tournament) order of csrc/
 * fsnap_spectral_body.h, whose rounds hold disjoint pairs and rotate from the matrix before the round.  Reaching the cap is
 * status 2, not an error.  (2) The eigenpairs are sorted ascending by (lambda, position on the rotated diagonal); every sum
 * over i below runs in that order, so a setting's result does not depend on the rest of the grid.  lambda_max = max |lambda_i|,
 * z_i = v_i . q[L].  (3) Setting q = ia Qr + ir = (alpha = alphas[ia] >= 0, rcond = rconds[ir] >= 0): cut = max(rcond^2,
 * 4 n_live eps) lambda_max (the floor of fsnap_solve's SOLVE_LSTSQ); direction i is kept iff lambda_i > cut; g_i = z_i /
 * (lambda_i + alpha) when kept, else 0; beta[L] = V g, beta = 0 on dead columns; rank = the kept directions; dof = sum_kept
 * lambda_i / (lambda_i + alpha); sse = max(y2 - 2 g . z + sum lambda_i g_i^2, 0).  Without a live column: no eigenpairs, rank
 * 0, beta = 0.  Outputs: eig[K] and z[K] ascending, zero past n_live; info[6] = n_live, sweeps, final off / diag ratio,
 * lambda_max, smallest lambda, status; set[Qa Qr][3] = rank, dof, sse; coef[Qa Qr][K].  FSNAP_E_ARG for K < 1, Qa < 1, Qr < 1,
 * a negative or non-finite alpha or rcond or a NULL pointer (diag_ref may be NULL); FSNAP_NUM_NONFINITE for a NaN/Inf in the
 * statistics.  Host side, no context needed. */
int fsnap_spectral_gram(int64_t K, const double* Q, const double* q, double y2, const double* diag_ref, const double* alphas,
                        int64_t Qa, const double* rconds, int64_t Qr, double* eig, double* z, double* info, double* set,
                        double* coef);

/* Same solve, taking the packed statistics [G | c | ...] from DEVICE memory (the buffer
 * fsnap_normal_eq_async / the all-reduce left in HBM).  Small systems are copied to the host
 * (page-locked staging) and solved there (faster than any GPU factorisation of a 128-step recurrence); for
 * K >= 232 (option "device_solve") a blocked Cholesky runs on the GPU and only beta crosses PCIe, provided the
 * system is well conditioned after Jacobi scaling -- otherwise the general host path decides.  Same status codes and semantics as fsnap_solve. */
int fsnap_solve_device(fsnap_ctx* ctx, int kind, double param, int64_t K, const double* d_packed, double* beta,
                       int* rank, double* rcond_est);

/* One call per fit on resident rows: fsnap_normal_eq_resident followed by fsnap_solve_device on its buffer
 * (the whole of SVD / RIDGE.perform_fit, svd.py:44-54 / ridge.py:37-59, for rows and weights already on the
 * device).  *d_packed (may be NULL) receives the address of the statistics, as fsnap_normal_eq_resident does. */
int fsnap_fit_resident(fsnap_ctx* ctx, int kind, double param, double* beta, int* rank, double* rcond_est,
                       double** d_packed);

/* Same as fsnap_solve_device with the right-hand side replaced by rhs (HOST, K doubles; NULL = the c part of the
 * packed buffer): G delta = s of an iterative-refinement step (solver.py has no counterpart: the reference's
 * lstsq works on the rows, see fsnap_residual_rhs) without bringing G to the host.
 * Factor reuse (K >= 232, option chol_reuse): when d_packed is the context's OWN statistics buffer (the address
 * fsnap_fit_resident / fsnap_normal_eq_resident / fsnap_fit_dist handed out) and the last solve of it left its factor on the
 * device, a call with rhs runs two sweeps instead of a factorisation; every library call that rewrites that buffer
 * forgets the factor.  A caller-owned device buffer is factorised on every call -- the library cannot see writes to it. */
int fsnap_solve_device_rhs(fsnap_ctx* ctx, int kind, double param, int64_t K, const double* d_packed, const double* rhs,
                           double* beta, int* rank, double* rcond_est);

/* ---- row-space least squares (ill-conditioned / rank-deficient systems) --------------------------------------- */

/* Optional dense kernel of the host language for the K x K end of fsnap_lstsq_rows when a TRUNCATION is needed and the
 * factor is large (K > 256): x = pinv_rcond(T) y for the n x n upper triangular T (row-major), singular values below
 * rcond * sigma_max dropped, *rank = number kept.  `token` changes with every new T (a caller may cache its
 * decomposition per token; two applications per solve).  Return 0 on success; anything else makes the library fall back
 * on its own one-sided Jacobi SVD -- exact, but O(n^3) per sweep on one core (~20 s at n = 1595, where LAPACK's gesdd
 * takes ~1 s).  fn = NULL removes the hook.  The Python host layer installs scipy.linalg.svd. */
typedef int (*fsnap_dense_pinv_fn)(void* user, int64_t token, int64_t n, const double* T, double rcond, const double* y,
                                   double* x, int* rank);
int fsnap_set_dense_pinv(fsnap_ctx* ctx, fsnap_dense_pinv_fn fn, void* user);

/* fit = scipy.linalg.lstsq(aw, bw, rcond) of the resident rows, computed on the ROWS like the reference's dgelsd
 * (fitsnap3lib/solvers/svd.py:44-54) instead of from the normal equations -- for systems whose K x K statistics are
 * numerically singular (kappa(A_w) beyond ~1e7) or rank deficient: shifted CholeskyQR passes on the GPU
 * (A_w = Q R_hat, Q m x K with orthonormal columns, kept in HBM next to A), then the K x K end of dgelsd on R_hat
 * (singular values below rcond * sigma_max dropped, minimum-norm solution) and one refinement step with the residual
 * of the original rows.  Needs m * K * 8 more bytes of HBM.  Collective when the context has a communicator (a rank
 * without rows passes K and contributes nothing).  *rank = numerical rank used.  info (may be NULL, 8 doubles):
 * passes, last max|Q^T Q - I|, converged (0/1), how the K x K end was solved (0 = back substitution: nothing to drop;
 * 3 = back substitution between two projections: 1...24 dropped directions found by subspace iteration, every other
 * singular value certified above the cut; 1 = the library's one-sided Jacobi SVD; 2 = the host language's dense kernel),
 * sigma_max, sigma_min estimate (bounds unless the SVD ran), relative size of the refinement step, last shift.
 * FSNAP_ROWSPACE_DEFLATE=0 in the environment takes form 3 out (A/B). */
int fsnap_lstsq_rows(fsnap_ctx* ctx, double rcond, int64_t K, double* beta, int* rank, double* info);

/* The two host steps of that solve for callers that run the passes themselves (rows streamed through
 * fsnap_normal_eq_accumulate, or the CPU tests): no context, no GPU.
 * fsnap_rowspace_factor: G = Gram matrix Q^T Q of the current Q (K x K).  first = 1 initialises R_hat (K x K,
 *   A_w = Q R_hat) to the identity.  Unless first, a deviation max|G - I| <= tol means Q is done: info[1] = 1 and nothing
 *   else changes.  Otherwise Rp (K x K, upper triangular) receives the factor to divide out (Q <- Q Rp^-1 by
 *   substitution) and R_hat <- Rp R_hat.  info (may be NULL, 3 doubles): deviation, converged, shift.
 * fsnap_rowspace_solve: beta = pinv_rcond(R_hat) z with z = Q^T (w b), dgelsd semantics; info (may be NULL, 4 doubles):
 *   how it was solved (0 / 3 / 1 as in fsnap_lstsq_rows), sigma_max, sigma_min kept, Jacobi sweeps. */
int fsnap_rowspace_factor(int64_t K, const double* G, int first, double tol, double* Rhat, double* Rp, double* info);
int fsnap_rowspace_solve(int64_t K, const double* Rhat, const double* z, double rcond, double* beta, int* rank, double* info);

/* ONE pass Q <- X R^-1 of that solve on its own (kernels 13B / 13C of fsnap_trsm.hip), for tests and diagnosis: R = K x K
 * row-major on the host, its upper triangle is read (K = columns of the resident rows); the call pads it to K16 = K rounded
 * up to 16 with an identity, forms the inverses of its 16 x 16 diagonal blocks, uploads both, runs the pass on the context's
 * stream and waits -- what a pass of fsnap_lstsq_rows does with the factor of fsnap_rowspace_factor.  first = 1: X =
 * diag(w_eff) A of the resident rows and weights (rows with w_eff = 0 become +0.0 whatever they hold), written to d_Q
 * (device, m x K, leading dimension K); first = 0: X = d_Q, in place.  family: 0 = the kernel fsnap_lstsq_rows launches at
 * (m, K); 1 = kernel 13C (K16 <= 144); 2 = kernel 13B with 16-row tiles, 3 = with 32-row tiles (K16 > 128) -- at row counts
 * where fsnap_lstsq_rows would pick another one as well.  FSNAP_E_ARG for a family outside its range of widths.
 * *family_run (may be NULL) = the family that ran: with family = 0, what the rule of fsnap_lstsq_rows picked.
 * fsnap_qpack_device: the per-row pairs (w_eff != 0 ? 1 : 0, w_eff b) that the statistics of Q are taken with, into d_qpack
 * (device, 2 m doubles). */
int fsnap_trsm_pass(fsnap_ctx* ctx, const double* R, int first, int family, double* d_Q, int* family_run);
int fsnap_qpack_device(fsnap_ctx* ctx, double* d_qpack);

/* The same K x K end for K > 256, where fsnap_lstsq_rows keeps the factors of the passes apart: R = nfac upper triangular
 * K x K factors, R[0] the first pass (R_hat = R[nfac-1] ... R[0] is NOT formed unless a truncation is needed: the product costs
 * K^3 / 3 flops per pass on one host core).  beta = pinv_rcond(R_hat) z: by nfac back substitutions when an upper estimate
 * of cond(R_hat) (sqrt(||R||_1 ||R||_inf) x Hager / Higham 1-norm estimates of the inverses, per factor) shows that no singular value can fall
 * below rcond sigma_max, through the multiplied-out factor and fsnap_rowspace_solve's path otherwise.  active (may be NULL =
 * all): columns that take part (zero columns of A_w get beta = 0).  The chain is taken only when the estimate of cond(R_hat)
 * leaves two orders of margin (estimate x rcond < 1e-2: the estimators are lower bounds x safety factors, not bounds);
 * otherwise the multiplied-out factor is judged with provable Frobenius bounds and, if those cannot exclude a truncation,
 * by the SVD.  info[4] = {1 if solved through the chain, estimate of ||R_hat||, of ||R_hat^-1||, their product}.  Host side,
 * no context needed. */
int fsnap_rowspace_chain(int64_t K, int64_t nfac, const double* R, const unsigned char* active, const double* z, double rcond,
                         double* beta, int* rank, double* info);

/* Grouped error statistics of Solver.error_analysis (solver.py:108-133: the function applied to every
 * (Groups, Testing, Row_Type) group of the DataFrame, solver.py:391-405) for the resident rows and weights:
 * cat[m] (host) = category id of each row in [0, ncat) (negative = skip; NULL = the categories of the previous call
 * are still valid: re-weighting loops re-use them), beta = coefficients.
 * stats[ncat][10] (host) = n, count_nonzero(w), sum t, sum w t, sum|r|, sum r^2, sum (t - mean t)^2,
 * sum|w r|, sum (w r)^2, sum (w t - sum(w t)/n_w)^2 with r = t - a.beta; mae = sum|r| / n,
 * rmse = sqrt(sum r^2 / n), rsq = 1 - sum r^2 / sum (t - mean)^2 (weighted: w_mae = sum|w r| / n,
 * w_rmse = sqrt(sum (w r)^2 / n_w), ...).  Predictions (GEMV) and both reduction passes run on the GPU. */
int fsnap_error_stats(fsnap_ctx* ctx, const double* beta, const int32_t* cat, int ncat, double* stats);

/* ---- batched candidate fits of a weight search ------------------------------------------------------------------
 * A candidate p scales the base weight w0_i of every row of category c by S[p][c] (the genetic algorithm's
 * new_w[i] = table[group(i)][eweight | fweight | vweight], examples/library/genetic_algorithm/libmod_optimize.py).  Its
 * statistics are then G_p = sum_c S[p][c]^2 G_c, c_p = sum_c S[p][c]^2 r_c: one pass over the rows gives the per-category
 * G_c, r_c, and a candidate costs a C x (K^2 + K + 3) combination and a K x K solve.  Results are bit-identical run to
 * run, and a candidate's results do not depend on the other candidates of its batch. */

/* Upper bound of the per-category statistics, ncat * FSNAP_PACKED_LEN(K) * 8 bytes, and of the P candidates' packed
 * statistics of one fsnap_fit_candidates call, P * FSNAP_PACKED_LEN(K) * 8 bytes; past it the calls return FSNAP_E_ARG. */
#define FSNAP_CAT_STATS_MAX_BYTES ((int64_t)2 << 30)

/* Work layout of the candidate kernels for the resident rows: cat[m] (host) = category id of each row in [0, ncat)
 * (negative = the row takes no part, as in fsnap_error_stats).  The row ids are stable-sorted by category (counting sort)
 * and cut into chunks of at most 1024 rows of one category, once for the training rows of the resident mask and once
 * for all categorised rows; the resident weights are copied as the base weights w0.  *layout receives the tag of this
 * layout (unique in the process); every later call of the group names it and fails with FSNAP_E_STATE when the context
 * no longer holds it -- a context holds ONE layout: another fsnap_cat_prepare replaces it, and any change of the resident
 * rows (fsnap_upload_rows, fsnap_bind_rows, fsnap_rows_alloc, fsnap_drop_rows, fsnap_assemble) drops it.  Mask and weights
 * are those of this call (later changes do not reach the layout).  At most 2^31 - 1 rows.  Synchronous. */
int fsnap_cat_prepare(fsnap_ctx* ctx, const int32_t* cat, int ncat, int64_t* layout);

/* What the context holds (ctx may be NULL: the first three entries are then 0): info[0] = tag of its layout (0 = none),
 * info[1] = its number of categories, info[2] = the order of its per-category statistics (0 = none computed yet),
 * info[3] = rows per chunk (1024), info[4] = candidates per launch of the row kernel (16).  n <= 5 entries. */
int fsnap_cat_info(const fsnap_ctx* ctx, int64_t* info, int n);

/* The host half of fsnap_cat_prepare, no context needed: idx (capacity m) receives the ids of the rows with cat >= 0 (and
 * mask != 0 unless mask is NULL) stably sorted by category; chunks (capacity 3 (m + ncat)) receives *nchunks triples
 * (category, first position in idx, rows) in category order, at most 1024 rows each, none empty. */
int fsnap_cat_chunks(int64_t m, const int32_t* cat, const uint8_t* mask, int ncat, int32_t* idx, int64_t* chunks,
                     int64_t* nchunks);

/* Per-category statistics of the training rows with the base weights, one pass over the rows (kernels C1 + C1R of
 * csrc/fsnap_cand.hip): *d_stats (device, owned by the context, valid until the next call of this group) receives
 * ncat blocks of FSNAP_PACKED_LEN(K) doubles, each [G_c | r_c | b^T W^2 b, sum w b, n_train] as fsnap_normal_eq_resident
 * lays them out.  Asynchronous. */
int fsnap_cat_normal_eq(fsnap_ctx* ctx, int64_t layout, double** d_stats);

/* Multi-GPU form (collective, every rank of the communicator): each rank computes the statistics of ITS rows and one
 * in-place all-reduce of ncat * FSNAP_PACKED_LEN(K) doubles -- the transport of fsnap_fit_dist -- leaves the sums on every
 * rank (K and ncat must agree on all ranks).  *layout = the rank's prepared layout, or 0 on a rank without rows: it
 * contributes zeros and receives the tag of a layout that holds the statistics only (for fsnap_fit_candidates). */
int fsnap_cat_normal_eq_dist(fsnap_ctx* ctx, int64_t* layout, int64_t K, int ncat, double** d_stats);

/* P candidates from the per-category statistics of layout `layout` (ncat categories, order K: both must be those of the
 * statistics the context holds, else FSNAP_E_ARG; S must hold P x ncat doubles, beta P x K): kernel C2 forms
 * G_p, c_p = sum_c S[p][c]^2 (G_c, r_c) (S: host, P x ncat, row-major), then each candidate is solved by
 * fsnap_solve_device (K < 232 on the host, from 232 on by the device Cholesky): beta[P][K], rank[P] and rcond_est[P]
 * exactly as fsnap_fit_resident reports them.  *d_packed (may be NULL) receives the device address of the P packed
 * buffers (p at offset p * FSNAP_PACKED_LEN(K)), valid until the next call of this group.  Synchronous; the first solve
 * that fails ends the call with its status. */
int fsnap_fit_candidates(fsnap_ctx* ctx, int64_t layout, int kind, double param, const double* S, int P, int ncat, int64_t K,
                         double* beta, int* rank, double* rcond_est, double** d_packed);

/* One pass over the rows of layout `layout` (ncat and K must be its own, else FSNAP_E_ARG) for P coefficient vectors
 * beta[P][K] (host), y_p = a . beta_p, r = t - y_p (kernel C3, at
 * most 16 candidates per launch; more take several launches):
 *   what = FSNAP_CAND_ERROR_SUMS: out[P][ncat][4] = sum|r|, sum r^2, sum|w0 r|, sum (w0 r)^2 over all rows of each
 *          category (S may be NULL) -- the candidate-dependent sums of fsnap_error_stats; the weighted ones scale
 *          with |S[p][c]| and S[p][c]^2;
 *   what = FSNAP_CAND_RHS: out[P][K] = A^T (S[p][c(i)]^2 w0_i^2 r_i) over the training rows, fsnap_residual_rhs for P
 *          candidates (S: host, P x ncat).
 * Synchronous. */
#define FSNAP_CAND_ERROR_SUMS 0
#define FSNAP_CAND_RHS 1
int fsnap_candidate_rows(fsnap_ctx* ctx, int64_t layout, const double* beta, const double* S, int P, int ncat, int64_t K,
                         int what, double* out);

/* Grouped K-fold cross-validation of weight candidates on per-(fold, category) statistics (kernels V0, V1 of
 * csrc/fsnap_cv.hip; the folds, routes and tables are solvers/candidates_cv.py).  The context holds, for `layout`, F * C
 * packed blocks B[f][c] as fsnap_cat_normal_eq / fsnap_cat_normal_eq_dist leave them, composite category f * C + c (fold f of
 * the row's unit, category c of the weight search); T[c] = sum_f B[f][c], folds added in index order.  S (host, P x C,
 * row-major, finite) scales category c of candidate p.  Problem (p, f), 0 <= f < F, is the refit of candidate p without fold f:
 *     Qm = sum_c S[p][c]^2 (T[c].G - B[f][c].G),  qv = sum_c S[p][c]^2 (T[c].r - B[f][c].r)     (c ascending, one fma per term)
 *     Tp_jj = sum_c S[p][c]^2 T[c].G_jj
 *     H = Qm + alpha I,  D = sqrt(diag H),  beta = D^-1 (D^-1 H D^-1)^-1 D^-1 qv                 (Cholesky, live columns only)
 * Column j is dead -- coefficient 0, its row, column and qv_j removed -- when Tp_jj == 0 or Qm_jj <= 1e-10 Tp_jj (the fold
 * alone touched the column and the subtraction left noise: the rule of fsnap_lasso_path).  A pivot of the scaled matrix that
 * is not > 1e-10 ends the problem with status 1 and NaN coefficients (the rule of fsnap_ridge_path); the call still returns
 * FSNAP_OK.  These are plain Jacobi-scaled Cholesky solves of the normal equations: no probe, no refinement with the row
 * residual, no row-space solve.  Outputs (host): coef_out[P][F][K]; info_out[P][F][4] = status (0 / 1), the smallest scaled
 * pivot met (inf when no column is live), live columns, sum_c S[p][c]^2 (T[c].n - B[f][c].n) (the training rows of the
 * problem, each counted with the square of its category's scale).  FSNAP_E_ARG: K outside 1 ... 144 or not the order of the
 * statistics, F < 2, C < 1, P < 1, F * C != the layout's number of categories, a non-finite S or a negative or non-finite
 * alpha, a NULL pointer, P * F > FSNAP_CV_MAX_PROBLEMS or P * F * K doubles past FSNAP_CAT_STATS_MAX_BYTES.  FSNAP_E_STATE:
 * the context no longer holds the layout or its statistics.  fp64, no atomics; every sum runs in an order fixed by the
 * problem alone: a problem's bits do not depend on the batch, the grid or the run.  The resident rows, weights, mask, the
 * layout and its statistics are not touched.  Synchronous. */
#define FSNAP_CV_MAX_PROBLEMS (1 << 20)
int fsnap_cv_candidates(fsnap_ctx* ctx, int64_t layout, double alpha, const double* S, int P, int F, int C, int64_t K,
                        double* coef_out, double* info_out);

/* Held-out sums of the refits above (kernel V2 of csrc/fsnap_cv.hip, reduced by kernel C3R of csrc/fsnap_cand.hip): one pass
 * over the categorised rows of `layout` per 16 candidates.  A chunk of the layout holds rows of ONE composite category, so of
 * one fold f = category / C; its rows are multiplied with coef[p][f] (host, P x F x K), r = t - a . coef[p][f]: the row's
 * residual under the refit that did not see its unit.  out (host): P x (F * C) x 4 = sum|r|, sum r^2, sum|w0 r|, sum (w0 r)^2
 * per candidate and composite category, chunks and their waves added in index order; the weighted sums scale with |S[p][c]|
 * and S[p][c]^2.  NaN coefficients give NaN sums for that (p, f) only.  K must be the width of the resident rows (any K) and
 * F * C the layout's number of categories, else FSNAP_E_ARG; FSNAP_E_STATE when the context no longer holds the layout.
 * Bit-identical run to run; a candidate's sums do not depend on the other candidates.  Nothing resident is changed.
 * Synchronous. */
int fsnap_cv_candidate_rows(fsnap_ctx* ctx, int64_t layout, const double* coef, int P, int F, int C, int64_t K, double* out);

/* Gradient of a cross-validated cost over the scales S (kernels G1, G2 of csrc/fsnap_cvgrad.hip; the objective and omega are
 * solvers/candidates_cv_grad.py).  For a cost J[p] = sum_t wt[t] phi(E[p][t] / n_t) of the base-weighted held-out sums
 * E[p][t] = sum (w0 r)^2 over the training categories of row type t, the caller passes omega[p][c] = dJ/dE of the type of
 * category c (host, P x C, finite; 0 for categories that take no part) and coef[p][f][K] = the refits of fsnap_cv_candidates for the
 * same layout, alpha and S (host; NaN where a refit failed).  With B[f][c] the blocks, R[f][c] = T[c] - B[f][c] and
 * H = sum_c S[p][c]^2 R[f][c].G + alpha I on the live columns of problem (p, f) (the live rule above; the live set is treated as
 * fixed, dead columns have beta_j = lambda_j = 0):
 *     g[p][f]      = 2 sum_c omega[p][c] (B[f][c].G beta[p][f] - B[f][c].r)       (four quarters of ceil(C / 4) categories, c ascending
 *                                                                                  in each, added in index order; per c, k in steps of 8)
 *     lambda[p][f] = H^-1 g[p][f]                          (kernel V1's Jacobi-scaled Cholesky, live rule and pivot rule)
 *     D[p][f][c]   = lambda[p][f] . (R[f][c].r - R[f][c].G beta[p][f])            (rows ascending per wave, waves in index order)
 *     grad_S_out[p][c]      = 2 S[p][c] sum_f D[p][f][c]                          (f in index order, on the host)
 *     grad_log_alpha_out[p] = -alpha sum_f lambda[p][f] . beta[p][f]              (k ascending, then f in index order, on the host)
 * grad_S_out is dJ/dS[p][c] (defined at S = 0 and for negative S; dJ/dlog|S| = S dJ/dS), grad_log_alpha_out dJ/dlog alpha.
 * Scaling every S[p][.]^2 and alpha by one factor changes no beta, so sum_c S dJ/dS = -2 dJ/dlog alpha.  Both sweeps over the
 * blocks run on v_mfma_f64_16x16x4_f64 for 16 candidates at a time: a block is read once per 16 candidates.  lambda_out (host,
 * P x F x K, may be NULL) receives lambda; info_out[P][F][2] = status (0 / 1) and the smallest scaled pivot of the adjoint solve,
 * those of the refit.  A problem of status 1 has NaN lambda: the gradient row and grad_log_alpha of ITS candidate are NaN, no
 * other candidate changes; the call still returns FSNAP_OK.  T[c] and R[f][c] are formed again from the blocks the context holds
 * (kernel V0).  Arguments, state and limits as fsnap_cv_candidates (K <= 144; also the coefficient tables, 16 ceil(P / 16) F K
 * doubles, and 16 ceil(P / 16) F C doubles of D within FSNAP_CAT_STATS_MAX_BYTES); a non-finite omega is FSNAP_E_ARG.  fp64, no
 * atomics; every sum runs in an order fixed by the problem alone: a candidate's bits do not depend on the batch, the grid or the
 * run.  Nothing resident is touched.  Synchronous. */
int fsnap_cv_candidates_grad(fsnap_ctx* ctx, int64_t layout, double alpha, const double* S, const double* omega, const double* coef,
                             int P, int F, int C, int64_t K, double* grad_S_out, double* grad_log_alpha_out, double* lambda_out,
                             double* info_out);

/* The adjoint right-hand sides g[P][F][K] (above) of the last successful fsnap_cv_candidates_grad call on this context, for tests
 * and diagnostics: g_out (host) receives n = P * F * K doubles.  FSNAP_E_STATE without such a call, FSNAP_E_ARG when n is not
 * its P * F * K.  Synchronous. */
int fsnap_cv_candidates_grad_rhs(fsnap_ctx* ctx, int64_t n, double* g_out);

/* Device times of the last successful fsnap_cv_candidates_grad call on this context, from events on its stream: ms_out[3] =
 * kernels V0 + G1 (RHS epilogue), kernel G2, kernel G1 (bilinear epilogue), in milliseconds.  FSNAP_E_STATE without such a call. */
int fsnap_cv_candidates_grad_times(fsnap_ctx* ctx, double* ms_out);

/* Marginal likelihood (evidence) of weight candidates from the per-category statistics of `layout` (kernels E1, E2, E3 of
 * csrc/fsnap_evidence.hip; the definitions, the float64 assembly of L and its gradients, and the ascent are
 * solvers/candidates_evidence.py).  S (host, P x ncat, row-major, finite) scales category c of candidate p; active (host,
 * P x ncat, uint8) is 0 where the category takes no part (a testing category, S = 0, no row of non-zero base weight): its scale
 * counts as 0.  Per candidate, with lambda_c = S[p][c]^2 over the active categories (c ascending, one fma per term):
 *     H = sum_c lambda_c G_c + alpha I,  D = sqrt(diag H),  beta = D^-1 (D^-1 H D^-1)^-1 D^-1 sum_c lambda_c r_c   (live columns)
 * by fsnap_cv_candidates' Jacobi-scaled Cholesky; column j is dead (beta_j = 0, left out) when sum_c lambda_c G_c,jj == 0; a pivot
 * of the scaled matrix that is not > 1e-10 ends the candidate with status 1; the call still returns FSNAP_OK.  Outputs (host):
 *     beta_out[P][K]        beta (NaN with status 1)
 *     info_out[P][6]        status (0 / 1), the smallest scaled pivot met (inf without a live column), live columns,
 *                           log|H| = 2 sum_j (log l_jj + log d_j) (j ascending), tr(H^-1), 0          (NaN with status 1)
 *     terms_out[P][ncat][2] T_c = tr(H^-1 G_c) and Q_c = bb_c - 2 beta . r_c + beta' G_c beta         (0 with status 1)
 * The terms are one fp64 MFMA product of the blocks with two table columns per candidate, [H^-1 | 0 | 0,0,0] and
 * [beta beta' | -2 beta | 1,0,0], the K^2 + K + 3 elements in slices of 512 added in index order: a block is read once per 8
 * candidates.  FSNAP_E_ARG: K outside 1 ... 144 or not the order of the statistics, ncat not the layout's, P < 1, a non-finite S,
 * a negative or non-finite alpha, a NULL pointer, or P candidates whose packed buffers, tables (16 ceil(P / 8) (K^2 + K + 3)
 * doubles) or slice partials pass FSNAP_CAT_STATS_MAX_BYTES.  FSNAP_E_STATE: the context no longer holds the layout or its
 * statistics.  fp64, no atomics; every sum runs in an order fixed by K and ncat alone: a candidate's bits do not depend on the
 * batch, the grid or the run.  Nothing resident is touched.  Synchronous. */
int fsnap_candidates_evidence(fsnap_ctx* ctx, int64_t layout, double alpha, const double* S, int P, int ncat, int64_t K,
                              const uint8_t* active, double* beta_out, double* info_out, double* terms_out);

/* Device times of the last successful fsnap_candidates_evidence call on this context, from events on its stream: ms_out[2] =
 * kernel E1, kernels E2 + E3, in milliseconds.  FSNAP_E_STATE without such a call. */
int fsnap_candidates_evidence_times(fsnap_ctx* ctx, double* ms_out);

/* ---- multi-GPU: one process per GPU; RCCL or one-shot peer-to-peer over xGMI -------- */

/* The reference's data-parallel form of this path (examples/library/transpose_trick/example.py:230-254): every MPI
 * rank accumulates c += aw.T aw, d += aw.T bw over ITS configurations, then comm.Allreduce(c), comm.Allreduce(d)
 * (:245-246) and one solve.  Here a rank is a process that owns one context (= one GPU) holding the rows of its
 * configurations (config i -> rank i % nranks, fitsnap3lib/parallel_tools.py:612-651); the two Allreduce calls are
 * ONE in-place ncclAllReduce(ncclDouble, ncclSum) of the packed statistics on the context's stream.  librccl is
 * loaded on the first call of this group (dlopen), never at library load. */
#define FSNAP_COMM_ID_BYTES 128

/* Every wait behind a collective (fsnap_comm_init itself, the host-buffer collectives, the solve that follows the
 * all-reduce of a fit) is bounded by the environment variable FSNAP_COMM_TIMEOUT (seconds, default 300): when a peer died
 * or never arrived the call returns FSNAP_E_HIP with one line in fsnap_last_error naming rank, world size and the wait
 * that ran out, instead of hanging; the context then aborts its communicator (ncclCommAbort) when it is destroyed.
 * A failure that only ONE rank sees before a collective of fsnap_fit_dist / fsnap_lstsq_rows (wrong K, no weights, an
 * allocation that failed) does not keep that rank out of the collective: it contributes NaN statistics, so that every
 * rank returns FSNAP_NUM_NONFINITE from the same call and the failing rank returns its own error. */

/* Rank 0: create the communicator id (ncclGetUniqueId).  The caller distributes the 128 bytes to every rank by
 * whatever it has -- mpi4py comm.bcast on the reference side, a file or a socket in fitsnap_amd/rendezvous.py.
 * With FSNAP_DIST_TRANSPORT=p2p in the environment the id is one of the peer-to-peer transport (next entry). */
int fsnap_comm_id(char* id);

/* Rank 0: the id of a PEER-TO-PEER communicator (csrc/fsnap_p2p.cpp) -- the second transport, for the GPUs of ONE node.
 * The transport travels with the id: fsnap_comm_init recognises it, so every rank takes the same one.  Every rank
 * exports a double-buffered window of device memory through a hipIpc handle (exchanged, like the joins, through a POSIX
 * shared-memory segment named after the id); the all-reduce of a fit is then ONE launch per rank: own statistics ->
 * own window, a flag pushed into every peer's window, a bounded wait for the peers' flags, the sum of the N windows in
 * RANK ORDER (bit-identical on every rank).  The host-buffer collectives below go through mailboxes in the same
 * segment (no launch, no staging).  hipIpc handles open between processes that share a device, so this transport also
 * runs N ranks on ONE GPU -- what RCCL refuses -- which is how the N > 1 paths are tested on one-GPU boxes.
 * FSNAP_P2P_SLOT_MB (default 24; larger payloads travel in pieces) / FSNAP_P2P_MAILBOX_MB (default 4) size the window
 * slots and the mailboxes; needs HSA_ENABLE_IPC_MODE_LEGACY=0 where the host driver only supports dmabuf IPC. */
int fsnap_comm_id_p2p(char* id);

/* Collective: join the communicator of `nranks` ranks as `rank` (ncclCommInitRank on the context's device, or the
 * peer-to-peer rendezvous when `id` comes from fsnap_comm_id_p2p). */
int fsnap_comm_init(fsnap_ctx* ctx, int nranks, int rank, const char* id);
int fsnap_comm_destroy(fsnap_ctx* ctx);

/* *transport = 0 (no communicator), 1 (RCCL), 2 (peer-to-peer). */
int fsnap_comm_transport(fsnap_ctx* ctx, int* transport);

/* *nranks / *rank of the context's communicator (1 / 0 without one); either pointer may be NULL. */
int fsnap_comm_info(fsnap_ctx* ctx, int* nranks, int* rank);

/* In-place sum over the ranks of n doubles in DEVICE memory (e.g. the packed statistics of fsnap_normal_eq_async),
 * asynchronous on the context's stream: comm.Allreduce(c), comm.Allreduce(d) of transpose_trick/example.py:245-246. */
int fsnap_allreduce_device(fsnap_ctx* ctx, double* d_buf, int64_t n);

/* Same for n doubles in HOST memory (staged through HBM; synchronous).  op: 0 = sum, 1 = max, 2 = min.  The scalar
 * reductions around a fit: row / configuration counts (parallel_tools.py:562-577), the refinement right-hand side,
 * the max-over-ranks wall time of the benchmark. */
int fsnap_allreduce_host(fsnap_ctx* ctx, double* buf, int64_t n, int op);

/* Broadcast nbytes of host memory from rank `root` (comm.bcast, parallel_tools.py:579-592); synchronous. */
int fsnap_bcast_host(fsnap_ctx* ctx, void* buf, int64_t nbytes, int root);

/* recv[rank * nbytes ...] = send of every rank (equal sizes; comm.allgather of the fixed-size error tables and of the
 * pickled row-label lists, parallel_tools.py:426-441); host memory, synchronous. */
int fsnap_allgather_host(fsnap_ctx* ctx, const void* send, int64_t nbytes, void* recv);

/* All ranks reach this point and the context's stream is idle (comm.Barrier, parallel_tools.py:245-249). */
int fsnap_barrier(fsnap_ctx* ctx);

/* One call per fit of a multi-GPU job (the whole of transpose_trick/example.py:230-254 for resident rows): this
 * rank's fused statistics, in-place all-reduce on the same stream, then the K x K solve of fsnap_solve_device -- on
 * EVERY rank (the solve is deterministic and the ranks hold bit-identical sums, so no broadcast of beta is needed;
 * the host layer keeps the reference's "fit on rank 0" contract).  K must be given because a rank may own no rows
 * (it then contributes zeros).  Without a communicator: FSNAP_E_STATE (a single-GPU fit is fsnap_fit_resident; there is
 * no silent fallback that would fit one rank's shard).  *d_packed (may be NULL) receives the address of the reduced
 * statistics (context-owned device memory, valid until the next fit). */
int fsnap_fit_dist(fsnap_ctx* ctx, int kind, double param, int64_t K, double* beta, int* rank, double* rcond_est,
                   double** d_packed);

/* ---- raw device memory for callers without a HIP binding of their own --------------- */

/* hipMalloc / hipFree on the context's device; fsnap_dev_sync waits for the context's stream. */
int fsnap_dev_alloc(fsnap_ctx* ctx, int64_t nbytes, void** d_ptr);
int fsnap_dev_free(fsnap_ctx* ctx, void* d_ptr);
int fsnap_dev_sync(fsnap_ctx* ctx);
/* Synchronous copies between host memory and memory of fsnap_dev_alloc (or any device pointer of this GPU). */
int fsnap_dev_upload(fsnap_ctx* ctx, void* d_dst, const void* h_src, int64_t nbytes);
int fsnap_dev_download(fsnap_ctx* ctx, void* h_dst, const void* d_src, int64_t nbytes);

/* ---- measurement ------------------------------------------------------------------ */

/* HIP-event timings of the last fsnap_normal_eq* call, milliseconds:
 * ms[0] = SYRK kernel, ms[1] = partial reduction kernel, ms[2] = last H2D upload,
 * ms[3] = last stand-alone weighting kernel, ms[4] = last predict kernel; about the last large fsnap_upload_rows:
 * ms[5] = GB/s at which the host filled the first page-locked slots (0: not probed), ms[6] = 1 if the whole matrix went
 * through the page-locked double buffer.
 * Synchronises the context's stream.  n = number of entries of ms to fill (<= 8). */
int fsnap_timing(fsnap_ctx* ctx, double* ms, int n);

/* Kernel times (ms) of the last n event-bracketed fits (option "timing_every") of this context, oldest first (n <= 256): syrk_ms[i] = SYRK kernel,
 * reduce_ms[i] (may be NULL) = partial reduction.  HIP events on the kernels' stream, read after the fact, so a
 * timed loop does not have to synchronise for its measurements.  Synchronises the context's stream. */
int fsnap_timing_history(fsnap_ctx* ctx, double* syrk_ms, double* reduce_ms, int n);

/* For the same n event-bracketed fits: allreduce_ms[i] = time between the end of this rank's partial reduction and the end
 * of the collective of fsnap_fit_dist on this rank's stream (ncclAllReduce, or the peer-to-peer kernel) -- it
 * includes waiting for the slowest peer -- or -1 for a fit without a collective.  Synchronises the context's stream. */
int fsnap_timing_history_comm(fsnap_ctx* ctx, double* allreduce_ms, int n);

/* How many SYRK launches this context has made (*launches) and how many of them were bracketed by events (*sampled:
 * what fsnap_timing_history can return); either pointer may be NULL.  Measurement plumbing of bench.py, no reference
 * counterpart. */
int fsnap_timing_count(fsnap_ctx* ctx, int64_t* sampled, int64_t* launches);

/* Launch geometry of the SYRK kernel for the current rows: info[0] = workgroups,
 * info[1] = threads per workgroup, info[2] = 4-row chunks per row-wave (kernel 1) / per
 * workgroup (kernel 1L) / per wave (tiled), info[3] = NB (16-column blocks), info[4] =
 * split (kernel 1) or waves per workgroup (kernel 1L), info[5] = compute units of the
 * device, info[6] = kernel id (1 wave-triangle, 2 LDS-shared, 3 one-wave triangle 1A, 4 packed
 * wave-triangle 1P, 5 workgroup triangle 1Q -- info[2] is then chunks per WORKGROUP; 7 short-system
 * kernel 1S -- info[0] = row chunks (two workgroups each), info[2] = ROWS per chunk; tiled:
 * superblock pairs), info[7] = row splits (tiled kernel) / 1 when the kernel packs the
 * per-row pairs itself. */
int fsnap_launch_info(fsnap_ctx* ctx, int64_t* info, int n);

#ifdef __cplusplus
}
#endif
#endif /* FSNAP_HIP_H */
