// fsnap_kernels.h — internal C++ interface between the gfx950 kernels
// (fsnap_syrk.hip, fsnap_rows.hip, fsnap_chol.hip) and the C-ABI layer (fsnap_capi.cpp).  Not part of the public
// boundary; the public boundary is include/fsnap_hip.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fsnap {

struct SyrkArgs {
    const double* A;            // device, row-major m x K, leading dimension lda
    int64_t lda;
    const double* b;            // device, m
    const double* w;            // device, m
    const unsigned char* mask;  // device, m (1 = training row) or nullptr
    int64_t m;
    int K;
    int nblocks;                // workgroups (4 row-waves each)
    int split;                  // (1)
    int64_t chunks_per_wave;    // 4-row chunks per wave
    bool nontemporal;           // use nt loads for the A stream
    double* part;               // [nblocks][NT][4][64]
    double* cpart;              // [nblocks*4][NB][16]
    double* spart;              // [nblocks*4][4]
    const double* wpack = nullptr;  // kernel 1A: packed (w_eff, w_eff * b) per row (launch_pack_weights)
    int* flow_words = nullptr;      // kernel 1QC: flow-control words, 4 ints per cluster (zero once, never reset)
    int flow_tag = 0;               // kernel 1QC: + 2^20 per launch
    bool fused_pack = false;        // kernels 1A / 1P: the kernel packs (w_eff, w_eff b) of its rows into LDS itself (b, w, mask,
                                    // spart instead of wpack; needs chunks_per_wave <= syrk_acc_max_fused_cpw())
};

struct TiledArgs {
    const double* A;
    int64_t lda;
    const double* wpack;        // (w_eff, w_eff b) per row (fsnap_pack_weights_k)
    int64_t m;
    int K;
    int NSB;                    // 64-column superblocks
    int npairs;                 // NSB*(NSB+1)/2
    int nsplit;                 // row splits
    int64_t chunks_per_split;   // 4-row chunks per split (each split = 4 waves)
    bool nontemporal;
    double* part;               // [nsplit*npairs][16][4][64]
    double* cpart;              // [(nsplit*NSB)*4][4][16]
    const double* spart;        // [ns][4]: partial b-only scalars of fsnap_pack_weights_k
    int ns;
};

int syrk_num_blocks(int K);
int syrk_waves_per_simd(int K, int split);
hipError_t launch_syrk_wave_p(const SyrkArgs& a, hipStream_t st);   // K <= 80, packed weights (a.wpack)
hipError_t launch_syrk_acc(const SyrkArgs& a, hipStream_t st);
// kernel 1Q (144 < K <= 288, fsnap_syrk_quad.hip): a.chunks_per_wave = chunks per WORKGROUP; pairs from a.wpack or (a.fused_pack,
// chunks per workgroup <= syrk_quad_max_cpg()) formed by the kernel
hipError_t launch_syrk_quad(const SyrkArgs& a, hipStream_t st);
int64_t syrk_quad_max_cpg();
// workgroups per cluster for K columns: 1 = kernel 1Q (K <= 288), 2 / 4 = kernel 1QC (289 ... 512 columns; a.nblocks = clusters,
// a.chunks_per_wave = chunks per cluster, fused packing only)
int syrk_quad_cluster(int K);
int64_t syrk_acc_max_fused_cpw();
// kernel 1S (fsnap_syrk_short.hip; 80 < K <= 144, short systems): a.nblocks = CHUNKS of a.chunks_per_wave ROWS (a multiple of 4),
// two workgroups per chunk; part[chunk][NT][4][64] | cpart[chunk][NB][16] | spart[chunk][4] (one c / scalar partial per chunk);
// pairs from a.wpack or (a.fused_pack) formed by the kernel, any chunk length (phases of syrk_short_phase_rows() rows)
hipError_t launch_syrk_short(const SyrkArgs& a, hipStream_t st);
bool syrk_short_takes(int K);
int syrk_short_phase_rows(int K);
int64_t syrk_wave_p_max_fused_cpw(int K, int wg_per_cu);   // kernel 1P: same for its (smaller, shared) LDS budget
// mirror: optional page-locked HOST buffer that receives the same packed statistics (zero-copy D2H)
// accumulate: out += statistics instead of out = statistics
// ns: number of scalar partials in spart (< 0: nblocks * cs_per_block, like the c partials)
// upper_mirror: the mirror receives the triangle at its upper positions only
hipError_t launch_reduce(const double* part, const double* cpart, const double* spart, int nblocks,
                         int cs_per_block, int ns, int K, double* out, double* mirror, bool accumulate, hipStream_t st,
                         bool upper_mirror = false);
int pack_weights_num_blocks(int64_t m);
// wpack[m][2] = (w_eff, w_eff * b); spart[pack_weights_num_blocks(m)][4] = partial b^T W^2 b, sum(w b), n_train, 0
hipError_t launch_pack_weights(const double* b, const double* w, const unsigned char* mask, int64_t m, double* wpack,
                               double* spart, hipStream_t st);
hipError_t launch_syrk_tiled(const TiledArgs& a, hipStream_t st);
hipError_t launch_reduce_tiled(const TiledArgs& a, double* out, bool accumulate, hipStream_t st);
hipError_t launch_weight_rows(const double* A, int64_t lda, const double* b, const double* w,
                              const unsigned char* mask, int64_t m, int K, double* aw, int64_t ldaw, double* bw,
                              hipStream_t st);
hipError_t launch_assemble(const double* raw, int64_t raw_ld, int64_t nrows, const int64_t* src_row, const int* kind,
                           const int* frac, const double* dval, const double* truth, const double* weight,
                           const double* fractions, const double* blank2J, int ntypes, int ncoeff, int off, double* A,
                           int64_t lda, double* b, double* w, hipStream_t st);
// fused assembly + accumulation (fsnap_fused.hip): b, w, 16-byte row records; then kernel 1T's partials from the raw batch
size_t assemble_row_record_bytes();
hipError_t launch_assemble_bw(const double* raw, int64_t raw_ld, int64_t nrows, const int64_t* src_row, const int* kind,
                              const int* frac, const double* d, const double* truth, const double* weight, int icolref,
                              double* b, double* w, void* recs, hipStream_t st);
hipError_t launch_assemble_syrk(const double* raw, int64_t raw_ld, const void* recs, const double* dval, const double* fractions,
                                const double* blank2J, int ntypes, int ncoeff, int off, const TiledArgs& a, hipStream_t st);
hipError_t launch_mirror_copy(const double* src, int K, double* mirror, hipStream_t st);
// packed [G | c | scalars] <-> [upper triangle of G row-major | c | scalars]: the payload of the multi-GPU all-reduce for wide systems
hipError_t launch_tri_pack(const double* packed, int K, double* tri, hipStream_t st);
hipError_t launch_tri_unpack(const double* tri, int K, double* packed, hipStream_t st);
// blocked Cholesky solve for large K: work (chol_large_work_doubles(K) doubles), dsc, z (np = K rounded up to 64),
// beta (K), status (1 int), minpiv (np / 64) are device scratch / outputs
// cvec: device right-hand side (NULL = the c part of packed)
size_t chol_large_work_doubles(int n);
hipError_t launch_chol_large(const double* packed, const double* cvec, int n, double alpha, double* work, double* dsc, double* z,
                             double* beta, int* status, double* minpiv, double* host_out, bool clear_status, double* probe_out,
                             hipStream_t st);
// probe_out (may be NULL): receives the CHOL_PROBES x CHOL_PROBES matrix Z^T Z of the probe vectors the strip carries (condition
// estimate, see fsnap_chol_probe_gram_k); the probe at (row, p), p = 1 .. CHOL_PROBES, is chol_probe(row, p)
constexpr int CHOL_PROBES = 31;
double chol_probe(int row, int p);
// one more right-hand side (n doubles, device) for the factor the last launch_chol_large of the same n left in `work`
hipError_t launch_chol_resolve(const double* d_rhs, int n, double* work, const double* dsc, double* z, double* beta, int* status,
                               const double* minpiv, double* host_out, hipStream_t st);
// factor only (pass factor of the row-space solve, K >= 384): R = chol(D^-1 G D^-1 + shift I) D for the n x n Gram matrix G in
// device memory, written as the K16 x K16 padded factor + inverse blocks that launch_trsm_rows reads (trsm_factor_doubles(K16)
// doubles at Rout); status: bit 0 non-finite input, bit 1 failed pivot (retry with a larger shift).  work / dsc / minpiv as
// for launch_chol_large.
hipError_t launch_chol_factor(const double* G, int n, double shift, double* work, double* dsc, int* status, double* minpiv,
                              int K16, double* Rout, hipStream_t st);
// out[0 .. n) = row maxima of |G - I|, out[n .. 2 n) = row sums of the squared Jacobi-scaled entries (active columns; NaN row
// maximum = non-finite input): the steering numbers of a row-space pass, so that G itself can stay in HBM
hipError_t launch_gram_scan(const double* G, int n, double* out, hipStream_t st);
int gemv_num_blocks(int64_t m);
hipError_t launch_gemv_rows(const double* A, int64_t lda, const double* beta, int64_t m, int K, double* preds,
                            const double* b, const double* w, const unsigned char* mask, double* sse_part,
                            double* uout, hipStream_t st, bool uplain = false);   // uplain: u = w (b - a.beta), not w^2 (...)
int gemvT_num_blocks(int64_t m);
int residual_num_blocks(int64_t m, int K);
// one-pass s = (wA)^T (wb - wA beta) for K <= 288 (kernels 4 + 7 fused): partial[residual_num_blocks(m, K)][K] scratch,
// sse_part[residual_num_blocks(m, K)] per-workgroup partial SSE (nullptr: none), out[K]
hipError_t launch_residual_rows(const double* A, int64_t lda, const double* beta, int64_t m, int K, const double* b,
                                const double* w, const unsigned char* mask, double* partial, double* sse_part, double* out,
                                hipStream_t st);
hipError_t launch_colsum(const double* partial, int nparts, int ncols, double* out, hipStream_t st);
// w[row] = mask[row] ? wtrain[rank[row]] : 0   (rank = exclusive prefix sum of the mask)
hipError_t launch_expand_weights(const double* wtrain, const unsigned char* mask, const int* rank, int64_t m, double* w,
                                 hipStream_t st);
int error_stats_num_blocks(int64_t m);
// pass 0: partial[grid][ncat][4] = n, n_w, sum t, sum w t; pass 1: partial[grid][ncat][6] (see kernel 9)
hipError_t launch_error_stats(const double* truth, const double* pred, const double* wgt, const int* cat, int64_t m, int ncat,
                              int pass, const double* means, double* partial, hipStream_t st);
hipError_t launch_gemvT_rows(const double* A, int64_t lda, const double* u, int64_t m, int K, double* partial,
                             double* out, hipStream_t st);

// MERR log-posterior pass (fsnap_merr.hip).  method: MERR_IID / MERR_ABC (MERR_FULL is computed as MERR_IID);
// cq[2K] = [c | q] on the device; out[2K + 1] = [g | h | val].  Scratch: partial[merr_num_blocks(m, K)][2K + 1]; for
// K > MERR_ONE_PASS_MAX_K also u[2m] (per-row alpha w, beta w^2) and val_part[merr_num_blocks(m, K)]
constexpr int MERR_IID = 0, MERR_ABC = 1, MERR_FULL = 2;
constexpr int MERR_ONE_PASS_MAX_K = 288;
int merr_num_blocks(int64_t m, int K);
hipError_t launch_merr(const double* A, int64_t lda, const double* cq, int64_t m, int K, const double* b, const double* w,
                       const unsigned char* mask, int method, double d, double* u, double* val_part, double* partial,
                       double* out, hipStream_t st);

// Weighted residual sums of up to SSE_MAX_P coefficient vectors (fsnap_mcmc.hip, kernels S1 / S1G).  Up: the vectors packed by
// sse_pack_u (host) into the MFMA operand order, 4 ceil(K / 16) x 64 doubles, on the device.  out[SSE_MAX_P + 1] =
// [sse_0 .. sse_15 | n] (slots past P are zero).  Scratch: partial[sse_num_blocks(m)][SSE_MAX_P + 1].  m >= 1.
constexpr int SSE_MAX_P = 16;
int sse_num_blocks(int64_t m);
void sse_pack_u(const double* U, int P, int K, double* Up);
hipError_t launch_sse_batch(const double* A, int64_t lda, int64_t m, int K, const double* Up, const double* b, const double* w,
                            const unsigned char* mask, double* partial, double* out, hipStream_t st);

// Batched candidate fits (fsnap_cand.hip).  Rows are gathered through an index sorted by category and cut into chunks of
// at most CAT_CHUNK_ROWS rows of one category; every chunk has at least one row.
struct CatChunk {
    int64_t first;   // position of the chunk's first row in the sorted index
    int32_t cat;     // category of all its rows
    int32_t count;   // rows, 1 ... CAT_CHUNK_ROWS
};
constexpr int CAT_CHUNK_ROWS = 1024;
// doubles of one chunk's partial of kernel C1: tile triangle [pair][4][64] | c [NT * 16] | scalars [3]
int cat_partial_doubles(int K);
// kernel C1 / C1G: part[chunk][NT (NT + 1) / 2][4][64], cpart[chunk][NT * 16], spart[chunk][3] (NT = ceil(K / 16))
hipError_t launch_cat_syrk(const double* A, int64_t lda, const double* b, const double* w0, const int* idx,
                           const CatChunk* chunks, int64_t nchunks, int K, double* part, double* cpart, double* spart,
                           hipStream_t st);
// kernel C1R: stats[c][K^2 + K + 3] = packed [G | c | b^T W^2 b, sum wb, n_train] of category c; cbeg[ncat + 1] = first chunk
hipError_t launch_cat_reduce(const double* part, const double* cpart, const double* spart, const int* cbeg, int ncat, int K,
                             double* stats, hipStream_t st);
// kernel C2: out[p][K^2 + K + 3] = sum_c S[p][c]^2 stats[c] (S[p][c] for sum wb, 1 for n_train)
hipError_t launch_cand_combine(const double* stats, const double* S, int P, int ncat, int K, double* out, hipStream_t st);
// kernel C3: at most CAND_ROWS_MAX_P candidates per launch, betaT[ceil(K / 8) * 8][16] (zero-padded);
// what = 0: error sums over the chunks of all rows, what = 1: refinement right-hand sides over the training chunks.
// partial: cand_rows_partial_doubles(what, K) doubles per chunk
constexpr int CAND_ROWS_MAX_P = 16;
int64_t cand_rows_partial_doubles(int what, int K);
hipError_t launch_cand_rows(int what, const double* A, int64_t lda, const double* b, const double* w0, const int* idx,
                            const CatChunk* chunks, int64_t nchunks, int K, const double* betaT, double* partial,
                            hipStream_t st);
// kernel C3R for the np candidates p0 ... p0 + np - 1 of one launch: what = 0: out[p][ncat][4] sums; what = 1: out[p][K] =
// sum_c S[p][c]^2 s_c (S: [P][ncat] on the device)
hipError_t launch_cand_reduce(int what, const double* partial, const int* cbeg, const double* S, int ncat, int np, int p0,
                              int K, double* out, hipStream_t st);

// Predictive variance of rows (fsnap_uq.hip).  Mp: device, Kp x Jp row-major with Kp = 16 ceil(K / 16), Jp = 16 ceil(J / 16),
// zero outside the K x J matrix; bp: device, Kp doubles (beta, zero-padded), read only when preds != nullptr.
// var[m] (may be nullptr): QUAD a^T M a (J = K), NORM ||a M||^2; preds[m] (may be nullptr): a . beta.
constexpr int UQ_QUAD = 0;
constexpr int UQ_NORM = 1;
hipError_t launch_uq_rows(int mode, const double* A, int64_t lda, int64_t m, int K, const double* Mp, int Jp, const double* bp,
                          double* var, double* preds, hipStream_t st);
// kernels U2 + U3: per-category sum / max of scale_i var_i (scale may be nullptr) over the chunks of a category-sorted index
// (fsnap_cat_chunks); part: 2 nchunks doubles of scratch; cbeg[ncat + 1] = first chunk of each category; cat_sum / cat_max
// (ncat, either may be nullptr)
hipError_t launch_uq_cat(const double* var, const double* scale, const int* idx, const CatChunk* chunks, int64_t nchunks,
                         const int* cbeg, int ncat, double* part, double* cat_sum, double* cat_max, hipStream_t st);

// Greedy batch selection (fsnap_select.hip).  Kernel B1 / B1G: var[i] -= ||a_i V||^2 in place (Vp: device, Kp x Jp row-major,
// zero-padded as Mp of launch_uq_rows; the subtracted value has the bits of launch_uq_rows in NORM mode).
hipError_t launch_sel_rows(const double* A, int64_t lda, int64_t m, int K, const double* Vp, int Jp, double* var,
                           hipStream_t st);
// kernels B2 + B3: launch_uq_cat over the categories with alive[c] != 0 (the others keep their cat_sum / cat_max)
hipError_t launch_sel_scores(const double* var, const double* scale, const int* idx, const CatChunk* chunks, int64_t nchunks,
                             const int* cbeg, const int* alive, int ncat, double* part, double* cat_sum, double* cat_max,
                             hipStream_t st);
// kernel B4: out[0] = best score over the live categories (SEL_SUM: cat_sum, SEL_MAX: cat_max, SEL_MEAN: cat_sum / count),
// out[1] = its category as a double (ties: the lowest id; -1: none alive); retire != 0 clears alive[] of the winner
constexpr int SEL_SUM = 0;
constexpr int SEL_MAX = 1;
constexpr int SEL_MEAN = 2;
hipError_t launch_sel_pick(const double* cat_sum, const double* cat_max, const int64_t* count, int* alive, int ncat,
                           int objective, int retire, double* out, hipStream_t st);

// Leave-one-configuration-out predictions (fsnap_loco.hip).  Kernel L1: for the npos positions of the sorted row index idx,
// Z[p] = a_idx[p] M (Jp doubles per position; Mp: device, Kp x Jp row-major, zero-padded as for launch_uq_rows), pb[p] =
// a . beta (bp: Kp doubles), pw[p] = w_eff, pe[p] = w_eff b - w_eff (a . beta) from wpack (kernel 1A's pairs).
hipError_t launch_loco_zeta(const double* A, int64_t lda, int K, const int* idx, int64_t npos, const double* wpack,
                            const double* Mp, int Jp, const double* bp, double* Z, double* pw, double* pe, double* pb,
                            hipStream_t st);
// Kernel L2 over the configurations clist[ncl] (positions off[c] .. off[c + 1]); D = 32 / 64 / 128: d_c = min(n_c, J) <= D,
// H in LDS; D = 0: any d_c <= dmax, H in Hg (nblocks x loco_scratch_doubles(dmax)).  vg: nblocks x Jp doubles of scratch.
// pred[idx[p]] = LOO prediction (NaN for a configuration that is not identifiable); info[4 c ..] = (d_c, smallest pivot,
// identifiable, n space).
constexpr int LOCO_MAX_LDS_D = 128;
constexpr double LOCO_PIVOT_TOL = 1e-10;     // pivots of I - S_c (diagonal <= 1) at or below this: not identifiable
// One workgroup's slice of Hg (D = 0), in doubles, for the host that sizes Hg and the kernel that indexes it: H (dmax x dmax)
// and one dmax-vector (kernels L2 and J2), or three (kernels L3 and I1)
constexpr int64_t loco_scratch_doubles(int64_t dmax) { return dmax * dmax + dmax; }
constexpr int64_t loco_uq_scratch_doubles(int64_t dmax) { return dmax * dmax + 3 * dmax; }
hipError_t launch_loco_cfg(int D, int nblocks, const double* Z, int Jp, int J, const double* pw, const double* pe,
                           const double* pb, const int* idx, const int64_t* off, const int* clist, int ncl, double* Hg,
                           int dmax, double* vg, double* pred, double* info, hipStream_t st);
// Kernel L3 (fsnap_loco_uq.hip): launch_loco_cfg's geometry and predictions (bit for bit), plus lev[idx[p]] = the leave-out
// leverage q_i of every row (NaN for a configuration that is not identifiable) and info[6 c ..] = (d_c, smallest pivot,
// identifiable, n space, log det H_c, e_c^T H_c^-1 e_c; the last two NaN when not identifiable).  D = 0: Hg holds
// nblocks x loco_uq_scratch_doubles(dmax).
hipError_t launch_loco_uq_cfg(int D, int nblocks, const double* Z, int Jp, int J, const double* pw, const double* pe,
                              const double* pb, const int* idx, const int64_t* off, const int* clist, int ncl, double* Hg,
                              int dmax, double* vg, double* pred, double* lev, double* info, hipStream_t st);

// Influence vectors and outer-product sums (fsnap_influence.hip).  Kernel I1: launch_loco_cfg's geometry, predictions and info
// (bit for bit), plus per unit c of the list V[c Jp ..] = v_c (zeros when not identifiable), S[c Jp ..] = s_c = Z_c^T e_c and
// unit[3 c ..] = (|v_c|^2, |s_c|^2, s_c . v_c) (first and third NaN when not identifiable); columns J ... Jp - 1 of V and S are
// written as zeros.  D = 0: Hg holds nblocks x loco_uq_scratch_doubles(dmax).
hipError_t launch_infl_cfg(int D, int nblocks, const double* Z, int Jp, int J, const double* pw, const double* pe,
                           const double* pb, const int* idx, const int64_t* off, const int* clist, int ncl, double* Hg,
                           int dmax, double* vg, double* pred, double* info, double* V, double* S, double* unit,
                           hipStream_t st);
// Kernel I0: S[c Jp ..] and unit[3 c ..] = (NaN, |s_c|^2, NaN) of the units clist[ncl] from kernel L1's Z, pw, pe alone; the bits
// of kernel I1's S and |s_c|^2.
hipError_t launch_infl_scores(int nblocks, const double* Z, int Jp, int J, const double* pw, const double* pe,
                              const int64_t* off, const int* clist, int ncl, double* S, double* unit, hipStream_t st);
// Kernel I2 and its fold: W (J x J, device) = X^T X of X (nunits x Jp, device; columns >= J are ignored), chunks of INFL_CHUNK
// units in index order.  part: infl_chunks(nunits) x (Jp / 16)(Jp / 16 + 1) / 2 x 256 doubles of scratch.  nunits <= 0: nothing is
// launched (W is left alone).
constexpr int INFL_CHUNK = 512;
inline int64_t infl_chunks(int64_t nunits) { return (nunits + INFL_CHUNK - 1) / INFL_CHUNK; }
hipError_t launch_infl_outer(const double* X, int64_t nunits, int Jp, int J, double* part, double* W, hipStream_t st);

// Leave-one-unit-out refits over a grid of alphas (fsnap_path.hip, kernel P1; K <= PATH_MAX_K).  For every unit u (positions
// off[u] .. off[u + 1] of idx) and alpha_q: beta = (G - G_u + alpha_q I)^-1 (c - c_u) by a Jacobi-scaled blocked Cholesky,
// sums[((q nunits + u) nclass + cls) 4 ..] = (n, sum |r|, sum r^2, sum (w r)^2) of r_i = b_i - a_i . beta over the unit's rows
// of class rcls[row] = cls, info[(q nunits + u) 2 ..] = (smallest pivot, identifiable 1 / 0), pred[q m + row] = a_i . beta
// (pred may be nullptr; NaN for a unit that is not identifiable at alpha_q).  Units without rows get zero sums and info (inf, 1).  G, c,
// alphas: device.  Bg: nblocks x path_base_doubles(K) doubles of scratch.
constexpr int PATH_MAX_K = 144;
constexpr int PATH_QCHUNK = 16;
constexpr int PATH_MAX_CLASS = 8;
inline size_t path_base_doubles(int K) { return (size_t)((K + 15) / 16) * (size_t)((K + 15) / 16 + 1) / 2 * 256; }
int path_blocks_per_cu(int K);
hipError_t launch_ridge_path(int nblocks, const double* A, int64_t lda, int K, const double* wpack, const double* b,
                             const int* idx, const int64_t* off, int nunits, const double* G, const double* c,
                             const double* alphas, int Q, const unsigned char* rcls, int nclass, double* Bg, double* sums,
                             double* info, double* pred, int64_t m, hipStream_t st);

// The fold sums of the grouped K-fold paths (kernel S1, in fsnap_lasso.hip; shared by the LASSO, ARD and OMP paths): folds[f]
// (F packed blocks of K^2 + K + 3 doubles; nullptr with nsub = 1, where the blocks of stats are the folds) = the sum of blocks
// f nsub ... f nsub + nsub - 1 of stats, total = the sum of the folds, both in index order.
hipError_t launch_fold_sums(const double* stats, int F, int nsub, int K, double* folds, double* total, hipStream_t st);
// Grouped K-fold LASSO alpha paths (fsnap_lasso.hip; K <= LASSO_MAX_K).
constexpr int LASSO_MAX_K = 144;
// Kernel S2: problem p = f Q + q (f = F: no fold left out) is fsnap_lasso_gram on (total - folds[f]) with l1_reg = alphas[q] n,
// from zeros; a coordinate j with total G_jj = 0 or downdated G_jj <= LOCO_PIVOT_TOL total G_jj is skipped.  coef[p][K],
// info[p][4] = (sweeps, last duality gap, l1_reg, n), heldout[p][3] (p < F Q) = (n_f, bb_f - 2 beta . c_f + beta^T G_f beta, bb_f).
// One wave per workgroup, nblocks workgroups stride over the problems.  All pointers: device.
size_t lasso_lds_bytes(int K);
int lasso_blocks_per_cu(int K);
hipError_t launch_lasso_cd(int nblocks, const double* folds, const double* total, const double* alphas, int K, int F, int Q,
                           int max_iter, double tol, double* coef, double* info, double* heldout, hipStream_t st);

// Grouped K-fold ARD threshold paths (fsnap_ard.hip; K <= ARD_MAX_K) on the folds and the total of kernel S1.  Kernel A1:
// problem p = f Q + q (f = F: no fold left out) is ARD._ard_loop on (total - folds[f]) with hyper[p][6] = (alpha_1, alpha_2,
// lambda_1, lambda_2, threshold_lambda, alpha_init), the inverse of every iteration from a Cholesky factor of the equilibrated
// matrix of the kept columns and the residual sum of squares from the statistics; a column j with total G_jj = 0 or downdated
// G_jj <= LOCO_PIVOT_TOL total G_jj is never kept.  coef[p][K], lambda[p][K], info[p][6] = (iterations, kept columns, final
// alpha_, last sum |coef_old - coef|, smallest pivot, status 0 converged or emptied / 1 failed / 2 max_iter reached),
// heldout[p][3] (p < F Q) = (n_f, bb_f - 2 beta . c_f + beta^T G_f beta, bb_f).  One workgroup of 256 threads per problem,
// nblocks workgroups stride over the problems.  All pointers: device.
constexpr int ARD_MAX_K = 144;
size_t ard_lds_bytes(int K);
int ard_blocks_per_cu(int K);
hipError_t launch_ard_path(int nblocks, const double* folds, const double* total, const double* hyper, int K, int F, int Q,
                           int max_iter, double tol, double* coef, double* lambda, double* info, double* heldout, hipStream_t st);

// Grouped K-fold greedy forward-selection paths (fsnap_omp.hip; K <= OMP_MAX_K, S <= OMP_MAX_S) on the folds and the total of
// kernel S1.  Kernel O1: problem f (f = F: no fold left out) is fsnap_omp_gram on (total - folds[f]) with diag_ref = the
// total's diagonal, statement for statement: order[f][S], path[f][S][3] = (e_s, score, pivot), coef[f][Q][K] at the steps
// levels[Q] (ascending, 1 ... S), heldout[f][S][3] (f < F) = (n_f, bb_f - 2 beta . c_f + beta^T G_f beta, bb_f) after every
// step.  forced[nforced] (may be nullptr with nforced = 0) and levels: device.  One wave per workgroup, nblocks workgroups
// stride over the problems; LDS holds W (S rows of an odd stride >= K), z, beta and one dense coefficient row.
constexpr int OMP_MAX_K = 144;
constexpr int OMP_MAX_S = 128;
size_t omp_lds_bytes(int K, int S);
int omp_blocks_per_cu(int K, int S);
hipError_t launch_omp_path(int nblocks, const double* folds, const double* total, int K, int F, int criterion, const int* forced,
                           int nforced, int S, const int* levels, int Q, int* order, double* path, double* heldout, double* coef,
                           hipStream_t st);

// Grouped K-fold BCS sparsity paths (fsnap_bcs.hip; K <= BCS_MAX_K, max_active <= min(K, BCS_MAX_ACTIVE)) on the folds and the
// total of kernel S1.  Kernel B1: problem p = f Q + q (f = F: no fold left out) is fsnap_bcs_gram's recurrence on (total -
// folds[f]) with diag_ref = the total's diagonal and hyper[q][4] = (sigma2 or 0, scale, eta, itermax); sigma2 = 0 takes scale x
// the variance of the problem's own rows.  coef[p][K], active[p][max_active] (-1 past the active set), alpha and
// errbars[p][max_active] by position, picks[p][P][2] (P >= every itermax), info[p][6] = (iterations, status 0 ended / 1 failed /
// 2 itermax reached, sigma2 used, sigma2 re-estimated, rss, margin), heldout[p][3] (p < F Q) = (n_f, bb_f - 2 beta . c_f +
// beta^T G_f beta, bb_f), sig[q][max_active][max_active] of the f = F problems.  exact: 0 = the reference's deletion, 1 = Tipping
// & Faul's.  One workgroup of 256 threads per problem, nblocks workgroups stride over the problems.  All pointers: device.
constexpr int BCS_MAX_K = 144;
constexpr int BCS_MAX_ACTIVE = 64;
size_t bcs_lds_bytes(int K, int max_active);
int bcs_blocks_per_cu(int K, int max_active);
hipError_t launch_bcs_path(int nblocks, const double* folds, const double* total, const double* hyper, int K, int F, int Q,
                           int max_active, int P, int exact, double* coef, int* active, double* alpha, double* errbars, int* picks,
                           double* info, double* heldout, double* sig, hipStream_t st);

// Grouped K-fold spectral paths (fsnap_spectral.hip; K <= SPEC_MAX_K) on the folds and the total of kernel S1.  Kernel E1:
// problem f (f = F: no fold left out) is the Jacobi eigendecomposition of the live block of (total - folds[f]) under the
// round-robin ordering of fsnap_spectral_body.h: eig[f][K] and z[f][K] ascending (zero past n_live), V[f][K][K] (row r < n_live:
// eigenvector r in the K original coordinates), info[f][6] = (n_live, sweeps, final off / diag ratio, lambda_max, smallest
// lambda, status 0 converged / 2 sweep cap).  vwork: nblocks x K^2 doubles of scratch (read and written only where
// spectral_vectors_in_lds(K) is false).  Kernel E2: work item (f, slice of 16 settings) evaluates the settings (alphas[q],
// rconds[q]), q < Q: set[f][Q][3] = (rank, dof, sse), fit[Q][K] (f = F), coef[F][Q][K] (may be nullptr), held[F][Q][nsub][3] =
// (n_{f,s}, bb_{f,s} - 2 beta . c_{f,s} + beta^T G_{f,s} beta, bb_{f,s}) against block f nsub + s of stats.  One workgroup (E1: 1024
// threads, E2: 256) per problem / work item, nblocks workgroups stride over them.  All pointers: device.
constexpr int SPEC_MAX_K = 144;
size_t spectral_eig_lds_bytes(int K);
bool spectral_vectors_in_lds(int K);
int spectral_eig_blocks_per_cu(int K);
size_t spectral_eval_lds_bytes(int K);
int spectral_eval_blocks_per_cu(int K);
int spectral_slices(int Q);
hipError_t launch_spectral_eig(int nblocks, const double* folds, const double* total, int K, int F, double* vwork, double* eig,
                               double* z, double* V, double* info, hipStream_t st);
hipError_t launch_spectral_eval(int nblocks, const double* stats, const double* folds, const double* total, const double* eig,
                                const double* z, const double* V, const double* info, const double* alphas, const double* rconds,
                                int K, int F, int nsub, int Q, double* set, double* fit, double* coef, double* held,
                                hipStream_t st);

// Grouped K-fold cross-validation of weight candidates (fsnap_cv.hip; V1: K <= CV_MAX_K) on the F * C packed blocks of
// fsnap_cat_normal_eq with composite category f * C + c.  Kernel V0: total[c] = sum_f stats[f * C + c], folds in index order,
// and rest[f * C + c] = total[c] - stats[f * C + c] (F C blocks).
// Kernel V1: problem p * F + f is the Jacobi-scaled Cholesky solve of Qm + alpha I, Qm = sum_c S[p][c]^2 rest[f * C + c]
// (c ascending, one fma per term), over the live columns (dead: sum_c S^2 total[c].G_jj == 0 or Qm_jj <=
// LOCO_PIVOT_TOL times it); a scaled pivot that is not > LOCO_PIVOT_TOL ends the problem with status 1 and NaN coefficients.
// coef[P F][K], info[P F][4] = (status, smallest scaled pivot, live columns, sum_c S^2 (total.n - stats.n)).  One workgroup
// of 256 threads per problem, nblocks workgroups stride over the problems.  Kernel V2: the chunks of the layout times the
// coefficient table of their fold, betaT[F][K8][16] (K8 = K rounded up to 8; zero-padded), partials as launch_cand_rows
// (what = 0) leaves them, for launch_cand_reduce (what = 0) with ncat = F C.  All pointers: device.
constexpr int CV_MAX_K = 144;
size_t cv_lds_bytes(int K);
int cv_blocks_per_cu(int K);
hipError_t launch_cv_total(const double* stats, int F, int C, int K, double* total, double* rest, hipStream_t st);
hipError_t launch_cv_solve(int nblocks, const double* rest, const double* total, const double* S, int P, int F, int C, int K,
                           double alpha, double* coef, double* info, hipStream_t st);
hipError_t launch_cv_rows(const double* A, int64_t lda, const double* b, const double* w0, const int* idx, const CatChunk* chunks,
                          int64_t nchunks, int K, int C, const double* betaT, double* partial, hipStream_t st);

// Gradient of the cross-validated cost over the candidates' scales (fsnap_cvgrad.hip, K <= CV_MAX_K), on the blocks stats[f * C + c]
// and rest[f * C + c] above.  Candidates come in tiles of 16: betaT / lamT[tile][f][K8][16] (K8 = K rounded up to 8) and
// omegaT[tile][C][16] are zero-padded tables, candidate 16 tile + e in slot e.
// Kernel G1 (RHS epilogue):      g[(16 tile + e) F + f][K] = 2 sum_c omega[c][e] (stats[f C + c].G beta[f][.][e] - stats[f C + c].r)
//                                (the categories in four contiguous quarters of ceil(C / 4), each c ascending, added in index order)
// Kernel G2: problem p F + f is kernel V1's system with g as the right-hand side: lam[P F][K] (0 on dead columns, NaN with status
//            1), the same value into lamT, info[P F][2] = (status, smallest scaled pivot)
// Kernel G1 (bilinear epilogue): D[((tile F + f) C + c) 16 + e] = lam[f][.][e] . (rest[f C + c].r - rest[f C + c].G beta[f][.][e])
// All pointers: device.
hipError_t launch_cvgrad_rhs(const double* stats, const double* betaT, const double* omegaT, int P, int F, int C, int K, double* g,
                             hipStream_t st);
hipError_t launch_cvgrad_solve(int nblocks, const double* rest, const double* total, const double* S, const double* g, int P, int F,
                               int C, int K, double alpha, double* lam, double* lamT, double* info, hipStream_t st);
hipError_t launch_cvgrad_bilinear(const double* rest, const double* betaT, const double* lamT, int P, int F, int C, int K, double* D,
                                  hipStream_t st);

// Marginal likelihood of weight candidates (fsnap_evidence.hip, K <= CV_MAX_K) on the C packed blocks stats[c] of fsnap_cat_normal_eq.
// S[P][C]: the scales, 0 for the categories that take no part.  Candidates come in tiles of 8 = 16 table columns:
// tab[ceil(P / 8)][K^2 + K + 3][16], column 2 (p % 8) = [H^-1 scattered to K x K, zeros at dead columns | 0_K | 0, 0, 0], column
// 2 (p % 8) + 1 = [beta beta' | -2 beta | 1, 0, 0]; the columns of a last tile without a candidate must be zeroed by the caller.
// Kernel E1: kernel V1's Jacobi-scaled Cholesky solve of H = sum_c S[p][c]^2 stats[c].G + alpha I on the live columns (dead:
//            the combined diagonal is 0), log|H|, the in-place inverse; beta[P][K], info[P][6] = (status, smallest scaled pivot,
//            live columns, log|H|, tr(H^-1), 0), the table columns.  nblocks workgroups of 256 threads stride over the candidates.
// Kernels E2 + E3: Y[pt][c][16] = sum_e stats[c][e] tab[pt][e][.], the elements in slices of EV_SLICE (partials in
//            part[ceil(C / 16) ceil(P / 8) evidence_slices(K)][256]), the slices added in index order.  All pointers: device.
constexpr int EV_SLICE = 512;
int evidence_slices(int K);
hipError_t launch_evidence_factor(int nblocks, const double* stats, const double* S, int P, int C, int K, double alpha, double* beta,
                                  double* info, double* tab, hipStream_t st);
hipError_t launch_evidence_sweep(const double* stats, const double* tab, int P, int C, int K, double* part, double* Y,
                                 hipStream_t st);

// Joint unit scores (fsnap_joint.hip).  Kernel J1: for the npos positions of the unit-sorted row index idx,
// ZP[p] = om[p] a_idx[p] [M | M B] (Wp doubles per position; Fp: device, Kp x Wp row-major, zero-padded: columns [0, Jp) the
// factor M, columns [Jp, Wp) the target block M B; Wp = Jp without a target; om: the weight of every position).
hipError_t launch_joint_rows(const double* A, int64_t lda, int K, const int* idx, int64_t npos, const double* om,
                             const double* Fp, int Wp, double* ZP, hipStream_t st);
// Kernel J2 for the ncl units of ulist (D = 32 / 64 / 128: S in LDS for dim S = min(n_u, J) <= D; D = 0: S in a slice of
// loco_scratch_doubles(dmax) of Sg per workgroup, the right-hand-side fragments in joint_yslice(dmax) doubles of Yg per workgroup):
// S = I + Z Z^T / tau (n_u <= J) or I + Z^T Z / tau = L L^T; out[2 u] = gain = sum log L_ii; out[2 u + 1] = reduction (only
// with rp > 0) = ||L^-1 Pi||_F^2 / tau (n space; Pi = columns [Jp, Jp + rp) of ZP) or ||B||_F^2 - ||L^-1 B||_F^2 (J space; Bp:
// device, Jp x rp row-major, zero-padded); info[4 u ..] = (dim S, n space 1 / 0, smallest pivot, n_u).
constexpr int JOINT_MAX_LDS_D = 128;
constexpr int64_t joint_yslice(int64_t dmax) { return 4 * ((dmax + 15) / 16) * 4 * 64; }
hipError_t launch_joint_units(int D, int nblocks, const double* ZP, int Wp, int Jp, int J, int rp, const double* Bp, double tau,
                              const int64_t* off, const int* ulist, int ncl, double* Sg, int dmax, double* Yg, double* out,
                              double* info, hipStream_t st);

// Robust M-estimator fits by IRLS (fsnap_robust.hip).  pcat[m]: class of every participating row (training row with w > 0),
// -1 for the others (kernel R0).  Kernel R1 / R3 (launch_robust_rows): e_in == nullptr: e_out[i] = w_i (b_i - a_i . beta) from
// one pass over A; e_in != nullptr: A, beta, b are not read.  do_weights: r_out[i] = sqrt(omega), wr_out[i] = w_i r_i (rows that
// do not take part: r = 1, w r = w) and sums[ncat][6] = (n, rows with r < 1, rows with r = 0, sum omega, sum e^2, sum rho) per
// class, from scale[ncat] on the device; partial: robust_num_blocks(m, K) x ncat x 6 doubles of scratch.  A launch with the
// rows and one without them give the same bits when m and K agree.  1 <= ncat <= ROBUST_MAX_CLASSES.
constexpr int ROBUST_HUBER = 0, ROBUST_BISQUARE = 1, ROBUST_CAUCHY = 2;
constexpr int ROBUST_MAX_CLASSES = 32;
int robust_num_blocks(int64_t m, int K);
hipError_t launch_robust_pcat(const double* w, const unsigned char* mask, const int* cat, int64_t m, int* pcat, hipStream_t st);
hipError_t launch_robust_rows(const double* A, int64_t lda, const double* beta, int64_t m, int K, const double* b, const double* w,
                              const int* pcat, const double* e_in, double* e_out, bool do_weights, int loss, double c,
                              const double* scale, double* r_out, double* wr_out, double* partial, double* sums, int ncat,
                              hipStream_t st);
// Kernel R2: exact per-class medians of |e| by radix selection over the 8 bytes of the bit pattern.  state:
// robust_state_bytes(ncat) bytes on the device, zeroed before pass 0.  Per pass: launch_robust_hist (m = 0: nothing), then --
// in a communicator -- launch_robust_table_to_double, an all-reduce of robust_table_doubles() (512 ncat doubles), and
// launch_robust_choose (summed = the doubles hold the counts).  After pass 7 robust_scale_ptr() holds 1.4826 x median per class
// (0 for an empty class) and robust_count_ptr() the rows per class.
size_t robust_state_bytes(int ncat);
hipError_t launch_robust_hist(const double* e, const int* pcat, int64_t m, int pass, int ncat, void* state, hipStream_t st);
hipError_t launch_robust_table_to_double(void* state, int ncat, hipStream_t st);
hipError_t launch_robust_choose(void* state, int pass, int ncat, bool summed, hipStream_t st);
double* robust_table_doubles(void* state, int ncat);
double* robust_scale_ptr(void* state, int ncat);
long long* robust_count_ptr(void* state, int ncat);

// Row-space solve (fsnap_trsm.hip).  Q <- X R^-1 by blocked substitution over the columns, one wave per 64 rows:
// first pass X = diag(w_eff) A (src = A, leading dimension lds, per-row pairs wpack = (w_eff, w_eff b); rows with
// w_eff = 0 become zero rows), later passes X = Q in place (src = Q, wpack = nullptr).  R: device, K16 x K16 row-major
// upper triangular, K16 = K rounded up to 16, identity in the padding, FOLLOWED by the inverses of its K16 / 16 diagonal
// 16 x 16 blocks ([block][16][16], row-major, upper triangular: what kernel 13B multiplies by and refines against):
// trsm_factor_doubles(K16) doubles in all, the second part filled by trsm_invert_diagonal_blocks on the host.
inline size_t trsm_factor_doubles(int K16) { return (size_t)K16 * K16 + (size_t)K16 * 16; }
inline void trsm_invert_diagonal_blocks(double* Rpad, int K16) {
    double* inv = Rpad + (size_t)K16 * K16;
    for (int jb = 0; jb < K16 / 16; ++jb) {
        const double* T = Rpad + (size_t)(jb * 16) * K16 + jb * 16;      // T[i][j] = T[i * K16 + j]
        double* X = inv + (size_t)jb * 256;
        // X = T^-1 column by column: T x_c = e_c, back substitution (x_c has zeros below row c)
        for (int c = 0; c < 16; ++c) {
            for (int i = 15; i >= 0; --i) {
                double v = (i == c) ? 1.0 : 0.0;
                for (int k = i + 1; k <= c; ++k) v -= T[(size_t)i * K16 + k] * X[k * 16 + c];
                X[i * 16 + c] = (i <= c) ? v / T[(size_t)i * K16 + i] : 0.0;
            }
        }
    }
}
hipError_t launch_trsm_rows(const double* src, int64_t lds, const double* wpack, double* Q, int64_t ldq, int64_t m, int K,
                            const double* R, int K16, hipStream_t st);
// launch_trsm_rows = trsm_family (the rule that picks the kernel from the shape) + launch_trsm_family (the launcher of a
// named family: kernel 13C, K16 <= 144; kernel 13B with 16-row tiles (TR = 1, KG = 64) or 32-row tiles (TR = 2, KG = 16),
// K16 > 128).  A family that the rule can never pick at K16 is refused (hipErrorInvalidValue).  fsnap_trsm_pass hands the
// tests a single pass of a named family.
enum : int { TRSM_ACC2 = 1, TRSM_PANEL16 = 2, TRSM_PANEL32 = 3 };
int trsm_family(int64_t m, int K16);
hipError_t launch_trsm_family(int family, const double* src, int64_t lds, const double* wpack, double* Q, int64_t ldq, int64_t m,
                              int K, const double* R, int K16, hipStream_t st);
// qpack[row] = (w_eff != 0 ? 1 : 0, w_eff b): per-row pairs that make the SYRK kernels compute Q^T Q and Q^T (w b)
hipError_t launch_qpack(const double* wpack, int64_t m, double* qpack, hipStream_t st);

}  // namespace fsnap
