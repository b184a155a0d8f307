// fsnap_capi.cpp — the C-ABI layer of libfsnap_hip.so (declared in include/fsnap_hip.h).
// Owns the device-resident copy of the reference's shared arrays a / b / w
// (fitsnap3lib/parallel_tools.py:352-389, calculator.py:287-289), the training mask
// derived from fitsnap_dict['Testing'] (svd.py:35-40), launch geometry, HIP-event
// timing, and error text.  All compute is in fsnap_syrk.hip / fsnap_rows.hip / fsnap_chol.hip; the host K x K solve in
// fsnap_solve.cpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <atomic>
#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <limits>
#include <new>
#include <queue>
#include <string>
#include <thread>
#include <vector>

#include "../../include/fsnap_hip.h"
#include "fsnap_kernels.h"

// fsnap_solve with a contiguous copy of diag(G) (fsnap_solve.cpp; not part of the public ABI)
extern "C" int fsnap_solve_diag_tagged(int kind, double param, int64_t K, const double* G, const double* c, const double* diag,
                                       double* beta, int* rank, double* rcond_est, int upper, const void* owner,
                                       unsigned long long generation);
extern "C" int fsnap_solve_diag_upper(int kind, double param, int64_t K, const double* G, const double* c, const double* diag,
                                      double* beta, int* rank, double* rcond_est);
extern "C" int fsnap_solve_diag(int kind, double param, int64_t K, const double* G, const double* c, const double* diag,
                                double* beta, int* rank, double* rcond_est);
extern "C" void fsnap_cond_note(double min_pivot, double lambda_min, int steps, int where);
extern "C" double fsnap_gen_eig_max(const double* M, const double* N, int k);

#include "fsnap_ctx.h"
#include "fsnap_condest.h"

namespace fsnap {
std::string& library_error() {
    static thread_local std::string text;
    return text;
}
}  // namespace fsnap

#define g_last_error (fsnap::library_error())

namespace {

// process-wide fill counter of the host mirrors: a (context, generation) tag is never reused, not even by a context that is
// created at the address of a destroyed one
unsigned long long next_mirror_generation() {
    static std::atomic<unsigned long long> counter{0};
    return ++counter;
}

// the one rule for "fsnap_solve_device factorises this K x K system on the GPU" (blocked kernels 8a-8s): launch_normal_eq and
// fsnap_mirror_packed skip the host mirror then, fsnap_solve_device_rhs takes the device path
inline bool device_factor(const fsnap_ctx* ctx, int64_t K) {
    if (ctx->opt_device_solve == 2) return false;
    return K >= fsnap::DEVICE_CHOL_MIN_K || (K > 128 && ctx->opt_device_solve == 1);
}

struct Geometry {
    int nblocks, split, threads;
    int64_t cpw;
    int NB;
    bool acc;       // kernel 1A: whole triangle in one wave (accumulation registers), one wave per SIMD
    bool packed;    // kernel 1P (K <= 80)
    bool fused_pack = false;   // kernel 1A packs (w_eff, w_eff b) of its rows into LDS itself: no fsnap_pack_weights_k launch
    bool quad = false;         // kernel 1Q: the triangle dealt to the four waves of a workgroup (144 < K <= 288); cpw = chunks per workgroup
    bool shortk = false;       // kernel 1S (80 < K <= 144, short systems): nblocks = chunks, cpw = ROWS per chunk, two workgroups per chunk
    int cluster = 1;           // kernel 1QC (288 < K <= 512): workgroups per cluster; nblocks = clusters, cpw = chunks per cluster
};

// rows below which the tiled kernel keeps 145 ... 288 columns: kernel 1Q writes one partial triangle per workgroup
// (2 KiB x 55 ... 171 tiles), which short systems do not amortise
constexpr int64_t QUAD_MIN_ROWS = 8192;
constexpr int64_t QUAD_MIN_CPG = 24;        // fewest 4-row chunks per workgroup before the grid shrinks (profiles/r05_quad_min_cpg_ab.txt)
// widest system the accumulator-resident kernel 1A takes (NB = 9 column blocks: the ACE width 142 of examples/Ta_PACE_RIDGE)
constexpr int64_t ACC_MAX_K = 144;
// longest system kernel 1S takes by default, in staging phases (128 rows, 112 at NB = 9) per workgroup with half the CUs' worth of
// chunks (two workgroups share a chunk): 43 008 ... 49 152 rows on 256 CUs.  Measured (profiles/r06_short_kernel.txt, kernel us,
// 1S | 1A): 13 035 x 142 18.3 | 32.1, 20 000 x 142 22.9 | 35.1, 28 672 x 142 25.2 | 36.7, 40 000 x 142 32.0 | 37.0 (x 128: 27.7 | 32.3,
// x 96: 23.3 | 22.8), 60 000 x 142 43.5 | 41.3, 125 000 x 128 62.4 | 55.2
constexpr int64_t SHORT_MAX_PHASES = 3;
constexpr int64_t SHORT_MIN_CHUNK_ROWS = 32;
constexpr int64_t ACC_MIN_CPW = 12;         // kernel 1A: fewest 4-row chunks per row-wave before its grid shrinks below one workgroup per CU
// kernel 1QC (289 ... 512 columns on clusters of workgroups) against the tiled kernel, round 5 (profiles/r05_quadc_ab.txt):
// 500 000 x 368 1.19 against 1.24 ms, 367 900 x 480 1.40 / 1.38 ms (with 1.43 instead of 6.14 GB of HBM reads and a 17 instead of
// 42 us reduction: the complete fit 1.61 / 1.62 ms), 200 000 x 320 0.41 / 0.37, 100 000 x 512 0.51 / 0.43: a cluster's partial
// triangle (up to 1 MiB) and its prologue want ~5 000 rows per cluster to amortise
constexpr int64_t QUADC_MIN_ROWS = 300000;

// chunks per workgroup of kernel 1Q (per CLUSTER of kernel 1QC, 288 < K <= 512) for this context's rows, 0 = neither kernel
// takes them
int64_t quad_chunks_per_wg(const fsnap_ctx* ctx, int64_t* nblocks_out) {
    if (ctx->opt_tiled) return 0;
    if (ctx->K <= ACC_MAX_K || ctx->K > 512) return 0;
    const int cluster = fsnap::syrk_quad_cluster((int)ctx->K);
    // kernel 1QC exists with fused packing only: pairs brought by a row-space pass, or rows beyond the LDS, stay on the tiled kernel
    if (cluster > 1 && (!ctx->opt_fused_pack || ctx->wpack_override)) return 0;
    const int64_t min_rows = ctx->opt_quad_min_rows >= 0 ? ctx->opt_quad_min_rows : (cluster > 1 ? QUADC_MIN_ROWS : QUAD_MIN_ROWS);
    if (ctx->m < min_rows || ctx->m < 4) return 0;
    const int64_t nchunks = (ctx->m + 3) / 4;
    int64_t nblocks = ctx->opt_nblocks > 0 ? ctx->opt_nblocks : (int64_t)ctx->num_cu;
    nblocks /= cluster;                                  // clusters
    const int64_t max_blocks = (nchunks + QUAD_MIN_CPG - 1) / QUAD_MIN_CPG;
    if (nblocks > max_blocks) nblocks = max_blocks;
    if (nblocks < 1) nblocks = 1;
    const int64_t cpg = (nchunks + nblocks - 1) / nblocks;
    const int64_t off_limit = (int64_t)0xFFF00000;
    if (cpg > off_limit / (ctx->lda * 32)) return 0;    // a workgroup's rows beyond 32-bit buffer offsets: tiled kernel
    if (cluster > 1 && cpg > fsnap::syrk_quad_max_cpg()) return 0;
    nblocks = (nchunks + cpg - 1) / cpg;
    if (nblocks_out) *nblocks_out = nblocks;
    return cpg;
}

inline bool use_tiled(const fsnap_ctx* ctx) {
    if (ctx->opt_tiled) return true;
    if (ctx->K <= ACC_MAX_K) return false;
    return quad_chunks_per_wg(ctx, nullptr) == 0;
}

int plan_geometry(fsnap_ctx* ctx, Geometry* g) {
    const int K = (int)ctx->K;
    const int64_t m = ctx->m;
    g->NB = fsnap::syrk_num_blocks(K);
    const int64_t off_limit = (int64_t)0xFFF00000;  // 32-bit buffer offsets, 1 MiB of slack for prefetch overshoot
    g->acc = false;
    g->packed = false;
    if (g->NB >= 10) {
        // kernel 1Q (use_tiled() sent everything else of this width to the tiled kernel)
        int64_t nblocks = 0;
        const int64_t cpg = quad_chunks_per_wg(ctx, &nblocks);
        if (cpg <= 0) return ctx->fail(FSNAP_E_ARG, "no accumulator-resident kernel for %d columns", K);
        g->nblocks = (int)nblocks;
        g->cpw = cpg;
        g->split = 1;
        g->threads = 256;
        g->quad = true;
        g->cluster = fsnap::syrk_quad_cluster(K);
        // fused packing: the workgroup's per-row pairs must fit the LDS; the row-space passes bring pairs of their own
        g->fused_pack = ctx->opt_fused_pack && !ctx->wpack_override && cpg <= fsnap::syrk_quad_max_cpg();
        return FSNAP_OK;
    }
    if (g->NB >= 6 && ctx->opt_short != 0 && (ctx->opt_short == 1 || m <= SHORT_MAX_PHASES * (int64_t)fsnap::syrk_short_phase_rows(K) * (ctx->num_cu / 2)) &&
        ctx->lda * 8 * (int64_t)136 + 16 <= (int64_t)0xFFFFF000) {
        // kernel 1S: chunks of rows staged through LDS, the triangle dealt over the 16 waves of the two workgroups of a chunk
        int64_t want = ctx->opt_nblocks > 0 ? ctx->opt_nblocks : std::max<int64_t>(1, (int64_t)ctx->num_cu / 2);
        int64_t rpc = ((m + want - 1) / want + 3) / 4 * 4;
        if (rpc < SHORT_MIN_CHUNK_ROWS) rpc = SHORT_MIN_CHUNK_ROWS;
        const int64_t nchunk = (m + rpc - 1) / rpc;
        if (rpc <= 0x7FFFFFF0 && nchunk <= 0x3FFFFFF) {
            g->nblocks = (int)nchunk;
            g->cpw = rpc;
            g->split = 1;
            g->threads = 512;
            g->shortk = true;
            g->fused_pack = ctx->opt_fused_pack && !ctx->wpack_override;
            return FSNAP_OK;
        }
    }
    if (g->NB >= 6) {
        // kernel 1A: one 4-wave workgroup per CU, every wave streams its own rows and owns the whole triangle
        const int64_t nchunks = (m + 3) / 4;
        int64_t nblocks = ctx->opt_nblocks > 0 ? ctx->opt_nblocks : (int64_t)ctx->num_cu;
        const int64_t max_blocks = (nchunks + 4 * ACC_MIN_CPW - 1) / (4 * ACC_MIN_CPW);   // >= ACC_MIN_CPW chunks per row-wave
        if (nblocks > max_blocks) nblocks = max_blocks;
        if (nblocks < 1) nblocks = 1;
        int64_t cpw = (nchunks + nblocks * 4 - 1) / (nblocks * 4);
        const int64_t max_cpw = off_limit / (ctx->lda * 32);
        if (max_cpw < 1) return ctx->fail(FSNAP_E_ARG, "leading dimension %lld too large", (long long)ctx->lda);
        if (cpw > max_cpw) cpw = max_cpw;
        nblocks = (nchunks + cpw * 4 - 1) / (cpw * 4);
        if (nblocks > 0x7FFFFFF) return ctx->fail(FSNAP_E_ARG, "too many workgroups");
        g->nblocks = (int)nblocks;
        g->cpw = cpw;
        g->split = 1;
        g->threads = 256;
        g->acc = true;
        // fused packing: the workgroup's per-row pairs must fit the LDS; the row-space passes bring pairs of their own
        g->fused_pack = ctx->opt_fused_pack && !ctx->wpack_override && cpw <= fsnap::syrk_acc_max_fused_cpw();
        return FSNAP_OK;
    }
    // K <= 80: kernel 1P
    g->packed = true;
    g->split = 1;
    g->threads = 256;
    const int64_t nchunks = (m + 3) / 4;
    // workgroups resident per CU: waves per SIMD the register budget admits
    int wg_per_cu = fsnap::syrk_waves_per_simd(K, 1);
    if (wg_per_cu < 1) wg_per_cu = 1;
    int64_t nblocks = ctx->opt_nblocks > 0 ? ctx->opt_nblocks : (int64_t)ctx->num_cu * wg_per_cu;
    // keep >= 8 chunks (32 rows) per row-wave so the pipeline prologue amortises
    const int64_t max_blocks = (nchunks + 31) / 32;
    if (nblocks > max_blocks) nblocks = max_blocks;
    if (nblocks < 1) nblocks = 1;
    int64_t cpw = (nchunks + nblocks * 4 - 1) / (nblocks * 4);
    if (cpw < 1) cpw = 1;
    // 32-bit buffer offsets: a row-wave's byte range must stay below 4 GiB
    const int64_t max_cpw = off_limit / (ctx->lda * 32);
    if (max_cpw < 1) return ctx->fail(FSNAP_E_ARG, "leading dimension %lld too large", (long long)ctx->lda);
    if (cpw > max_cpw) cpw = max_cpw;
    nblocks = (nchunks + cpw * 4 - 1) / (cpw * 4);
    if (nblocks < 1) nblocks = 1;
    if (nblocks > 0x7FFFFFF) return ctx->fail(FSNAP_E_ARG, "too many workgroups");
    g->nblocks = (int)nblocks;
    g->cpw = cpw;
    // kernel 1P packs the pairs of its rows itself when they fit its LDS budget (contiguous chunk ranges only)
    g->fused_pack = ctx->opt_fused_pack && !ctx->wpack_override && cpw <= fsnap::syrk_wave_p_max_fused_cpw(K, wg_per_cu);
    return FSNAP_OK;
}

// Host memory -> device memory on the context's stream through the page-locked staging slots, WITHOUT a stream
// synchronisation: the bytes are copied into a slot in 1 MiB pieces, each piece's DMA starts as soon as it is in the
// slot (the memcpy of piece i + 1 overlaps the DMA of piece i), and the caller's buffer is free on return.  A slot is
// reused only after the event of its previous DMA has completed.  Up to two independent transfers per slot rotation
// (weights + mask); larger requests than a slot holds grow the slot.
// A few MB of host data (one weight per row, a mask, the rank array) -> device memory, ordered before everything launched later
// on the context's stream; the caller's buffer is free when the function returns.  Two ways:
//   1 staged    pieces of 1 MB through a page-locked slot: the caller's thread copies piece i + 1 while the DMA engine drains
//               piece i; returns when the last piece is queued.  Host time 0.23 ms for 8 MB (memcpy 0.16 + 8 DMA calls).
//   0 pageable  ONE hipMemcpyAsync from the caller's buffer and a wait for it (the runtime may read the buffer after the call
//               returns, so the wait is what frees it).  0.15 ms for 8 MB, 0.26 for 14 MB on the round-5 boxes
//               (profiles/r05_class_overhead.txt) -- the runtime pins the pages in place and the copy runs at PCIe speed,
//               where the staged form is bound by one core's memcpy.
// Which one is faster depends on the box (a pageable copy of 1 GB ran at 10 GB/s on one and 37 GB/s on another): from 1 MB on,
// the first three uploads go the pageable way and the next three the staged way, each timed until the data is on the device
// (the first of either kind not counted); the better one is kept for the context.  FSNAP_H2D_SMALL=pageable|staged fixes the choice.
static int h2d_forced() {
    static const int v = [] {
        const char* e = getenv("FSNAP_H2D_SMALL");
        if (!e) return -1;
        if (!strcmp(e, "pageable")) return 0;
        if (!strcmp(e, "staged")) return 1;
        return -1;
    }();
    return v;
}

int staged_h2d(fsnap_ctx* ctx, void* dst, const void* src, size_t bytes) {
    if (bytes == 0) return FSNAP_OK;
    int method = 1, probing = 0;
    if (bytes >= ((size_t)1 << 20)) {
        if (h2d_forced() >= 0) method = h2d_forced();
        else if (ctx->h2d_method >= 0) method = ctx->h2d_method;
        else {
            probing = 1;
            method = ctx->h2d_probes < 3 ? 0 : 1;
        }
    }
    if ((method == 0 || probing) && !ctx->h2d_ev &&
        hipEventCreateWithFlags(&ctx->h2d_ev, hipEventDisableTiming) != hipSuccess) {
        ctx->h2d_ev = nullptr;
        method = 1;
        probing = 0;
    }
    std::chrono::steady_clock::time_point t0;
    if (probing) {
        int wrc;
        if ((wrc = fsnap::wait_stream(ctx, nullptr, "upload probe"))) return wrc;      // time the copy, not what is queued before it
        t0 = std::chrono::steady_clock::now();
    }
    if (method == 0) {
        FSNAP_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, ctx->stream), "hipMemcpy(H2D)");
        FSNAP_HIP(hipEventRecord(ctx->h2d_ev, ctx->stream), "hipEventRecord");
        int wrc;
        if ((wrc = fsnap::wait_stream(ctx, ctx->h2d_ev, "upload"))) return wrc;
    } else {
        const int slot = ctx->wstage_next;
        ctx->wstage_next ^= 1;
        if (ctx->wstage_ev[slot]) {
            FSNAP_HIP(hipEventSynchronize(ctx->wstage_ev[slot]), "hipEventSynchronize(staging)");   // normally long done
        } else {
            FSNAP_HIP(hipEventCreateWithFlags(&ctx->wstage_ev[slot], hipEventDisableTiming), "hipEventCreate");
        }
        if (ctx->wstage_bytes[slot] < bytes) {
            if (ctx->wstage[slot]) (void)hipHostFree(ctx->wstage[slot]);
            ctx->wstage[slot] = nullptr;
            ctx->wstage_bytes[slot] = 0;
            if (hipHostMalloc((void**)&ctx->wstage[slot], bytes, hipHostMallocDefault) != hipSuccess)
                return ctx->fail(FSNAP_E_NOMEM, "hipHostMalloc(%zu) for the weight staging failed", bytes);
            ctx->wstage_bytes[slot] = bytes;
        }
        const size_t piece = (size_t)1 << 20;
        for (size_t off = 0; off < bytes; off += piece) {
            const size_t n = bytes - off < piece ? bytes - off : piece;
            memcpy(ctx->wstage[slot] + off, (const char*)src + off, n);
            FSNAP_HIP(hipMemcpyAsync((char*)dst + off, ctx->wstage[slot] + off, n, hipMemcpyHostToDevice, ctx->stream), "hipMemcpy(staged H2D)");
        }
        FSNAP_HIP(hipEventRecord(ctx->wstage_ev[slot], ctx->stream), "hipEventRecord");
        if (probing) {
            int wrc;
            if ((wrc = fsnap::wait_stream(ctx, ctx->wstage_ev[slot], "upload probe"))) return wrc;
        }
    }
    if (probing) {
        // per byte, so that a mask (1 byte per row) and the weights (8) of the same fit can share the probes
        const double t = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() / (double)bytes;
        const bool first_of_its_kind = ctx->h2d_probes == 0 || ctx->h2d_probes == 3;      // pays the runtime's first-use costs: not counted
        if (!first_of_its_kind && t < ctx->h2d_best[method]) ctx->h2d_best[method] = t;
        if (++ctx->h2d_probes >= 6) ctx->h2d_method = ctx->h2d_best[0] <= ctx->h2d_best[1] ? 0 : 1;
    }
    return FSNAP_OK;
}

// Rows of a host matrix -> device memory through two page-locked slots: the host copies piece i + 1 into one slot (a few
// threads, each a contiguous part) while the DMA engine drains piece i from the other.  A pageable hipMemcpyAsync of the
// 1 GB matrix of the headline shape ran at 10 GB/s on one box and 37 GB/s on another (the runtime pins or stages the
// user's pages itself, single-threaded); rows with a leading dimension wider than the row are packed on the way.
// Returns with every byte handed to the stream (the caller's buffer is free); not synchronised.
// probe (optional): after two pieces the host-side fill rate (bytes copied into the slots per second of memcpy time) is
// compared with min_fill_rate; below it the function stops, *rows_done says how far it got, and the caller sends the rest
// another way.
int staged_rows_h2d(fsnap_ctx* ctx, void* dst, const void* src, size_t rows, size_t row_bytes, size_t src_pitch,
                    double min_fill_rate = 0.0, size_t* rows_done = nullptr, double* fill_rate = nullptr) {
    const size_t total = rows * row_bytes;
    if (rows_done) *rows_done = 0;
    if (total == 0) return FSNAP_OK;
    const size_t slot_bytes = (size_t)16 << 20;
    double fill_s = 0.0;
    size_t fill_bytes = 0;
    int pieces = 0;
    for (int i = 0; i < 2; ++i) {
        if (!ctx->rstage[i] && hipHostMalloc((void**)&ctx->rstage[i], slot_bytes, hipHostMallocDefault) != hipSuccess) {
            ctx->rstage[i] = nullptr;
            return FSNAP_E_NOMEM;               // the caller falls back on the plain copy
        }
        if (!ctx->rstage_ev[i]) FSNAP_HIP(hipEventCreateWithFlags(&ctx->rstage_ev[i], hipEventDisableTiming), "hipEventCreate");
    }
    static const int nthreads = [] {
        const char* e = getenv("FSNAP_UPLOAD_THREADS");
        int n = e ? atoi(e) : 4;
        const unsigned hc = std::thread::hardware_concurrency();
        if (hc > 0 && n > (int)hc) n = (int)hc;
        return n < 1 ? 1 : (n > 16 ? 16 : n);
    }();
    const bool dense = src_pitch == row_bytes;
    size_t rows_per_piece = slot_bytes / row_bytes;
    if (rows_per_piece < 1) return FSNAP_E_NOMEM;      // a row wider than a slot: the caller falls back on the plain copy
    // `rstage_busy[slot]`: a DMA out of this slot was enqueued and its event not waited for since -- kept in the CONTEXT: a
    // call that returned early (a failed copy further on, a failing plan copy of the assembly before its stream
    // synchronisation) must not let the next call fill a slot the DMA engine is still reading
    bool* used = ctx->rstage_busy;
    int slot = 0;
    for (size_t r0 = 0; r0 < rows; r0 += rows_per_piece, slot ^= 1) {
        const size_t nr = rows - r0 < rows_per_piece ? rows - r0 : rows_per_piece;
        if (used[slot]) {
            FSNAP_HIP(hipEventSynchronize(ctx->rstage_ev[slot]), "hipEventSynchronize(row staging)");
            used[slot] = false;
        }
        char* stage = ctx->rstage[slot];
        const char* from = (const char*)src + r0 * src_pitch;
        auto copy_part = [&](size_t a, size_t b) {           // rows [a, b) of this piece
            if (dense) {
                memcpy(stage + a * row_bytes, from + a * row_bytes, (b - a) * row_bytes);
            } else {
                for (size_t r = a; r < b; ++r) memcpy(stage + r * row_bytes, from + r * src_pitch, row_bytes);
            }
        };
        const int nt = (nr * row_bytes >= ((size_t)4 << 20)) ? nthreads : 1;
        const auto tf0 = std::chrono::steady_clock::now();
        if (nt <= 1) {
            copy_part(0, nr);
        } else {
            std::vector<std::thread> th;
            th.reserve(nt - 1);
            for (int t = 1; t < nt; ++t) th.emplace_back(copy_part, nr * t / nt, nr * (t + 1) / nt);
            copy_part(0, nr / nt);
            for (auto& x : th) x.join();
        }
        fill_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - tf0).count();
        fill_bytes += nr * row_bytes;
        FSNAP_HIP(hipMemcpyAsync((char*)dst + r0 * row_bytes, stage, nr * row_bytes, hipMemcpyHostToDevice, ctx->stream),
                  "hipMemcpy(staged rows)");
        FSNAP_HIP(hipEventRecord(ctx->rstage_ev[slot], ctx->stream), "hipEventRecord");
        used[slot] = true;
        if (rows_done) *rows_done = r0 + nr;
        if (fill_rate) *fill_rate = fill_s > 0.0 ? (double)fill_bytes / fill_s : 0.0;
        if (++pieces == 2 && min_fill_rate > 0.0 && fill_s > 0.0 && (double)fill_bytes / fill_s < min_fill_rate) return FSNAP_OK;
    }
    return FSNAP_OK;
}

// the category layout of the candidate kernels belongs to the rows it was prepared for: any change of the resident rows drops it
void cand_forget(fsnap_ctx* ctx) {
    ctx->sel_active = false;          // a selection session (fsnap_select_*) belongs to the rows as well
    ctx->joint_active = false;        // ... and so does a joint-score session (fsnap_joint_*)
    ctx->cand_layout = 0;
    ctx->cand_dA = nullptr;
    ctx->cand_stats_K = 0;
}

// a robust session (fsnap_robust_*) belongs to the rows AND the weights it was begun with: new rows or new weights end it
// without restoring anything.  new_rows: the session's w r are not weights of the new rows -- none until the caller sets some
void robust_forget(fsnap_ctx* ctx, bool new_rows) {
    if (new_rows && ctx->rob_active && ctx->rob_pointed && ctx->dw == (const double*)ctx->rob_wr.p) {
        ctx->dw = nullptr;
        ctx->dmask = nullptr;
        ctx->wpack_valid = false;
    }
    ctx->rob_active = ctx->rob_pointed = false;
    if (new_rows) ctx->rob_have_e = ctx->rob_have_r = false;      // (new weights: e, r, w r of the last pass stay downloadable)
}

int check_rows(fsnap_ctx* ctx) {
    if (!ctx->dA || !ctx->db || ctx->m <= 0) return ctx->fail(FSNAP_E_STATE, "no rows: call fsnap_upload_rows/fsnap_bind_rows first");
    return FSNAP_OK;
}

int check_weights(fsnap_ctx* ctx) {
    if (!ctx->dw) return ctx->fail(FSNAP_E_STATE, "no weights: call fsnap_set_weights/fsnap_bind_weights first");
    return FSNAP_OK;
}

int ensure_ones(fsnap_ctx* ctx) {
    const size_t need = (size_t)ctx->m;
    if (ctx->ones.p && ctx->ones.bytes >= need) return FSNAP_OK;
    if (!ctx->ones.ensure(need)) return ctx->fail(FSNAP_E_NOMEM, "hipMalloc(mask) failed");
    FSNAP_HIP(hipMemsetAsync(ctx->ones.p, 1, need, ctx->stream), "hipMemsetAsync(mask)");
    return FSNAP_OK;
}

struct TiledGeometry {
    int NSB, npairs, nsplit;
    int64_t cps;  // chunks per split
};

// event triple {before SYRK, after SYRK, after reduction} of the fit being launched: a ring, so that the kernel times
// of many consecutive fits can be read AFTER a timed loop instead of synchronising inside it
// Option timing_every = N: only every N-th launch is bracketed (0: none).  An event record between two dependent kernels
// costs ~5.6 us of idle stream on this runtime (rocprof timeline of the C1 shape: pack 5.0 | 5.6 | kernel 4.0 | 5.8 |
// reduce 4.3 us), i.e. 11 us of a 0.34 ms headline step; *slot stays null on the launches that are not sampled.
int fit_events(fsnap_ctx* ctx, hipEvent_t** slot) {
    *slot = nullptr;
    ctx->cur_events = nullptr;
    ++ctx->nlaunch;
    const int64_t phase = ctx->timing_phase++;         // 0 right after the option was set: that launch is sampled
    if (ctx->opt_timing_every <= 0 || phase % ctx->opt_timing_every != 0) return FSNAP_OK;
    hipEvent_t* sl = ctx->ring[ctx->nfit % fsnap_ctx::RING];
    for (int i = 0; i < 4; ++i)
        if (!sl[i]) FSNAP_HIP(hipEventCreate(&sl[i]), "hipEventCreate");
    ctx->ring_comm[ctx->nfit % fsnap_ctx::RING] = false;
    ++ctx->nfit;
    *slot = sl;
    ctx->cur_events = sl;
    return FSNAP_OK;
}

// Row splits of the tiled kernel.  Work items (split, superblock pair) are NOT equal: an off-diagonal pair runs 16
// MFMAs per chunk, a diagonal pair 10, pairs with the (half-empty) last superblock 8 / 3, and two workgroups per CU
// are resident -- with one or two rounds of items the short ones leave their slots idle (367 900 x 480: 27 splits
// 1.84 ms, 57 splits 1.60 ms).  So the split count comes from a small model: greedy list scheduling of one XCD's
// item range on its slots (the hardware dispatches the next workgroup when a slot frees up) + the reduction of the
// partial triangles; it reproduces the measured kernel times within ~5 %.  The result is cached per shape.
double tiled_makespan_units(const std::vector<int>& tiles, int64_t n, int64_t chunks_per_wave, int64_t groups, int64_t slots,
                            double ovh) {
    const int64_t npairs = (int64_t)tiles.size();
    const int64_t nitems = npairs * n;
    const int64_t per = (nitems + groups - 1) / groups;
    std::priority_queue<double, std::vector<double>, std::greater<double>> free_at;
    for (int64_t i = 0; i < slots; ++i) free_at.push(0.0);
    double makespan = 0.0;
    for (int64_t it = 0; it < per && it < nitems; ++it) {
        const double t0 = free_at.top();
        free_at.pop();
        // ovh: prologue + 4-wave fold + partial store, in units of one chunk of one tile
        const double t1 = t0 + ovh + (double)chunks_per_wave * tiles[(size_t)(it % npairs)];
        free_at.push(t1);
        if (t1 > makespan) makespan = t1;
    }
    return makespan;
}

// geometry of the tiled kernel for m rows of K columns (leading dimension lda).  Pure function of the shape and the context's options.
int tiled_geometry(fsnap_ctx* ctx, int64_t m, int64_t K, int64_t lda, TiledGeometry* g) {
    if (K > 32768) return ctx->fail(FSNAP_E_ARG, "K = %lld too large", (long long)K);
    g->NSB = (int)((K + 63) / 64);
    g->npairs = g->NSB * (g->NSB + 1) / 2;
    const int64_t nchunks = (m + 3) / 4;
    const int64_t bytes = m * lda * 8;
    // keep a split's rows resident in the Infinity Cache (256 MiB) while all pairs sweep them
    const int64_t min_split_cache = (bytes + (96ll << 20) - 1) / (96ll << 20);
    // work items of one split and their cost in MFMA tiles per chunk
    const int tail = (int)(K & 63);
    const bool half = tail != 0 && tail <= 32;                   // last superblock: second 32-column group empty
    std::vector<int> tiles;
    for (int I = 0; I < g->NSB; ++I)                 // kernel 1T's item order: off-diagonal pairs, then the diagonal
        for (int J = I + 1; J < g->NSB; ++J) tiles.push_back((half && J == g->NSB - 1) ? 8 : 16);
    for (int I = 0; I < g->NSB; ++I) tiles.push_back((half && I == g->NSB - 1) ? 3 : 10);
    int64_t nsplit = ctx->opt_nsplit;
    if (nsplit <= 0) {
        const int64_t groups = 8;         // contiguous work-item ranges per XCD
        // two workgroups (8 waves) per CU share the matrix pipe, 66 ns per tile and chunk at ~80 % issue
        const int64_t slots = (int64_t)ctx->num_cu * 2 / groups;
        const double unit = 66.0e-9, ovh = 128.0;
        const int64_t part_bytes = (int64_t)g->npairs * 32768;                        // partial triangles of one split
        int64_t n_hi = std::max<int64_t>(1, std::min<int64_t>(1024, nchunks / 128));  // >= 32 chunks per wave
        n_hi = std::min(n_hi, std::max<int64_t>(1, (256ll << 20) / part_bytes));      // <= 256 MiB of partials
        const int64_t n_lo = std::min(n_hi, std::max<int64_t>(1, min_split_cache));
        double best = 1.0e300;
        for (int64_t n = n_lo; n <= n_hi; ++n) {
            const int64_t cps = (nchunks + n - 1) / n;
            const int64_t cpw = (cps + 3) / 4;
            // Long items drift apart: the pairs of a split start together and share every row segment through their
            // XCD's L2, but they cost 16 / 10 / 8 / 3 tiles per chunk, and the longer they run the less of a split's rows is
            // still in L2 when the slower ones get there (367 900 x 480: 7.4 GB fetched per launch for a 1.4 GB matrix, the
            // kernel at 5.2 TB/s of fabric traffic as much memory- as MFMA-bound).  Measured with the split count forced
            // (round 3): the kernel time grows by ~2e-4 per chunk a wave owns -- 367 900 x 480: 64 splits 1.44 ms, 128
            // 1.40, 192 1.37; 200 000 x 1 000: 23 splits 3.83 ms, 64 3.48 -- and by a quarter of that when the whole
            // matrix stays in the Infinity Cache (15 213 x 1 595).
            // (scaled by how much there is to share: a row segment is wanted by NSB pairs -- with 3 superblocks at most 3 x
            // the matrix can be fetched, and many splits only buy a long reduction: 1 772 880 x 142 took 744)
            const double share = std::min(1.0, (double)(g->NSB - 1) / 7.0);
            const double drift = 1.0 + share * (bytes > (200ll << 20) ? 2.0e-4 : 0.5e-4) * (double)cpw;
            const double cost = unit * drift * tiled_makespan_units(tiles, n, cpw, groups, slots, ovh) + (double)n * (double)part_bytes / 3.0e12;
            if (cost < best) {
                best = cost;
                nsplit = n;
            }
        }
    }
    // >= 8 chunks per wave (4 waves per split)
    const int64_t max_split = (nchunks + 31) / 32;
    if (nsplit > max_split) nsplit = max_split;
    if (nsplit < 1) nsplit = 1;
    int64_t cps = (nchunks + nsplit - 1) / nsplit;
    cps = (cps + 3) / 4 * 4;
    // 32-bit buffer offsets per wave
    const int64_t max_cpw = (int64_t)0xFFF00000 / (lda * 32);
    if (max_cpw < 1) return ctx->fail(FSNAP_E_ARG, "leading dimension %lld too large", (long long)lda);
    if (cps / 4 > max_cpw) cps = max_cpw * 4;
    nsplit = (nchunks + cps - 1) / cps;
    if ((int64_t)g->npairs * nsplit > 0x7FFFFFFF) return ctx->fail(FSNAP_E_ARG, "too many workgroups");
    g->nsplit = (int)nsplit;
    g->cps = cps;
    return FSNAP_OK;
}

// the same for the resident rows, cached per shape
int plan_tiled(fsnap_ctx* ctx, TiledGeometry* g) {
    const int64_t m = ctx->m, K = ctx->K;
    if (ctx->tplan_valid && ctx->tplan_key[0] == m && ctx->tplan_key[1] == K && ctx->tplan_key[2] == ctx->lda &&
        ctx->tplan_key[3] == ctx->opt_nsplit) {
        g->NSB = ctx->tplan[0];
        g->npairs = ctx->tplan[1];
        g->nsplit = ctx->tplan[2];
        g->cps = ctx->tplan_cps;
        return FSNAP_OK;
    }
    int rc;
    if ((rc = tiled_geometry(ctx, m, K, ctx->lda, g))) return rc;
    ctx->tplan_key[0] = m;
    ctx->tplan_key[1] = K;
    ctx->tplan_key[2] = ctx->lda;
    ctx->tplan_key[3] = ctx->opt_nsplit;
    ctx->tplan[0] = g->NSB;
    ctx->tplan[1] = g->npairs;
    ctx->tplan[2] = g->nsplit;
    ctx->tplan_cps = g->cps;
    ctx->tplan_valid = true;
    return FSNAP_OK;
}

// (w_eff, w_eff b) per row for kernels 1A / 1T, packed once per (b, w, mask) -- every time if any of them lives in
// memory the caller owns (fsnap_bind_rows / fsnap_bind_weights: it may have changed without notice).  *npk = number
// of partial b-only scalars in ctx->wpack_spart.
int ensure_wpack(fsnap_ctx* ctx, int* npk) {
    *npk = fsnap::pack_weights_num_blocks(ctx->m);
    if (ctx->wpack_override) {                     // rows and per-row pairs of the row-space passes (normal_eq_launch_on)
        if (!ctx->wpack_spart.ensure((size_t)*npk * 4 * 8)) return ctx->fail(FSNAP_E_NOMEM, "hipMalloc(packed weights) failed");
        return FSNAP_OK;
    }
    if (!ctx->wpack.ensure((size_t)ctx->m * 16 + 64) || !ctx->wpack_spart.ensure((size_t)*npk * 4 * 8))
        return ctx->fail(FSNAP_E_NOMEM, "hipMalloc(packed weights) failed");
    const bool caller_owned = ctx->db != (const double*)ctx->ownb.p || ctx->dw != (const double*)ctx->ownw.p ||
                              (ctx->dmask && ctx->dmask != (const unsigned char*)ctx->ownmask.p);
    if (!ctx->wpack_valid || caller_owned || ctx->opt_repack) {
        FSNAP_HIP(fsnap::launch_pack_weights(ctx->db, ctx->dw, ctx->dmask, ctx->m, (double*)ctx->wpack.p,
                                             (double*)ctx->wpack_spart.p, ctx->stream),
                  "launch fsnap_pack_weights_k");
        ctx->wpack_valid = true;
    }
    return FSNAP_OK;
}

int launch_normal_eq_tiled(fsnap_ctx* ctx, double* d_packed, bool accumulate) {
    int rc;
    TiledGeometry g;
    if ((rc = plan_tiled(ctx, &g))) return rc;
    int npk = 0;
    if ((rc = ensure_wpack(ctx, &npk))) return rc;
    if (!ctx->part.ensure((size_t)g.nsplit * g.npairs * 4096 * sizeof(double)) ||
        !ctx->cpart.ensure((size_t)g.nsplit * g.NSB * 4 * 64 * sizeof(double)))
        return ctx->fail(FSNAP_E_NOMEM, "hipMalloc(partials) failed");
    fsnap::TiledArgs a;
    a.A = ctx->dA;
    a.lda = ctx->lda;
    a.wpack = ctx->wpack_override ? ctx->wpack_override : (const double*)ctx->wpack.p;
    a.m = ctx->m;
    a.K = (int)ctx->K;
    a.NSB = g.NSB;
    a.npairs = g.npairs;
    a.nsplit = g.nsplit;
    a.chunks_per_split = g.cps;
    a.nontemporal = false;  // rows are re-read by the other column pairs: keep them cached
    a.part = (double*)ctx->part.p;
    a.cpart = (double*)ctx->cpart.p;
    a.spart = (const double*)ctx->wpack_spart.p;
    a.ns = npk;
    // every c slot (split, superblock, wave) is rewritten by the diagonal pair of its split on every launch (also by
    // waves whose row range is empty: they store zeros), so the buffer is cleared only when its geometry changes -- a
    // memset per fit was a 4 us kernel plus a stream boundary in front of a 27 us SYRK at the ACE shape 13 035 x 142
    const int64_t cpart_key = ((int64_t)g.nsplit << 32) | (int64_t)g.NSB;
    if (ctx->cpart_key != cpart_key || ctx->cpart_ptr != ctx->cpart.p) {
        FSNAP_HIP(hipMemsetAsync(a.cpart, 0, (size_t)g.nsplit * g.NSB * 4 * 64 * sizeof(double), ctx->stream), "hipMemsetAsync");
        ctx->cpart_key = cpart_key;
        ctx->cpart_ptr = ctx->cpart.p;
    }
    hipEvent_t* evs;
    if ((rc = fit_events(ctx, &evs))) return rc;
    if (evs) FSNAP_HIP(hipEventRecord(evs[0], ctx->stream), "hipEventRecord");
    FSNAP_HIP(fsnap::launch_syrk_tiled(a, ctx->stream), "launch fsnap_syrk_tiled");
    if (evs) FSNAP_HIP(hipEventRecord(evs[1], ctx->stream), "hipEventRecord");
    FSNAP_HIP(fsnap::launch_reduce_tiled(a, d_packed, accumulate, ctx->stream), "launch fsnap_reduce_tiled");
    if (evs) FSNAP_HIP(hipEventRecord(evs[2], ctx->stream), "hipEventRecord");
    if (evs) ctx->t_syrk = true;
    return FSNAP_OK;
}

int launch_normal_eq(fsnap_ctx* ctx, double* d_packed, bool want_mirror = false, bool accumulate = false) {
    int rc;
    ctx->mirror_of = nullptr;
    ctx->chol_factor_of = nullptr;              // the statistics are about to change: the factor on the device is of the old ones
    if ((rc = check_rows(ctx)) || (rc = check_weights(ctx))) return rc;
    if (use_tiled(ctx)) return launch_normal_eq_tiled(ctx, d_packed, accumulate);
    Geometry g;
    if ((rc = plan_geometry(ctx, &g))) return rc;
    const unsigned char* mask = ctx->dmask;
    if (!mask) {
        if ((rc = ensure_ones(ctx))) return rc;
        mask = (const unsigned char*)ctx->ones.p;
    }
    const int NT = g.NB * (g.NB + 1) / 2;
    const int cs_per_block = g.shortk ? 1 : 4 * g.cluster;   // c / scalar partials per workgroup (kernel 1QC: 4 per member; kernel 1S: one per chunk)
    if (!ctx->part.ensure((size_t)g.nblocks * NT * 256 * sizeof(double)) ||
        !ctx->cpart.ensure((size_t)g.nblocks * cs_per_block * g.NB * 16 * sizeof(double)) ||
        !ctx->spart.ensure((size_t)g.nblocks * cs_per_block * 4 * sizeof(double)))
        return ctx->fail(FSNAP_E_NOMEM, "hipMalloc(partials) failed");
    fsnap::SyrkArgs a;
    a.A = ctx->dA;
    a.lda = ctx->lda;
    a.b = ctx->db;
    a.w = ctx->dw;
    a.mask = mask;
    a.m = ctx->m;
    a.K = (int)ctx->K;
    a.nblocks = g.nblocks;
    a.split = g.split;
    a.chunks_per_wave = g.cpw;
    a.nontemporal = true;
    a.part = (double*)ctx->part.p;
    a.cpart = (double*)ctx->cpart.p;
    a.spart = (double*)ctx->spart.p;
    int ns = -1;                      // scalar partials: from the SYRK kernel, or (kernel 1A) from the weight packing
    const double* spart_src = a.spart;
    if (g.fused_pack) {
        a.fused_pack = true;          // b, w, mask -> pairs in LDS + the b-only scalars per row-wave, inside the SYRK launch
    } else {
        int npk = 0;
        if ((rc = ensure_wpack(ctx, &npk))) return rc;
        a.wpack = ctx->wpack_override ? ctx->wpack_override : (const double*)ctx->wpack.p;
        spart_src = (const double*)ctx->wpack_spart.p;
        ns = npk;
    }
    hipEvent_t* evs;
    if ((rc = fit_events(ctx, &evs))) return rc;
    if (evs) FSNAP_HIP(hipEventRecord(evs[0], ctx->stream), "hipEventRecord");
    if (g.quad && g.cluster > 1) {
        const size_t need = (size_t)g.nblocks * 4 * sizeof(int);
        if (ctx->quad_flow.bytes < need) {
            if (!ctx->quad_flow.ensure(need)) return ctx->fail(FSNAP_E_NOMEM, "hipMalloc(flow words) failed");
            FSNAP_HIP(hipMemsetAsync(ctx->quad_flow.p, 0, ctx->quad_flow.bytes, ctx->stream), "hipMemset(flow words)");
            ctx->quad_flow_tag = 0;
        }
        ctx->quad_flow_tag += 1u << 20;                                  // (unsigned: wraps after 4096 launches, see quad_flow_wait)
        a.flow_words = (int*)ctx->quad_flow.p;
        // low byte: flow-control mode (2 bits) and lead (6 bits).  Lead 63 = by cluster size, as measured (HBM reads / algorithmic):
        // clusters of 4 (367 900 x 480) lead 2: 1.01 x, lead 4: 1.5 x; clusters of 2 (500 000 x 368: twice as many clusters share an
        // XCD's L2) lead 0: 1.01 x, lead 1: 1.33 x, lead 2: 1.78 x -- at the same kernel time in every case
        const int flow = 2 | ((g.cluster == 2 ? 0 : 2) << 2);      // mode 2: publish at the start of a trip, judge at its end
        a.flow_tag = (int)(ctx->quad_flow_tag | (unsigned)flow);
    }
    if (g.shortk) FSNAP_HIP(fsnap::launch_syrk_short(a, ctx->stream), "launch fsnap_syrk_short");
    else if (g.quad) FSNAP_HIP(fsnap::launch_syrk_quad(a, ctx->stream), "launch fsnap_syrk_quad");
    else if (g.acc) FSNAP_HIP(fsnap::launch_syrk_acc(a, ctx->stream), "launch fsnap_syrk_acc");
    else FSNAP_HIP(fsnap::launch_syrk_wave_p(a, ctx->stream), "launch fsnap_syrk_wave_p");
    if (evs) FSNAP_HIP(hipEventRecord(evs[1], ctx->stream), "hipEventRecord");
    // K <= 128 and the context owns the output: the reduction also writes a page-locked host mirror, so the solve
    // needs no D2H copy (the copy's launch latency was 12 us of a 440 us step)
    double* mirror = nullptr;
    // (a system the GPU factorises -- fsnap_solve_device_rhs's rule -- needs no mirror: DEVICE_CHOL_MIN_K columns and more)
    if (want_mirror && !device_factor(ctx, ctx->K)) {
        const size_t need = ((size_t)FSNAP_PACKED_LEN(ctx->K) + (size_t)ctx->K) * 8;   // + compact diagonal
        if (ctx->mirror_bytes < need) {
            if (ctx->mirror) (void)hipHostFree(ctx->mirror);
            ctx->mirror = nullptr;
            ctx->mirror_bytes = 0;
            // coherent (fine-grained) host memory: the kernel's stores are visible to the host once the event has completed
            if (hipHostMalloc((void**)&ctx->mirror, need, hipHostMallocCoherent | hipHostMallocMapped) == hipSuccess)
                ctx->mirror_bytes = need;
        }
        if (ctx->mirror && !ctx->mirror_ev && hipEventCreateWithFlags(&ctx->mirror_ev, hipEventDisableTiming) != hipSuccess)
            ctx->mirror_ev = nullptr;
        if (ctx->mirror && ctx->mirror_ev) mirror = ctx->mirror;
    }
    const bool upper_mirror = mirror != nullptr;      // the mirror's triangle is written once per element, at its upper position
    FSNAP_HIP(fsnap::launch_reduce(a.part, a.cpart, spart_src, g.nblocks, cs_per_block, ns, a.K, d_packed, mirror, accumulate,
                                   ctx->stream, upper_mirror),
              "launch fsnap_reduce_partials");
    if (evs) FSNAP_HIP(hipEventRecord(evs[2], ctx->stream), "hipEventRecord");
    if (mirror) {
        FSNAP_HIP(hipEventRecord(ctx->mirror_ev, ctx->stream), "hipEventRecord");
        ctx->mirror_of = d_packed;
        ctx->mirror_K = ctx->K;
        ctx->mirror_upper = upper_mirror;
        ctx->mirror_gen = next_mirror_generation();
    }
    if (evs) ctx->t_syrk = true;
    return FSNAP_OK;
}

}  // namespace

namespace fsnap {

int wpack_current(fsnap_ctx* ctx) {
    int rc, npk = 0;
    if ((rc = check_rows(ctx)) || (rc = check_weights(ctx))) return rc;
    return ensure_wpack(ctx, &npk);
}

int normal_eq_launch_on(fsnap_ctx* ctx, const double* Q, int64_t ldq, const double* qpack, double* d_packed) {
    const double* const save_A = ctx->dA;
    const int64_t save_lda = ctx->lda;
    ctx->dA = Q;
    ctx->lda = ldq;
    ctx->wpack_override = qpack;
    const int rc = launch_normal_eq(ctx, d_packed);
    ctx->wpack_override = nullptr;
    ctx->dA = save_A;
    ctx->lda = save_lda;
    return rc;
}

}  // namespace fsnap

extern "C" {

int fsnap_version(void) { return 201; }

int fsnap_device_count(int* count) {
    if (!count) return FSNAP_E_ARG;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) {
        g_last_error = std::string("hipGetDeviceCount: ") + hipGetErrorString(e);
        *count = 0;
        return FSNAP_E_HIP;
    }
    *count = n;
    return FSNAP_OK;
}

const char* fsnap_last_error(const fsnap_ctx* ctx) { return ctx ? ctx->err.c_str() : g_last_error.c_str(); }

int fsnap_ctx_create(int device, fsnap_ctx** out) {
    if (!out) return FSNAP_E_ARG;
    *out = nullptr;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) {
        g_last_error = std::string("no HIP device: ") + (e != hipSuccess ? hipGetErrorString(e) : "device count is 0");
        return FSNAP_E_HIP;
    }
    if (device < 0 || device >= n) {
        g_last_error = "device index out of range";
        return FSNAP_E_ARG;
    }
    fsnap_ctx* ctx = new (std::nothrow) fsnap_ctx();
    if (!ctx) return FSNAP_E_NOMEM;
    ctx->device = device;
    if ((e = hipSetDevice(device)) != hipSuccess) {
        g_last_error = std::string("hipSetDevice: ") + hipGetErrorString(e);
        delete ctx;
        return FSNAP_E_HIP;
    }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess) {
        ctx->num_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
        if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
            g_last_error = std::string("libfsnap_hip is built for gfx950 (MI355X) only; device is ") + prop.gcnArchName;
            delete ctx;
            return FSNAP_E_HIP;
        }
    }
    if ((e = hipStreamCreateWithFlags(&ctx->own_stream, hipStreamNonBlocking)) != hipSuccess) {
        g_last_error = std::string("hipStreamCreate: ") + hipGetErrorString(e);
        delete ctx;
        return FSNAP_E_HIP;
    }
    ctx->stream = ctx->own_stream;
    for (auto& ev : ctx->ev) {
        if ((e = hipEventCreate(&ev)) != hipSuccess) {
            g_last_error = std::string("hipEventCreate: ") + hipGetErrorString(e);
            fsnap_ctx_destroy(ctx);
            return FSNAP_E_HIP;
        }
    }
    *out = ctx;
    return FSNAP_OK;
}

int fsnap_ctx_destroy(fsnap_ctx* ctx) {
    if (!ctx) return FSNAP_OK;
    (void)hipSetDevice(ctx->device);
    if (ctx->stream && !ctx->comm_broken) (void)hipStreamSynchronize(ctx->stream);
    (void)fsnap_comm_destroy(ctx);                    // a broken communicator is aborted: its stuck kernel leaves the stream
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    fsnap::rowspace_release(ctx);
    ctx->commbuf.release();
    DevBuf* bufs[] = {&ctx->ownA, &ctx->ownb, &ctx->ownw, &ctx->ownmask, &ctx->ones, &ctx->part, &ctx->cpart,
                      &ctx->spart, &ctx->packed, &ctx->beta, &ctx->preds, &ctx->sse, &ctx->aw, &ctx->bw,
                      &ctx->st_raw, &ctx->st_plan, &ctx->st_frac, &ctx->st_blank, &ctx->dsolve, &ctx->dchol, &ctx->dcat, &ctx->dstat, &ctx->wpack, &ctx->wpack_spart,
                      &ctx->du, &ctx->dspart, &ctx->dsvec};
    for (DevBuf* b : bufs) b->release();
    for (int i = 0; i < 2; ++i) {
        if (ctx->rstage[i]) (void)hipHostFree(ctx->rstage[i]);
        if (ctx->rstage_ev[i]) (void)hipEventDestroy(ctx->rstage_ev[i]);
        if (ctx->wstage[i]) (void)hipHostFree(ctx->wstage[i]);
        if (ctx->wstage_ev[i]) (void)hipEventDestroy(ctx->wstage_ev[i]);
    }
    ctx->wtrain.release();
    ctx->wrank.release();
    if (ctx->pinned) (void)hipHostFree(ctx->pinned);
    if (ctx->mirror) (void)hipHostFree(ctx->mirror);
    if (ctx->mirror_ev) (void)hipEventDestroy(ctx->mirror_ev);
    if (ctx->h2d_ev) (void)hipEventDestroy(ctx->h2d_ev);
    if (ctx->chol_host) (void)hipHostFree(ctx->chol_host);
    if (ctx->chol_ev) (void)hipEventDestroy(ctx->chol_ev);
    for (auto& ev : ctx->cvg_ev)
        if (ev) (void)hipEventDestroy(ev);
    for (auto& ev : ctx->evd_ev)
        if (ev) (void)hipEventDestroy(ev);
    for (auto& ev : ctx->spec_ev)
        if (ev) (void)hipEventDestroy(ev);
    for (auto& ev : ctx->ev)
        if (ev) (void)hipEventDestroy(ev);
    for (auto& sl : ctx->ring)
        for (auto& ev : sl)
            if (ev) (void)hipEventDestroy(ev);
    if (ctx->own_stream) (void)hipStreamDestroy(ctx->own_stream);
    delete ctx;
    return FSNAP_OK;
}

int fsnap_ctx_set_stream(fsnap_ctx* ctx, void* hip_stream) {
    if (!ctx) return FSNAP_E_ARG;
    FSNAP_HIP(hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");
    ctx->stream = (hipStream_t)hip_stream;  // NULL = the HIP legacy default stream
    return FSNAP_OK;
}

int fsnap_ctx_use_own_stream(fsnap_ctx* ctx) {
    if (!ctx) return FSNAP_E_ARG;
    FSNAP_HIP(hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");
    ctx->stream = ctx->own_stream;
    return FSNAP_OK;
}

int fsnap_set_option(fsnap_ctx* ctx, const char* key, int64_t value) {
    if (!ctx || !key) return FSNAP_E_ARG;
    if (!strcmp(key, "device_solve")) {
        if (value < 0 || value > 2) return ctx->fail(FSNAP_E_ARG, "device_solve must be 0 (auto), 1 (always) or 2 (never)");
        ctx->opt_device_solve = (int)value;
    } else if (!strcmp(key, "tiled")) {
        ctx->opt_tiled = value != 0;
    } else if (!strcmp(key, "short")) {
        if (value < -1 || value > 1) return ctx->fail(FSNAP_E_ARG, "short must be -1 (by the row count), 0 (never) or 1 (always)");
        ctx->opt_short = (int)value;
    } else if (!strcmp(key, "timing_every")) {
        if (value < 0 || value > (1 << 20)) return ctx->fail(FSNAP_E_ARG, "timing_every out of range");
        ctx->opt_timing_every = (int)value;
        ctx->timing_phase = 0;
    } else if (!strcmp(key, "repack")) {
        ctx->opt_repack = value != 0;
    } else if (!strcmp(key, "comm_timeout")) {
        if (value < 0 || value > 86400) return ctx->fail(FSNAP_E_ARG, "comm_timeout must be 0 (FSNAP_COMM_TIMEOUT) ... 86400 seconds");
        ctx->opt_comm_timeout = (int)value;
    } else if (!strcmp(key, "chol_reuse")) {
        ctx->opt_chol_reuse = value != 0;
        ctx->chol_factor_of = nullptr;
    } else if (!strcmp(key, "rowspace_reuse_stats")) {
        ctx->opt_rowspace_reuse = value != 0;
    } else if (!strcmp(key, "quad_min_rows")) {
        if (value < -1) return ctx->fail(FSNAP_E_ARG, "quad_min_rows must be >= -1");
        ctx->opt_quad_min_rows = value;
    } else if (!strcmp(key, "reduce_triangle")) {
        if (value < -1 || value > 1) return ctx->fail(FSNAP_E_ARG, "reduce_triangle must be -1 (K >= 256), 0 (never) or 1 (always)");
        ctx->opt_reduce_triangle = (int)value;
    } else if (!strcmp(key, "staged_upload")) {
        if (value < 0 || value > 2) return ctx->fail(FSNAP_E_ARG, "staged_upload must be 0 (pageable copy), 1 (probe) or 2 (double buffer)");
        ctx->opt_staged_upload = (int)value;
    } else if (!strcmp(key, "fused_residual")) {
        if (value < 0 || value > 1) return ctx->fail(FSNAP_E_ARG, "fused_residual must be 0 (two kernels) or 1 (one pass)");
        ctx->opt_fused_residual = (int)value;
    } else if (!strcmp(key, "fused_pack")) {
        ctx->opt_fused_pack = value != 0;
    } else if (!strcmp(key, "nsplit")) {
        if (value < 0 || value > (1 << 24)) return ctx->fail(FSNAP_E_ARG, "nsplit out of range");
        ctx->opt_nsplit = (int)value;
    } else if (!strcmp(key, "nblocks")) {
        if (value < 0 || value > (1 << 24)) return ctx->fail(FSNAP_E_ARG, "nblocks out of range");
        ctx->opt_nblocks = (int)value;
    } else {
        return ctx->fail(FSNAP_E_ARG, "unknown option '%s'", key);
    }
    return FSNAP_OK;
}

int fsnap_upload_rows(fsnap_ctx* ctx, const double* A, int64_t m, int64_t K, int64_t lda, const double* b) {
    if (!ctx) return FSNAP_E_ARG;
    if (!A || !b || m <= 0 || K <= 0 || lda < K) return ctx->fail(FSNAP_E_ARG, "fsnap_upload_rows: bad argument");
    FSNAP_HIP(hipSetDevice(ctx->device), "hipSetDevice");
    // rows are stored densely (lda_dev = K) + 256 B of zeroed tail padding for the
    // 16-byte over-read of the last row
    const size_t abytes = (size_t)m * K * sizeof(double);
    if (!ctx->ownA.ensure(abytes + 256) || !ctx->ownb.ensure((size_t)m * sizeof(double)))
        return ctx->fail(FSNAP_E_NOMEM, "hipMalloc of %zu bytes for A failed", abytes);
    FSNAP_HIP(hipEventRecord(ctx->ev[3], ctx->stream), "hipEventRecord");
    FSNAP_HIP(hipMemsetAsync((char*)ctx->ownA.p + abytes, 0, 256, ctx->stream), "hipMemsetAsync");
    // Large matrices: which way is faster depends on the box.  The runtime's pageable copy of a matrix this size pins the
    // caller's pages and lets the DMA engine read them in place: 1.03 GB in 27 ms (38 GB/s) on the boxes of round 4, 100 ms
    // on the driver's box of round 3.  The page-locked double buffer (staged_rows_h2d) costs host memcpy time instead: 104 ms
    // on the round-4 boxes, whose CPU quota holds four copying threads at ~10 GB/s together, and the first touch of its
    // freshly pinned slots alone cost ~60 ms there (0.6 GB/s over the first 32 MiB) -- a probe of either path on a small
    // piece says nothing about the large copy (a 64 MiB pageable probe ran at 7 GB/s where the 1 GB copy ran at 38).
    // So the default stays the pageable copy (option staged_upload = 0); 2 = double buffer (hosts with free cores and slow
    // pinning), 1 = double buffer that hands the rest to the pageable copy when its first two slots fill at < 20 GB/s.
    size_t done_rows = 0;
    int staged = FSNAP_E_STATE;
    const bool fits = (size_t)K * 8 <= ((size_t)16 << 20);
    if (ctx->opt_staged_upload == 2 && abytes >= ((size_t)8 << 20) && fits) {
        staged = staged_rows_h2d(ctx, ctx->ownA.p, A, (size_t)m, (size_t)K * 8, (size_t)lda * 8, 0.0, &done_rows);
        if (staged != FSNAP_OK && staged != FSNAP_E_NOMEM) return staged;
        if (staged != FSNAP_OK) done_rows = 0;
    } else if (ctx->opt_staged_upload == 1 && abytes >= ((size_t)256 << 20) && fits) {
        double rate = 0.0;
        staged = staged_rows_h2d(ctx, ctx->ownA.p, A, (size_t)m, (size_t)K * 8, (size_t)lda * 8, 20.0e9, &done_rows, &rate);
        if (staged != FSNAP_OK && staged != FSNAP_E_NOMEM) return staged;
        if (staged != FSNAP_OK) done_rows = 0;
        ctx->upload_probe_gbps = rate / 1e9;
    }
    const size_t rest = (size_t)m - done_rows;
    if (rest > 0) {
        staged = FSNAP_E_STATE;                 // (part of) the matrix goes through the runtime's pageable copy
        if (lda == K) {
            FSNAP_HIP(hipMemcpyAsync((char*)ctx->ownA.p + done_rows * (size_t)K * 8, A + done_rows * (size_t)lda, rest * (size_t)K * 8,
                                     hipMemcpyHostToDevice, ctx->stream),
                      "hipMemcpy(A)");
        } else {
            FSNAP_HIP(hipMemcpy2DAsync((char*)ctx->ownA.p + done_rows * (size_t)K * 8, (size_t)K * 8, A + done_rows * (size_t)lda,
                                       (size_t)lda * 8, (size_t)K * 8, rest, hipMemcpyHostToDevice, ctx->stream),
                      "hipMemcpy2D(A)");
        }
    }
    ctx->upload_staged = staged == FSNAP_OK;
    FSNAP_HIP(hipMemcpyAsync(ctx->ownb.p, b, (size_t)m * 8, hipMemcpyHostToDevice, ctx->stream), "hipMemcpy(b)");
    FSNAP_HIP(hipEventRecord(ctx->ev[4], ctx->stream), "hipEventRecord");
    FSNAP_HIP(hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");  // host buffers may be reused now
    ctx->t_upload = true;
    ctx->dA = (const double*)ctx->ownA.p;
    ctx->db = (const double*)ctx->ownb.p;
    ctx->wpack_valid = false;
    if (m != ctx->m) {  // weights / mask of a previous matrix no longer apply
        ctx->dw = nullptr;
        ctx->dmask = nullptr;
        ctx->ntrain_resident = -1;
        ctx->ones.release();
    }
    ctx->m = m;
    ctx->K = K;
    ctx->lda = K;
    cand_forget(ctx);
    robust_forget(ctx, true);
    return FSNAP_OK;
}

int fsnap_drop_rows(fsnap_ctx* ctx) {
    if (!ctx) return FSNAP_E_ARG;
    (void)hipSetDevice(ctx->device);
    if (ctx->stream && !ctx->comm_broken) (void)hipStreamSynchronize(ctx->stream);   // a launch may still read them
    ctx->dA = nullptr;
    ctx->db = nullptr;
    ctx->dw = nullptr;
    ctx->dmask = nullptr;
    ctx->m = 0;
    cand_forget(ctx);
    robust_forget(ctx, true);
    ctx->ntrain_resident = -1;
    ctx->wpack_valid = false;
    ctx->mirror_of = nullptr;
    ctx->ownA.release();
    ctx->ownb.release();
    ctx->ownw.release();
    ctx->ownmask.release();
    ctx->ones.release();
    return FSNAP_OK;
}

int fsnap_bind_rows(fsnap_ctx* ctx, const double* dA, int64_t m, int64_t K, int64_t lda, const double* db) {
    if (!ctx) return FSNAP_E_ARG;
    if (!dA || !db || m <= 0 || K <= 0 || lda < K) return ctx->fail(FSNAP_E_ARG, "fsnap_bind_rows: bad argument");
    if (m != ctx->m) {
        ctx->dw = nullptr;
        ctx->dmask = nullptr;
        ctx->ntrain_resident = -1;
        ctx->ones.release();
    }
    ctx->dA = dA;
    ctx->db = db;
    ctx->wpack_valid = false;
    ctx->m = m;
    ctx->K = K;
    ctx->lda = lda;
    cand_forget(ctx);
    robust_forget(ctx, true);
    return FSNAP_OK;
}

int fsnap_rows_alloc(fsnap_ctx* ctx, int64_t m, int64_t K) {
    if (!ctx) return FSNAP_E_ARG;
    if (m <= 0 || K <= 0) return ctx->fail(FSNAP_E_ARG, "fsnap_rows_alloc: bad argument");
    FSNAP_HIP(hipSetDevice(ctx->device), "hipSetDevice");
    const size_t abytes = (size_t)m * K * sizeof(double);
    if (!ctx->ownA.ensure(abytes + 256) || !ctx->ownb.ensure((size_t)m * 8) || !ctx->ownw.ensure((size_t)m * 8))
        return ctx->fail(FSNAP_E_NOMEM, "hipMalloc of %zu bytes for A failed", abytes);
    FSNAP_HIP(hipMemsetAsync(ctx->ownA.p, 0, abytes + 256, ctx->stream), "hipMemsetAsync(A)");
    FSNAP_HIP(hipMemsetAsync(ctx->ownb.p, 0, (size_t)m * 8, ctx->stream), "hipMemsetAsync(b)");
    FSNAP_HIP(hipMemsetAsync(ctx->ownw.p, 0, (size_t)m * 8, ctx->stream), "hipMemsetAsync(w)");
    FSNAP_HIP(hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");
    ctx->dA = (const double*)ctx->ownA.p;
    ctx->db = (const double*)ctx->ownb.p;
    ctx->wpack_valid = false;
    ctx->dw = (const double*)ctx->ownw.p;
    ctx->dmask = nullptr;
    ctx->ntrain_resident = -1;
    ctx->ones.release();
    ctx->m = m;
    ctx->K = K;
    ctx->lda = K;
    cand_forget(ctx);
    robust_forget(ctx, true);
    return FSNAP_OK;
}

namespace {

struct AssemblyPlanDev {           // device views of a staged batch (fsnap_assemble / fsnap_assemble_accumulate)
    const double* raw;
    const int64_t* src_row;
    const int *kind, *frac;
    const double *d, *truth, *weight, *fractions, *blank2J;
};

// argument checks and H2D staging shared by the two assembly entry points; K = ntypes * (ncoeff + offcol)
int stage_assembly(fsnap_ctx* ctx, const char* who, const double* raw, int64_t raw_rows, int64_t raw_ld, int64_t nrows,
                   const int64_t* src_row, const int32_t* kind, const int32_t* frac, const double* d, const double* truth,
                   const double* weight, const double* fractions, int64_t nfrac, const double* blank2J, int32_t ntypes,
                   int32_t ncoeff, int32_t offcol, AssemblyPlanDev* out) {
    if (!raw || !src_row || !kind || !frac || !d || !truth || !weight || !blank2J || raw_rows <= 0 || nrows <= 0 ||
        ntypes <= 0 || ncoeff <= 0 || (offcol != 0 && offcol != 1) || raw_ld < (int64_t)ntypes * ncoeff + 1 ||
        (nfrac > 0 && !fractions) || raw_rows > 0x7FFFFFFF)
        return ctx->fail(FSNAP_E_ARG, "%s: bad argument", who);
    for (int64_t r = 0; r < nrows; ++r)
        if (src_row[r] < 0 || src_row[r] >= raw_rows || kind[r] < 0 || kind[r] > 3 || frac[r] >= nfrac || frac[r] < -1)
            return ctx->fail(FSNAP_E_ARG, "%s: plan entry %lld out of range", who, (long long)r);
    FSNAP_HIP(hipSetDevice(ctx->device), "hipSetDevice");
    const int64_t K = (int64_t)ntypes * (ncoeff + offcol);
    const size_t rawb = (size_t)raw_rows * raw_ld * 8;
    // plan layout on the device: src_row (8n) | d (8n) | truth (8n) | weight (8n) | kind (4n) | frac (4n)
    const size_t n = (size_t)nrows;
    const size_t planb = n * 40;
    const size_t fracb = (size_t)(nfrac > 0 ? nfrac : 1) * ntypes * 8;
    if (!ctx->st_raw.ensure(rawb) || !ctx->st_plan.ensure(planb) || !ctx->st_frac.ensure(fracb) ||
        !ctx->st_blank.ensure((size_t)K * 8))
        return ctx->fail(FSNAP_E_NOMEM, "hipMalloc(assembly staging) failed");
    char* pl = (char*)ctx->st_plan.p;
    hipStream_t st = ctx->stream;
    // the raw LAMMPS block of the batch (tens of MB): through the page-locked double buffer like fsnap_upload_rows
    int staged = FSNAP_E_STATE;
    if (ctx->opt_staged_upload == 2 && rawb >= ((size_t)8 << 20) && st == ctx->stream) {
        staged = staged_rows_h2d(ctx, ctx->st_raw.p, raw, (size_t)raw_rows, (size_t)raw_ld * 8, (size_t)raw_ld * 8);
        if (staged != FSNAP_OK && staged != FSNAP_E_NOMEM) return staged;
    }
    if (staged != FSNAP_OK) FSNAP_HIP(hipMemcpyAsync(ctx->st_raw.p, raw, rawb, hipMemcpyHostToDevice, st), "hipMemcpy(raw)");
    FSNAP_HIP(hipMemcpyAsync(pl, src_row, n * 8, hipMemcpyHostToDevice, st), "hipMemcpy(plan)");
    FSNAP_HIP(hipMemcpyAsync(pl + n * 8, d, n * 8, hipMemcpyHostToDevice, st), "hipMemcpy(plan)");
    FSNAP_HIP(hipMemcpyAsync(pl + n * 16, truth, n * 8, hipMemcpyHostToDevice, st), "hipMemcpy(plan)");
    FSNAP_HIP(hipMemcpyAsync(pl + n * 24, weight, n * 8, hipMemcpyHostToDevice, st), "hipMemcpy(plan)");
    FSNAP_HIP(hipMemcpyAsync(pl + n * 32, kind, n * 4, hipMemcpyHostToDevice, st), "hipMemcpy(plan)");
    FSNAP_HIP(hipMemcpyAsync(pl + n * 36, frac, n * 4, hipMemcpyHostToDevice, st), "hipMemcpy(plan)");
    if (nfrac > 0)
        FSNAP_HIP(hipMemcpyAsync(ctx->st_frac.p, fractions, (size_t)nfrac * ntypes * 8, hipMemcpyHostToDevice, st),
                  "hipMemcpy(fractions)");
    FSNAP_HIP(hipMemcpyAsync(ctx->st_blank.p, blank2J, (size_t)K * 8, hipMemcpyHostToDevice, st), "hipMemcpy(blank2J)");
    out->raw = (const double*)ctx->st_raw.p;
    out->src_row = (const int64_t*)pl;
    out->d = (const double*)(pl + n * 8);
    out->truth = (const double*)(pl + n * 16);
    out->weight = (const double*)(pl + n * 24);
    out->kind = (const int*)(pl + n * 32);
    out->frac = (const int*)(pl + n * 36);
    out->fractions = (const double*)ctx->st_frac.p;
    out->blank2J = (const double*)ctx->st_blank.p;
    return FSNAP_OK;
}

}  // namespace

int fsnap_assemble(fsnap_ctx* ctx, const double* raw, int64_t raw_rows, int64_t raw_ld, int64_t nrows, int64_t row0,
                   const int64_t* src_row, const int32_t* kind, const int32_t* frac, const double* d,
                   const double* truth, const double* weight, const double* fractions, int64_t nfrac,
                   const double* blank2J, int32_t ntypes, int32_t ncoeff, int32_t offcol) {
    if (!ctx) return FSNAP_E_ARG;
    int rc;
    if ((rc = check_rows(ctx))) return rc;
    if (ctx->dA != (const double*)ctx->ownA.p || ctx->dw != (const double*)ctx->ownw.p)
        return ctx->fail(FSNAP_E_STATE, "fsnap_assemble needs rows allocated by fsnap_rows_alloc");
    if (nrows <= 0 || row0 < 0 || row0 + nrows > ctx->m || ntypes <= 0 || ncoeff <= 0 || (offcol != 0 && offcol != 1) ||
        (int64_t)ntypes * (ncoeff + offcol) != ctx->K)
        return ctx->fail(FSNAP_E_ARG, "fsnap_assemble: bad argument");
    AssemblyPlanDev pd;
    if ((rc = stage_assembly(ctx, "fsnap_assemble", raw, raw_rows, raw_ld, nrows, src_row, kind, frac, d, truth, weight,
                             fractions, nfrac, blank2J, ntypes, ncoeff, offcol, &pd)))
        return rc;
    hipStream_t st = ctx->stream;
    ctx->wpack_valid = false;      // the kernel below writes b and w of these rows
    cand_forget(ctx);
    robust_forget(ctx, true);
    FSNAP_HIP(fsnap::launch_assemble(pd.raw, raw_ld, nrows, pd.src_row, pd.kind, pd.frac, pd.d, pd.truth, pd.weight,
                                     pd.fractions, pd.blank2J, ntypes, ncoeff, offcol,
                                     (double*)ctx->ownA.p + row0 * ctx->lda, ctx->lda, (double*)ctx->ownb.p + row0,
                                     (double*)ctx->ownw.p + row0, st),
              "launch fsnap_assemble_k");
    FSNAP_HIP(hipStreamSynchronize(st), "hipStreamSynchronize");   // host staging may be reused by the caller
    return FSNAP_OK;
}

int fsnap_assemble_accumulate(fsnap_ctx* ctx, const double* raw, int64_t raw_rows, int64_t raw_ld, int64_t nrows,
                              const int64_t* src_row, const int32_t* kind, const int32_t* frac, const double* d,
                              const double* truth, const double* weight, const double* fractions, int64_t nfrac,
                              const double* blank2J, int32_t ntypes, int32_t ncoeff, int32_t offcol, double* d_packed) {
    if (!ctx) return FSNAP_E_ARG;
    if (!d_packed) return ctx->fail(FSNAP_E_ARG, "fsnap_assemble_accumulate: d_packed is NULL");
    ctx->chol_factor_of = nullptr;              // the statistics in d_packed change: neither a factor on the device ...
    if (ctx->mirror_of == d_packed) ctx->mirror_of = nullptr;      // ... nor the host mirror is of them any more
    int rc;
    AssemblyPlanDev pd;
    if ((rc = stage_assembly(ctx, "fsnap_assemble_accumulate", raw, raw_rows, raw_ld, nrows, src_row, kind, frac, d, truth,
                             weight, fractions, nfrac, blank2J, ntypes, ncoeff, offcol, &pd)))
        return rc;
    const int64_t K = (int64_t)ntypes * (ncoeff + offcol);
    // geometry of the tiled kernel for a batch of this shape as fsnap_rows_alloc would hold it (lda = K): the fused
    // launch sums in the order of fsnap_assemble + fsnap_normal_eq_accumulate on the tiled kernel
    TiledGeometry g;
    if ((rc = tiled_geometry(ctx, nrows, K, K, &g))) return rc;
    const int npk = fsnap::pack_weights_num_blocks(nrows);
    const size_t recb = fsnap::assemble_row_record_bytes();
    // per-row scratch: b | w | (w_eff, w_eff b) pairs | row records -- 48 bytes per row, nothing of A
    if (!ctx->fz_rows.ensure((size_t)nrows * (16 + recb + 16) + 64) || !ctx->fz_spart.ensure((size_t)npk * 4 * 8) ||
        !ctx->fz_part.ensure((size_t)g.nsplit * g.npairs * 4096 * sizeof(double)) ||
        !ctx->fz_cpart.ensure((size_t)g.nsplit * g.NSB * 4 * 64 * sizeof(double)))
        return ctx->fail(FSNAP_E_NOMEM, "hipMalloc(fused assembly scratch) failed");
    hipStream_t st = ctx->stream;
    double* db = (double*)ctx->fz_rows.p;
    double* dw = db + nrows;
    double* wpack = dw + nrows;
    char* recs = (char*)(wpack + 2 * nrows);
    FSNAP_HIP(fsnap::launch_assemble_bw(pd.raw, raw_ld, nrows, pd.src_row, pd.kind, pd.frac, pd.d, pd.truth, pd.weight,
                                        ntypes * ncoeff, db, dw, recs, st),
              "launch fsnap_assemble_bw_k");
    FSNAP_HIP(fsnap::launch_pack_weights(db, dw, nullptr, nrows, wpack, (double*)ctx->fz_spart.p, st),
              "launch fsnap_pack_weights_k");
    fsnap::TiledArgs a;
    a.A = nullptr;
    a.lda = K;
    a.wpack = wpack;
    a.m = nrows;
    a.K = (int)K;
    a.NSB = g.NSB;
    a.npairs = g.npairs;
    a.nsplit = g.nsplit;
    a.chunks_per_split = g.cps;
    a.nontemporal = false;
    a.part = (double*)ctx->fz_part.p;
    a.cpart = (double*)ctx->fz_cpart.p;
    a.spart = (const double*)ctx->fz_spart.p;
    a.ns = npk;
    // c slots of waves that own no rows are written (zeros) by the kernel, like kernel 1T's: no memset
    FSNAP_HIP(fsnap::launch_assemble_syrk(pd.raw, raw_ld, recs, pd.d, pd.fractions, pd.blank2J, ntypes, ncoeff, offcol, a, st),
              "launch fsnap_assemble_syrk_k");
    FSNAP_HIP(fsnap::launch_reduce_tiled(a, d_packed, true, st), "launch fsnap_reduce_tiled");
    FSNAP_HIP(hipStreamSynchronize(st), "hipStreamSynchronize");   // host staging may be reused by the caller
    return FSNAP_OK;
}

int fsnap_download_rows(fsnap_ctx* ctx, double* A, int64_t lda, double* b, double* w) {
    if (!ctx) return FSNAP_E_ARG;
    int rc;
    if ((rc = check_rows(ctx))) return rc;
    if (A && lda < ctx->K) return ctx->fail(FSNAP_E_ARG, "fsnap_download_rows: lda < K");
    if (w && !ctx->dw) return ctx->fail(FSNAP_E_STATE, "no weights on the device");
    FSNAP_HIP(hipSetDevice(ctx->device), "hipSetDevice");
    const size_t m = (size_t)ctx->m, K = (size_t)ctx->K;
    if (A)
        FSNAP_HIP(hipMemcpy2DAsync(A, (size_t)lda * 8, ctx->dA, (size_t)ctx->lda * 8, K * 8, m, hipMemcpyDeviceToHost,
                                   ctx->stream),
                  "hipMemcpy2D(A)");
    if (b) FSNAP_HIP(hipMemcpyAsync(b, ctx->db, m * 8, hipMemcpyDeviceToHost, ctx->stream), "hipMemcpy(b)");
    if (w) FSNAP_HIP(hipMemcpyAsync(w, ctx->dw, m * 8, hipMemcpyDeviceToHost, ctx->stream), "hipMemcpy(w)");
    FSNAP_HIP(hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");
    return FSNAP_OK;
}

int fsnap_set_weights(fsnap_ctx* ctx, const double* w, const uint8_t* mask) {
    if (!ctx) return FSNAP_E_ARG;
    int rc;
    if ((rc = check_rows(ctx))) return rc;
    if (!w) return ctx->fail(FSNAP_E_ARG, "fsnap_set_weights: w is NULL");
    FSNAP_HIP(hipSetDevice(ctx->device), "hipSetDevice");
    const size_t m = (size_t)ctx->m;
    if (!ctx->ownw.ensure(m * 8)) return ctx->fail(FSNAP_E_NOMEM, "hipMalloc(w) failed");
    if ((rc = staged_h2d(ctx, ctx->ownw.p, w, m * 8))) return rc;
    ctx->dw = (const double*)ctx->ownw.p;
    ctx->wpack_valid = false;
    robust_forget(ctx, false);
    if (mask) {
        if (!ctx->ownmask.ensure(m)) return ctx->fail(FSNAP_E_NOMEM, "hipMalloc(mask) failed");
        if ((rc = staged_h2d(ctx, ctx->ownmask.p, mask, m))) return rc;
        ctx->dmask = (const unsigned char*)ctx->ownmask.p;
        ctx->ntrain_resident = -1;          // the mask buffer no longer matches the resident prefix sum
    } else {
        ctx->dmask = nullptr;
    }
    return FSNAP_OK;     // asynchronous: the copies are ordered before everything launched later on this context
}

int fsnap_set_weights_train(fsnap_ctx* ctx, const double* w_train, int64_t ntrain, const uint8_t* mask, const int32_t* rank) {
    if (!ctx) return FSNAP_E_ARG;
    int rc;
    if ((rc = check_rows(ctx))) return rc;
    if (!w_train || ntrain < 0 || ntrain > ctx->m || (mask == nullptr) != (rank == nullptr))
        return ctx->fail(FSNAP_E_ARG, "fsnap_set_weights_train: bad argument");
    if (!mask && ctx->ntrain_resident != ntrain)
        return ctx->fail(FSNAP_E_STATE, "fsnap_set_weights_train: no resident training mask with %lld training rows", (long long)ntrain);
    FSNAP_HIP(hipSetDevice(ctx->device), "hipSetDevice");
    const size_t m = (size_t)ctx->m;
    if (!ctx->ownw.ensure(m * 8) || !ctx->wtrain.ensure((size_t)(ntrain > 0 ? ntrain : 1) * 8))
        return ctx->fail(FSNAP_E_NOMEM, "hipMalloc(w) failed");
    if (mask) {
        if (!ctx->ownmask.ensure(m) || !ctx->wrank.ensure(m * 4)) return ctx->fail(FSNAP_E_NOMEM, "hipMalloc(mask) failed");
        if ((rc = staged_h2d(ctx, ctx->ownmask.p, mask, m))) return rc;
        if ((rc = staged_h2d(ctx, ctx->wrank.p, rank, m * 4))) return rc;
        ctx->ntrain_resident = ntrain;
    }
    if ((rc = staged_h2d(ctx, ctx->wtrain.p, w_train, (size_t)ntrain * 8))) return rc;
    FSNAP_HIP(fsnap::launch_expand_weights((const double*)ctx->wtrain.p, (const unsigned char*)ctx->ownmask.p,
                                           (const int*)ctx->wrank.p, ctx->m, (double*)ctx->ownw.p, ctx->stream),
              "launch fsnap_expand_weights_k");
    ctx->dw = (const double*)ctx->ownw.p;
    ctx->dmask = (const unsigned char*)ctx->ownmask.p;
    ctx->wpack_valid = false;
    robust_forget(ctx, false);
    return FSNAP_OK;
}

int fsnap_bind_weights(fsnap_ctx* ctx, const double* dw, const uint8_t* dmask) {
    if (!ctx) return FSNAP_E_ARG;
    int rc;
    if ((rc = check_rows(ctx))) return rc;
    if (!dw) return ctx->fail(FSNAP_E_ARG, "fsnap_bind_weights: dw is NULL");
    ctx->dw = dw;
    ctx->dmask = dmask;
    ctx->wpack_valid = false;
    robust_forget(ctx, false);
    ctx->ntrain_resident = -1;
    return FSNAP_OK;
}

int fsnap_normal_eq_async(fsnap_ctx* ctx, double* d_packed) {
    if (!ctx) return FSNAP_E_ARG;
    if (!d_packed) return ctx->fail(FSNAP_E_ARG, "fsnap_normal_eq_async: d_packed is NULL");
    FSNAP_HIP(hipSetDevice(ctx->device), "hipSetDevice");
    return launch_normal_eq(ctx, d_packed);
}

int fsnap_normal_eq(fsnap_ctx* ctx, double* G, double* c, double* scalars) {
    if (!ctx) return FSNAP_E_ARG;
    int rc;
    if ((rc = check_rows(ctx))) return rc;
    FSNAP_HIP(hipSetDevice(ctx->device), "hipSetDevice");
    const int64_t K = ctx->K;
    if (!ctx->packed.ensure((size_t)FSNAP_PACKED_LEN(K) * 8)) return ctx->fail(FSNAP_E_NOMEM, "hipMalloc(packed) failed");
    double* dp = (double*)ctx->packed.p;
    if ((rc = launch_normal_eq(ctx, dp))) return rc;
    if (G) FSNAP_HIP(hipMemcpyAsync(G, dp, (size_t)K * K * 8, hipMemcpyDeviceToHost, ctx->stream), "hipMemcpy(G)");
    if (c) FSNAP_HIP(hipMemcpyAsync(c, dp + K * K, (size_t)K * 8, hipMemcpyDeviceToHost, ctx->stream), "hipMemcpy(c)");
    if (scalars)
        FSNAP_HIP(hipMemcpyAsync(scalars, dp + K * K + K, 3 * 8, hipMemcpyDeviceToHost, ctx->stream), "hipMemcpy(scalars)");
    FSNAP_HIP(hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");
    return FSNAP_OK;
}

int fsnap_normal_eq_accumulate(fsnap_ctx* ctx, double* d_packed) {
    if (!ctx) return FSNAP_E_ARG;
    if (!d_packed) return ctx->fail(FSNAP_E_ARG, "fsnap_normal_eq_accumulate: d_packed is NULL");
    int rc;
    if ((rc = check_rows(ctx))) return rc;
    FSNAP_HIP(hipSetDevice(ctx->device), "hipSetDevice");
    return launch_normal_eq(ctx, d_packed, false, true);
}

int fsnap_normal_eq_resident(fsnap_ctx* ctx, double** d_packed) {
    if (!ctx) return FSNAP_E_ARG;
    if (!d_packed) return ctx->fail(FSNAP_E_ARG, "fsnap_normal_eq_resident: d_packed is NULL");
    int rc;
    if ((rc = check_rows(ctx))) return rc;
    FSNAP_HIP(hipSetDevice(ctx->device), "hipSetDevice");
    if (!ctx->packed.ensure((size_t)FSNAP_PACKED_LEN(ctx->K) * 8)) return ctx->fail(FSNAP_E_NOMEM, "hipMalloc(packed) failed");
    if ((rc = launch_normal_eq(ctx, (double*)ctx->packed.p, true))) return rc;
    *d_packed = (double*)ctx->packed.p;
    return FSNAP_OK;
}

int fsnap_mirror_packed(fsnap_ctx* ctx, const double* d_packed, int64_t K) {
    if (!ctx) return FSNAP_E_ARG;
    if (!d_packed || K <= 0) return ctx->fail(FSNAP_E_ARG, "fsnap_mirror_packed: bad argument");
    ctx->mirror_of = nullptr;
    if (device_factor(ctx, K)) return FSNAP_OK;     // factorised on the GPU: nothing to mirror
    FSNAP_HIP(hipSetDevice(ctx->device), "hipSetDevice");
    const size_t need = ((size_t)FSNAP_PACKED_LEN(K) + (size_t)K) * 8;
    if (ctx->mirror_bytes < need) {
        if (ctx->mirror) (void)hipHostFree(ctx->mirror);
        ctx->mirror = nullptr;
        ctx->mirror_bytes = 0;
        if (hipHostMalloc((void**)&ctx->mirror, need, hipHostMallocCoherent | hipHostMallocMapped) != hipSuccess)
            return FSNAP_OK;                                 // no mirror: fsnap_solve_device copies instead
        ctx->mirror_bytes = need;
    }
    if (!ctx->mirror_ev && hipEventCreateWithFlags(&ctx->mirror_ev, hipEventDisableTiming) != hipSuccess) {
        ctx->mirror_ev = nullptr;
        return FSNAP_OK;
    }
    FSNAP_HIP(fsnap::launch_mirror_copy(d_packed, (int)K, ctx->mirror, ctx->stream), "launch fsnap_mirror_copy_k");
    FSNAP_HIP(hipEventRecord(ctx->mirror_ev, ctx->stream), "hipEventRecord");
    ctx->mirror_of = d_packed;
    ctx->mirror_K = K;
    ctx->mirror_upper = true;                   // the copy kernel fills the upper triangle (from the pair of the diagonal on)
    ctx->mirror_gen = next_mirror_generation();
    return FSNAP_OK;
}

int fsnap_download_packed(fsnap_ctx* ctx, const double* d_packed, int64_t K, double* G, double* c, double* scalars) {
    if (!ctx) return FSNAP_E_ARG;
    if (!d_packed || K <= 0) return ctx->fail(FSNAP_E_ARG, "fsnap_download_packed: bad argument");
    FSNAP_HIP(hipSetDevice(ctx->device), "hipSetDevice");
    if (G) FSNAP_HIP(hipMemcpyAsync(G, d_packed, (size_t)K * K * 8, hipMemcpyDeviceToHost, ctx->stream), "hipMemcpy(G)");
    if (c) FSNAP_HIP(hipMemcpyAsync(c, d_packed + K * K, (size_t)K * 8, hipMemcpyDeviceToHost, ctx->stream), "hipMemcpy(c)");
    if (scalars)
        FSNAP_HIP(hipMemcpyAsync(scalars, d_packed + K * K + K, 3 * 8, hipMemcpyDeviceToHost, ctx->stream), "hipMemcpy(s)");
    FSNAP_HIP(hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");
    return FSNAP_OK;
}

int fsnap_weight_rows_device(fsnap_ctx* ctx, double* d_aw, int64_t ldaw, double* d_bw) {
    if (!ctx) return FSNAP_E_ARG;
    int rc;
    if ((rc = check_rows(ctx)) || (rc = check_weights(ctx))) return rc;
    if (!d_aw || !d_bw || ldaw < ctx->K) return ctx->fail(FSNAP_E_ARG, "fsnap_weight_rows: bad argument");
    FSNAP_HIP(hipSetDevice(ctx->device), "hipSetDevice");
    const unsigned char* mask = ctx->dmask;
    if (!mask) {
        if ((rc = ensure_ones(ctx))) return rc;
        mask = (const unsigned char*)ctx->ones.p;
    }
    FSNAP_HIP(hipEventRecord(ctx->ev[5], ctx->stream), "hipEventRecord");
    FSNAP_HIP(fsnap::launch_weight_rows(ctx->dA, ctx->lda, ctx->db, ctx->dw, mask, ctx->m, (int)ctx->K, d_aw, ldaw,
                                        d_bw, ctx->stream),
              "launch fsnap_weight_rows_k");
    FSNAP_HIP(hipEventRecord(ctx->ev[6], ctx->stream), "hipEventRecord");
    ctx->t_weight = true;
    return FSNAP_OK;
}

int fsnap_weight_rows(fsnap_ctx* ctx, double* aw, int64_t ldaw, double* bw) {
    if (!ctx) return FSNAP_E_ARG;
    int rc;
    if ((rc = check_rows(ctx))) return rc;
    if (!aw || !bw || ldaw < ctx->K) return ctx->fail(FSNAP_E_ARG, "fsnap_weight_rows: bad argument");
    const size_t m = (size_t)ctx->m, K = (size_t)ctx->K;
    if (!ctx->aw.ensure(m * K * 8) || !ctx->bw.ensure(m * 8)) return ctx->fail(FSNAP_E_NOMEM, "hipMalloc(aw) failed");
    if ((rc = fsnap_weight_rows_device(ctx, (double*)ctx->aw.p, (int64_t)K, (double*)ctx->bw.p))) return rc;
    FSNAP_HIP(hipMemcpy2DAsync(aw, (size_t)ldaw * 8, ctx->aw.p, K * 8, K * 8, m, hipMemcpyDeviceToHost, ctx->stream),
              "hipMemcpy2D(aw)");
    FSNAP_HIP(hipMemcpyAsync(bw, ctx->bw.p, m * 8, hipMemcpyDeviceToHost, ctx->stream), "hipMemcpy(bw)");
    FSNAP_HIP(hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");
    return FSNAP_OK;
}

int fsnap_predict(fsnap_ctx* ctx, const double* beta, double* preds, double* sse) {
    if (!ctx) return FSNAP_E_ARG;
    int rc;
    if ((rc = check_rows(ctx))) return rc;
    if (!beta) return ctx->fail(FSNAP_E_ARG, "fsnap_predict: beta is NULL");
    if (sse && (rc = check_weights(ctx))) return rc;
    FSNAP_HIP(hipSetDevice(ctx->device), "hipSetDevice");
    const size_t m = (size_t)ctx->m, K = (size_t)ctx->K;
    const int nb = fsnap::gemv_num_blocks(ctx->m);
    if (!ctx->beta.ensure(K * 8) || (preds && !ctx->preds.ensure(m * 8)) || (sse && !ctx->sse.ensure((size_t)nb * 8)))
        return ctx->fail(FSNAP_E_NOMEM, "hipMalloc(preds) failed");
    const unsigned char* mask = ctx->dmask;
    if (sse && !mask) {
        if ((rc = ensure_ones(ctx))) return rc;
        mask = (const unsigned char*)ctx->ones.p;
    }
    FSNAP_HIP(hipMemcpyAsync(ctx->beta.p, beta, K * 8, hipMemcpyHostToDevice, ctx->stream), "hipMemcpy(beta)");
    FSNAP_HIP(hipEventRecord(ctx->ev[7], ctx->stream), "hipEventRecord");
    FSNAP_HIP(fsnap::launch_gemv_rows(ctx->dA, ctx->lda, (const double*)ctx->beta.p, ctx->m, (int)ctx->K,
                                      preds ? (double*)ctx->preds.p : nullptr, ctx->db, ctx->dw, mask,
                                      sse ? (double*)ctx->sse.p : nullptr, nullptr, ctx->stream),
              "launch fsnap_gemv_rows_k");
    FSNAP_HIP(hipEventRecord(ctx->ev[8], ctx->stream), "hipEventRecord");
    ctx->t_predict = true;
    if (preds) FSNAP_HIP(hipMemcpyAsync(preds, ctx->preds.p, m * 8, hipMemcpyDeviceToHost, ctx->stream), "hipMemcpy(preds)");
    if (sse) {
        std::string tmp;
        tmp.resize((size_t)nb * 8);
        FSNAP_HIP(hipMemcpyAsync(&tmp[0], ctx->sse.p, (size_t)nb * 8, hipMemcpyDeviceToHost, ctx->stream), "hipMemcpy(sse)");
        FSNAP_HIP(hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");
        const double* ps = (const double*)tmp.data();
        long double s = 0.0L;  // fixed-order host sum of the per-workgroup partials
        for (int i = 0; i < nb; ++i) s += ps[i];
        *sse = (double)s;
    } else {
        FSNAP_HIP(hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");
    }
    return FSNAP_OK;
}

int fsnap_error_stats(fsnap_ctx* ctx, const double* beta, const int32_t* cat, int ncat, double* stats) {
    if (!ctx) return FSNAP_E_ARG;
    int rc;
    if ((rc = check_rows(ctx)) || (rc = check_weights(ctx))) return rc;
    if (!beta || !stats || ncat <= 0) return ctx->fail(FSNAP_E_ARG, "fsnap_error_stats: bad argument");
    if (!cat && (ctx->dcat_rows != ctx->m || !ctx->dcat.p))
        return ctx->fail(FSNAP_E_STATE, "fsnap_error_stats: no categories on the device for these rows");
    if (ncat > 3000) return ctx->fail(FSNAP_E_ARG, "fsnap_error_stats: more than 3000 categories");   // LDS table
    FSNAP_HIP(hipSetDevice(ctx->device), "hipSetDevice");
    const size_t m = (size_t)ctx->m, K = (size_t)ctx->K;
    const int nb = fsnap::error_stats_num_blocks(ctx->m);
    if (!ctx->beta.ensure(K * 8) || !ctx->preds.ensure(m * 8) || !ctx->dcat.ensure(m * 4) ||
        !ctx->dstat.ensure(((size_t)nb * ncat * 6 + (size_t)ncat * 2 + (size_t)ncat * 6) * 8))
        return ctx->fail(FSNAP_E_NOMEM, "hipMalloc(error statistics) failed");
    double* d_partial = (double*)ctx->dstat.p;
    double* d_means = d_partial + (size_t)nb * ncat * 6;
    double* d_table = d_means + (size_t)ncat * 2;                 // per-category sums of a pass, folded over the workgroups
    FSNAP_HIP(hipMemcpyAsync(ctx->beta.p, beta, K * 8, hipMemcpyHostToDevice, ctx->stream), "hipMemcpy(beta)");
    if (cat) {
        FSNAP_HIP(hipMemcpyAsync(ctx->dcat.p, cat, m * 4, hipMemcpyHostToDevice, ctx->stream), "hipMemcpy(categories)");
        ctx->dcat_rows = ctx->m;
    }
    FSNAP_HIP(fsnap::launch_gemv_rows(ctx->dA, ctx->lda, (const double*)ctx->beta.p, ctx->m, (int)ctx->K, (double*)ctx->preds.p,
                                      ctx->db, ctx->dw, nullptr, nullptr, nullptr, ctx->stream),
              "launch fsnap_gemv_rows_k");
    std::vector<double> h((size_t)ncat * 6), means((size_t)ncat * 2);
    // pass 0: counts and sums -> category means.  The per-workgroup tables are folded on the device (fixed order); only
    // ncat x 4 doubles come back (the host used to add 245 tables of ncat x 4 entries itself: ~1 ms at 240 categories)
    FSNAP_HIP(fsnap::launch_error_stats(ctx->db, (const double*)ctx->preds.p, ctx->dw, (const int*)ctx->dcat.p, ctx->m, ncat, 0,
                                        nullptr, d_partial, ctx->stream),
              "launch fsnap_error_stats_k");
    FSNAP_HIP(fsnap::launch_colsum(d_partial, nb, ncat * 4, d_table, ctx->stream), "launch fsnap_colsum_partials_k");
    FSNAP_HIP(hipMemcpyAsync(h.data(), d_table, (size_t)ncat * 4 * 8, hipMemcpyDeviceToHost, ctx->stream), "hipMemcpy(stats)");
    FSNAP_HIP(hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");
    for (int c = 0; c < ncat; ++c) {
        const double* e = h.data() + (size_t)c * 4;
        double* o = stats + (size_t)c * 10;
        o[0] = e[0]; o[1] = e[1]; o[2] = e[2]; o[3] = e[3];
        means[2 * c] = e[0] > 0 ? e[2] / e[0] : 0.0;            // (truths / n).sum()
        means[2 * c + 1] = e[1] > 0 ? e[3] / e[1] : 0.0;        // (w * truths / n_w).sum()
    }
    FSNAP_HIP(hipMemcpyAsync(d_means, means.data(), (size_t)ncat * 2 * 8, hipMemcpyHostToDevice, ctx->stream), "hipMemcpy(means)");
    FSNAP_HIP(fsnap::launch_error_stats(ctx->db, (const double*)ctx->preds.p, ctx->dw, (const int*)ctx->dcat.p, ctx->m, ncat, 1,
                                        d_means, d_partial, ctx->stream),
              "launch fsnap_error_stats_k");
    FSNAP_HIP(fsnap::launch_colsum(d_partial, nb, ncat * 6, d_table, ctx->stream), "launch fsnap_colsum_partials_k");
    FSNAP_HIP(hipMemcpyAsync(h.data(), d_table, (size_t)ncat * 6 * 8, hipMemcpyDeviceToHost, ctx->stream), "hipMemcpy(stats)");
    FSNAP_HIP(hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");
    for (int c = 0; c < ncat; ++c) {
        double* o = stats + (size_t)c * 10;
        for (int k = 0; k < 6; ++k) o[4 + k] = h[(size_t)c * 6 + k];
    }
    return FSNAP_OK;
}

int fsnap_solve_device(fsnap_ctx* ctx, int kind, double param, int64_t K, const double* d_packed, double* beta,
                       int* rank, double* rcond_est) {
    return fsnap_solve_device_rhs(ctx, kind, param, K, d_packed, nullptr, beta, rank, rcond_est);
}

int fsnap_solve_device_rhs(fsnap_ctx* ctx, int kind, double param, int64_t K, const double* d_packed, const double* rhs,
                           double* beta, int* rank, double* rcond_est) {
    if (!ctx) return FSNAP_E_ARG;
    if (!d_packed || !beta || K <= 0 || kind < FSNAP_SOLVE_CHOL || kind > FSNAP_SOLVE_RIDGE_INV_PROBE)
        return ctx->fail(FSNAP_E_ARG, "fsnap_solve_device: bad argument");
    FSNAP_HIP(hipSetDevice(ctx->device), "hipSetDevice");
    const double alpha = (kind == FSNAP_SOLVE_RIDGE || kind == FSNAP_SOLVE_RIDGE_INV || kind == FSNAP_SOLVE_RIDGE_PROBE ||
                          kind == FSNAP_SOLVE_RIDGE_INV_PROBE) ? param : 0.0;
    // large systems: blocked Cholesky on the GPU (kernels 8a-8e); option device_solve = 2 disables it
    // (threshold and measurements: fsnap::DEVICE_CHOL_MIN_K; below it the host is faster: the panel kernels are latency-bound
    // launches)
    if (device_factor(ctx, K)) {
        const int n = (int)K, np = (n + 63) / 64 * 64, npanel = np / 64;
        const size_t head = (size_t)n + npanel + 1;            // [beta | min pivots | status]
        constexpr int NPR = fsnap::CHOL_PROBES;
        const size_t head_all = head + (size_t)NPR * NPR;      // ... | Z^T Z of the probes (condition estimate, LSTSQ kinds)
        if (!ctx->dchol.ensure(fsnap::chol_large_work_doubles(n) * 8) || !ctx->dsolve.ensure((head + 2 * (size_t)np) * 8))
            return ctx->fail(FSNAP_E_NOMEM, "hipMalloc(device Cholesky) failed");
        double* dv = (double*)ctx->dsolve.p;
        double* d_beta = dv;
        double* d_minpiv = dv + n;
        int* d_status = (int*)(dv + n + npanel);
        double* d_dsc = dv + head;
        double* d_z = d_dsc + np;
        // results come back through page-locked, GPU-visible host memory written by the last launch of the chain (the
        // host polls an event: no D2H copy, whose launch latency was ~10 us); the plain staging buffer + copy remain
        // as the fallback when that allocation fails
        if (ctx->chol_host_bytes < head_all * 8) {
            if (ctx->chol_host) (void)hipHostFree(ctx->chol_host);
            ctx->chol_host = nullptr;
            ctx->chol_host_bytes = 0;
            if (hipHostMalloc((void**)&ctx->chol_host, head_all * 8, hipHostMallocCoherent | hipHostMallocMapped) == hipSuccess)
                ctx->chol_host_bytes = head_all * 8;
        }
        if (ctx->chol_host && !ctx->chol_ev && hipEventCreateWithFlags(&ctx->chol_ev, hipEventDisableTiming) != hipSuccess)
            ctx->chol_ev = nullptr;
        double* host_out = (ctx->chol_host && ctx->chol_ev) ? ctx->chol_host : nullptr;
        if (!host_out && ctx->pinned_bytes < head * 8) {
            if (ctx->pinned) (void)hipHostFree(ctx->pinned);
            ctx->pinned = nullptr;
            ctx->pinned_bytes = 0;
            if (hipHostMalloc((void**)&ctx->pinned, head * 8, hipHostMallocDefault) != hipSuccess)
                return ctx->fail(FSNAP_E_NOMEM, "hipHostMalloc(%zu) failed", head * 8);
            ctx->pinned_bytes = head * 8;
        }
        const double* d_rhs = nullptr;
        if (rhs) {
            if (!ctx->dsvec.ensure((size_t)n * 8)) return ctx->fail(FSNAP_E_NOMEM, "hipMalloc(rhs) failed");
            FSNAP_HIP(hipMemcpyAsync(ctx->dsvec.p, rhs, (size_t)n * 8, hipMemcpyHostToDevice, ctx->stream), "hipMemcpy(rhs)");
            d_rhs = (const double*)ctx->dsvec.p;
        }
        // a right-hand side of its own for statistics this context has just factorised (the refinement steps of a fit): the
        // factor, the scaling and the inverses of the diagonal blocks are still in the work buffers -- two sweeps instead of a
        // factorisation (kernel 8f + the backward sweep)
        const bool lstsq = kind == FSNAP_SOLVE_LSTSQ || kind == FSNAP_SOLVE_LSTSQ_PROBE;
        const bool reuse = rhs && host_out && ctx->opt_chol_reuse && ctx->chol_factor_of == d_packed && ctx->chol_factor_K == K &&
                           ctx->chol_factor_alpha == alpha;
        if (reuse) {
            FSNAP_HIP(fsnap::launch_chol_resolve(d_rhs, n, (double*)ctx->dchol.p, d_dsc, d_z, d_beta, d_status, d_minpiv, host_out,
                                                 ctx->stream),
                      "launch device Cholesky (sweeps)");
            FSNAP_HIP(hipEventRecord(ctx->chol_ev, ctx->stream), "hipEventRecord");
            int wrc;
            if ((wrc = fsnap::wait_stream(ctx, ctx->chol_ev, "device Cholesky sweeps"))) return wrc;
            int status;
            memcpy(&status, host_out + n + npanel, sizeof(int));
            bool fin = status == 0;
            for (int i = 0; i < n && fin; ++i) fin = (host_out[i] - host_out[i] == 0.0);
            if (fin) {
                double mp = 1.0e300;
                for (int p = 0; p < npanel; ++p) mp = host_out[n + p] < mp ? host_out[n + p] : mp;
                for (int i = 0; i < n; ++i) beta[i] = host_out[i];
                if (rank) *rank = n;
                if (rcond_est) *rcond_est = ctx->chol_factor_rcond;         // of the factor, as its own solve reported it
                fsnap_cond_note(ctx->chol_factor_piv, ctx->chol_factor_lam, 0, 1);
                return FSNAP_OK;
            }
            ctx->chol_factor_of = nullptr;          // (a non-finite right-hand side: the full path below reports it)
        }
        ctx->chol_factor_of = nullptr;
        // the status word lives behind beta and the pivots: its address depends on K.  The chain leaves it cleared; a
        // clearing launch is needed only when this word has not been through a chain yet
        const bool clear_status = ctx->chol_status_word != (const void*)d_status;
        ctx->chol_status_word = host_out ? (const void*)d_status : nullptr;
        FSNAP_HIP(fsnap::launch_chol_large(d_packed, d_rhs, n, alpha, (double*)ctx->dchol.p, d_dsc, d_z, d_beta, d_status,
                                           d_minpiv, host_out, clear_status, (lstsq && host_out) ? host_out + head : nullptr, ctx->stream),
                  "launch device Cholesky");
        const double* h;
        if (host_out) {
            FSNAP_HIP(hipEventRecord(ctx->chol_ev, ctx->stream), "hipEventRecord");
            int wrc;
            if ((wrc = fsnap::wait_stream(ctx, ctx->chol_ev, "device Cholesky"))) return wrc;
            h = host_out;
        } else {
            FSNAP_HIP(hipMemcpyAsync(ctx->pinned, dv, head * 8, hipMemcpyDeviceToHost, ctx->stream), "hipMemcpy(beta)");
            int wrc;
            if ((wrc = fsnap::wait_stream(ctx, nullptr, "device Cholesky"))) return wrc;
            h = ctx->pinned;
        }
        int status;
        memcpy(&status, h + n + npanel, sizeof(int));
        double mp = 1.0e300;
        for (int p = 0; p < npanel; ++p) mp = h[n + p] < mp ? h[n + p] : mp;
        if (getenv("FSNAP_SOLVE_TIMING"))
            fprintf(stderr, "[fsnap_solve_device] blocked Cholesky on the GPU: K = %d, status %d, min pivot %.3e, beta[0] %.6e\n", n,
                    status, mp, h[0]);
        if (status == 0 && mp > 1.0e-3) {
            bool fin = true;
            for (int i = 0; i < n; ++i) fin = fin && (h[i] - h[i] == 0.0);
            if (fin) {
                for (int i = 0; i < n; ++i) beta[i] = h[i];
                // LSTSQ stands in for an SVD of the rows, which knows the conditioning; the smallest pivot bounds lambda_min of
                // the scaled matrix from above only.  The factorisation carried 31 probe vectors in its right-hand-side strip:
                // Z^T Z = B^T S^-1 B came back with the results, its largest generalised eigenvalue against B^T B is a lower
                // bound of 1 / lambda_min that holds at least ~0.4 x 31 / K of it (fsnap_chol_probe_gram_k) -- so the estimate
                // 1 / theta is scaled by 120 / K: what the host layer divides by its margin of 10 is then below lambda_min.
                // No sweep with the factor (round 6's first form ran 2 ... 5 Lanczos steps of 0.06 ... 0.40 ms each here).
                // Same bits on every rank: deterministic kernels on bit-identical statistics.
                fsnap::CondEstimate ce;
                if (lstsq && host_out) {
                    if (ctx->probe_n != n) {
                        ctx->probe_gram.assign((size_t)NPR * NPR, 0.0);
                        std::vector<double> row(NPR);
                        for (int r = 0; r < n; ++r) {
                            for (int p = 0; p < NPR; ++p) row[p] = fsnap::chol_probe(r, p + 1);
                            for (int p = 0; p < NPR; ++p)
                                for (int q = 0; q < NPR; ++q) ctx->probe_gram[(size_t)p * NPR + q] += row[p] * row[q];
                        }
                        ctx->probe_n = n;
                    }
                    const double theta = fsnap_gen_eig_max(host_out + head, ctx->probe_gram.data(), NPR);
                    ce.steps = 1;
                    ce.lambda_min = theta > 0.0 ? (1.0 / theta) * (n > 120 ? 120.0 / n : 1.0) : 0.0;
                }
                const double rc_est = (ce.steps && ce.lambda_min < mp) ? ce.lambda_min : mp;
                fsnap_cond_note(mp, ce.lambda_min, ce.steps, 1);
                if (!ce.steps || ce.lambda_min > 64.0 * n * std::numeric_limits<double>::epsilon()) {
                    if (rank) *rank = n;
                    if (rcond_est) *rcond_est = rc_est;
                    // the factor of these statistics stays on the device for further right-hand sides.  Only for the
                    // context's OWN statistics buffer: every launch that rewrites it clears the tag, while a caller-owned
                    // device buffer can change behind the library's back (a torch tensor accumulated between solves)
                    if (d_packed == (const double*)ctx->packed.p) {
                        ctx->chol_factor_of = d_packed;
                        ctx->chol_factor_K = K;
                        ctx->chol_factor_alpha = alpha;
                        ctx->chol_factor_rcond = rc_est;
                        ctx->chol_factor_piv = mp;
                        ctx->chol_factor_lam = ce.lambda_min;
                    }
                    return FSNAP_OK;
                }
                // every pivot passed and the factor still says lambda_min is at the rounding level of the statistics: for
                // a probe that is "unresolved" (the caller goes to the rows); the plain kinds take the general host path
                if (kind >= FSNAP_SOLVE_LSTSQ_PROBE) {
                    for (int i = 0; i < n; ++i) beta[i] = 0.0;
                    if (rank) *rank = -1;
                    if (rcond_est) *rcond_est = rc_est > 0.0 ? rc_est : 0.0;
                    return FSNAP_OK;
                }
            }
        }
        // A probe (FSNAP_SOLVE_*_PROBE: "come straight back when no Cholesky factorisation resolves the system") whose
        // factorisation met a non-positive pivot, or one below the host path's own acceptance threshold 64 n eps, is unresolved
        // for the host Cholesky too -- the same algorithm on the same matrix.  Downloading G (20 MB at K = 1595) for two more
        // failing factorisations cost 36 ms of an 87 ms ill-conditioned SVD fit at 15 213 x 1 595.
        if (kind >= FSNAP_SOLVE_LSTSQ_PROBE && !(status & 1) &&
            ((status & 2) || !(mp > 64.0 * n * std::numeric_limits<double>::epsilon()))) {
            for (int i = 0; i < n; ++i) beta[i] = 0.0;
            if (rank) *rank = -1;
            if (rcond_est) *rcond_est = (mp > 0.0 && mp < 1.0e300) ? mp : 0.0;
            return FSNAP_OK;
        }
        // ill-conditioned / indefinite / non-finite: the general host path decides
    }
    // statistics already mirrored in page-locked host memory by the reduction kernel: wait for it (polling the
    // event: the blocking wait's wake-up latency is several microseconds) and solve
    if (ctx->mirror_of == d_packed && ctx->mirror && K == ctx->mirror_K) {
        int wrc;
        if ((wrc = fsnap::wait_stream(ctx, ctx->mirror_ev, "statistics mirror"))) return wrc;
        const double* Gm = ctx->mirror;
        // tagged with (context, fill count of the mirror): the refinement solves of a fit reuse the factor of its first solve
        const int rcm = fsnap_solve_diag_tagged(kind, param, K, Gm, rhs ? rhs : Gm + K * K, Gm + K * K + K + 3, beta, rank, rcond_est,
                                                ctx->mirror_upper ? 1 : 0, ctx, ctx->mirror_gen);
        if (rcm) ctx->fail(rcm, "fsnap_solve: numerical status %d", rcm);
        return rcm;
    }
    // general path: statistics to the host (page-locked staging), full solver
    const size_t need = (size_t)(K * K + K) * 8;
    if (ctx->pinned_bytes < need) {
        if (ctx->pinned) (void)hipHostFree(ctx->pinned);
        ctx->pinned = nullptr;
        ctx->pinned_bytes = 0;
        if (hipHostMalloc((void**)&ctx->pinned, need, hipHostMallocDefault) != hipSuccess)
            return ctx->fail(FSNAP_E_NOMEM, "hipHostMalloc(%zu) failed", need);
        ctx->pinned_bytes = need;
    }
    FSNAP_HIP(hipMemcpyAsync(ctx->pinned, d_packed, need, hipMemcpyDeviceToHost, ctx->stream), "hipMemcpy(G)");
    {
        int wrc;
        if ((wrc = fsnap::wait_stream(ctx, nullptr, "statistics download"))) return wrc;
    }
    const double* G = ctx->pinned;
    const int rc = fsnap_solve(kind, param, K, G, rhs ? rhs : G + K * K, beta, rank, rcond_est);
    if (rc) ctx->fail(rc, "fsnap_solve: numerical status %d", rc);
    return rc;
}

int fsnap_fit_resident(fsnap_ctx* ctx, int kind, double param, double* beta, int* rank, double* rcond_est,
                       double** d_packed) {
    if (!ctx) return FSNAP_E_ARG;
    double* dp = nullptr;
    int rc = fsnap_normal_eq_resident(ctx, &dp);
    if (rc) return rc;
    if (d_packed) *d_packed = dp;
    // tiled kernel + host factorisation (144 < K < DEVICE_CHOL_MIN_K): a copy kernel fills the page-locked mirror the host solve polls
    // -- the D2H copy it replaces cost 10 us of launch latency + 7.7 us on the ACE shape (13 035 x 142: 95 us per fit)
    if (ctx->mirror_of != dp && ctx->K > 128 && (rc = fsnap_mirror_packed(ctx, dp, ctx->K))) return rc;     // (no-op from DEVICE_CHOL_MIN_K on)
    return fsnap_solve_device_rhs(ctx, kind, param, ctx->K, dp, nullptr, beta, rank, rcond_est);
}

int fsnap_fit_dist(fsnap_ctx* ctx, int kind, double param, int64_t K, double* beta, int* rank, double* rcond_est,
                   double** d_packed) {
    if (!ctx) return FSNAP_E_ARG;
    if (d_packed) *d_packed = nullptr;
    if (!beta || K <= 0) return ctx->fail(FSNAP_E_ARG, "fsnap_fit_dist: bad argument");
    // no silent single-GPU fallback: a job that lost its communicator (context re-created after ParallelTools.free())
    // would otherwise fit every rank's own shard and publish rank 0's as the global fit
    if (!ctx->comm) return ctx->fail(FSNAP_E_STATE, "fsnap_fit_dist: no communicator (fsnap_comm_init first; single-GPU fits call fsnap_fit_resident)");
    FSNAP_HIP(hipSetDevice(ctx->device), "hipSetDevice");
    const int64_t n = FSNAP_PACKED_LEN(K);
    // the one thing a rank cannot recover from locally: without the buffer it cannot take part in the collective at all
    // (its peers run into FSNAP_COMM_TIMEOUT)
    if (!ctx->packed.ensure((size_t)n * 8) || !fsnap::allreduce_packed_reserve(ctx, K))
        return ctx->fail(FSNAP_E_NOMEM, "hipMalloc(packed) failed");
    double* dp = (double*)ctx->packed.p;
    // Everything that can fail on THIS rank alone happens before the collective -- and must not keep the rank out of
    // it (the peers would wait forever): a rank that fails contributes a buffer of NaNs, every rank then sees
    // non-finite statistics and returns FSNAP_NUM_NONFINITE, the failing rank returns its own error.
    const bool have_rows = ctx->dA && ctx->m > 0;
    int local_rc = FSNAP_OK;
    std::string local_err;
    ctx->cur_events = nullptr;
    if (have_rows && ctx->K != K) {
        local_rc = ctx->fail(FSNAP_E_ARG, "fsnap_fit_dist: K = %lld but the resident rows have %lld columns", (long long)K,
                             (long long)ctx->K);
    } else if (have_rows) {
        local_rc = launch_normal_eq(ctx, dp);
    } else {
        ctx->mirror_of = nullptr;
        if (hipMemsetAsync(dp, 0, (size_t)n * 8, ctx->stream) != hipSuccess)   // a rank without rows
            local_rc = ctx->fail(FSNAP_E_HIP, "hipMemsetAsync(packed) failed");
    }
    if (local_rc != FSNAP_OK) {
        local_err = ctx->err;
        ctx->mirror_of = nullptr;
        ctx->cur_events = nullptr;
        (void)hipMemsetAsync(dp, 0xFF, (size_t)n * 8, ctx->stream);            // all bits set = NaN in every double
    }
    hipEvent_t* evs = ctx->cur_events;
    int rc;
    {
        if ((rc = fsnap::allreduce_packed(ctx, dp, K))) return rc;       // wide systems: the upper triangle only
        if (evs) {
            FSNAP_HIP(hipEventRecord(evs[3], ctx->stream), "hipEventRecord");
            ctx->ring_comm[(ctx->nfit - 1) % fsnap_ctx::RING] = true;
        }
        if (local_rc == FSNAP_OK) {
            if ((rc = fsnap_mirror_packed(ctx, dp, K))) return rc;     // host-factorised orders: page-locked mirror instead of a D2H copy
            if (d_packed) *d_packed = dp;
            rc = fsnap_solve_device_rhs(ctx, kind, param, K, dp, nullptr, beta, rank, rcond_est);
        }
    }
    if (local_rc != FSNAP_OK) return ctx->fail(local_rc, "%s", local_err.c_str());
    if (rc == FSNAP_NUM_NONFINITE)
        ctx->fail(rc, "non-finite statistics after the all-reduce: NaN/Inf in a training row of some rank, or a rank failed "
                      "before the collective (see that rank's error)");
    return rc;
}

int fsnap_dev_alloc(fsnap_ctx* ctx, int64_t nbytes, void** d_ptr) {
    if (!ctx) return FSNAP_E_ARG;
    if (!d_ptr || nbytes <= 0) return ctx->fail(FSNAP_E_ARG, "fsnap_dev_alloc: bad argument");
    *d_ptr = nullptr;
    FSNAP_HIP(hipSetDevice(ctx->device), "hipSetDevice");
    const hipError_t e = hipMalloc(d_ptr, (size_t)nbytes);
    if (e != hipSuccess) {
        *d_ptr = nullptr;
        return ctx->hipfail(e, "hipMalloc");
    }
    return FSNAP_OK;
}

int fsnap_dev_free(fsnap_ctx* ctx, void* d_ptr) {
    if (!ctx) return FSNAP_E_ARG;
    if (!d_ptr) return FSNAP_OK;
    FSNAP_HIP(hipSetDevice(ctx->device), "hipSetDevice");
    FSNAP_HIP(hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");     // nothing in flight may still use it
    FSNAP_HIP(hipFree(d_ptr), "hipFree");
    return FSNAP_OK;
}

int fsnap_dev_upload(fsnap_ctx* ctx, void* d_dst, const void* h_src, int64_t nbytes) {
    if (!ctx) return FSNAP_E_ARG;
    if (!d_dst || !h_src || nbytes <= 0) return ctx->fail(FSNAP_E_ARG, "fsnap_dev_upload: bad argument");
    FSNAP_HIP(hipSetDevice(ctx->device), "hipSetDevice");
    ctx->chol_factor_of = nullptr;              // (the destination may be a statistics buffer)
    FSNAP_HIP(hipMemcpyAsync(d_dst, h_src, (size_t)nbytes, hipMemcpyHostToDevice, ctx->stream), "hipMemcpy(H2D)");
    FSNAP_HIP(hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");
    return FSNAP_OK;
}

int fsnap_dev_download(fsnap_ctx* ctx, void* h_dst, const void* d_src, int64_t nbytes) {
    if (!ctx) return FSNAP_E_ARG;
    if (!h_dst || !d_src || nbytes <= 0) return ctx->fail(FSNAP_E_ARG, "fsnap_dev_download: bad argument");
    FSNAP_HIP(hipSetDevice(ctx->device), "hipSetDevice");
    FSNAP_HIP(hipMemcpyAsync(h_dst, d_src, (size_t)nbytes, hipMemcpyDeviceToHost, ctx->stream), "hipMemcpy(D2H)");
    FSNAP_HIP(hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");
    return FSNAP_OK;
}

int fsnap_dev_sync(fsnap_ctx* ctx) {
    if (!ctx) return FSNAP_E_ARG;
    FSNAP_HIP(hipSetDevice(ctx->device), "hipSetDevice");
    FSNAP_HIP(hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");
    return FSNAP_OK;
}

int fsnap_residual_rhs(fsnap_ctx* ctx, const double* beta, double* s, double* sse) {
    if (!ctx) return FSNAP_E_ARG;
    int rc;
    if ((rc = check_rows(ctx)) || (rc = check_weights(ctx))) return rc;
    if (!beta || !s) return ctx->fail(FSNAP_E_ARG, "fsnap_residual_rhs: NULL argument");
    FSNAP_HIP(hipSetDevice(ctx->device), "hipSetDevice");
    const size_t m = (size_t)ctx->m, K = (size_t)ctx->K;
    // K <= 288: kernels 4 + 7 fused, the rows are read once (option fused_residual = 0: the two-kernel form, A/B)
    const bool fused = ctx->opt_fused_residual && K <= 288;
    const int nb = fused ? fsnap::residual_num_blocks(ctx->m, (int)ctx->K) : fsnap::gemv_num_blocks(ctx->m);
    const int nbt = fused ? nb : fsnap::gemvT_num_blocks(ctx->m);
    if (!ctx->beta.ensure(K * 8) || (!fused && !ctx->du.ensure(m * 8)) || !ctx->dspart.ensure((size_t)nbt * K * 8) ||
        !ctx->dsvec.ensure(K * 8) || (sse && !ctx->sse.ensure((size_t)nb * 8)))
        return ctx->fail(FSNAP_E_NOMEM, "hipMalloc(refinement) failed");
    const unsigned char* mask = ctx->dmask;
    if (!mask) {
        if ((rc = ensure_ones(ctx))) return rc;
        mask = (const unsigned char*)ctx->ones.p;
    }
    FSNAP_HIP(hipMemcpyAsync(ctx->beta.p, beta, K * 8, hipMemcpyHostToDevice, ctx->stream), "hipMemcpy(beta)");
    if (fused) {
        FSNAP_HIP(fsnap::launch_residual_rows(ctx->dA, ctx->lda, (const double*)ctx->beta.p, ctx->m, (int)ctx->K, ctx->db, ctx->dw,
                                              mask, (double*)ctx->dspart.p, sse ? (double*)ctx->sse.p : nullptr,
                                              (double*)ctx->dsvec.p, ctx->stream),
                  "launch fsnap_residual_rows_k");
    } else {
        FSNAP_HIP(fsnap::launch_gemv_rows(ctx->dA, ctx->lda, (const double*)ctx->beta.p, ctx->m, (int)ctx->K, nullptr, ctx->db,
                                          ctx->dw, mask, sse ? (double*)ctx->sse.p : nullptr, (double*)ctx->du.p, ctx->stream),
                  "launch fsnap_gemv_rows_k");
        FSNAP_HIP(fsnap::launch_gemvT_rows(ctx->dA, ctx->lda, (const double*)ctx->du.p, ctx->m, (int)ctx->K,
                                           (double*)ctx->dspart.p, (double*)ctx->dsvec.p, ctx->stream),
                  "launch fsnap_gemvT_rows_k");
    }
    FSNAP_HIP(hipMemcpyAsync(s, ctx->dsvec.p, K * 8, hipMemcpyDeviceToHost, ctx->stream), "hipMemcpy(s)");
    if (sse) {
        std::string tmp;
        tmp.resize((size_t)nb * 8);
        FSNAP_HIP(hipMemcpyAsync(&tmp[0], ctx->sse.p, (size_t)nb * 8, hipMemcpyDeviceToHost, ctx->stream), "hipMemcpy(sse)");
        FSNAP_HIP(hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");
        const double* ps = (const double*)tmp.data();
        long double acc = 0.0L;
        for (int i = 0; i < nb; ++i) acc += ps[i];
        *sse = (double)acc;
    } else {
        FSNAP_HIP(hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");
    }
    return FSNAP_OK;
}

int fsnap_merr_eval(fsnap_ctx* ctx, int method, int64_t K, const double* c, const double* q, double d, double* val,
                    double* g, double* h) {
    if (!ctx) return FSNAP_E_ARG;
    int rc;
    if ((rc = check_rows(ctx)) || (rc = check_weights(ctx))) return rc;
    if (!c || !q || !val || !g || !h) return ctx->fail(FSNAP_E_ARG, "fsnap_merr_eval: NULL argument");
    if (K != ctx->K) return ctx->fail(FSNAP_E_ARG, "fsnap_merr_eval: K = %lld, the resident rows have %lld columns",
                                      (long long)K, (long long)ctx->K);
    if (method != FSNAP_MERR_IID && method != FSNAP_MERR_ABC && method != FSNAP_MERR_FULL)
        return ctx->fail(FSNAP_E_ARG, "fsnap_merr_eval: unknown method %d", method);
    if (K > 0x3FFFFFFF) return ctx->fail(FSNAP_E_ARG, "fsnap_merr_eval: K = %lld too large", (long long)K);
    FSNAP_HIP(hipSetDevice(ctx->device), "hipSetDevice");
    const int nb = fsnap::merr_num_blocks(ctx->m, (int)K);
    const bool two = K > fsnap::MERR_ONE_PASS_MAX_K;
    const size_t nout = 2 * (size_t)K + 1;
    if (!ctx->merr_cq.ensure(2 * (size_t)K * 8) || !ctx->merr_part.ensure((size_t)nb * nout * 8) ||
        !ctx->merr_out.ensure(nout * 8) ||
        (two && (!ctx->merr_u.ensure(2 * (size_t)ctx->m * 8) || !ctx->merr_vpart.ensure((size_t)nb * 8))))
        return ctx->fail(FSNAP_E_NOMEM, "hipMalloc(merr) failed");
    const unsigned char* mask = ctx->dmask;
    if (!mask) {
        if ((rc = ensure_ones(ctx))) return rc;
        mask = (const unsigned char*)ctx->ones.p;
    }
    double* dcq = (double*)ctx->merr_cq.p;
    FSNAP_HIP(hipMemcpyAsync(dcq, c, (size_t)K * 8, hipMemcpyHostToDevice, ctx->stream), "hipMemcpy(c)");
    FSNAP_HIP(hipMemcpyAsync(dcq + K, q, (size_t)K * 8, hipMemcpyHostToDevice, ctx->stream), "hipMemcpy(q)");
    FSNAP_HIP(fsnap::launch_merr(ctx->dA, ctx->lda, dcq, ctx->m, (int)K, ctx->db, ctx->dw, mask,
                                 method == FSNAP_MERR_ABC ? fsnap::MERR_ABC : fsnap::MERR_IID, d,
                                 two ? (double*)ctx->merr_u.p : nullptr, two ? (double*)ctx->merr_vpart.p : nullptr,
                                 (double*)ctx->merr_part.p, (double*)ctx->merr_out.p, ctx->stream),
              "launch fsnap_merr_rows_k");
    const double* out = (const double*)ctx->merr_out.p;
    FSNAP_HIP(hipMemcpyAsync(g, out, (size_t)K * 8, hipMemcpyDeviceToHost, ctx->stream), "hipMemcpy(g)");
    FSNAP_HIP(hipMemcpyAsync(h, out + K, (size_t)K * 8, hipMemcpyDeviceToHost, ctx->stream), "hipMemcpy(h)");
    FSNAP_HIP(hipMemcpyAsync(val, out + 2 * K, 8, hipMemcpyDeviceToHost, ctx->stream), "hipMemcpy(val)");
    FSNAP_HIP(hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");
    return FSNAP_OK;
}

int fsnap_sse_batch(fsnap_ctx* ctx, int64_t K, const double* U, int P, double* sse, int64_t* n_train) {
    if (!ctx) return FSNAP_E_ARG;
    if (!U || !sse) return ctx->fail(FSNAP_E_ARG, "fsnap_sse_batch: NULL argument");
    if (P < 1 || P > fsnap::SSE_MAX_P)
        return ctx->fail(FSNAP_E_ARG, "fsnap_sse_batch: P = %d, expected 1 ... %d", P, fsnap::SSE_MAX_P);
    if (K < 1 || K > 0x3FFFFFFF) return ctx->fail(FSNAP_E_ARG, "fsnap_sse_batch: K = %lld", (long long)K);
    if (ctx->m <= 0) {                   // no rows on this context (a rank without rows): nothing to add
        for (int p = 0; p < P; ++p) sse[p] = 0.0;
        if (n_train) *n_train = 0;
        return FSNAP_OK;
    }
    int rc;
    if ((rc = check_rows(ctx)) || (rc = check_weights(ctx))) return rc;
    if (K != ctx->K) return ctx->fail(FSNAP_E_ARG, "fsnap_sse_batch: K = %lld, the resident rows have %lld columns",
                                      (long long)K, (long long)ctx->K);
    FSNAP_HIP(hipSetDevice(ctx->device), "hipSetDevice");
    const int nb = fsnap::sse_num_blocks(ctx->m);
    const size_t ncol = fsnap::SSE_MAX_P + 1;
    const size_t nup = (size_t)4 * ((K + 15) / 16) * 64;
    if (!ctx->sse_U.ensure(nup * 8) || !ctx->sse_part.ensure((size_t)nb * ncol * 8) || !ctx->sse_out.ensure(ncol * 8))
        return ctx->fail(FSNAP_E_NOMEM, "hipMalloc(sse) failed");
    const unsigned char* mask = ctx->dmask;
    if (!mask) {
        if ((rc = ensure_ones(ctx))) return rc;
        mask = (const unsigned char*)ctx->ones.p;
    }
    ctx->sse_hU.resize(nup);
    fsnap::sse_pack_u(U, P, (int)K, ctx->sse_hU.data());
    FSNAP_HIP(hipMemcpyAsync(ctx->sse_U.p, ctx->sse_hU.data(), nup * 8, hipMemcpyHostToDevice, ctx->stream), "hipMemcpy(U)");
    FSNAP_HIP(fsnap::launch_sse_batch(ctx->dA, ctx->lda, ctx->m, (int)K, (const double*)ctx->sse_U.p, ctx->db, ctx->dw, mask,
                                      (double*)ctx->sse_part.p, (double*)ctx->sse_out.p, ctx->stream),
              "launch fsnap_sse_rows_k");
    double out[fsnap::SSE_MAX_P + 1];
    FSNAP_HIP(hipMemcpyAsync(out, ctx->sse_out.p, ncol * 8, hipMemcpyDeviceToHost, ctx->stream), "hipMemcpy(sse)");
    FSNAP_HIP(hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");
    for (int p = 0; p < P; ++p) sse[p] = out[p];
    if (n_train) *n_train = (int64_t)out[fsnap::SSE_MAX_P];
    return FSNAP_OK;
}

int fsnap_timing(fsnap_ctx* ctx, double* ms, int n) {
    if (!ctx || !ms || n < 0 || n > 8) return FSNAP_E_ARG;
    FSNAP_HIP(hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");
    double out[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    float t = 0.f;
    if (ctx->t_syrk && ctx->nfit > 0) {
        hipEvent_t* sl = ctx->ring[(ctx->nfit - 1) % fsnap_ctx::RING];
        if (hipEventElapsedTime(&t, sl[0], sl[1]) == hipSuccess) out[0] = t;
        if (n > 1 && hipEventElapsedTime(&t, sl[1], sl[2]) == hipSuccess) out[1] = t;
    }
    if (n > 2 && ctx->t_upload && hipEventElapsedTime(&t, ctx->ev[3], ctx->ev[4]) == hipSuccess) out[2] = t;
    if (n > 3 && ctx->t_weight && hipEventElapsedTime(&t, ctx->ev[5], ctx->ev[6]) == hipSuccess) out[3] = t;
    if (n > 4 && ctx->t_predict && hipEventElapsedTime(&t, ctx->ev[7], ctx->ev[8]) == hipSuccess) out[4] = t;
    out[5] = ctx->upload_probe_gbps;          // last large fsnap_upload_rows: rate of the probed pageable copy (0: no probe)
    out[6] = ctx->upload_staged ? 1.0 : 0.0;  // ... and whether the rest went through the page-locked double buffer
    for (int i = 0; i < n; ++i) ms[i] = out[i];
    return FSNAP_OK;
}

int fsnap_timing_history(fsnap_ctx* ctx, double* syrk_ms, double* reduce_ms, int n) {
    if (!ctx || !syrk_ms || n < 0) return FSNAP_E_ARG;
    if (n > fsnap_ctx::RING || n > ctx->nfit) return ctx->fail(FSNAP_E_ARG, "fsnap_timing_history: only the last %d fits are kept",
                                                             (int)(ctx->nfit < fsnap_ctx::RING ? ctx->nfit : fsnap_ctx::RING));
    FSNAP_HIP(hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");
    for (int i = 0; i < n; ++i) {
        hipEvent_t* sl = ctx->ring[(ctx->nfit - n + i) % fsnap_ctx::RING];
        float t = 0.f;
        FSNAP_HIP(hipEventElapsedTime(&t, sl[0], sl[1]), "hipEventElapsedTime");
        syrk_ms[i] = t;
        if (reduce_ms) {
            FSNAP_HIP(hipEventElapsedTime(&t, sl[1], sl[2]), "hipEventElapsedTime");
            reduce_ms[i] = t;
        }
    }
    return FSNAP_OK;
}

int fsnap_timing_history_comm(fsnap_ctx* ctx, double* allreduce_ms, int n) {
    if (!ctx || !allreduce_ms || n < 0) return FSNAP_E_ARG;
    if (n > fsnap_ctx::RING || n > ctx->nfit) return ctx->fail(FSNAP_E_ARG, "fsnap_timing_history_comm: only the last %d fits are kept",
                                                             (int)(ctx->nfit < fsnap_ctx::RING ? ctx->nfit : fsnap_ctx::RING));
    int wrc;
    if ((wrc = fsnap::wait_stream(ctx, nullptr, "timing history"))) return wrc;
    for (int i = 0; i < n; ++i) {
        const int64_t k = (ctx->nfit - n + i) % fsnap_ctx::RING;
        float t = 0.f;
        allreduce_ms[i] = -1.0;                         // not a multi-GPU fit
        if (ctx->ring_comm[k]) {
            FSNAP_HIP(hipEventElapsedTime(&t, ctx->ring[k][2], ctx->ring[k][3]), "hipEventElapsedTime");
            allreduce_ms[i] = t;
        }
    }
    return FSNAP_OK;
}

int fsnap_timing_count(fsnap_ctx* ctx, int64_t* sampled, int64_t* launches) {
    if (!ctx) return FSNAP_E_ARG;
    if (sampled) *sampled = ctx->nfit;
    if (launches) *launches = ctx->nlaunch;
    return FSNAP_OK;
}

int fsnap_launch_info(fsnap_ctx* ctx, int64_t* info, int n) {
    if (!ctx || !info || n < 0 || n > 8) return FSNAP_E_ARG;
    int rc;
    if ((rc = check_rows(ctx))) return rc;
    int64_t out[8] = {0, 0, 0, 0, 0, ctx->num_cu, 0, 0};
    if (use_tiled(ctx)) {
        TiledGeometry t;
        if ((rc = plan_tiled(ctx, &t))) return rc;
        out[0] = (int64_t)t.npairs * t.nsplit;
        out[1] = 256;
        out[2] = t.cps / 4;
        out[3] = 4 * t.NSB;
        out[4] = 0;  // 0 = tiled kernel
        out[6] = t.npairs;
        out[7] = t.nsplit;
    } else {
        Geometry g;
        if ((rc = plan_geometry(ctx, &g))) return rc;
        out[0] = g.nblocks;
        out[1] = g.threads;
        out[2] = g.cpw;
        out[3] = g.NB;
        out[4] = g.split;
        out[6] = g.shortk ? 7 : g.quad ? (g.cluster > 1 ? 6 : 5) : g.acc ? 3 : 4;
        out[7] = g.fused_pack ? 1 : 0;  // kernel id: 1 = wave-triangle, 2 = LDS-shared, 3 = one-wave triangle (1A), 4 = wave-triangle on packed weights (1P), 5 = triangle dealt to the four waves of a workgroup (1Q; chunks per WORKGROUP)
    }
    for (int i = 0; i < n; ++i) info[i] = out[i];
    return FSNAP_OK;
}

}  // extern "C"

// ---- batched candidate fits ------------------------------------------------------------------------------------

namespace {

int cand_check_layout(fsnap_ctx* ctx, int64_t layout, const char* who) {
    if (!ctx->cand_dA || ctx->cand_dA != ctx->dA || ctx->cand_m != ctx->m || layout <= 0 || layout != ctx->cand_layout)
        return ctx->fail(FSNAP_E_STATE, "%s: layout %lld is not the one the context holds (%lld): fsnap_cat_prepare again", who,
                         (long long)layout, (long long)ctx->cand_layout);
    return FSNAP_OK;
}

std::atomic<int64_t> cand_layout_counter{0};   // layout tags are unique over all contexts of the process

bool cand_fits(int64_t n, int64_t K) {
    return n > 0 && K > 0 && (double)n * (double)FSNAP_PACKED_LEN(K) * 8.0 <= (double)FSNAP_CAT_STATS_MAX_BYTES;
}

// The front that fsnap_lasso_path, fsnap_ard_path and fsnap_omp_path share ("The fold frame").  fold_check: the
// arguments they have in common, ahead of the entry point's own -- the statistics, K against the kernel's limit, F folds of
// nsub blocks, Q, and (F + 1) per_fold problems (per_fold: Q, or 1 where a problem walks all Q levels).  fold_stage: the size
// cap, the device, ctx->fold_sys and kernel S1; *folds are the F fold blocks (d_stats itself with nsub = 1, where the caller's
// blocks are the folds) and *total their sum.  fold_grid: the workgroups of a grid-stride launch over nprob problems.
// fold_finish: the copies back, the wait, and the scan of one output (nscan doubles; none: nullptr) for non-finite values.
int fold_check(fsnap_ctx* ctx, const char* who, int64_t K, int max_K, int64_t F, int64_t nsub, int64_t Q, int64_t per_fold,
               const double* d_stats) {
    if (!d_stats) return ctx->fail(FSNAP_E_ARG, "%s: NULL argument", who);
    if (K < 1 || K > max_K) return ctx->fail(FSNAP_E_ARG, "%s: K = %lld (1 ... %d)", who, (long long)K, max_K);
    if (F < 1 || nsub < 1 || F > 0x3FFFFFFF || nsub > 0x3FFFFFFF)
        return ctx->fail(FSNAP_E_ARG, "%s: F = %lld, nsub = %lld", who, (long long)F, (long long)nsub);
    if (Q < 1 || Q > 0xFFFFF || (F + 1) * per_fold > 0x3FFFFFFF) return ctx->fail(FSNAP_E_ARG, "%s: Q = %lld", who, (long long)Q);
    return FSNAP_OK;
}

int fold_stage(fsnap_ctx* ctx, const char* who, int64_t K, int64_t F, int64_t nsub, const double* d_stats, const double** folds,
               const double** total) {
    if (!cand_fits(F * nsub, K))
        return ctx->fail(FSNAP_E_ARG, "%s: %lld blocks x %lld doubles exceed FSNAP_CAT_STATS_MAX_BYTES", who, (long long)(F * nsub),
                         (long long)FSNAP_PACKED_LEN(K));
    FSNAP_HIP(hipSetDevice(ctx->device), "hipSetDevice");
    const int64_t T = FSNAP_PACKED_LEN(K);
    const int64_t nfold = nsub > 1 ? F : 0;                 // nsub = 1: the caller's blocks are the folds
    if (!ctx->fold_sys.ensure((size_t)(nfold + 1) * T * 8)) return ctx->fail(FSNAP_E_NOMEM, "hipMalloc(fold sums) failed");
    double* dfolds = nfold ? (double*)ctx->fold_sys.p : nullptr;
    double* dtotal = (double*)ctx->fold_sys.p + nfold * T;
    FSNAP_HIP(fsnap::launch_fold_sums(d_stats, (int)F, (int)nsub, (int)K, dfolds, dtotal, ctx->stream),
              "launch fsnap_fold_sums_k");
    *folds = dfolds ? dfolds : d_stats;
    *total = dtotal;
    return FSNAP_OK;
}

int fold_grid(const fsnap_ctx* ctx, int64_t nprob, int per_cu) {
    return (int)std::min<int64_t>(nprob, (int64_t)per_cu * std::max(1, ctx->num_cu));
}

struct FoldCopy { void* host; const void* dev; size_t bytes; };

int fold_finish(fsnap_ctx* ctx, std::initializer_list<FoldCopy> copies, const double* scan, int64_t nscan) {
    for (const FoldCopy& c : copies)
        FSNAP_HIP(hipMemcpyAsync(c.host, c.dev, c.bytes, hipMemcpyDeviceToHost, ctx->stream), "hipMemcpy(fold path results)");
    FSNAP_HIP(hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");
    for (int64_t i = 0; i < nscan; ++i)
        if (!std::isfinite(scan[i])) return FSNAP_NUM_NONFINITE;
    return FSNAP_OK;
}

// kernels C1 + C1R into ctx->cand_stats (the rows must be prepared)
int cand_stats_launch(fsnap_ctx* ctx) {
    const int K = (int)ctx->K, ncat = ctx->cand_ncat;
    const int64_t T = FSNAP_PACKED_LEN(K), nch = ctx->cand_nch_t;
    const int64_t per = fsnap::cat_partial_doubles(K), NT = (K + 15) / 16, NP = NT * (NT + 1) / 2;
    if (!ctx->cand_stats.ensure((size_t)ncat * T * 8) || !ctx->cand_part.ensure((size_t)(nch > 0 ? nch : 1) * per * 8))
        return ctx->fail(FSNAP_E_NOMEM, "hipMalloc(category statistics) failed");
    double* part = (double*)ctx->cand_part.p;
    double* cpart = part + nch * NP * 256;
    double* spart = cpart + nch * NT * 16;
    FSNAP_HIP(fsnap::launch_cat_syrk(ctx->dA, ctx->lda, ctx->db, (const double*)ctx->cand_w0.p, (const int*)ctx->cand_idx_t.p,
                                     (const fsnap::CatChunk*)ctx->cand_ch_t.p, nch, K, part, cpart, spart, ctx->stream),
              "launch fsnap_cat_syrk_k");
    FSNAP_HIP(fsnap::launch_cat_reduce(part, cpart, spart, (const int*)ctx->cand_cb_t.p, ncat, K, (double*)ctx->cand_stats.p,
                                       ctx->stream),
              "launch fsnap_cat_reduce_k");
    ctx->cand_stats_K = K;
    return FSNAP_OK;
}

}  // namespace

extern "C" {

int fsnap_cat_chunks(int64_t m, const int32_t* cat, const uint8_t* mask, int ncat, int32_t* idx, int64_t* chunks,
                     int64_t* nchunks) {
    if (m < 0 || m > 0x7FFFFFFF || (m > 0 && !cat) || ncat <= 0 || !idx || !chunks || !nchunks) {
        fsnap::library_error() = "fsnap_cat_chunks: bad argument";
        return FSNAP_E_ARG;
    }
    std::vector<int64_t> start((size_t)ncat + 1, 0);
    for (int64_t i = 0; i < m; ++i) {
        if (cat[i] >= ncat) {
            char buf[160];
            snprintf(buf, sizeof buf, "fsnap_cat_chunks: category %d of row %lld is not below %d", cat[i], (long long)i, ncat);
            fsnap::library_error() = buf;
            return FSNAP_E_ARG;
        }
        if (cat[i] >= 0 && (!mask || mask[i])) ++start[(size_t)cat[i] + 1];
    }
    for (int c = 0; c < ncat; ++c) start[(size_t)c + 1] += start[(size_t)c];
    std::vector<int64_t> pos(start.begin(), start.end() - 1);
    for (int64_t i = 0; i < m; ++i)
        if (cat[i] >= 0 && (!mask || mask[i])) idx[pos[(size_t)cat[i]]++] = (int32_t)i;
    int64_t n = 0;
    for (int c = 0; c < ncat; ++c)
        for (int64_t f = start[(size_t)c]; f < start[(size_t)c + 1]; f += fsnap::CAT_CHUNK_ROWS) {
            chunks[3 * n] = c;
            chunks[3 * n + 1] = f;
            chunks[3 * n + 2] = std::min<int64_t>(fsnap::CAT_CHUNK_ROWS, start[(size_t)c + 1] - f);
            ++n;
        }
    *nchunks = n;
    return FSNAP_OK;
}

int fsnap_cat_info(const fsnap_ctx* ctx, int64_t* info, int n) {
    if (!info || n < 0 || n > 5) return FSNAP_E_ARG;
    const int64_t out[5] = {ctx ? ctx->cand_layout : 0, ctx && ctx->cand_layout ? ctx->cand_ncat : 0,
                            ctx && ctx->cand_layout ? ctx->cand_stats_K : 0, fsnap::CAT_CHUNK_ROWS, fsnap::CAND_ROWS_MAX_P};
    for (int i = 0; i < n; ++i) info[i] = out[i];
    return FSNAP_OK;
}

int fsnap_cat_prepare(fsnap_ctx* ctx, const int32_t* cat, int ncat, int64_t* layout) {
    if (!ctx) return FSNAP_E_ARG;
    int rc;
    cand_forget(ctx);                 // a prepare that fails leaves no layout behind
    if ((rc = check_rows(ctx)) || (rc = check_weights(ctx))) return rc;
    if (!cat || ncat <= 0 || !layout) return ctx->fail(FSNAP_E_ARG, "fsnap_cat_prepare: bad argument");
    if (ctx->m > 0x7FFFFFFF) return ctx->fail(FSNAP_E_ARG, "fsnap_cat_prepare: more than 2^31 - 1 rows");
    if (!cand_fits(ncat, ctx->K))
        return ctx->fail(FSNAP_E_ARG, "fsnap_cat_prepare: %d categories x %lld doubles exceed FSNAP_CAT_STATS_MAX_BYTES", ncat,
                         (long long)FSNAP_PACKED_LEN(ctx->K));
    FSNAP_HIP(hipSetDevice(ctx->device), "hipSetDevice");
    const int64_t m = ctx->m;
    std::vector<unsigned char> mask;
    if (ctx->dmask) {
        mask.resize((size_t)m);
        FSNAP_HIP(hipMemcpyAsync(mask.data(), ctx->dmask, (size_t)m, hipMemcpyDeviceToHost, ctx->stream), "hipMemcpy(mask)");
        FSNAP_HIP(hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");
    }
    // stable counting sort of the row ids by category, once over the training rows and once over all rows
    std::vector<int32_t> idx_t((size_t)m + 1), idx_a((size_t)m + 1);
    std::vector<int64_t> raw_t(3 * ((size_t)m + ncat)), raw_a(3 * ((size_t)m + ncat));
    int64_t n_t = 0, n_a = 0;
    if ((rc = fsnap_cat_chunks(m, cat, mask.empty() ? nullptr : mask.data(), ncat, idx_t.data(), raw_t.data(), &n_t)) ||
        (rc = fsnap_cat_chunks(m, cat, nullptr, ncat, idx_a.data(), raw_a.data(), &n_a)))
        return ctx->fail(rc, "%s", fsnap::library_error().c_str());
    std::vector<fsnap::CatChunk> ch_t, ch_a;
    std::vector<int32_t> cb_t((size_t)ncat + 1, 0), cb_a((size_t)ncat + 1, 0);
    auto to_chunks = [&](const std::vector<int64_t>& raw, int64_t n, std::vector<fsnap::CatChunk>& ch, std::vector<int32_t>& cb) {
        for (int64_t i = 0; i < n; ++i) ch.push_back(fsnap::CatChunk{raw[3 * i + 1], (int32_t)raw[3 * i], (int32_t)raw[3 * i + 2]});
        // cbeg[c] = first chunk of category c (chunks are in category order)
        int64_t j = 0;
        for (int c = 0; c <= ncat; ++c) {
            while (j < n && raw[3 * j] < c) ++j;
            cb[(size_t)c] = (int32_t)j;
        }
    };
    to_chunks(raw_t, n_t, ch_t, cb_t);
    to_chunks(raw_a, n_a, ch_a, cb_a);
    const size_t csz = sizeof(fsnap::CatChunk);
    if (!ctx->cand_idx_t.ensure(idx_t.size() * 4) || !ctx->cand_idx_a.ensure(idx_a.size() * 4) ||
        !ctx->cand_ch_t.ensure((ch_t.size() + 1) * csz) || !ctx->cand_ch_a.ensure((ch_a.size() + 1) * csz) ||
        !ctx->cand_cb_t.ensure(cb_t.size() * 4) || !ctx->cand_cb_a.ensure(cb_a.size() * 4) || !ctx->cand_w0.ensure((size_t)m * 8))
        return ctx->fail(FSNAP_E_NOMEM, "hipMalloc(category layout) failed");
    FSNAP_HIP(hipMemcpyAsync(ctx->cand_idx_t.p, idx_t.data(), idx_t.size() * 4, hipMemcpyHostToDevice, ctx->stream), "hipMemcpy(index)");
    FSNAP_HIP(hipMemcpyAsync(ctx->cand_idx_a.p, idx_a.data(), idx_a.size() * 4, hipMemcpyHostToDevice, ctx->stream), "hipMemcpy(index)");
    if (!ch_t.empty())
        FSNAP_HIP(hipMemcpyAsync(ctx->cand_ch_t.p, ch_t.data(), ch_t.size() * csz, hipMemcpyHostToDevice, ctx->stream), "hipMemcpy(chunks)");
    if (!ch_a.empty())
        FSNAP_HIP(hipMemcpyAsync(ctx->cand_ch_a.p, ch_a.data(), ch_a.size() * csz, hipMemcpyHostToDevice, ctx->stream), "hipMemcpy(chunks)");
    FSNAP_HIP(hipMemcpyAsync(ctx->cand_cb_t.p, cb_t.data(), cb_t.size() * 4, hipMemcpyHostToDevice, ctx->stream), "hipMemcpy(chunks)");
    FSNAP_HIP(hipMemcpyAsync(ctx->cand_cb_a.p, cb_a.data(), cb_a.size() * 4, hipMemcpyHostToDevice, ctx->stream), "hipMemcpy(chunks)");
    FSNAP_HIP(hipMemcpyAsync(ctx->cand_w0.p, ctx->dw, (size_t)m * 8, hipMemcpyDeviceToDevice, ctx->stream), "hipMemcpy(w0)");
    FSNAP_HIP(hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");
    ctx->cand_dA = ctx->dA;
    ctx->cand_m = m;
    ctx->cand_nch_t = (int64_t)ch_t.size();
    ctx->cand_nch_a = (int64_t)ch_a.size();
    ctx->cand_ncat = ncat;
    ctx->cand_stats_K = 0;
    ctx->cand_layout = ++cand_layout_counter;
    *layout = ctx->cand_layout;
    return FSNAP_OK;
}

int fsnap_cat_normal_eq(fsnap_ctx* ctx, int64_t layout, double** d_stats) {
    if (!ctx) return FSNAP_E_ARG;
    int rc;
    if (!d_stats) return ctx->fail(FSNAP_E_ARG, "fsnap_cat_normal_eq: d_stats is NULL");
    if ((rc = check_rows(ctx)) || (rc = cand_check_layout(ctx, layout, "fsnap_cat_normal_eq"))) return rc;
    FSNAP_HIP(hipSetDevice(ctx->device), "hipSetDevice");
    if ((rc = cand_stats_launch(ctx))) return rc;
    *d_stats = (double*)ctx->cand_stats.p;
    return FSNAP_OK;
}

int fsnap_cat_normal_eq_dist(fsnap_ctx* ctx, int64_t* layout, int64_t K, int ncat, double** d_stats) {
    if (!ctx) return FSNAP_E_ARG;
    if (!layout || !d_stats || !cand_fits(ncat, K)) return ctx->fail(FSNAP_E_ARG, "fsnap_cat_normal_eq_dist: bad argument");
    if (!ctx->comm) return ctx->fail(FSNAP_E_STATE, "fsnap_cat_normal_eq_dist: no communicator (fsnap_comm_init first)");
    FSNAP_HIP(hipSetDevice(ctx->device), "hipSetDevice");
    const int64_t n = (int64_t)ncat * FSNAP_PACKED_LEN(K);
    // as in fsnap_fit_dist: a rank that fails alone still takes part in the collective, with NaN statistics
    if (!ctx->cand_stats.ensure((size_t)n * 8)) return ctx->fail(FSNAP_E_NOMEM, "hipMalloc(category statistics) failed");
    double* dp = (double*)ctx->cand_stats.p;
    const bool have_rows = *layout != 0;
    int local_rc = FSNAP_OK;
    std::string local_err;
    if (have_rows && cand_check_layout(ctx, *layout, "fsnap_cat_normal_eq_dist")) {
        local_rc = FSNAP_E_STATE;
    } else if (have_rows && (ctx->K != K || ctx->cand_ncat != ncat)) {
        local_rc = ctx->fail(FSNAP_E_ARG, "fsnap_cat_normal_eq_dist: K = %lld, ncat = %d but the prepared rows have %lld, %d",
                             (long long)K, ncat, (long long)ctx->K, ctx->cand_ncat);
    } else if (have_rows) {
        local_rc = cand_stats_launch(ctx);
    } else if (hipMemsetAsync(dp, 0, (size_t)n * 8, ctx->stream) != hipSuccess) {
        local_rc = ctx->fail(FSNAP_E_HIP, "hipMemsetAsync(category statistics) failed");
    }
    if (local_rc != FSNAP_OK) {
        local_err = ctx->err;
        (void)hipMemsetAsync(dp, 0xFF, (size_t)n * 8, ctx->stream);
    }
    int rc = fsnap_allreduce_device(ctx, dp, n);
    if (local_rc != FSNAP_OK) return ctx->fail(local_rc, "%s", local_err.c_str());
    if (rc) return rc;
    if (!have_rows) {                 // a rank without rows: a layout of statistics only (no row pass can use it)
        cand_forget(ctx);
        ctx->cand_layout = ++cand_layout_counter;
        *layout = ctx->cand_layout;
    }
    ctx->cand_ncat = ncat;
    ctx->cand_stats_K = K;
    *d_stats = dp;
    return FSNAP_OK;
}

int fsnap_fit_candidates(fsnap_ctx* ctx, int64_t layout, int kind, double param, const double* S, int P, int ncat, int64_t K,
                         double* beta, int* rank, double* rcond_est, double** d_packed) {
    if (!ctx) return FSNAP_E_ARG;
    if (!S || P <= 0 || !beta || !rank || !rcond_est) return ctx->fail(FSNAP_E_ARG, "fsnap_fit_candidates: bad argument");
    if (layout <= 0 || layout != ctx->cand_layout || ctx->cand_stats_K <= 0 || !ctx->cand_stats.p)
        return ctx->fail(FSNAP_E_STATE, "fsnap_fit_candidates: no per-category statistics of layout %lld on the context "
                                        "(fsnap_cat_prepare + fsnap_cat_normal_eq first)", (long long)layout);
    if (ncat != ctx->cand_ncat || K != ctx->cand_stats_K)
        return ctx->fail(FSNAP_E_ARG, "fsnap_fit_candidates: ncat = %d, K = %lld but the statistics have %d, %lld", ncat,
                         (long long)K, ctx->cand_ncat, (long long)ctx->cand_stats_K);
    if (!cand_fits(P, K))
        return ctx->fail(FSNAP_E_ARG, "fsnap_fit_candidates: %d candidates x %lld doubles exceed FSNAP_CAT_STATS_MAX_BYTES", P,
                         (long long)FSNAP_PACKED_LEN(K));
    FSNAP_HIP(hipSetDevice(ctx->device), "hipSetDevice");
    const int64_t T = FSNAP_PACKED_LEN(K);
    if (!ctx->cand_S.ensure((size_t)P * ncat * 8) || !ctx->cand_out.ensure((size_t)P * T * 8))
        return ctx->fail(FSNAP_E_NOMEM, "hipMalloc(candidate statistics) failed");
    FSNAP_HIP(hipMemcpyAsync(ctx->cand_S.p, S, (size_t)P * ncat * 8, hipMemcpyHostToDevice, ctx->stream), "hipMemcpy(S)");
    double* out = (double*)ctx->cand_out.p;
    FSNAP_HIP(fsnap::launch_cand_combine((const double*)ctx->cand_stats.p, (const double*)ctx->cand_S.p, P, ncat, (int)K, out,
                                         ctx->stream),
              "launch fsnap_cand_combine_k");
    if (ctx->mirror_of == out) ctx->mirror_of = nullptr;     // the buffer was rewritten
    ctx->chol_factor_of = nullptr;
    for (int p = 0; p < P; ++p) {
        int rc = fsnap_solve_device_rhs(ctx, kind, param, K, out + (int64_t)p * T, nullptr, beta + (int64_t)p * K, rank + p,
                                        rcond_est + p);
        if (rc) return rc;
    }
    if (d_packed) *d_packed = out;
    return FSNAP_OK;
}

int fsnap_candidate_rows(fsnap_ctx* ctx, int64_t layout, const double* beta, const double* S, int P, int ncat, int64_t K_,
                         int what, double* out) {
    if (!ctx) return FSNAP_E_ARG;
    int rc;
    if ((rc = check_rows(ctx)) || (rc = cand_check_layout(ctx, layout, "fsnap_candidate_rows"))) return rc;
    if (!beta || P <= 0 || !out || (what != FSNAP_CAND_ERROR_SUMS && what != FSNAP_CAND_RHS) || (what == FSNAP_CAND_RHS && !S))
        return ctx->fail(FSNAP_E_ARG, "fsnap_candidate_rows: bad argument");
    if (ncat != ctx->cand_ncat || K_ != ctx->K)
        return ctx->fail(FSNAP_E_ARG, "fsnap_candidate_rows: ncat = %d, K = %lld but the layout has %d, the rows %lld", ncat,
                         (long long)K_, ctx->cand_ncat, (long long)ctx->K);
    FSNAP_HIP(hipSetDevice(ctx->device), "hipSetDevice");
    const int K = (int)ctx->K;
    const int64_t K8 = (K + 7) / 8 * 8;
    const bool sums = what == FSNAP_CAND_ERROR_SUMS;
    const int64_t nch = sums ? ctx->cand_nch_a : ctx->cand_nch_t;
    const int64_t nout = sums ? (int64_t)ncat * 4 : K;
    const int64_t per = fsnap::cand_rows_partial_doubles(what, K);
    if (!ctx->cand_betaT.ensure((size_t)K8 * 16 * 8) || !ctx->cand_rpart.ensure((size_t)(nch > 0 ? nch : 1) * per * 8) ||
        !ctx->cand_res.ensure((size_t)P * nout * 8) || (!sums && !ctx->cand_S.ensure((size_t)P * ncat * 8)))
        return ctx->fail(FSNAP_E_NOMEM, "hipMalloc(candidate rows) failed");
    if (!sums)
        FSNAP_HIP(hipMemcpyAsync(ctx->cand_S.p, S, (size_t)P * ncat * 8, hipMemcpyHostToDevice, ctx->stream), "hipMemcpy(S)");
    if (nch == 0) FSNAP_HIP(hipMemsetAsync(ctx->cand_res.p, 0, (size_t)P * nout * 8, ctx->stream), "hipMemsetAsync");
    std::vector<double> bt((size_t)K8 * 16);
    for (int p0 = 0; p0 < P; p0 += fsnap::CAND_ROWS_MAX_P) {
        const int np = std::min(fsnap::CAND_ROWS_MAX_P, P - p0);
        std::fill(bt.begin(), bt.end(), 0.0);
        for (int p = 0; p < np; ++p)
            for (int k = 0; k < K; ++k) bt[(size_t)k * 16 + p] = beta[(int64_t)(p0 + p) * K + k];
        // the launch before may still read betaT: the copy is ordered after it on the stream, the host buffer must outlive it
        FSNAP_HIP(hipMemcpyAsync(ctx->cand_betaT.p, bt.data(), bt.size() * 8, hipMemcpyHostToDevice, ctx->stream), "hipMemcpy(beta)");
        if (nch == 0) continue;
        FSNAP_HIP(fsnap::launch_cand_rows(what, ctx->dA, ctx->lda, ctx->db, (const double*)ctx->cand_w0.p,
                                          (const int*)(sums ? ctx->cand_idx_a.p : ctx->cand_idx_t.p),
                                          (const fsnap::CatChunk*)(sums ? ctx->cand_ch_a.p : ctx->cand_ch_t.p), nch, K,
                                          (const double*)ctx->cand_betaT.p, (double*)ctx->cand_rpart.p, ctx->stream),
                  "launch fsnap_cand_rows_k");
        FSNAP_HIP(fsnap::launch_cand_reduce(what, (const double*)ctx->cand_rpart.p, (const int*)(sums ? ctx->cand_cb_a.p : ctx->cand_cb_t.p),
                                            (const double*)ctx->cand_S.p, ncat, np, p0, K, (double*)ctx->cand_res.p, ctx->stream),
                  "launch fsnap_cand_reduce_k");
        FSNAP_HIP(hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");   // bt is rewritten for the next group
    }
    FSNAP_HIP(hipMemcpyAsync(out, ctx->cand_res.p, (size_t)P * nout * 8, hipMemcpyDeviceToHost, ctx->stream), "hipMemcpy(out)");
    FSNAP_HIP(hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");
    return FSNAP_OK;
}

}  // extern "C"

// ---- predictive variance of the resident rows (kernels U1 / U1G, U2, U3 of fsnap_uq.hip) ----------------------------

namespace {

// dev_out: var / preds / cat_sum / cat_max / cat_count are device pointers and the call returns once the work is queued;
// scale is then a device pointer too.  Otherwise everything is host memory and the call is synchronous.
int row_variance(fsnap_ctx* ctx, int mode, int64_t K, int64_t J, const double* M, const double* beta, const double* scale,
                 const int32_t* cat, int ncat, double* var, double* preds, double* cat_sum, double* cat_max,
                 int64_t* cat_count, bool dev_out) {
    if (!ctx) return FSNAP_E_ARG;
    const char* who = dev_out ? "fsnap_row_variance_device" : "fsnap_row_variance";
    if (mode != FSNAP_UQ_QUAD && mode != FSNAP_UQ_NORM) return ctx->fail(FSNAP_E_ARG, "%s: unknown mode %d", who, mode);
    const bool want_cat = cat != nullptr;
    if (want_cat && ncat <= 0) return ctx->fail(FSNAP_E_ARG, "%s: cat given with ncat = %d", who, ncat);
    if (!want_cat && (cat_sum || cat_max || cat_count))
        return ctx->fail(FSNAP_E_ARG, "%s: category outputs without categories", who);
    const bool need_v = var || want_cat;
    if (need_v && !M) return ctx->fail(FSNAP_E_ARG, "%s: M is NULL", who);
    if (preds && !beta) return ctx->fail(FSNAP_E_ARG, "%s: preds wanted but beta is NULL", who);
    if (J < 1 || J > 0x3FFFFFFF) return ctx->fail(FSNAP_E_ARG, "%s: J = %lld", who, (long long)J);
    if (mode == FSNAP_UQ_QUAD && J != K)
        return ctx->fail(FSNAP_E_ARG, "%s: QUAD needs J = K (J = %lld, K = %lld)", who, (long long)J, (long long)K);
    const int64_t m = ctx->m;
    if (m > 0 && K != ctx->K)        // no rows (a rank that owns none): nothing to check K against
        return ctx->fail(FSNAP_E_ARG, "%s: K = %lld, the resident rows have %lld columns", who, (long long)K, (long long)ctx->K);
    if (K < 1 || K > 0x3FFFFFFF) return ctx->fail(FSNAP_E_ARG, "%s: K = %lld", who, (long long)K);
    if (want_cat && m > 0x7FFFFFFF) return ctx->fail(FSNAP_E_ARG, "%s: categories need m < 2^31", who);
    if (m > 0) {
        int rc = check_rows(ctx);
        if (rc) return rc;
    }
    FSNAP_HIP(hipSetDevice(ctx->device), "hipSetDevice");
    if (ctx->uq_inflight) {
        FSNAP_HIP(hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");
        ctx->uq_inflight = false;
    }
    // categories first: an id >= ncat is an argument error before anything is queued
    int64_t nch = 0;
    if (want_cat) {
        ctx->uq_hidx.resize((size_t)std::max<int64_t>(m, 1));
        ctx->uq_hch.resize(3 * (size_t)(m + ncat));
        if (fsnap_cat_chunks(m, cat, nullptr, ncat, ctx->uq_hidx.data(), ctx->uq_hch.data(), &nch) != FSNAP_OK)
            return ctx->fail(FSNAP_E_ARG, "%s: %s", who, fsnap::library_error().c_str());
        ctx->uq_hcount.assign((size_t)ncat, 0);
        ctx->uq_hcbeg.assign((size_t)ncat + 1, 0);
        // CatChunk records in place of the triples (16 bytes each: first, then category and count as int32)
        std::vector<int64_t>& h = ctx->uq_hch;
        for (int64_t i = 0; i < nch; ++i) {
            const int64_t c = h[3 * i], first = h[3 * i + 1], cnt = h[3 * i + 2];
            ctx->uq_hcount[(size_t)c] += cnt;
            ctx->uq_hcbeg[(size_t)c + 1] += 1;
            fsnap::CatChunk rec{first, (int32_t)c, (int32_t)cnt};
            std::memcpy(&h[2 * i], &rec, sizeof rec);
        }
        for (int c = 0; c < ncat; ++c) ctx->uq_hcbeg[(size_t)c + 1] += ctx->uq_hcbeg[(size_t)c];
    }
    const int64_t Kp = (K + 15) / 16 * 16, Jp = (J + 15) / 16 * 16;
    double* dvar = nullptr;
    double* dpreds = nullptr;
    if (m > 0 && (need_v || preds)) {
        // staging [M padded to Kp x Jp | beta padded to Kp], one copy up
        const size_t nM = (size_t)(Kp * Jp);
        ctx->uq_hM.assign(nM + (size_t)Kp, 0.0);
        if (need_v)
            for (int64_t k = 0; k < K; ++k) std::memcpy(&ctx->uq_hM[(size_t)(k * Jp)], M + k * J, (size_t)J * 8);
        if (preds) std::memcpy(&ctx->uq_hM[nM], beta, (size_t)K * 8);
        if (!ctx->uq_M.ensure((nM + (size_t)Kp) * 8)) return ctx->fail(FSNAP_E_NOMEM, "hipMalloc(uq) failed");
        FSNAP_HIP(hipMemcpyAsync(ctx->uq_M.p, ctx->uq_hM.data(), (nM + (size_t)Kp) * 8, hipMemcpyHostToDevice, ctx->stream),
                  "hipMemcpy(M)");
        if (need_v) {
            if (dev_out && var) {
                dvar = var;
            } else {
                if (!ctx->uq_var.ensure((size_t)m * 8)) return ctx->fail(FSNAP_E_NOMEM, "hipMalloc(var) failed");
                dvar = (double*)ctx->uq_var.p;
            }
        }
        if (preds) {
            if (dev_out) {
                dpreds = preds;
            } else {
                if (!ctx->uq_preds.ensure((size_t)m * 8)) return ctx->fail(FSNAP_E_NOMEM, "hipMalloc(preds) failed");
                dpreds = (double*)ctx->uq_preds.p;
            }
        }
        FSNAP_HIP(fsnap::launch_uq_rows(mode == FSNAP_UQ_QUAD ? fsnap::UQ_QUAD : fsnap::UQ_NORM, ctx->dA, ctx->lda, m, (int)K,
                                        (const double*)ctx->uq_M.p, (int)Jp, (const double*)ctx->uq_M.p + Kp * Jp, dvar, dpreds,
                                        ctx->stream),
                  "launch fsnap_uq_rows_k");
    }
    double* dsum = nullptr;
    double* dmax = nullptr;
    if (want_cat) {
        if (!ctx->uq_idx.ensure((size_t)std::max<int64_t>(m, 1) * 4) || !ctx->uq_ch.ensure((size_t)std::max<int64_t>(nch, 1) * 16) ||
            !ctx->uq_cbeg.ensure(((size_t)ncat + 1) * 4) || !ctx->uq_part.ensure((size_t)std::max<int64_t>(nch, 1) * 16) ||
            (!dev_out && !ctx->uq_cat.ensure((size_t)ncat * 16)) || (scale && !dev_out && !ctx->uq_scale.ensure((size_t)m * 8 + 8)))
            return ctx->fail(FSNAP_E_NOMEM, "hipMalloc(uq categories) failed");
        if (m > 0) {
            FSNAP_HIP(hipMemcpyAsync(ctx->uq_idx.p, ctx->uq_hidx.data(), (size_t)m * 4, hipMemcpyHostToDevice, ctx->stream),
                      "hipMemcpy(idx)");
        }
        if (nch > 0)
            FSNAP_HIP(hipMemcpyAsync(ctx->uq_ch.p, ctx->uq_hch.data(), (size_t)nch * 16, hipMemcpyHostToDevice, ctx->stream),
                      "hipMemcpy(chunks)");
        FSNAP_HIP(hipMemcpyAsync(ctx->uq_cbeg.p, ctx->uq_hcbeg.data(), ((size_t)ncat + 1) * 4, hipMemcpyHostToDevice, ctx->stream),
                  "hipMemcpy(cbeg)");
        const double* dscale = nullptr;
        if (scale && m > 0) {
            if (dev_out) {
                dscale = scale;
            } else {
                FSNAP_HIP(hipMemcpyAsync(ctx->uq_scale.p, scale, (size_t)m * 8, hipMemcpyHostToDevice, ctx->stream),
                          "hipMemcpy(scale)");
                dscale = (const double*)ctx->uq_scale.p;
            }
        }
        dsum = dev_out ? cat_sum : (double*)ctx->uq_cat.p;
        dmax = dev_out ? cat_max : (double*)ctx->uq_cat.p + ncat;
        FSNAP_HIP(fsnap::launch_uq_cat(dvar, dscale, (const int*)ctx->uq_idx.p, (const fsnap::CatChunk*)ctx->uq_ch.p,
                                       m > 0 ? nch : 0, (const int*)ctx->uq_cbeg.p, ncat, (double*)ctx->uq_part.p, dsum, dmax,
                                       ctx->stream),
                  "launch fsnap_uq_chunk_k");
        if (cat_count) {
            if (dev_out)
                FSNAP_HIP(hipMemcpyAsync(cat_count, ctx->uq_hcount.data(), (size_t)ncat * 8, hipMemcpyHostToDevice, ctx->stream),
                          "hipMemcpy(cat_count)");
            else
                std::memcpy(cat_count, ctx->uq_hcount.data(), (size_t)ncat * 8);
        }
    }
    if (dev_out) {
        ctx->uq_inflight = true;
        return FSNAP_OK;
    }
    if (var && m > 0) FSNAP_HIP(hipMemcpyAsync(var, dvar, (size_t)m * 8, hipMemcpyDeviceToHost, ctx->stream), "hipMemcpy(var)");
    if (preds && m > 0)
        FSNAP_HIP(hipMemcpyAsync(preds, dpreds, (size_t)m * 8, hipMemcpyDeviceToHost, ctx->stream), "hipMemcpy(preds)");
    if (cat_sum) FSNAP_HIP(hipMemcpyAsync(cat_sum, dsum, (size_t)ncat * 8, hipMemcpyDeviceToHost, ctx->stream), "hipMemcpy(sum)");
    if (cat_max) FSNAP_HIP(hipMemcpyAsync(cat_max, dmax, (size_t)ncat * 8, hipMemcpyDeviceToHost, ctx->stream), "hipMemcpy(max)");
    FSNAP_HIP(hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");
    return FSNAP_OK;
}

}  // namespace

int fsnap_row_variance(fsnap_ctx* ctx, int mode, int64_t K, int64_t J, const double* M, const double* beta, const double* scale,
                       const int32_t* cat, int ncat, double* var, double* preds, double* cat_sum, double* cat_max,
                       int64_t* cat_count) {
    return row_variance(ctx, mode, K, J, M, beta, scale, cat, ncat, var, preds, cat_sum, cat_max, cat_count, false);
}

int fsnap_row_variance_device(fsnap_ctx* ctx, int mode, int64_t K, int64_t J, const double* M, const double* beta,
                              const double* d_scale, const int32_t* cat, int ncat, double* d_var, double* d_preds,
                              double* d_cat_sum, double* d_cat_max, int64_t* d_cat_count) {
    return row_variance(ctx, mode, K, J, M, beta, d_scale, cat, ncat, d_var, d_preds, d_cat_sum, d_cat_max, d_cat_count, true);
}

// ---- greedy batch selection on the resident rows (kernels B1 ... B4 of fsnap_select.hip) -----------------------------

namespace {

int select_session(fsnap_ctx* ctx, const char* who) {
    if (!ctx->sel_active)
        return ctx->fail(FSNAP_E_ARG, "%s: no selection session (fsnap_select_begin; new rows or a new category layout end one)",
                         who);
    return FSNAP_OK;
}

int select_refresh(fsnap_ctx* ctx) {
    double* dcat = (double*)ctx->sel_cat.p;
    FSNAP_HIP(fsnap::launch_sel_scores((const double*)ctx->sel_var.p, ctx->sel_has_scale ? (const double*)ctx->sel_scale.p : nullptr,
                                       (const int*)ctx->sel_idx.p, (const fsnap::CatChunk*)ctx->sel_ch.p, ctx->sel_nch,
                                       (const int*)ctx->sel_cbeg.p, (const int*)ctx->sel_alive.p, ctx->sel_ncat,
                                       (double*)ctx->sel_part.p, dcat, dcat + ctx->sel_ncat, ctx->stream),
              "launch fsnap_sel_chunk_k");
    return FSNAP_OK;
}

}  // namespace

int fsnap_select_begin(fsnap_ctx* ctx, int mode, int64_t K, int64_t J, const double* M, const double* scale, const int32_t* cat,
                       int ncat, int objective) {
    if (!ctx) return FSNAP_E_ARG;
    ctx->sel_active = false;
    if (objective != FSNAP_SELECT_SUM && objective != FSNAP_SELECT_MAX && objective != FSNAP_SELECT_MEAN)
        return ctx->fail(FSNAP_E_ARG, "fsnap_select_begin: unknown objective %d", objective);
    if (ncat <= 0 || (ctx->m > 0 && !cat)) return ctx->fail(FSNAP_E_ARG, "fsnap_select_begin: categories are needed (ncat = %d)", ncat);
    if (!M) return ctx->fail(FSNAP_E_ARG, "fsnap_select_begin: M is NULL");
    const int64_t m = ctx->m;
    static const int32_t no_rows = -1;
    if (!cat) cat = &no_rows;             // m = 0: never read
    FSNAP_HIP(hipSetDevice(ctx->device), "hipSetDevice");
    if (!ctx->sel_var.ensure((size_t)std::max<int64_t>(m, 1) * 8) || !ctx->sel_cat.ensure((size_t)ncat * 16) ||
        !ctx->sel_count.ensure((size_t)ncat * 8) || !ctx->sel_alive.ensure((size_t)ncat * 4) || !ctx->sel_out.ensure(16) ||
        (scale && !ctx->sel_scale.ensure((size_t)std::max<int64_t>(m, 1) * 8)))
        return ctx->fail(FSNAP_E_NOMEM, "hipMalloc(select) failed");
    if (scale && m > 0)
        FSNAP_HIP(hipMemcpyAsync(ctx->sel_scale.p, scale, (size_t)m * 8, hipMemcpyHostToDevice, ctx->stream), "hipMemcpy(scale)");
    // the initial variances and scores are those of fsnap_row_variance (kernels U1 / U1G, U2, U3), left on the device
    double* dcat = (double*)ctx->sel_cat.p;
    int rc = row_variance(ctx, mode, K, J, M, nullptr, scale && m > 0 ? (const double*)ctx->sel_scale.p : nullptr, cat, ncat,
                          m > 0 ? (double*)ctx->sel_var.p : nullptr, nullptr, dcat, dcat + ncat, nullptr, true);
    if (rc) return rc;
    // the session's own copy of the category layout: a later fsnap_row_variance call may replace the context's
    const int64_t nch = ctx->uq_hcbeg[(size_t)ncat];
    if (!ctx->sel_idx.ensure((size_t)std::max<int64_t>(m, 1) * 4) || !ctx->sel_ch.ensure((size_t)std::max<int64_t>(nch, 1) * 16) ||
        !ctx->sel_cbeg.ensure(((size_t)ncat + 1) * 4) || !ctx->sel_part.ensure((size_t)std::max<int64_t>(nch, 1) * 16))
        return ctx->fail(FSNAP_E_NOMEM, "hipMalloc(select categories) failed");
    if (m > 0) FSNAP_HIP(hipMemcpyAsync(ctx->sel_idx.p, ctx->uq_idx.p, (size_t)m * 4, hipMemcpyDeviceToDevice, ctx->stream), "hipMemcpy(idx)");
    if (nch > 0)
        FSNAP_HIP(hipMemcpyAsync(ctx->sel_ch.p, ctx->uq_ch.p, (size_t)nch * 16, hipMemcpyDeviceToDevice, ctx->stream), "hipMemcpy(chunks)");
    FSNAP_HIP(hipMemcpyAsync(ctx->sel_cbeg.p, ctx->uq_cbeg.p, ((size_t)ncat + 1) * 4, hipMemcpyDeviceToDevice, ctx->stream),
              "hipMemcpy(cbeg)");
    ctx->sel_hcount = ctx->uq_hcount;
    ctx->sel_halive.resize((size_t)ncat);
    for (int c = 0; c < ncat; ++c) ctx->sel_halive[(size_t)c] = ctx->sel_hcount[(size_t)c] > 0;    // an empty category is never picked
    FSNAP_HIP(hipMemcpyAsync(ctx->sel_count.p, ctx->sel_hcount.data(), (size_t)ncat * 8, hipMemcpyHostToDevice, ctx->stream),
              "hipMemcpy(count)");
    FSNAP_HIP(hipMemcpyAsync(ctx->sel_alive.p, ctx->sel_halive.data(), (size_t)ncat * 4, hipMemcpyHostToDevice, ctx->stream),
              "hipMemcpy(alive)");
    FSNAP_HIP(hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");
    ctx->uq_inflight = false;
    ctx->sel_m = m;
    ctx->sel_nch = m > 0 ? nch : 0;
    ctx->sel_ncat = ncat;
    ctx->sel_objective = objective;
    ctx->sel_has_scale = scale && m > 0;
    ctx->sel_active = true;
    return FSNAP_OK;
}

int fsnap_select_pick(fsnap_ctx* ctx, int retire, int32_t* category, double* score) {
    if (!ctx) return FSNAP_E_ARG;
    int rc = select_session(ctx, "fsnap_select_pick");
    if (rc) return rc;
    if (!category || !score) return ctx->fail(FSNAP_E_ARG, "fsnap_select_pick: NULL argument");
    FSNAP_HIP(hipSetDevice(ctx->device), "hipSetDevice");
    const double* dcat = (const double*)ctx->sel_cat.p;
    FSNAP_HIP(fsnap::launch_sel_pick(dcat, dcat + ctx->sel_ncat, (const int64_t*)ctx->sel_count.p, (int*)ctx->sel_alive.p,
                                     ctx->sel_ncat, ctx->sel_objective, retire != 0, (double*)ctx->sel_out.p, ctx->stream),
              "launch fsnap_sel_pick_k");
    double out[2] = {0.0, -1.0};
    FSNAP_HIP(hipMemcpyAsync(out, ctx->sel_out.p, 16, hipMemcpyDeviceToHost, ctx->stream), "hipMemcpy(pick)");
    FSNAP_HIP(hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");
    const int32_t c = (int32_t)out[1];
    if (c >= ctx->sel_ncat) return ctx->fail(FSNAP_E_HIP, "fsnap_select_pick: category %d out of range", c);
    if (retire && c >= 0) ctx->sel_halive[(size_t)c] = 0;
    *category = c < 0 ? -1 : c;
    *score = out[0];
    return FSNAP_OK;
}

int fsnap_select_retire(fsnap_ctx* ctx, int32_t category) {
    if (!ctx) return FSNAP_E_ARG;
    int rc = select_session(ctx, "fsnap_select_retire");
    if (rc) return rc;
    if (category < 0 || category >= ctx->sel_ncat || !ctx->sel_halive[(size_t)category])
        return ctx->fail(FSNAP_E_ARG, "fsnap_select_retire: category %d is not alive", category);
    FSNAP_HIP(hipSetDevice(ctx->device), "hipSetDevice");
    FSNAP_HIP(hipMemsetAsync((int32_t*)ctx->sel_alive.p + category, 0, 4, ctx->stream), "hipMemset(alive)");
    ctx->sel_halive[(size_t)category] = 0;
    return FSNAP_OK;
}

int fsnap_select_downdate(fsnap_ctx* ctx, int64_t K, int64_t J, const double* V) {
    if (!ctx) return FSNAP_E_ARG;
    int rc = select_session(ctx, "fsnap_select_downdate");
    if (rc) return rc;
    if (!V) return ctx->fail(FSNAP_E_ARG, "fsnap_select_downdate: V is NULL");
    if (K < 1 || K > 0x3FFFFFFF || J < 1 || J > 0x3FFFFFFF)
        return ctx->fail(FSNAP_E_ARG, "fsnap_select_downdate: K = %lld, J = %lld", (long long)K, (long long)J);
    const int64_t m = ctx->sel_m;
    if (m == 0) return FSNAP_OK;
    if (m != ctx->m || K != ctx->K)
        return ctx->fail(FSNAP_E_ARG, "fsnap_select_downdate: K = %lld, the resident rows have %lld columns", (long long)K,
                         (long long)ctx->K);
    if ((rc = check_rows(ctx))) return rc;
    FSNAP_HIP(hipSetDevice(ctx->device), "hipSetDevice");
    const int64_t Kp = (K + 15) / 16 * 16, Jp = (J + 15) / 16 * 16;
    const size_t nV = (size_t)(Kp * Jp);
    ctx->sel_hV.assign(nV, 0.0);
    for (int64_t k = 0; k < K; ++k) std::memcpy(&ctx->sel_hV[(size_t)(k * Jp)], V + k * J, (size_t)J * 8);
    if (!ctx->sel_V.ensure(nV * 8)) return ctx->fail(FSNAP_E_NOMEM, "hipMalloc(V) failed");
    FSNAP_HIP(hipMemcpyAsync(ctx->sel_V.p, ctx->sel_hV.data(), nV * 8, hipMemcpyHostToDevice, ctx->stream), "hipMemcpy(V)");
    FSNAP_HIP(fsnap::launch_sel_rows(ctx->dA, ctx->lda, m, (int)K, (const double*)ctx->sel_V.p, (int)Jp, (double*)ctx->sel_var.p,
                                     ctx->stream),
              "launch fsnap_sel_rows_k");
    if ((rc = select_refresh(ctx))) return rc;
    FSNAP_HIP(hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");     // the staging of V may be reused
    return FSNAP_OK;
}

int fsnap_select_state(fsnap_ctx* ctx, double* var, double* cat_sum, double* cat_max, int64_t* cat_count, int32_t* alive) {
    if (!ctx) return FSNAP_E_ARG;
    int rc = select_session(ctx, "fsnap_select_state");
    if (rc) return rc;
    FSNAP_HIP(hipSetDevice(ctx->device), "hipSetDevice");
    const int ncat = ctx->sel_ncat;
    const double* dcat = (const double*)ctx->sel_cat.p;
    if (var && ctx->sel_m > 0)
        FSNAP_HIP(hipMemcpyAsync(var, ctx->sel_var.p, (size_t)ctx->sel_m * 8, hipMemcpyDeviceToHost, ctx->stream), "hipMemcpy(var)");
    if (cat_sum) FSNAP_HIP(hipMemcpyAsync(cat_sum, dcat, (size_t)ncat * 8, hipMemcpyDeviceToHost, ctx->stream), "hipMemcpy(sum)");
    if (cat_max) FSNAP_HIP(hipMemcpyAsync(cat_max, dcat + ncat, (size_t)ncat * 8, hipMemcpyDeviceToHost, ctx->stream), "hipMemcpy(max)");
    if (alive) FSNAP_HIP(hipMemcpyAsync(alive, ctx->sel_alive.p, (size_t)ncat * 4, hipMemcpyDeviceToHost, ctx->stream), "hipMemcpy(alive)");
    FSNAP_HIP(hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");
    if (cat_count) std::memcpy(cat_count, ctx->sel_hcount.data(), (size_t)ncat * 8);
    return FSNAP_OK;
}

int fsnap_select_end(fsnap_ctx* ctx) {
    if (!ctx) return FSNAP_E_ARG;
    ctx->sel_active = false;
    return FSNAP_OK;
}

namespace {

// The sorted row index of a unit layout (configurations, units): offsets[0 ... count] (the caller's name for them: what) start
// at 0 and do not decrease, there are at most m positions, and every position names a distinct row of the context -- a row
// written by two units would be a race.  per_row_check(p, row) runs on every position that passed; a non-zero return ends the
// check with that code.  rows_what / rows_given: the per-row arrays that must be there as soon as there is a position.
template <class PerRow>
int check_unit_index(fsnap_ctx* ctx, const char* who, const char* what, const int32_t* sorted_rows, const int64_t* offsets,
                     int64_t count, int64_t m, PerRow&& per_row_check, const char* rows_what = "sorted_rows",
                     bool rows_given = true) {
    if (offsets[0] != 0) return ctx->fail(FSNAP_E_ARG, "%s: %s[0] = %lld", who, what, (long long)offsets[0]);
    for (int64_t u = 0; u < count; ++u)
        if (offsets[u + 1] < offsets[u]) return ctx->fail(FSNAP_E_ARG, "%s: %s decrease at %lld", who, what, (long long)u);
    const int64_t npos = offsets[count];
    if (npos > m) return ctx->fail(FSNAP_E_ARG, "%s: %lld positions for %lld rows", who, (long long)npos, (long long)m);
    if (npos > 0 && (!sorted_rows || !rows_given)) return ctx->fail(FSNAP_E_ARG, "%s: %s is NULL", who, rows_what);
    std::vector<unsigned char> seen((size_t)std::max<int64_t>(m, 1), 0);
    for (int64_t p = 0; p < npos; ++p) {
        const int32_t r = sorted_rows[p];
        if (r < 0 || r >= m || seen[(size_t)r])
            return ctx->fail(FSNAP_E_ARG, "%s: sorted_rows[%lld] = %d is out of range or repeated", who, (long long)p, r);
        seen[(size_t)r] = 1;
        if (const int rc = per_row_check(p, r)) return rc;
    }
    return FSNAP_OK;
}

// Units by solve size d = min(n, J): the LDS kernels take d <= 32 / 64 / lds_max (bins 0 ... 2), global scratch the rest
// (bin 3, any d <= dmax).
struct UnitBins {
    int D[4];                          // the kernel class of each bin (0: global scratch)
    std::vector<int32_t> lists[4];     // the units of each bin, in unit order
    int nblk[4];                       // workgroups of each bin's launch
    int64_t dmax = 0;                  // the largest d of bin 3 (0 when it is empty)
};

// size(u): the rows of unit u = 0 ... count - 1, 0 leaves the unit out.  all: the four lists one after the other.  Bins 0 ... 2
// get at most 16 workgroups per CU; scratch(dmax) is the doubles of global scratch one workgroup of bin 3 needs: at most two
// workgroups per CU and ~1 GiB of scratch in all.
template <class Size, class Scratch>
UnitBins bin_units(int64_t count, Size&& size, int64_t J, int lds_max, int num_cu, Scratch&& scratch, std::vector<int32_t>& all) {
    UnitBins bins{{32, 64, lds_max, 0}, {}, {}, 0};
    for (int64_t u = 0; u < count; ++u) {
        const int64_t n = size(u);
        if (n == 0) continue;
        const int64_t d = std::min(n, J);
        const int b = d <= 32 ? 0 : d <= 64 ? 1 : d <= lds_max ? 2 : 3;
        bins.lists[b].push_back((int32_t)u);
        if (b == 3) bins.dmax = std::max(bins.dmax, d);
    }
    all.clear();
    for (auto& l : bins.lists) all.insert(all.end(), l.begin(), l.end());
    const int nblk_lds = std::max(1, 16 * num_cu);
    for (int b = 0; b < 3; ++b) bins.nblk[b] = (int)std::min<int64_t>((int64_t)bins.lists[b].size(), nblk_lds);
    bins.nblk[3] = bins.lists[3].empty()
                       ? 0
                       : (int)std::max<int64_t>(1, std::min<int64_t>({(int64_t)bins.lists[3].size(), 2 * (int64_t)num_cu,
                                                                      (int64_t)(1 << 27) / std::max<int64_t>(scratch(bins.dmax), 1)}));
    return bins;
}

// One launch per bin that has units: launch(D, workgroups, where the bin's list starts in the four lists, its units).
template <class Launch>
hipError_t launch_bins(const UnitBins& bins, Launch&& launch) {
    size_t first = 0;
    for (int b = 0; b < 4; ++b) {
        const int ncl = (int)bins.lists[b].size();
        if (ncl > 0)
            if (const hipError_t e = launch(bins.D[b], bins.nblk[b], first, ncl)) return e;
        first += (size_t)ncl;
    }
    return hipSuccess;
}

// What a pass over the resident rows with kernel 1A's pairs begins with: the context's device, the copies out of
// fsnap_row_variance's staging drained (once), the pairs current.  *wpack: the pairs to read.
int resident_weights(fsnap_ctx* ctx, const double** wpack) {
    FSNAP_HIP(hipSetDevice(ctx->device), "hipSetDevice");
    if (ctx->uq_inflight) {
        FSNAP_HIP(hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");
        ctx->uq_inflight = false;
    }
    int npk = 0;
    if (const int rc = ensure_wpack(ctx, &npk)) return rc;
    *wpack = ctx->wpack_override ? ctx->wpack_override : (const double*)ctx->wpack.p;
    return FSNAP_OK;
}

// The front that fsnap_loco_rows, fsnap_loco_rows_uq and fsnap_influence_rows share.  unit_pass_check: their common
// arguments against the resident rows.  unit_pass_stage (there is a position: npos > 0) queues everything up to kernel L1 and
// owns loco_hM / loco_hlist and loco_M / idx / off / list / Z / aux, of which UnitPass is the typed view; the outputs,
// loco_v, loco_H and the infl_* buffers are the entry point's own.
struct UnitPass {
    const double *Z, *pw, *pe, *pb;    // kernel L1's results per position: zeta (Jp doubles), w_eff, e, a . beta
    const int* idx;                    // on the device: the sorted row index, the configuration offsets, the bins' lists
    const int64_t* off;
    const int* lists;
    int Jp;                            // J in 16-multiples
    UnitBins bins;                     // configurations by solve size d_c = min(n_c, J)
    int dmax;                          // general path (bin 3): one slice of hslice = scratch_doubles(dmax) per workgroup
    int64_t hslice;
    int nvg;                           // the most workgroups of any bin's launch
};

int unit_pass_check(fsnap_ctx* ctx, const char* who, int64_t K, int64_t J, const int32_t* sorted_rows, const int64_t* cfg_offsets,
                    int64_t ncfg) {
    if (K < 1 || K > 0x3FFFFFFF) return ctx->fail(FSNAP_E_ARG, "%s: K = %lld", who, (long long)K);
    if (J < 1 || J > 0x3FFFFFFF) return ctx->fail(FSNAP_E_ARG, "%s: J = %lld", who, (long long)J);
    if (ncfg < 0 || ncfg > 0x7FFFFFFF) return ctx->fail(FSNAP_E_ARG, "%s: ncfg = %lld", who, (long long)ncfg);
    const int64_t m = ctx->m;
    if (m > 0 && K != ctx->K)
        return ctx->fail(FSNAP_E_ARG, "%s: K = %lld, the resident rows have %lld columns", who, (long long)K, (long long)ctx->K);
    if (m > 0x7FFFFFFF) return ctx->fail(FSNAP_E_ARG, "%s: needs m < 2^31", who);
    return check_unit_index(ctx, who, "cfg_offsets", sorted_rows, cfg_offsets, ncfg, m, [](int64_t, int32_t) { return 0; });
}

int unit_pass_stage(fsnap_ctx* ctx, const char* label, int64_t K, int64_t J, const double* M, const double* beta,
                    const int32_t* sorted_rows, const int64_t* cfg_offsets, int64_t ncfg, int64_t (*scratch_doubles)(int64_t),
                    UnitPass* pass) {
    int rc;
    if ((rc = check_rows(ctx)) || (rc = check_weights(ctx))) return rc;
    const double* wpack = nullptr;
    if ((rc = resident_weights(ctx, &wpack))) return rc;
    UnitBins bins = bin_units(
        ncfg, [&](int64_t c) { return cfg_offsets[c + 1] - cfg_offsets[c]; }, J, fsnap::LOCO_MAX_LDS_D, ctx->num_cu,
        scratch_doubles, ctx->loco_hlist);
    const int64_t npos = cfg_offsets[ncfg], dmax = bins.dmax;
    const int nvg = std::max({bins.nblk[0], bins.nblk[1], bins.nblk[2], bins.nblk[3], 1});
    const int64_t Kp = (K + 15) / 16 * 16, Jp = (J + 15) / 16 * 16;
    const size_t nM = (size_t)(Kp * Jp);
    ctx->loco_hM.assign(nM + (size_t)Kp, 0.0);
    for (int64_t k = 0; k < K; ++k) std::memcpy(&ctx->loco_hM[(size_t)(k * Jp)], M + k * J, (size_t)J * 8);
    std::memcpy(&ctx->loco_hM[nM], beta, (size_t)K * 8);
    if (!ctx->loco_M.ensure((nM + (size_t)Kp) * 8) || !ctx->loco_idx.ensure((size_t)npos * 4) ||
        !ctx->loco_off.ensure((size_t)(ncfg + 1) * 8) || !ctx->loco_list.ensure(ctx->loco_hlist.size() * 4) ||
        !ctx->loco_Z.ensure((size_t)npos * (size_t)Jp * 8) || !ctx->loco_aux.ensure((size_t)npos * 3 * 8))
        return ctx->fail(FSNAP_E_NOMEM, "hipMalloc(%s) failed", label);
    FSNAP_HIP(hipMemcpyAsync(ctx->loco_M.p, ctx->loco_hM.data(), (nM + (size_t)Kp) * 8, hipMemcpyHostToDevice, ctx->stream),
              "hipMemcpy(M)");
    FSNAP_HIP(hipMemcpyAsync(ctx->loco_idx.p, sorted_rows, (size_t)npos * 4, hipMemcpyHostToDevice, ctx->stream), "hipMemcpy(idx)");
    FSNAP_HIP(hipMemcpyAsync(ctx->loco_off.p, cfg_offsets, (size_t)(ncfg + 1) * 8, hipMemcpyHostToDevice, ctx->stream),
              "hipMemcpy(offsets)");
    // npos > 0: a configuration has rows, so there is a list
    FSNAP_HIP(hipMemcpyAsync(ctx->loco_list.p, ctx->loco_hlist.data(), ctx->loco_hlist.size() * 4, hipMemcpyHostToDevice,
                             ctx->stream),
              "hipMemcpy(lists)");
    double* aux = (double*)ctx->loco_aux.p;
    FSNAP_HIP(fsnap::launch_loco_zeta(ctx->dA, ctx->lda, (int)K, (const int*)ctx->loco_idx.p, npos, wpack,
                                      (const double*)ctx->loco_M.p, (int)Jp, (const double*)ctx->loco_M.p + nM,
                                      (double*)ctx->loco_Z.p, aux, aux + npos, aux + 2 * npos, ctx->stream),
              "launch fsnap_loco_zeta_k");
    // The entry point sizes and clears its own buffers from here on, so its memsets follow kernel L1 on the stream.  Either
    // order gives the same result: kernel L1 neither reads nor writes those buffers.
    *pass = UnitPass{(const double*)ctx->loco_Z.p, aux, aux + npos, aux + 2 * npos, (const int*)ctx->loco_idx.p,
                     (const int64_t*)ctx->loco_off.p, (const int*)ctx->loco_list.p, (int)Jp, std::move(bins), (int)dmax,
                     scratch_doubles(dmax), nvg};
    return FSNAP_OK;
}

}  // namespace

// ---- leave-one-configuration-out predictions of the resident training rows (kernels L1, L2 of fsnap_loco.hip) --------

int fsnap_loco_rows(fsnap_ctx* ctx, int64_t K, int64_t J, const double* M, const double* beta, const int32_t* sorted_rows,
                    const int64_t* cfg_offsets, int64_t ncfg, double* pred_out, double* cfg_info_out) {
    if (!ctx) return FSNAP_E_ARG;
    const char* who = "fsnap_loco_rows";
    if (!M || !beta || !cfg_offsets || !pred_out || (ncfg > 0 && !cfg_info_out))
        return ctx->fail(FSNAP_E_ARG, "%s: NULL argument", who);
    int rc = unit_pass_check(ctx, who, K, J, sorted_rows, cfg_offsets, ncfg);
    if (rc) return rc;
    const int64_t m = ctx->m, npos = cfg_offsets[ncfg];
    for (int64_t i = 0; i < m; ++i) pred_out[i] = std::numeric_limits<double>::quiet_NaN();
    for (int64_t c = 0; c < ncfg; ++c) {      // empty configurations: nothing to leave out
        cfg_info_out[4 * c] = 0.0;
        cfg_info_out[4 * c + 1] = std::numeric_limits<double>::infinity();
        cfg_info_out[4 * c + 2] = 1.0;
        cfg_info_out[4 * c + 3] = 1.0;
    }
    if (npos == 0) return FSNAP_OK;
    UnitPass ps;
    if ((rc = unit_pass_stage(ctx, "loco", K, J, M, beta, sorted_rows, cfg_offsets, ncfg, fsnap::loco_scratch_doubles, &ps)))
        return rc;
    const int nblk3 = ps.bins.nblk[3];
    if (!ctx->loco_pred.ensure((size_t)m * 8) || !ctx->loco_info.ensure((size_t)ncfg * 4 * 8) ||
        !ctx->loco_v.ensure((size_t)ps.nvg * (size_t)ps.Jp * 8) ||
        (nblk3 > 0 && !ctx->loco_H.ensure((size_t)nblk3 * (size_t)ps.hslice * 8)))
        return ctx->fail(FSNAP_E_NOMEM, "hipMalloc(loco) failed");
    FSNAP_HIP(hipMemsetAsync(ctx->loco_pred.p, 0xFF, (size_t)m * 8, ctx->stream), "hipMemset(pred)");   // all-ones: NaN
    const auto launch = [&](int D, int nblk, size_t first, int ncl) {
        return fsnap::launch_loco_cfg(D, nblk, ps.Z, ps.Jp, (int)J, ps.pw, ps.pe, ps.pb, ps.idx, ps.off, ps.lists + first, ncl,
                                      (double*)ctx->loco_H.p, ps.dmax, (double*)ctx->loco_v.p, (double*)ctx->loco_pred.p,
                                      (double*)ctx->loco_info.p, ctx->stream);
    };
    FSNAP_HIP(launch_bins(ps.bins, launch), "launch fsnap_loco_cfg_k");
    ctx->loco_hinfo.resize((size_t)ncfg * 4);
    FSNAP_HIP(hipMemcpyAsync(pred_out, ctx->loco_pred.p, (size_t)m * 8, hipMemcpyDeviceToHost, ctx->stream), "hipMemcpy(pred)");
    FSNAP_HIP(hipMemcpyAsync(ctx->loco_hinfo.data(), ctx->loco_info.p, (size_t)ncfg * 32, hipMemcpyDeviceToHost, ctx->stream),
              "hipMemcpy(info)");
    FSNAP_HIP(hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");
    for (int64_t c = 0; c < ncfg; ++c)
        if (cfg_offsets[c + 1] > cfg_offsets[c]) std::memcpy(cfg_info_out + 4 * c, &ctx->loco_hinfo[(size_t)(4 * c)], 32);
    return FSNAP_OK;
}

// ---- leave-one-configuration-out leverages, log-determinants and joint distances (kernels L1 of fsnap_loco.hip and L3 of
// fsnap_loco_uq.hip); fsnap_loco_rows's arguments, checks and predictions -----------------------------------------------

int fsnap_loco_rows_uq(fsnap_ctx* ctx, int64_t K, int64_t J, const double* M, const double* beta, const int32_t* sorted_rows,
                       const int64_t* cfg_offsets, int64_t ncfg, double* pred_out, double* lev_out, double* cfg_info_out) {
    if (!ctx) return FSNAP_E_ARG;
    const char* who = "fsnap_loco_rows_uq";
    if (!M || !beta || !cfg_offsets || !pred_out || !lev_out || (ncfg > 0 && !cfg_info_out))
        return ctx->fail(FSNAP_E_ARG, "%s: NULL argument", who);
    int rc = unit_pass_check(ctx, who, K, J, sorted_rows, cfg_offsets, ncfg);
    if (rc) return rc;
    const int64_t m = ctx->m, npos = cfg_offsets[ncfg];
    for (int64_t i = 0; i < m; ++i) pred_out[i] = lev_out[i] = std::numeric_limits<double>::quiet_NaN();
    for (int64_t c = 0; c < ncfg; ++c) {      // empty configurations: nothing to leave out
        cfg_info_out[6 * c] = 0.0;
        cfg_info_out[6 * c + 1] = std::numeric_limits<double>::infinity();
        cfg_info_out[6 * c + 2] = 1.0;
        cfg_info_out[6 * c + 3] = 1.0;
        cfg_info_out[6 * c + 4] = 0.0;      // log det and distance of nothing
        cfg_info_out[6 * c + 5] = 0.0;
    }
    if (npos == 0) return FSNAP_OK;
    UnitPass ps;
    if ((rc = unit_pass_stage(ctx, "loco", K, J, M, beta, sorted_rows, cfg_offsets, ncfg, fsnap::loco_uq_scratch_doubles, &ps)))
        return rc;
    const int nblk3 = ps.bins.nblk[3];
    if (!ctx->loco_pred.ensure((size_t)m * 8) || !ctx->loco_lev.ensure((size_t)m * 8) ||
        !ctx->loco_info.ensure((size_t)ncfg * 6 * 8) || !ctx->loco_v.ensure((size_t)ps.nvg * (size_t)ps.Jp * 8) ||
        (nblk3 > 0 && !ctx->loco_H.ensure((size_t)nblk3 * (size_t)ps.hslice * 8)))
        return ctx->fail(FSNAP_E_NOMEM, "hipMalloc(loco) failed");
    FSNAP_HIP(hipMemsetAsync(ctx->loco_pred.p, 0xFF, (size_t)m * 8, ctx->stream), "hipMemset(pred)");   // all-ones: NaN
    FSNAP_HIP(hipMemsetAsync(ctx->loco_lev.p, 0xFF, (size_t)m * 8, ctx->stream), "hipMemset(lev)");
    const auto launch = [&](int D, int nblk, size_t first, int ncl) {
        return fsnap::launch_loco_uq_cfg(D, nblk, ps.Z, ps.Jp, (int)J, ps.pw, ps.pe, ps.pb, ps.idx, ps.off, ps.lists + first, ncl,
                                         (double*)ctx->loco_H.p, ps.dmax, (double*)ctx->loco_v.p, (double*)ctx->loco_pred.p,
                                         (double*)ctx->loco_lev.p, (double*)ctx->loco_info.p, ctx->stream);
    };
    FSNAP_HIP(launch_bins(ps.bins, launch), "launch fsnap_loco_uq_cfg_k");
    ctx->loco_hinfo.resize((size_t)ncfg * 6);
    FSNAP_HIP(hipMemcpyAsync(pred_out, ctx->loco_pred.p, (size_t)m * 8, hipMemcpyDeviceToHost, ctx->stream), "hipMemcpy(pred)");
    FSNAP_HIP(hipMemcpyAsync(lev_out, ctx->loco_lev.p, (size_t)m * 8, hipMemcpyDeviceToHost, ctx->stream), "hipMemcpy(lev)");
    FSNAP_HIP(hipMemcpyAsync(ctx->loco_hinfo.data(), ctx->loco_info.p, (size_t)ncfg * 48, hipMemcpyDeviceToHost, ctx->stream),
              "hipMemcpy(info)");
    FSNAP_HIP(hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");
    for (int64_t c = 0; c < ncfg; ++c)
        if (cfg_offsets[c + 1] > cfg_offsets[c]) std::memcpy(cfg_info_out + 6 * c, &ctx->loco_hinfo[(size_t)(6 * c)], 48);
    return FSNAP_OK;
}

// ---- per-configuration influence vectors and the outer-product sums of the cluster-robust covariances (kernel L1 of
// fsnap_loco.hip, kernels I0 / I1 / I2 of fsnap_influence.hip); fsnap_loco_rows's arguments and checks ------------------------

int fsnap_influence_rows(fsnap_ctx* ctx, int mode, int64_t K, int64_t J, const double* M, const double* beta,
                         const int32_t* sorted_rows, const int64_t* cfg_offsets, int64_t ncfg, double* pred_out,
                         double* cfg_info_out, double* unit_out, double* S_out, double* V_out, double* Ws_out, double* Wv_out) {
    if (!ctx) return FSNAP_E_ARG;
    const char* who = "fsnap_influence_rows";
    if (mode != FSNAP_INFL_SCORES && mode != FSNAP_INFL_FULL) return ctx->fail(FSNAP_E_ARG, "%s: mode = %d", who, mode);
    const bool full = mode == FSNAP_INFL_FULL;
    if (!M || !beta || !cfg_offsets || (ncfg > 0 && (!cfg_info_out || !unit_out)))
        return ctx->fail(FSNAP_E_ARG, "%s: NULL argument", who);
    if (!full && (V_out || Wv_out || pred_out))
        return ctx->fail(FSNAP_E_ARG, "%s: V_out, Wv_out and pred_out need FSNAP_INFL_FULL", who);
    int rc = unit_pass_check(ctx, who, K, J, sorted_rows, cfg_offsets, ncfg);
    if (rc) return rc;
    const int64_t m = ctx->m, npos = cfg_offsets[ncfg];
    if (Ws_out) std::fill(Ws_out, Ws_out + J * J, 0.0);
    if (Wv_out) std::fill(Wv_out, Wv_out + J * J, 0.0);
    if (ncfg == 0 || m == 0) return FSNAP_OK;
    if (pred_out)
        for (int64_t i = 0; i < m; ++i) pred_out[i] = std::numeric_limits<double>::quiet_NaN();
    for (int64_t c = 0; c < ncfg; ++c) {      // configurations without rows; SCORES: every one (no factorisation, no pivot)
        const int64_t n = cfg_offsets[c + 1] - cfg_offsets[c];
        cfg_info_out[4 * c] = (double)std::min(n, J);
        cfg_info_out[4 * c + 1] = std::numeric_limits<double>::infinity();
        cfg_info_out[4 * c + 2] = 1.0;
        cfg_info_out[4 * c + 3] = n <= J ? 1.0 : 0.0;
        unit_out[3 * c] = unit_out[3 * c + 1] = unit_out[3 * c + 2] = 0.0;
    }
    if (S_out) std::fill(S_out, S_out + ncfg * J, 0.0);
    if (V_out) std::fill(V_out, V_out + ncfg * J, 0.0);
    if (npos == 0) return FSNAP_OK;
    const int64_t Jp = (J + 15) / 16 * 16, ntiles = (Jp / 16) * (Jp / 16 + 1) / 2;
    const bool want_ws = Ws_out != nullptr, want_wv = Wv_out != nullptr;
    if ((want_ws || want_wv) && fsnap::infl_chunks(ncfg) * ntiles > 0x7FFFFFFF)
        return ctx->fail(FSNAP_E_ARG, "%s: %lld units x %lld tiles are too many for one launch", who, (long long)ncfg, (long long)ntiles);
    // the bins and scratch of fsnap_loco_rows_uq (kernel I1 runs the body with UQ = true)
    UnitPass ps;
    if ((rc = unit_pass_stage(ctx, "influence", K, J, M, beta, sorted_rows, cfg_offsets, ncfg, fsnap::loco_uq_scratch_doubles, &ps)))
        return rc;
    const int nblk3 = ps.bins.nblk[3];
    const size_t nUJ = (size_t)ncfg * (size_t)Jp;
    if (!ctx->infl_S.ensure(nUJ * 8) || !ctx->infl_unit.ensure((size_t)ncfg * 3 * 8) ||
        ((want_ws || want_wv) && (!ctx->infl_part.ensure((size_t)(fsnap::infl_chunks(ncfg) * ntiles) * 256 * 8) ||
                                  !ctx->infl_W.ensure((size_t)(2 * J * J) * 8))) ||
        (full && (!ctx->loco_pred.ensure((size_t)m * 8) || !ctx->loco_info.ensure((size_t)ncfg * 4 * 8) ||
                  !ctx->infl_V.ensure(nUJ * 8) || !ctx->loco_v.ensure((size_t)ps.nvg * (size_t)Jp * 8) ||
                  (nblk3 > 0 && !ctx->loco_H.ensure((size_t)nblk3 * (size_t)ps.hslice * 8)))))
        return ctx->fail(FSNAP_E_NOMEM, "hipMalloc(influence) failed");
    // configurations without rows are in no list: their rows of S and V stay zero for kernel I2
    FSNAP_HIP(hipMemsetAsync(ctx->infl_S.p, 0, nUJ * 8, ctx->stream), "hipMemset(S)");
    if (full) {
        FSNAP_HIP(hipMemsetAsync(ctx->infl_V.p, 0, nUJ * 8, ctx->stream), "hipMemset(V)");
        FSNAP_HIP(hipMemsetAsync(ctx->loco_pred.p, 0xFF, (size_t)m * 8, ctx->stream), "hipMemset(pred)");   // all-ones: NaN
    }
    if (full) {
        const auto launch = [&](int D, int nblk, size_t first, int ncl) {
            return fsnap::launch_infl_cfg(D, nblk, ps.Z, ps.Jp, (int)J, ps.pw, ps.pe, ps.pb, ps.idx, ps.off, ps.lists + first, ncl,
                                          (double*)ctx->loco_H.p, ps.dmax, (double*)ctx->loco_v.p, (double*)ctx->loco_pred.p,
                                          (double*)ctx->loco_info.p, (double*)ctx->infl_V.p, (double*)ctx->infl_S.p,
                                          (double*)ctx->infl_unit.p, ctx->stream);
        };
        FSNAP_HIP(launch_bins(ps.bins, launch), "launch fsnap_infl_cfg_k");
    } else {
        const int ncl = (int)ctx->loco_hlist.size();      // the four lists one after the other: every configuration with rows
        FSNAP_HIP(fsnap::launch_infl_scores(std::min(ncl, std::max(1, 16 * ctx->num_cu)), ps.Z, ps.Jp, (int)J, ps.pw, ps.pe,
                                            ps.off, ps.lists, ncl, (double*)ctx->infl_S.p, (double*)ctx->infl_unit.p,
                                            ctx->stream),
                  "launch fsnap_infl_scores_k");
    }
    double* dW = (double*)ctx->infl_W.p;
    if (want_ws) {
        FSNAP_HIP(fsnap::launch_infl_outer((const double*)ctx->infl_S.p, ncfg, (int)Jp, (int)J, (double*)ctx->infl_part.p, dW,
                                           ctx->stream),
                  "launch fsnap_infl_outer_k");
        FSNAP_HIP(hipMemcpyAsync(Ws_out, dW, (size_t)(J * J) * 8, hipMemcpyDeviceToHost, ctx->stream), "hipMemcpy(Ws)");
    }
    if (want_wv) {      // the same partials buffer: the stream orders the two sums
        FSNAP_HIP(fsnap::launch_infl_outer((const double*)ctx->infl_V.p, ncfg, (int)Jp, (int)J, (double*)ctx->infl_part.p,
                                           dW + J * J, ctx->stream),
                  "launch fsnap_infl_outer_k");
        FSNAP_HIP(hipMemcpyAsync(Wv_out, dW + J * J, (size_t)(J * J) * 8, hipMemcpyDeviceToHost, ctx->stream), "hipMemcpy(Wv)");
    }
    ctx->loco_hinfo.resize((size_t)ncfg * 7);
    double* hunit = ctx->loco_hinfo.data() + (size_t)ncfg * 4;
    if (pred_out)
        FSNAP_HIP(hipMemcpyAsync(pred_out, ctx->loco_pred.p, (size_t)m * 8, hipMemcpyDeviceToHost, ctx->stream), "hipMemcpy(pred)");
    if (full)
        FSNAP_HIP(hipMemcpyAsync(ctx->loco_hinfo.data(), ctx->loco_info.p, (size_t)ncfg * 32, hipMemcpyDeviceToHost, ctx->stream),
                  "hipMemcpy(info)");
    FSNAP_HIP(hipMemcpyAsync(hunit, ctx->infl_unit.p, (size_t)ncfg * 24, hipMemcpyDeviceToHost, ctx->stream), "hipMemcpy(unit)");
    if (S_out)
        FSNAP_HIP(hipMemcpy2DAsync(S_out, (size_t)J * 8, ctx->infl_S.p, (size_t)Jp * 8, (size_t)J * 8, (size_t)ncfg,
                                   hipMemcpyDeviceToHost, ctx->stream),
                  "hipMemcpy(S)");
    if (V_out)
        FSNAP_HIP(hipMemcpy2DAsync(V_out, (size_t)J * 8, ctx->infl_V.p, (size_t)Jp * 8, (size_t)J * 8, (size_t)ncfg,
                                   hipMemcpyDeviceToHost, ctx->stream),
                  "hipMemcpy(V)");
    FSNAP_HIP(hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");
    for (int64_t c = 0; c < ncfg; ++c)
        if (cfg_offsets[c + 1] > cfg_offsets[c]) {
            if (full) std::memcpy(cfg_info_out + 4 * c, &ctx->loco_hinfo[(size_t)(4 * c)], 32);
            std::memcpy(unit_out + 3 * c, hunit + 3 * c, 24);
        }
    return FSNAP_OK;
}

// ---- leave-one-unit-out refits over a grid of alphas (kernel P1 of fsnap_path.hip) ---------------------------------------

int fsnap_ridge_path(fsnap_ctx* ctx, int64_t K, const double* G, const double* c, const double* alphas, int64_t Q,
                     const int32_t* sorted_rows, const int64_t* unit_offsets, int64_t nunits, const uint8_t* row_class,
                     int64_t nclass, double* sums_out, double* info_out, double* pred_out) {
    if (!ctx) return FSNAP_E_ARG;
    const char* who = "fsnap_ridge_path";
    if (!G || !c || !alphas || !unit_offsets || !sums_out || !info_out) return ctx->fail(FSNAP_E_ARG, "%s: NULL argument", who);
    if (K < 1 || K > fsnap::PATH_MAX_K)
        return ctx->fail(FSNAP_E_ARG, "%s: K = %lld (1 ... %d)", who, (long long)K, fsnap::PATH_MAX_K);
    if (Q < 1 || Q > 0xFFFFF) return ctx->fail(FSNAP_E_ARG, "%s: Q = %lld", who, (long long)Q);
    for (int64_t q = 0; q < Q; ++q)
        if (!std::isfinite(alphas[q]) || alphas[q] < 0.0)
            return ctx->fail(FSNAP_E_ARG, "%s: alphas[%lld] = %g is negative or not finite", who, (long long)q, alphas[q]);
    if (nclass < 1 || nclass > fsnap::PATH_MAX_CLASS)
        return ctx->fail(FSNAP_E_ARG, "%s: nclass = %lld (1 ... %d)", who, (long long)nclass, fsnap::PATH_MAX_CLASS);
    if (nunits < 0 || nunits > 0x3FFFFFFF) return ctx->fail(FSNAP_E_ARG, "%s: nunits = %lld", who, (long long)nunits);
    const int64_t m = ctx->m;
    if (m > 0 && K != ctx->K)
        return ctx->fail(FSNAP_E_ARG, "%s: K = %lld, the resident rows have %lld columns", who, (long long)K, (long long)ctx->K);
    if (m > 0x7FFFFFFF) return ctx->fail(FSNAP_E_ARG, "%s: needs m < 2^31", who);
    // the two trailing arguments keep this entry point's own message for a missing per-row array ("sorted_rows / row_class is
    // NULL", raised where the other callers raise "sorted_rows is NULL"); the class of every listed row is checked as it passes
    int rc = check_unit_index(
        ctx, who, "unit_offsets", sorted_rows, unit_offsets, nunits, m,
        [&](int64_t, int32_t r) {
            return row_class[r] < nclass ? FSNAP_OK
                                         : ctx->fail(FSNAP_E_ARG, "%s: row %d has class %d, nclass = %lld", who, r, (int)row_class[r],
                                                     (long long)nclass);
        },
        "sorted_rows / row_class", row_class != nullptr);
    if (rc) return rc;
    const int64_t npos = unit_offsets[nunits];
    const size_t nsum = (size_t)Q * (size_t)nunits * (size_t)nclass * 4, ninfo = (size_t)Q * (size_t)nunits * 2;
    if (npos == 0) {                              // no rows at all: every unit is empty, nothing to leave out
        std::fill(sums_out, sums_out + nsum, 0.0);
        for (size_t i = 0; i < ninfo; i += 2) {
            info_out[i] = std::numeric_limits<double>::infinity();
            info_out[i + 1] = 1.0;
        }
        if (pred_out) std::fill(pred_out, pred_out + (size_t)Q * (size_t)m, std::numeric_limits<double>::quiet_NaN());
        return FSNAP_OK;
    }
    if ((rc = check_rows(ctx)) || (rc = check_weights(ctx))) return rc;
    const double* wpack = nullptr;
    if ((rc = resident_weights(ctx, &wpack))) return rc;
    const int nblocks = (int)std::min<int64_t>(nunits, (int64_t)fsnap::path_blocks_per_cu((int)K) * std::max(1, ctx->num_cu));
    const size_t nin = (size_t)(K * K + K + Q);
    if (!ctx->path_in.ensure(nin * 8) || !ctx->path_cls.ensure((size_t)m) || !ctx->loco_idx.ensure((size_t)npos * 4) ||
        !ctx->loco_off.ensure((size_t)(nunits + 1) * 8) ||
        !ctx->path_base.ensure((size_t)nblocks * fsnap::path_base_doubles((int)K) * 8) || !ctx->path_sums.ensure(nsum * 8) ||
        !ctx->path_info.ensure(ninfo * 8) || (pred_out && !ctx->path_pred.ensure((size_t)Q * (size_t)m * 8)))
        return ctx->fail(FSNAP_E_NOMEM, "hipMalloc(ridge path) failed");
    double* din = (double*)ctx->path_in.p;
    FSNAP_HIP(hipMemcpyAsync(din, G, (size_t)(K * K) * 8, hipMemcpyHostToDevice, ctx->stream), "hipMemcpy(G)");
    FSNAP_HIP(hipMemcpyAsync(din + K * K, c, (size_t)K * 8, hipMemcpyHostToDevice, ctx->stream), "hipMemcpy(c)");
    FSNAP_HIP(hipMemcpyAsync(din + K * K + K, alphas, (size_t)Q * 8, hipMemcpyHostToDevice, ctx->stream), "hipMemcpy(alphas)");
    FSNAP_HIP(hipMemcpyAsync(ctx->path_cls.p, row_class, (size_t)m, hipMemcpyHostToDevice, ctx->stream), "hipMemcpy(classes)");
    FSNAP_HIP(hipMemcpyAsync(ctx->loco_idx.p, sorted_rows, (size_t)npos * 4, hipMemcpyHostToDevice, ctx->stream), "hipMemcpy(idx)");
    FSNAP_HIP(hipMemcpyAsync(ctx->loco_off.p, unit_offsets, (size_t)(nunits + 1) * 8, hipMemcpyHostToDevice, ctx->stream),
              "hipMemcpy(offsets)");
    // the kernel writes every entry of sums and info (units without rows: zero sums, info (inf, 1))
    if (pred_out) FSNAP_HIP(hipMemsetAsync(ctx->path_pred.p, 0xFF, (size_t)Q * (size_t)m * 8, ctx->stream), "hipMemset(pred)");
    FSNAP_HIP(fsnap::launch_ridge_path(nblocks, ctx->dA, ctx->lda, (int)K, wpack, ctx->db, (const int*)ctx->loco_idx.p,
                                       (const int64_t*)ctx->loco_off.p, (int)nunits, din, din + K * K, din + K * K + K, (int)Q,
                                       (const unsigned char*)ctx->path_cls.p, (int)nclass, (double*)ctx->path_base.p,
                                       (double*)ctx->path_sums.p, (double*)ctx->path_info.p,
                                       pred_out ? (double*)ctx->path_pred.p : nullptr, m, ctx->stream),
              "launch fsnap_path_k");
    FSNAP_HIP(hipMemcpyAsync(sums_out, ctx->path_sums.p, nsum * 8, hipMemcpyDeviceToHost, ctx->stream), "hipMemcpy(sums)");
    FSNAP_HIP(hipMemcpyAsync(info_out, ctx->path_info.p, ninfo * 8, hipMemcpyDeviceToHost, ctx->stream), "hipMemcpy(info)");
    if (pred_out)
        FSNAP_HIP(hipMemcpyAsync(pred_out, ctx->path_pred.p, (size_t)Q * (size_t)m * 8, hipMemcpyDeviceToHost, ctx->stream),
                  "hipMemcpy(pred)");
    FSNAP_HIP(hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");
    return FSNAP_OK;
}

// ---- grouped K-fold LASSO alpha paths on the per-fold statistics (kernels S1, S2 of fsnap_lasso.hip) -------------------

int fsnap_lasso_path(fsnap_ctx* ctx, int64_t K, int64_t F, int64_t nsub, const double* d_stats, const double* alphas, int64_t Q,
                     int64_t max_iter, double tol, double* coef_out, double* info_out, double* heldout_out) {
    if (!ctx) return FSNAP_E_ARG;
    const char* who = "fsnap_lasso_path";
    if (!alphas || !coef_out || !info_out || !heldout_out) return ctx->fail(FSNAP_E_ARG, "%s: NULL argument", who);
    int rc = fold_check(ctx, who, K, fsnap::LASSO_MAX_K, F, nsub, Q, Q, d_stats);
    if (rc) return rc;
    if (max_iter < 1 || max_iter > 0x7FFFFFFF) return ctx->fail(FSNAP_E_ARG, "%s: max_iter = %lld", who, (long long)max_iter);
    if (!std::isfinite(tol) || tol < 0.0) return ctx->fail(FSNAP_E_ARG, "%s: tol = %g is negative or not finite", who, tol);
    for (int64_t q = 0; q < Q; ++q)
        if (!std::isfinite(alphas[q]) || alphas[q] < 0.0)
            return ctx->fail(FSNAP_E_ARG, "%s: alphas[%lld] = %g is negative or not finite", who, (long long)q, alphas[q]);
    const double *dfolds, *dtotal;
    if ((rc = fold_stage(ctx, who, K, F, nsub, d_stats, &dfolds, &dtotal))) return rc;
    const int64_t nprob = (F + 1) * Q;
    if (!ctx->lasso_alphas.ensure((size_t)Q * 8) || !ctx->lasso_coef.ensure((size_t)nprob * K * 8) ||
        !ctx->lasso_info.ensure((size_t)nprob * 4 * 8) || !ctx->lasso_held.ensure((size_t)F * Q * 3 * 8))
        return ctx->fail(FSNAP_E_NOMEM, "hipMalloc(lasso path) failed");
    FSNAP_HIP(hipMemcpyAsync(ctx->lasso_alphas.p, alphas, (size_t)Q * 8, hipMemcpyHostToDevice, ctx->stream), "hipMemcpy(alphas)");
    FSNAP_HIP(fsnap::launch_lasso_cd(fold_grid(ctx, nprob, fsnap::lasso_blocks_per_cu((int)K)), dfolds, dtotal,
                                     (const double*)ctx->lasso_alphas.p, (int)K, (int)F, (int)Q, (int)max_iter, tol,
                                     (double*)ctx->lasso_coef.p, (double*)ctx->lasso_info.p, (double*)ctx->lasso_held.p,
                                     ctx->stream),
              "launch fsnap_lasso_cd_k");
    return fold_finish(ctx,
                       {{coef_out, ctx->lasso_coef.p, (size_t)nprob * K * 8},
                        {info_out, ctx->lasso_info.p, (size_t)nprob * 4 * 8},
                        {heldout_out, ctx->lasso_held.p, (size_t)F * Q * 3 * 8}},
                       coef_out, nprob * K);
}

// ---- grouped K-fold ARD threshold paths on the per-fold statistics (kernel S1 of fsnap_lasso.hip, A1 of fsnap_ard.hip) ----

int fsnap_ard_path(fsnap_ctx* ctx, int64_t K, int64_t F, int64_t nsub, const double* d_stats, const double* hyper, int64_t Q,
                   int64_t max_iter, double tol, double* coef_out, double* lambda_out, double* info_out, double* heldout_out) {
    if (!ctx) return FSNAP_E_ARG;
    const char* who = "fsnap_ard_path";
    if (!hyper || !coef_out || !lambda_out || !info_out || !heldout_out) return ctx->fail(FSNAP_E_ARG, "%s: NULL argument", who);
    int rc = fold_check(ctx, who, K, fsnap::ARD_MAX_K, F, nsub, Q, Q, d_stats);
    if (rc) return rc;
    if (max_iter < 1 || max_iter > 0x7FFFFFFF) return ctx->fail(FSNAP_E_ARG, "%s: max_iter = %lld", who, (long long)max_iter);
    if (!std::isfinite(tol) || tol < 0.0) return ctx->fail(FSNAP_E_ARG, "%s: tol = %g is negative or not finite", who, tol);
    const int64_t nprob = (F + 1) * Q;
    for (int64_t i = 0; i < nprob * 6; ++i) {
        const double h = hyper[i];
        // entries 4 and 5 of a problem: threshold_lambda and alpha_init, both positive
        if (!std::isfinite(h) || h < 0.0 || (i % 6 >= 4 && h <= 0.0))
            return ctx->fail(FSNAP_E_ARG, "%s: hyper[%lld][%lld] = %g", who, (long long)(i / 6), (long long)(i % 6), h);
    }
    const double *dfolds, *dtotal;
    if ((rc = fold_stage(ctx, who, K, F, nsub, d_stats, &dfolds, &dtotal))) return rc;
    if (!ctx->ard_hyper.ensure((size_t)nprob * 6 * 8) || !ctx->ard_coef.ensure((size_t)nprob * K * 8) ||
        !ctx->ard_lambda.ensure((size_t)nprob * K * 8) || !ctx->ard_info.ensure((size_t)nprob * 6 * 8) ||
        !ctx->ard_held.ensure((size_t)F * Q * 3 * 8))
        return ctx->fail(FSNAP_E_NOMEM, "hipMalloc(ard path) failed");
    FSNAP_HIP(hipMemcpyAsync(ctx->ard_hyper.p, hyper, (size_t)nprob * 6 * 8, hipMemcpyHostToDevice, ctx->stream), "hipMemcpy(hyper)");
    FSNAP_HIP(fsnap::launch_ard_path(fold_grid(ctx, nprob, fsnap::ard_blocks_per_cu((int)K)), dfolds, dtotal,
                                     (const double*)ctx->ard_hyper.p, (int)K, (int)F, (int)Q, (int)max_iter, tol,
                                     (double*)ctx->ard_coef.p, (double*)ctx->ard_lambda.p, (double*)ctx->ard_info.p,
                                     (double*)ctx->ard_held.p, ctx->stream),
              "launch fsnap_ard_path_k");
    // no scan: a failed problem is its own status 1, not the call's
    return fold_finish(ctx,
                       {{coef_out, ctx->ard_coef.p, (size_t)nprob * K * 8},
                        {lambda_out, ctx->ard_lambda.p, (size_t)nprob * K * 8},
                        {info_out, ctx->ard_info.p, (size_t)nprob * 6 * 8},
                        {heldout_out, ctx->ard_held.p, (size_t)F * Q * 3 * 8}},
                       nullptr, 0);
}

// ---- grouped K-fold greedy forward-selection paths on the per-fold statistics (kernel S1 of fsnap_lasso.hip, O1 of fsnap_omp.hip)

int fsnap_omp_path(fsnap_ctx* ctx, int64_t K, int64_t F, int64_t nsub, const double* d_stats, int criterion,
                   const int32_t* forced, int64_t nforced, int64_t S, const int32_t* levels, int64_t Q, int32_t* order_out,
                   double* path_out, double* heldout_out, double* coef_out) {
    if (!ctx) return FSNAP_E_ARG;
    const char* who = "fsnap_omp_path";
    if (!levels || !order_out || !path_out || !heldout_out || !coef_out || (nforced > 0 && !forced))
        return ctx->fail(FSNAP_E_ARG, "%s: NULL argument", who);
    int rc = fold_check(ctx, who, K, fsnap::OMP_MAX_K, F, nsub, Q, 1, d_stats);
    if (rc) return rc;
    if (S < 1 || S > K || S > fsnap::OMP_MAX_S)
        return ctx->fail(FSNAP_E_ARG, "%s: S = %lld (1 ... min(K, %d))", who, (long long)S, fsnap::OMP_MAX_S);
    if (criterion != FSNAP_OMP_OMP && criterion != FSNAP_OMP_OLS) return ctx->fail(FSNAP_E_ARG, "%s: criterion = %d", who, criterion);
    for (int64_t i = 0; i < Q; ++i)
        if (levels[i] < 1 || levels[i] > S || (i > 0 && levels[i] < levels[i - 1]))
            return ctx->fail(FSNAP_E_ARG, "%s: levels[%lld] = %d (ascending, 1 ... %lld)", who, (long long)i, (int)levels[i], (long long)S);
    if (nforced < 0 || nforced > K) return ctx->fail(FSNAP_E_ARG, "%s: nforced = %lld", who, (long long)nforced);
    for (int64_t i = 0; i < nforced; ++i) {
        bool bad = forced[i] < 0 || forced[i] >= K;
        for (int64_t k = 0; k < i && !bad; ++k) bad = forced[k] == forced[i];
        if (bad) return ctx->fail(FSNAP_E_ARG, "%s: forced[%lld] = %d is out of range or repeated", who, (long long)i, (int)forced[i]);
    }
    const double *dfolds, *dtotal;
    if ((rc = fold_stage(ctx, who, K, F, nsub, d_stats, &dfolds, &dtotal))) return rc;
    const int64_t nprob = F + 1;
    if (!ctx->omp_in.ensure((size_t)(nforced + Q) * 4) || !ctx->omp_order.ensure((size_t)nprob * S * 4) ||
        !ctx->omp_path.ensure((size_t)nprob * S * 3 * 8) || !ctx->omp_held.ensure((size_t)F * S * 3 * 8) ||
        !ctx->omp_coef.ensure((size_t)nprob * Q * K * 8))
        return ctx->fail(FSNAP_E_NOMEM, "hipMalloc(omp path) failed");
    int* dforced = nforced ? (int*)ctx->omp_in.p : nullptr;
    int* dlevels = (int*)ctx->omp_in.p + nforced;
    if (nforced)
        FSNAP_HIP(hipMemcpyAsync(dforced, forced, (size_t)nforced * 4, hipMemcpyHostToDevice, ctx->stream), "hipMemcpy(forced)");
    FSNAP_HIP(hipMemcpyAsync(dlevels, levels, (size_t)Q * 4, hipMemcpyHostToDevice, ctx->stream), "hipMemcpy(levels)");
    FSNAP_HIP(fsnap::launch_omp_path(fold_grid(ctx, nprob, fsnap::omp_blocks_per_cu((int)K, (int)S)), dfolds, dtotal, (int)K,
                                     (int)F, criterion, dforced, (int)nforced, (int)S, dlevels, (int)Q, (int*)ctx->omp_order.p,
                                     (double*)ctx->omp_path.p, (double*)ctx->omp_held.p, (double*)ctx->omp_coef.p, ctx->stream),
              "launch fsnap_omp_path_k");
    return fold_finish(ctx,
                       {{order_out, ctx->omp_order.p, (size_t)nprob * S * 4},
                        {path_out, ctx->omp_path.p, (size_t)nprob * S * 3 * 8},
                        {heldout_out, ctx->omp_held.p, (size_t)F * S * 3 * 8},
                        {coef_out, ctx->omp_coef.p, (size_t)nprob * Q * K * 8}},
                       coef_out, nprob * Q * K);
}

// ---- grouped K-fold BCS sparsity paths on the per-fold statistics (kernel S1 of fsnap_lasso.hip, B1 of fsnap_bcs.hip) ------

int fsnap_bcs_path(fsnap_ctx* ctx, int64_t K, int64_t F, int64_t nsub, const double* d_stats, const double* hyper, int64_t Q,
                   int64_t max_active, int deletion, double* coef_out, int32_t* active_out, double* alpha_out,
                   double* errbar_out, int32_t* picks_out, double* info_out, double* heldout_out, double* sig_out) {
    if (!ctx) return FSNAP_E_ARG;
    const char* who = "fsnap_bcs_path";
    if (!hyper || !coef_out || !active_out || !alpha_out || !errbar_out || !picks_out || !info_out || !heldout_out || !sig_out)
        return ctx->fail(FSNAP_E_ARG, "%s: NULL argument", who);
    int rc = fold_check(ctx, who, K, fsnap::BCS_MAX_K, F, nsub, Q, Q, d_stats);
    if (rc) return rc;
    if (max_active < 1 || max_active > K || max_active > fsnap::BCS_MAX_ACTIVE)
        return ctx->fail(FSNAP_E_ARG, "%s: max_active = %lld (1 ... min(K, %d))", who, (long long)max_active, fsnap::BCS_MAX_ACTIVE);
    if (deletion != FSNAP_BCS_REFERENCE && deletion != FSNAP_BCS_EXACT) return ctx->fail(FSNAP_E_ARG, "%s: deletion = %d", who, deletion);
    int64_t P = 1;
    for (int64_t i = 0; i < Q; ++i) {
        const double *h = hyper + i * 4, it = h[3];
        const bool ok = std::isfinite(h[0]) && std::isfinite(h[1]) && std::isfinite(h[2]) && std::isfinite(it) && h[0] >= 0.0 &&
                        (h[0] > 0.0 || h[1] > 0.0) && h[2] >= 0.0 && it >= 1.0 && it <= 65536.0 && it == std::floor(it);
        if (!ok)
            return ctx->fail(FSNAP_E_ARG, "%s: hyper[%lld] = (%g, %g, %g, %g)", who, (long long)i, h[0], h[1], h[2], h[3]);
        P = std::max<int64_t>(P, (int64_t)it);
    }
    const int64_t nprob = (F + 1) * Q, MA = max_active;
    if ((double)nprob * (double)P * 8.0 > (double)FSNAP_CAT_STATS_MAX_BYTES)
        return ctx->fail(FSNAP_E_ARG, "%s: %lld problems x %lld picks", who, (long long)nprob, (long long)P);
    const double *dfolds, *dtotal;
    if ((rc = fold_stage(ctx, who, K, F, nsub, d_stats, &dfolds, &dtotal))) return rc;
    if (!ctx->bcs_hyper.ensure((size_t)Q * 4 * 8) || !ctx->bcs_coef.ensure((size_t)nprob * K * 8) ||
        !ctx->bcs_int.ensure((size_t)nprob * (MA + 2 * P) * 4) || !ctx->bcs_pos.ensure((size_t)nprob * MA * 2 * 8) ||
        !ctx->bcs_info.ensure((size_t)nprob * 6 * 8) || !ctx->bcs_held.ensure((size_t)F * Q * 3 * 8) ||
        !ctx->bcs_sig.ensure((size_t)Q * MA * MA * 8))
        return ctx->fail(FSNAP_E_NOMEM, "hipMalloc(bcs path) failed");
    int* dactive = (int*)ctx->bcs_int.p;
    int* dpicks = dactive + nprob * MA;
    double* dalpha = (double*)ctx->bcs_pos.p;
    double* derr = dalpha + nprob * MA;
    FSNAP_HIP(hipMemcpyAsync(ctx->bcs_hyper.p, hyper, (size_t)Q * 4 * 8, hipMemcpyHostToDevice, ctx->stream), "hipMemcpy(hyper)");
    FSNAP_HIP(fsnap::launch_bcs_path(fold_grid(ctx, nprob, fsnap::bcs_blocks_per_cu((int)K, (int)MA)), dfolds, dtotal,
                                     (const double*)ctx->bcs_hyper.p, (int)K, (int)F, (int)Q, (int)MA, (int)P,
                                     deletion == FSNAP_BCS_EXACT ? 1 : 0, (double*)ctx->bcs_coef.p, dactive, dalpha, derr, dpicks,
                                     (double*)ctx->bcs_info.p, (double*)ctx->bcs_held.p, (double*)ctx->bcs_sig.p, ctx->stream),
              "launch fsnap_bcs_path_k");
    // no scan: a failed problem is its own status 1, not the call's
    return fold_finish(ctx,
                       {{coef_out, ctx->bcs_coef.p, (size_t)nprob * K * 8},
                        {active_out, dactive, (size_t)nprob * MA * 4},
                        {picks_out, dpicks, (size_t)nprob * P * 2 * 4},
                        {alpha_out, dalpha, (size_t)nprob * MA * 8},
                        {errbar_out, derr, (size_t)nprob * MA * 8},
                        {info_out, ctx->bcs_info.p, (size_t)nprob * 6 * 8},
                        {heldout_out, ctx->bcs_held.p, (size_t)F * Q * 3 * 8},
                        {sig_out, ctx->bcs_sig.p, (size_t)Q * MA * MA * 8}},
                       nullptr, 0);
}

// ---- grouped K-fold spectral paths on the per-fold statistics (kernel S1 of fsnap_lasso.hip, E1 / E2 of fsnap_spectral.hip) --

int fsnap_spectral_path(fsnap_ctx* ctx, int64_t K, int64_t F, int64_t nsub, const double* d_stats, const double* alphas,
                        int64_t Qa, const double* rconds, int64_t Qr, double* eig_out, double* z_out, double* info_out,
                        double* set_out, double* fit_out, double* coef_out, double* heldout_out) {
    if (!ctx) return FSNAP_E_ARG;
    const char* who = "fsnap_spectral_path";
    if (!alphas || !rconds || !eig_out || !z_out || !info_out || !set_out || !fit_out || !heldout_out)
        return ctx->fail(FSNAP_E_ARG, "%s: NULL argument", who);
    if (Qa < 1 || Qr < 1 || Qa > 0xFFFFF || Qr > 0xFFFFF)
        return ctx->fail(FSNAP_E_ARG, "%s: Qa = %lld, Qr = %lld", who, (long long)Qa, (long long)Qr);
    const int64_t Q = Qa * Qr;
    int rc = fold_check(ctx, who, K, fsnap::SPEC_MAX_K, F, nsub, Q, Q, d_stats);
    if (rc) return rc;
    for (int64_t i = 0; i < Qa; ++i)
        if (!std::isfinite(alphas[i]) || alphas[i] < 0.0)
            return ctx->fail(FSNAP_E_ARG, "%s: alphas[%lld] = %g is negative or not finite", who, (long long)i, alphas[i]);
    for (int64_t i = 0; i < Qr; ++i)
        if (!std::isfinite(rconds[i]) || rconds[i] < 0.0)
            return ctx->fail(FSNAP_E_ARG, "%s: rconds[%lld] = %g is negative or not finite", who, (long long)i, rconds[i]);
    const int64_t nprob = F + 1;
    const double cap = (double)FSNAP_CAT_STATS_MAX_BYTES;
    if ((double)F * (double)Q * (double)nsub * 24.0 > cap || (coef_out && (double)nprob * (double)Q * (double)K * 8.0 > cap))
        return ctx->fail(FSNAP_E_ARG, "%s: %lld folds x %lld settings of results exceed FSNAP_CAT_STATS_MAX_BYTES", who,
                         (long long)F, (long long)Q);
    if (!cand_fits(F * nsub, K))                                      // fold_stage's own refusal, taken before anything is forgotten
        return ctx->fail(FSNAP_E_ARG, "%s: %lld blocks x %lld doubles exceed FSNAP_CAT_STATS_MAX_BYTES", who, (long long)(F * nsub),
                         (long long)FSNAP_PACKED_LEN(K));
    ctx->spec_done = false;                                           // from here on kernels are queued: the last call's times go
    const double *dfolds, *dtotal;
    if ((rc = fold_stage(ctx, who, K, F, nsub, d_stats, &dfolds, &dtotal))) return rc;
    const int nb1 = fold_grid(ctx, nprob, fsnap::spectral_eig_blocks_per_cu((int)K));
    const int nb2 = fold_grid(ctx, nprob * fsnap::spectral_slices((int)Q), fsnap::spectral_eval_blocks_per_cu((int)K));
    const size_t nwork = fsnap::spectral_vectors_in_lds((int)K) ? 1 : (size_t)nb1 * K * K;
    const size_t ncoef = (size_t)(coef_out ? nprob : 1) * Q * K;       // [fit | coefficients of the F refits]
    if (!ctx->spec_grid.ensure((size_t)Q * 2 * 8) || !ctx->spec_eig.ensure((size_t)nprob * K * 8) ||
        !ctx->spec_z.ensure((size_t)nprob * K * 8) || !ctx->spec_V.ensure((size_t)nprob * K * K * 8) ||
        !ctx->spec_info.ensure((size_t)nprob * 6 * 8) || !ctx->spec_work.ensure(nwork * 8) ||
        !ctx->spec_set.ensure((size_t)nprob * Q * 3 * 8) || !ctx->spec_coef.ensure(ncoef * 8) ||
        !ctx->spec_held.ensure((size_t)F * Q * nsub * 3 * 8))
        return ctx->fail(FSNAP_E_NOMEM, "hipMalloc(spectral path) failed");
    std::vector<double> grid((size_t)Q * 2);                          // setting q = ia Qr + ir
    for (int64_t ia = 0; ia < Qa; ++ia)
        for (int64_t ir = 0; ir < Qr; ++ir) {
            grid[(size_t)(ia * Qr + ir)] = alphas[ia];
            grid[(size_t)(Q + ia * Qr + ir)] = rconds[ir];
        }
    for (auto& ev : ctx->spec_ev)
        if (!ev) FSNAP_HIP(hipEventCreate(&ev), "hipEventCreate");
    double* dgrid = (double*)ctx->spec_grid.p;
    double* dfit = (double*)ctx->spec_coef.p;
    double* dcoef = coef_out ? dfit + Q * K : nullptr;
    FSNAP_HIP(hipMemcpyAsync(dgrid, grid.data(), grid.size() * 8, hipMemcpyHostToDevice, ctx->stream), "hipMemcpy(grid)");
    FSNAP_HIP(hipEventRecord(ctx->spec_ev[0], ctx->stream), "hipEventRecord");
    FSNAP_HIP(fsnap::launch_spectral_eig(nb1, dfolds, dtotal, (int)K, (int)F, (double*)ctx->spec_work.p, (double*)ctx->spec_eig.p,
                                         (double*)ctx->spec_z.p, (double*)ctx->spec_V.p, (double*)ctx->spec_info.p, ctx->stream),
              "launch fsnap_spectral_eig_k");
    FSNAP_HIP(hipEventRecord(ctx->spec_ev[1], ctx->stream), "hipEventRecord");
    FSNAP_HIP(fsnap::launch_spectral_eval(nb2, d_stats, dfolds, dtotal, (const double*)ctx->spec_eig.p, (const double*)ctx->spec_z.p,
                                          (const double*)ctx->spec_V.p, (const double*)ctx->spec_info.p, dgrid, dgrid + Q, (int)K,
                                          (int)F, (int)nsub, (int)Q, (double*)ctx->spec_set.p, dfit, dcoef,
                                          (double*)ctx->spec_held.p, ctx->stream),
              "launch fsnap_spectral_eval_k");
    FSNAP_HIP(hipEventRecord(ctx->spec_ev[2], ctx->stream), "hipEventRecord");
    if (coef_out)
        FSNAP_HIP(hipMemcpyAsync(coef_out, dcoef, (size_t)F * Q * K * 8, hipMemcpyDeviceToHost, ctx->stream), "hipMemcpy(coef)");
    rc = fold_finish(ctx,
                     {{eig_out, ctx->spec_eig.p, (size_t)nprob * K * 8},
                      {z_out, ctx->spec_z.p, (size_t)nprob * K * 8},
                      {info_out, ctx->spec_info.p, (size_t)nprob * 6 * 8},
                      {set_out, ctx->spec_set.p, (size_t)nprob * Q * 3 * 8},
                      {fit_out, dfit, (size_t)Q * K * 8},
                      {heldout_out, ctx->spec_held.p, (size_t)F * Q * nsub * 3 * 8}},
                     fit_out, Q * K);
    if (rc) return rc;
    for (int i = 0; i < 2; ++i) {
        float ms = 0.0f;
        FSNAP_HIP(hipEventElapsedTime(&ms, ctx->spec_ev[i], ctx->spec_ev[i + 1]), "hipEventElapsedTime");
        ctx->spec_ms[i] = ms;
    }
    ctx->spec_done = true;
    return FSNAP_OK;
}

int fsnap_spectral_path_times(fsnap_ctx* ctx, double* ms_out) {
    if (!ctx) return FSNAP_E_ARG;
    const char* who = "fsnap_spectral_path_times";
    if (!ms_out) return ctx->fail(FSNAP_E_ARG, "%s: NULL argument", who);
    if (!ctx->spec_done) return ctx->fail(FSNAP_E_STATE, "%s: no fsnap_spectral_path call to read from", who);
    for (int i = 0; i < 2; ++i) ms_out[i] = ctx->spec_ms[i];
    return FSNAP_OK;
}

// ---- grouped K-fold cross-validation of weight candidates (kernels V0, V1, V2 of fsnap_cv.hip) -----------------------------

int fsnap_cv_candidates(fsnap_ctx* ctx, int64_t layout, double alpha, const double* S, int P, int F, int C, int64_t K,
                        double* coef_out, double* info_out) {
    if (!ctx) return FSNAP_E_ARG;
    const char* who = "fsnap_cv_candidates";
    if (!S || !coef_out || !info_out) return ctx->fail(FSNAP_E_ARG, "%s: NULL argument", who);
    if (K < 1 || K > fsnap::CV_MAX_K) return ctx->fail(FSNAP_E_ARG, "%s: K = %lld (1 ... %d)", who, (long long)K, fsnap::CV_MAX_K);
    if (F < 2 || C < 1 || P < 1) return ctx->fail(FSNAP_E_ARG, "%s: P = %d, F = %d, C = %d", who, P, F, C);
    if (!std::isfinite(alpha) || alpha < 0.0) return ctx->fail(FSNAP_E_ARG, "%s: alpha = %g is negative or not finite", who, alpha);
    if (layout <= 0 || layout != ctx->cand_layout || ctx->cand_stats_K <= 0 || !ctx->cand_stats.p)
        return ctx->fail(FSNAP_E_STATE, "%s: no per-category statistics of layout %lld on the context (fsnap_cat_prepare + "
                                        "fsnap_cat_normal_eq first)", who, (long long)layout);
    if ((int64_t)F * C != ctx->cand_ncat || K != ctx->cand_stats_K)
        return ctx->fail(FSNAP_E_ARG, "%s: F * C = %lld, K = %lld but the statistics have %d categories of order %lld", who,
                         (long long)F * C, (long long)K, ctx->cand_ncat, (long long)ctx->cand_stats_K);
    const int64_t nprob = (int64_t)P * F;
    if (nprob > FSNAP_CV_MAX_PROBLEMS || (double)nprob * (double)K * 8.0 > (double)FSNAP_CAT_STATS_MAX_BYTES)
        return ctx->fail(FSNAP_E_ARG, "%s: P * F = %lld problems of %lld coefficients (at most %d problems, "
                                      "FSNAP_CAT_STATS_MAX_BYTES of coefficients)", who, (long long)nprob, (long long)K,
                         FSNAP_CV_MAX_PROBLEMS);
    for (int64_t i = 0; i < (int64_t)P * C; ++i)
        if (!std::isfinite(S[i]))
            return ctx->fail(FSNAP_E_ARG, "%s: S[%lld][%lld] is not finite", who, (long long)(i / C), (long long)(i % C));
    FSNAP_HIP(hipSetDevice(ctx->device), "hipSetDevice");
    const int64_t T = FSNAP_PACKED_LEN(K);
    if (!ctx->cv_total.ensure((size_t)(C + (int64_t)F * C) * T * 8) || !ctx->cv_S.ensure((size_t)P * C * 8) ||
        !ctx->cv_coef.ensure((size_t)nprob * K * 8) || !ctx->cv_info.ensure((size_t)nprob * 4 * 8))
        return ctx->fail(FSNAP_E_NOMEM, "hipMalloc(candidate cross-validation) failed");
    FSNAP_HIP(hipMemcpyAsync(ctx->cv_S.p, S, (size_t)P * C * 8, hipMemcpyHostToDevice, ctx->stream), "hipMemcpy(S)");
    double* total = (double*)ctx->cv_total.p;
    double* rest = total + (int64_t)C * T;                 // F C blocks: T[c] - B[f][c]
    FSNAP_HIP(fsnap::launch_cv_total((const double*)ctx->cand_stats.p, F, C, (int)K, total, rest, ctx->stream),
              "launch fsnap_cv_total_k");
    const int nblocks = (int)std::min<int64_t>(nprob, (int64_t)fsnap::cv_blocks_per_cu((int)K) * std::max(1, ctx->num_cu));
    FSNAP_HIP(fsnap::launch_cv_solve(nblocks, rest, total, (const double*)ctx->cv_S.p, P, F, C, (int)K, alpha, (double*)ctx->cv_coef.p,
                                     (double*)ctx->cv_info.p, ctx->stream),
              "launch fsnap_cv_solve_k");
    FSNAP_HIP(hipMemcpyAsync(coef_out, ctx->cv_coef.p, (size_t)nprob * K * 8, hipMemcpyDeviceToHost, ctx->stream), "hipMemcpy(coef)");
    FSNAP_HIP(hipMemcpyAsync(info_out, ctx->cv_info.p, (size_t)nprob * 4 * 8, hipMemcpyDeviceToHost, ctx->stream), "hipMemcpy(info)");
    FSNAP_HIP(hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");
    return FSNAP_OK;                                        // a failed problem is its own status 1, not the call's
}

int fsnap_cv_candidate_rows(fsnap_ctx* ctx, int64_t layout, const double* coef, int P, int F, int C, int64_t K_, double* out) {
    if (!ctx) return FSNAP_E_ARG;
    const char* who = "fsnap_cv_candidate_rows";
    int rc;
    if ((rc = check_rows(ctx)) || (rc = cand_check_layout(ctx, layout, who))) return rc;
    if (!coef || !out || P < 1 || F < 1 || C < 1) return ctx->fail(FSNAP_E_ARG, "%s: bad argument", who);
    if ((int64_t)F * C != ctx->cand_ncat || K_ != ctx->K)
        return ctx->fail(FSNAP_E_ARG, "%s: F * C = %lld, K = %lld but the layout has %d categories, the rows %lld columns", who,
                         (long long)F * C, (long long)K_, ctx->cand_ncat, (long long)ctx->K);
    const int K = (int)ctx->K, ncat = ctx->cand_ncat;
    const int64_t K8 = (K + 7) / 8 * 8;
    if ((int64_t)P * F > FSNAP_CV_MAX_PROBLEMS || (double)F * (double)K8 * 16.0 * 8.0 > (double)FSNAP_CAT_STATS_MAX_BYTES)
        return ctx->fail(FSNAP_E_ARG, "%s: P * F = %lld problems, F = %d coefficient tables of %lld x 16", who,
                         (long long)P * F, F, (long long)K8);
    FSNAP_HIP(hipSetDevice(ctx->device), "hipSetDevice");
    const int64_t nch = ctx->cand_nch_a, nout = (int64_t)ncat * 4;
    const int64_t per = fsnap::cand_rows_partial_doubles(FSNAP_CAND_ERROR_SUMS, K);
    if (!ctx->cv_betaT.ensure((size_t)F * K8 * 16 * 8) || !ctx->cand_rpart.ensure((size_t)(nch > 0 ? nch : 1) * per * 8) ||
        !ctx->cand_res.ensure((size_t)P * nout * 8))
        return ctx->fail(FSNAP_E_NOMEM, "hipMalloc(candidate cross-validation rows) failed");
    if (nch == 0) FSNAP_HIP(hipMemsetAsync(ctx->cand_res.p, 0, (size_t)P * nout * 8, ctx->stream), "hipMemsetAsync");
    std::vector<double> bt((size_t)F * K8 * 16);
    for (int p0 = 0; p0 < P && nch > 0; p0 += fsnap::CAND_ROWS_MAX_P) {
        const int np = std::min(fsnap::CAND_ROWS_MAX_P, P - p0);
        std::fill(bt.begin(), bt.end(), 0.0);
        for (int f = 0; f < F; ++f)
            for (int p = 0; p < np; ++p)
                for (int k = 0; k < K; ++k)
                    bt[((size_t)f * K8 + k) * 16 + p] = coef[((int64_t)(p0 + p) * F + f) * K + k];
        // the launch before may still read the tables: the copy is ordered after it on the stream
        FSNAP_HIP(hipMemcpyAsync(ctx->cv_betaT.p, bt.data(), bt.size() * 8, hipMemcpyHostToDevice, ctx->stream), "hipMemcpy(coef)");
        FSNAP_HIP(fsnap::launch_cv_rows(ctx->dA, ctx->lda, ctx->db, (const double*)ctx->cand_w0.p, (const int*)ctx->cand_idx_a.p,
                                        (const fsnap::CatChunk*)ctx->cand_ch_a.p, nch, K, C, (const double*)ctx->cv_betaT.p,
                                        (double*)ctx->cand_rpart.p, ctx->stream),
                  "launch fsnap_cv_rows_k");
        FSNAP_HIP(fsnap::launch_cand_reduce(FSNAP_CAND_ERROR_SUMS, (const double*)ctx->cand_rpart.p, (const int*)ctx->cand_cb_a.p,
                                            nullptr, ncat, np, p0, K, (double*)ctx->cand_res.p, ctx->stream),
                  "launch fsnap_cand_reduce_k");
        FSNAP_HIP(hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");   // bt is rewritten for the next group
    }
    FSNAP_HIP(hipMemcpyAsync(out, ctx->cand_res.p, (size_t)P * nout * 8, hipMemcpyDeviceToHost, ctx->stream), "hipMemcpy(out)");
    FSNAP_HIP(hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");
    return FSNAP_OK;
}

// ---- gradient of the cross-validated cost over the candidates' scales (kernels G1, G2 of fsnap_cvgrad.hip) -------------------

int fsnap_cv_candidates_grad(fsnap_ctx* ctx, int64_t layout, double alpha, const double* S, const double* omega, const double* coef,
                             int P, int F, int C, int64_t K, double* grad_S_out, double* grad_log_alpha_out, double* lambda_out,
                             double* info_out) {
    if (!ctx) return FSNAP_E_ARG;
    const char* who = "fsnap_cv_candidates_grad";
    if (!S || !omega || !coef || !grad_S_out || !grad_log_alpha_out || !info_out) return ctx->fail(FSNAP_E_ARG, "%s: NULL argument", who);
    if (K < 1 || K > fsnap::CV_MAX_K) return ctx->fail(FSNAP_E_ARG, "%s: K = %lld (1 ... %d)", who, (long long)K, fsnap::CV_MAX_K);
    if (F < 2 || C < 1 || P < 1) return ctx->fail(FSNAP_E_ARG, "%s: P = %d, F = %d, C = %d", who, P, F, C);
    if (!std::isfinite(alpha) || alpha < 0.0) return ctx->fail(FSNAP_E_ARG, "%s: alpha = %g is negative or not finite", who, alpha);
    if (layout <= 0 || layout != ctx->cand_layout || ctx->cand_stats_K <= 0 || !ctx->cand_stats.p)
        return ctx->fail(FSNAP_E_STATE, "%s: no per-category statistics of layout %lld on the context (fsnap_cat_prepare + "
                                        "fsnap_cat_normal_eq first)", who, (long long)layout);
    if ((int64_t)F * C != ctx->cand_ncat || K != ctx->cand_stats_K)
        return ctx->fail(FSNAP_E_ARG, "%s: F * C = %lld, K = %lld but the statistics have %d categories of order %lld", who,
                         (long long)F * C, (long long)K, ctx->cand_ncat, (long long)ctx->cand_stats_K);
    const int64_t nprob = (int64_t)P * F, K8 = (K + 7) / 8 * 8, tiles = ((int64_t)P + 15) / 16;
    const int64_t ntab = tiles * F * K8 * 16, nD = tiles * F * C * 16;
    if (nprob > FSNAP_CV_MAX_PROBLEMS || (double)ntab * 8.0 > (double)FSNAP_CAT_STATS_MAX_BYTES ||
        (double)nD * 8.0 > (double)FSNAP_CAT_STATS_MAX_BYTES || F > 65535 || tiles * F * C >= ((int64_t)1 << 24))
        return ctx->fail(FSNAP_E_ARG, "%s: P * F = %lld problems of %lld coefficients and %d categories (at most %d problems, "
                                      "FSNAP_CAT_STATS_MAX_BYTES of coefficient tables and of per-category terms)", who,
                         (long long)nprob, (long long)K, C, FSNAP_CV_MAX_PROBLEMS);
    for (int64_t i = 0; i < (int64_t)P * C; ++i)
        if (!std::isfinite(S[i]) || !std::isfinite(omega[i]))
            return ctx->fail(FSNAP_E_ARG, "%s: S or omega [%lld][%lld] is not finite", who, (long long)(i / C), (long long)(i % C));
    FSNAP_HIP(hipSetDevice(ctx->device), "hipSetDevice");
    const int64_t T = FSNAP_PACKED_LEN(K);
    ctx->cvg_g_len = 0;
    if (!ctx->cv_total.ensure((size_t)(C + (int64_t)F * C) * T * 8) || !ctx->cv_S.ensure((size_t)P * C * 8) ||
        !ctx->cvg_betaT.ensure((size_t)ntab * 8) || !ctx->cvg_lamT.ensure((size_t)ntab * 8) ||
        !ctx->cvg_omegaT.ensure((size_t)tiles * C * 16 * 8) || !ctx->cvg_g.ensure((size_t)nprob * K * 8) ||
        !ctx->cvg_lam.ensure((size_t)nprob * K * 8) || !ctx->cvg_D.ensure((size_t)nD * 8) || !ctx->cvg_info.ensure((size_t)nprob * 2 * 8))
        return ctx->fail(FSNAP_E_NOMEM, "hipMalloc(candidate cross-validation gradient) failed");
    // the zero-padded tables of every 16-candidate tile: candidate 16 tile + e in slot e
    std::vector<double> bt((size_t)ntab, 0.0), ot((size_t)tiles * C * 16, 0.0);
    for (int p = 0; p < P; ++p) {
        const int64_t tile = p >> 4, e = p & 15;
        for (int f = 0; f < F; ++f)
            for (int64_t k = 0; k < K; ++k) bt[(size_t)(((tile * F + f) * K8 + k) * 16 + e)] = coef[((int64_t)p * F + f) * K + k];
        for (int c = 0; c < C; ++c) ot[(size_t)((tile * C + c) * 16 + e)] = omega[(int64_t)p * C + c];
    }
    FSNAP_HIP(hipMemcpyAsync(ctx->cv_S.p, S, (size_t)P * C * 8, hipMemcpyHostToDevice, ctx->stream), "hipMemcpy(S)");
    FSNAP_HIP(hipMemcpyAsync(ctx->cvg_betaT.p, bt.data(), bt.size() * 8, hipMemcpyHostToDevice, ctx->stream), "hipMemcpy(coef)");
    FSNAP_HIP(hipMemcpyAsync(ctx->cvg_omegaT.p, ot.data(), ot.size() * 8, hipMemcpyHostToDevice, ctx->stream), "hipMemcpy(omega)");
    FSNAP_HIP(hipMemsetAsync(ctx->cvg_lamT.p, 0, (size_t)ntab * 8, ctx->stream), "hipMemsetAsync");
    const double* stats = (const double*)ctx->cand_stats.p;
    double* total = (double*)ctx->cv_total.p;
    double* rest = total + (int64_t)C * T;
    for (auto& ev : ctx->cvg_ev)
        if (!ev) FSNAP_HIP(hipEventCreate(&ev), "hipEventCreate");
    FSNAP_HIP(hipEventRecord(ctx->cvg_ev[0], ctx->stream), "hipEventRecord");
    // kernel V0 again: the blocks of a tag may have been formed anew since the last fsnap_cv_candidates, and one elementwise
    // pass is small next to the two sweeps below
    FSNAP_HIP(fsnap::launch_cv_total(stats, F, C, (int)K, total, rest, ctx->stream), "launch fsnap_cv_total_k");
    FSNAP_HIP(fsnap::launch_cvgrad_rhs(stats, (const double*)ctx->cvg_betaT.p, (const double*)ctx->cvg_omegaT.p, P, F, C, (int)K,
                                       (double*)ctx->cvg_g.p, ctx->stream),
              "launch fsnap_cvgrad_rhs_k");
    FSNAP_HIP(hipEventRecord(ctx->cvg_ev[1], ctx->stream), "hipEventRecord");
    const int nblocks = (int)std::min<int64_t>(nprob, (int64_t)fsnap::cv_blocks_per_cu((int)K) * std::max(1, ctx->num_cu));
    FSNAP_HIP(fsnap::launch_cvgrad_solve(nblocks, rest, total, (const double*)ctx->cv_S.p, (const double*)ctx->cvg_g.p, P, F, C, (int)K,
                                         alpha, (double*)ctx->cvg_lam.p, (double*)ctx->cvg_lamT.p, (double*)ctx->cvg_info.p,
                                         ctx->stream),
              "launch fsnap_cvgrad_solve_k");
    FSNAP_HIP(hipEventRecord(ctx->cvg_ev[2], ctx->stream), "hipEventRecord");
    FSNAP_HIP(fsnap::launch_cvgrad_bilinear(rest, (const double*)ctx->cvg_betaT.p, (const double*)ctx->cvg_lamT.p, P, F, C, (int)K,
                                            (double*)ctx->cvg_D.p, ctx->stream),
              "launch fsnap_cvgrad_bilinear_k");
    FSNAP_HIP(hipEventRecord(ctx->cvg_ev[3], ctx->stream), "hipEventRecord");
    std::vector<double> lam((size_t)nprob * K), D((size_t)nD);
    FSNAP_HIP(hipMemcpyAsync(lam.data(), ctx->cvg_lam.p, lam.size() * 8, hipMemcpyDeviceToHost, ctx->stream), "hipMemcpy(lambda)");
    FSNAP_HIP(hipMemcpyAsync(D.data(), ctx->cvg_D.p, D.size() * 8, hipMemcpyDeviceToHost, ctx->stream), "hipMemcpy(D)");
    FSNAP_HIP(hipMemcpyAsync(info_out, ctx->cvg_info.p, (size_t)nprob * 2 * 8, hipMemcpyDeviceToHost, ctx->stream), "hipMemcpy(info)");
    FSNAP_HIP(hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");
    for (int i = 0; i < 3; ++i) {
        float ms = 0.0f;
        FSNAP_HIP(hipEventElapsedTime(&ms, ctx->cvg_ev[i], ctx->cvg_ev[i + 1]), "hipEventElapsedTime");
        ctx->cvg_ms[i] = ms;
    }
    // the sums over the folds, f in index order; lambda . beta with k ascending, one fma per term
    for (int p = 0; p < P; ++p) {
        const int64_t tile = p >> 4, e = p & 15;
        for (int c = 0; c < C; ++c) {
            double s = 0.0;
            for (int f = 0; f < F; ++f) s += D[(size_t)(((tile * F + f) * C + c) * 16 + e)];
            grad_S_out[(int64_t)p * C + c] = 2.0 * S[(int64_t)p * C + c] * s;
        }
        double la = 0.0;
        for (int f = 0; f < F; ++f) {
            const double* l = lam.data() + ((int64_t)p * F + f) * K;
            const double* b = coef + ((int64_t)p * F + f) * K;
            double d = 0.0;
            for (int64_t k = 0; k < K; ++k) d = std::fma(l[k], b[k], d);
            la += d;
        }
        grad_log_alpha_out[p] = -alpha * la;
    }
    if (lambda_out) std::copy(lam.begin(), lam.end(), lambda_out);
    ctx->cvg_g_len = nprob * K;
    return FSNAP_OK;                                        // a failed problem is its own status 1 and a NaN gradient row
}

int fsnap_cv_candidates_grad_times(fsnap_ctx* ctx, double* ms_out) {
    if (!ctx) return FSNAP_E_ARG;
    const char* who = "fsnap_cv_candidates_grad_times";
    if (!ms_out) return ctx->fail(FSNAP_E_ARG, "%s: NULL argument", who);
    if (ctx->cvg_g_len <= 0) return ctx->fail(FSNAP_E_STATE, "%s: no fsnap_cv_candidates_grad call to read from", who);
    for (int i = 0; i < 3; ++i) ms_out[i] = ctx->cvg_ms[i];
    return FSNAP_OK;
}

int fsnap_cv_candidates_grad_rhs(fsnap_ctx* ctx, int64_t n, double* g_out) {
    if (!ctx) return FSNAP_E_ARG;
    const char* who = "fsnap_cv_candidates_grad_rhs";
    if (!g_out) return ctx->fail(FSNAP_E_ARG, "%s: NULL argument", who);
    if (ctx->cvg_g_len <= 0 || !ctx->cvg_g.p) return ctx->fail(FSNAP_E_STATE, "%s: no fsnap_cv_candidates_grad call to read from", who);
    if (n != ctx->cvg_g_len)
        return ctx->fail(FSNAP_E_ARG, "%s: n = %lld but the last call left P * F * K = %lld doubles", who, (long long)n,
                         (long long)ctx->cvg_g_len);
    FSNAP_HIP(hipSetDevice(ctx->device), "hipSetDevice");
    FSNAP_HIP(hipMemcpyAsync(g_out, ctx->cvg_g.p, (size_t)n * 8, hipMemcpyDeviceToHost, ctx->stream), "hipMemcpy(g)");
    FSNAP_HIP(hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");
    return FSNAP_OK;
}

// ---- marginal likelihood of the candidates from the per-category statistics (kernels E1, E2, E3 of fsnap_evidence.hip) --------

int fsnap_candidates_evidence(fsnap_ctx* ctx, int64_t layout, double alpha, const double* S, int P, int ncat, int64_t K,
                              const uint8_t* active, double* beta_out, double* info_out, double* terms_out) {
    if (!ctx) return FSNAP_E_ARG;
    const char* who = "fsnap_candidates_evidence";
    if (!S || P <= 0 || !active || !beta_out || !info_out || !terms_out) return ctx->fail(FSNAP_E_ARG, "%s: bad argument", who);
    if (layout <= 0 || layout != ctx->cand_layout || ctx->cand_stats_K <= 0 || !ctx->cand_stats.p)
        return ctx->fail(FSNAP_E_STATE, "%s: no per-category statistics of layout %lld on the context (fsnap_cat_prepare + "
                                        "fsnap_cat_normal_eq first)", who, (long long)layout);
    if (ncat != ctx->cand_ncat || K != ctx->cand_stats_K)
        return ctx->fail(FSNAP_E_ARG, "%s: ncat = %d, K = %lld but the statistics have %d, %lld", who, ncat, (long long)K,
                         ctx->cand_ncat, (long long)ctx->cand_stats_K);
    if (K < 1 || K > fsnap::CV_MAX_K) return ctx->fail(FSNAP_E_ARG, "%s: K = %lld (1 ... %d)", who, (long long)K, fsnap::CV_MAX_K);
    if (!std::isfinite(alpha) || alpha < 0.0) return ctx->fail(FSNAP_E_ARG, "%s: alpha = %g is negative or not finite", who, alpha);
    const int C = ncat;
    const int64_t T = FSNAP_PACKED_LEN(K), PT = ((int64_t)P + 7) / 8, CT = ((int64_t)C + 15) / 16;
    const int64_t ns = fsnap::evidence_slices((int)K), npart = CT * PT * ns * 256, ntab = PT * T * 16;
    if (!cand_fits(P, K) || (double)ntab * 8.0 > (double)FSNAP_CAT_STATS_MAX_BYTES ||
        (double)npart * 8.0 > (double)FSNAP_CAT_STATS_MAX_BYTES || PT > 65535)
        return ctx->fail(FSNAP_E_ARG, "%s: %d candidates x %lld doubles (the tables or the slice partials) exceed "
                                      "FSNAP_CAT_STATS_MAX_BYTES", who, P, (long long)T);
    for (int64_t i = 0; i < (int64_t)P * C; ++i)
        if (!std::isfinite(S[i]))
            return ctx->fail(FSNAP_E_ARG, "%s: S[%lld][%lld] is not finite", who, (long long)(i / C), (long long)(i % C));
    FSNAP_HIP(hipSetDevice(ctx->device), "hipSetDevice");
    ctx->evd_done = false;
    if (!ctx->evd_S.ensure((size_t)P * C * 8) || !ctx->evd_beta.ensure((size_t)P * K * 8) || !ctx->evd_info.ensure((size_t)P * 6 * 8) ||
        !ctx->evd_tab.ensure((size_t)ntab * 8) || !ctx->evd_part.ensure((size_t)npart * 8) ||
        !ctx->evd_Y.ensure((size_t)PT * C * 16 * 8))
        return ctx->fail(FSNAP_E_NOMEM, "hipMalloc(candidate evidence) failed");
    std::vector<double> Sm((size_t)P * C);
    for (size_t i = 0; i < Sm.size(); ++i) Sm[i] = active[i] ? S[i] : 0.0;
    FSNAP_HIP(hipMemcpyAsync(ctx->evd_S.p, Sm.data(), Sm.size() * 8, hipMemcpyHostToDevice, ctx->stream), "hipMemcpy(S)");
    if (P % 8)                                             // the columns of the last tile that no candidate writes
        FSNAP_HIP(hipMemsetAsync((double*)ctx->evd_tab.p + (PT - 1) * T * 16, 0, (size_t)T * 16 * 8, ctx->stream), "hipMemsetAsync");
    for (auto& ev : ctx->evd_ev)
        if (!ev) FSNAP_HIP(hipEventCreate(&ev), "hipEventCreate");
    const double* stats = (const double*)ctx->cand_stats.p;
    const int nblocks = (int)std::min<int64_t>(P, (int64_t)fsnap::cv_blocks_per_cu((int)K) * std::max(1, ctx->num_cu));
    FSNAP_HIP(hipEventRecord(ctx->evd_ev[0], ctx->stream), "hipEventRecord");
    FSNAP_HIP(fsnap::launch_evidence_factor(nblocks, stats, (const double*)ctx->evd_S.p, P, C, (int)K, alpha, (double*)ctx->evd_beta.p,
                                            (double*)ctx->evd_info.p, (double*)ctx->evd_tab.p, ctx->stream),
              "launch fsnap_evidence_factor_k");
    FSNAP_HIP(hipEventRecord(ctx->evd_ev[1], ctx->stream), "hipEventRecord");
    FSNAP_HIP(fsnap::launch_evidence_sweep(stats, (const double*)ctx->evd_tab.p, P, C, (int)K, (double*)ctx->evd_part.p,
                                           (double*)ctx->evd_Y.p, ctx->stream),
              "launch fsnap_evidence_sweep_k");
    FSNAP_HIP(hipEventRecord(ctx->evd_ev[2], ctx->stream), "hipEventRecord");
    std::vector<double> Y((size_t)PT * C * 16);
    FSNAP_HIP(hipMemcpyAsync(beta_out, ctx->evd_beta.p, (size_t)P * K * 8, hipMemcpyDeviceToHost, ctx->stream), "hipMemcpy(beta)");
    FSNAP_HIP(hipMemcpyAsync(info_out, ctx->evd_info.p, (size_t)P * 6 * 8, hipMemcpyDeviceToHost, ctx->stream), "hipMemcpy(info)");
    FSNAP_HIP(hipMemcpyAsync(Y.data(), ctx->evd_Y.p, Y.size() * 8, hipMemcpyDeviceToHost, ctx->stream), "hipMemcpy(Y)");
    FSNAP_HIP(hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");
    for (int i = 0; i < 2; ++i) {
        float ms = 0.0f;
        FSNAP_HIP(hipEventElapsedTime(&ms, ctx->evd_ev[i], ctx->evd_ev[i + 1]), "hipEventElapsedTime");
        ctx->evd_ms[i] = ms;
    }
    for (int p = 0; p < P; ++p)
        for (int c = 0; c < C; ++c) {
            const double* y = Y.data() + (((size_t)(p >> 3) * C + c) * 16 + 2 * (p & 7));
            terms_out[((int64_t)p * C + c) * 2] = y[0];
            terms_out[((int64_t)p * C + c) * 2 + 1] = y[1];
        }
    ctx->evd_done = true;
    return FSNAP_OK;                                        // a failed candidate is its own status 1, not the call's
}

int fsnap_candidates_evidence_times(fsnap_ctx* ctx, double* ms_out) {
    if (!ctx) return FSNAP_E_ARG;
    const char* who = "fsnap_candidates_evidence_times";
    if (!ms_out) return ctx->fail(FSNAP_E_ARG, "%s: NULL argument", who);
    if (!ctx->evd_done) return ctx->fail(FSNAP_E_STATE, "%s: no fsnap_candidates_evidence call to read from", who);
    for (int i = 0; i < 2; ++i) ms_out[i] = ctx->evd_ms[i];
    return FSNAP_OK;
}

// ---- joint information-gain / variance-reduction scores of units (kernels J1, J2 of fsnap_joint.hip) ------------------

namespace {

int joint_session(fsnap_ctx* ctx, const char* who) {
    if (!ctx->joint_active)
        return ctx->fail(FSNAP_E_ARG, "%s: no joint-score session (fsnap_joint_begin; new rows or a new category layout end one)", who);
    return FSNAP_OK;
}

}  // namespace

int fsnap_joint_begin(fsnap_ctx* ctx, const int32_t* sorted_rows, const int64_t* unit_offsets, int64_t nunits, const double* omega) {
    if (!ctx) return FSNAP_E_ARG;
    const char* who = "fsnap_joint_begin";
    ctx->joint_active = false;
    if (!unit_offsets) return ctx->fail(FSNAP_E_ARG, "%s: NULL argument", who);
    if (nunits < 0 || nunits > 0x3FFFFFFF) return ctx->fail(FSNAP_E_ARG, "%s: nunits = %lld", who, (long long)nunits);
    const int64_t m = ctx->m;
    if (m > 0x7FFFFFFF) return ctx->fail(FSNAP_E_ARG, "%s: needs m < 2^31", who);
    if (const int rc = check_unit_index(ctx, who, "unit_offsets", sorted_rows, unit_offsets, nunits, m, [](int64_t, int32_t) { return 0; }))
        return rc;
    const int64_t npos = unit_offsets[nunits];
    std::vector<double> hom((size_t)std::max<int64_t>(npos, 1), 1.0);
    for (int64_t p = 0; omega && p < npos; ++p) hom[(size_t)p] = omega[sorted_rows[p]];
    if (npos > 0) {
        int rc = check_rows(ctx);
        if (rc) return rc;
    }
    FSNAP_HIP(hipSetDevice(ctx->device), "hipSetDevice");
    if (!ctx->joint_idx.ensure((size_t)std::max<int64_t>(npos, 1) * 4) || !ctx->joint_off.ensure((size_t)(nunits + 1) * 8) ||
        !ctx->joint_om.ensure((size_t)std::max<int64_t>(npos, 1) * 8))
        return ctx->fail(FSNAP_E_NOMEM, "hipMalloc(joint) failed");
    if (npos > 0) {
        FSNAP_HIP(hipMemcpyAsync(ctx->joint_idx.p, sorted_rows, (size_t)npos * 4, hipMemcpyHostToDevice, ctx->stream), "hipMemcpy(idx)");
        FSNAP_HIP(hipMemcpyAsync(ctx->joint_om.p, hom.data(), (size_t)npos * 8, hipMemcpyHostToDevice, ctx->stream), "hipMemcpy(omega)");
    }
    FSNAP_HIP(hipMemcpyAsync(ctx->joint_off.p, unit_offsets, (size_t)(nunits + 1) * 8, hipMemcpyHostToDevice, ctx->stream),
              "hipMemcpy(offsets)");
    FSNAP_HIP(hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");
    ctx->joint_hoff.assign(unit_offsets, unit_offsets + nunits + 1);
    ctx->joint_halive.assign((size_t)nunits, 0);
    for (int64_t u = 0; u < nunits; ++u) ctx->joint_halive[(size_t)u] = unit_offsets[u + 1] > unit_offsets[u];   // an empty unit is never scored
    ctx->joint_m = m;
    ctx->joint_npos = npos;
    ctx->joint_nunits = nunits;
    ctx->joint_active = true;
    return FSNAP_OK;
}

int fsnap_joint_score(fsnap_ctx* ctx, int64_t K, int64_t J, const double* M, int64_t r, const double* B, double tau,
                      double* gain, double* reduction, double* info) {
    if (!ctx) return FSNAP_E_ARG;
    const char* who = "fsnap_joint_score";
    int rc = joint_session(ctx, who);
    if (rc) return rc;
    if (!M) return ctx->fail(FSNAP_E_ARG, "%s: M is NULL", who);
    if (K < 1 || K > 0x3FFFFFFF || J < 1 || J > 0x3FFFFFFF) return ctx->fail(FSNAP_E_ARG, "%s: K = %lld, J = %lld", who, (long long)K, (long long)J);
    if (r < 0 || r > 0x3FFFFFFF || (r > 0 && !B)) return ctx->fail(FSNAP_E_ARG, "%s: r = %lld without B", who, (long long)r);
    if (!B) r = 0;
    if (reduction && r == 0) return ctx->fail(FSNAP_E_ARG, "%s: the reduction needs a target (B, r >= 1)", who);
    if (!reduction) r = 0;
    if (!(tau > 0.0) || tau == std::numeric_limits<double>::infinity()) return ctx->fail(FSNAP_E_ARG, "%s: tau = %g", who, tau);
    const int64_t nunits = ctx->joint_nunits, npos = ctx->joint_npos;
    if (npos > 0 && (ctx->joint_m != ctx->m || K != ctx->K))
        return ctx->fail(FSNAP_E_ARG, "%s: K = %lld, the resident rows have %lld columns", who, (long long)K, (long long)ctx->K);
    const double nan = std::numeric_limits<double>::quiet_NaN();
    for (int64_t u = 0; u < nunits; ++u) {
        if (gain) gain[u] = nan;
        if (reduction) reduction[u] = nan;
    }
    // live units by dim S = min(n_u, J); general path: S (dmax^2 + dmax) and the Y fragments per workgroup
    const UnitBins bins = bin_units(
        nunits,
        [&](int64_t u) { return ctx->joint_halive[(size_t)u] ? ctx->joint_hoff[(size_t)u + 1] - ctx->joint_hoff[(size_t)u] : 0; }, J,
        fsnap::JOINT_MAX_LDS_D, ctx->num_cu,
        [](int64_t dmax) { return fsnap::loco_scratch_doubles(dmax) + fsnap::joint_yslice(dmax); }, ctx->joint_hlist);
    const int64_t dmax = bins.dmax;
    const int* nblk = bins.nblk;
    if (ctx->joint_hlist.empty() || npos == 0) return FSNAP_OK;
    if ((rc = check_rows(ctx))) return rc;
    FSNAP_HIP(hipSetDevice(ctx->device), "hipSetDevice");
    // [M | M B], zero-padded to 16-multiples; M B on the host in index order (K J r flops)
    const int64_t Kp = (K + 15) / 16 * 16, Jp = (J + 15) / 16 * 16, rp = (r + 15) / 16 * 16, Wp = Jp + rp;
    ctx->joint_hF.assign((size_t)(Kp * Wp), 0.0);
    for (int64_t k = 0; k < K; ++k) {
        double* row = &ctx->joint_hF[(size_t)(k * Wp)];
        std::memcpy(row, M + k * J, (size_t)J * 8);
        for (int64_t j = 0; j < J; ++j) {
            const double mkj = M[k * J + j];
            const double* bj = B + j * r;
            for (int64_t c = 0; c < r; ++c) row[Jp + c] += mkj * bj[c];
        }
    }
    ctx->joint_hB.assign((size_t)std::max<int64_t>(Jp * rp, 1), 0.0);
    for (int64_t j = 0; j < J && r > 0; ++j) std::memcpy(&ctx->joint_hB[(size_t)(j * rp)], B + j * r, (size_t)r * 8);
    const int64_t sslice = fsnap::loco_scratch_doubles(dmax), yslice = fsnap::joint_yslice(dmax);
    if (!ctx->joint_F.ensure((size_t)(Kp * Wp) * 8) || !ctx->joint_B.ensure(ctx->joint_hB.size() * 8) ||
        !ctx->joint_ZP.ensure((size_t)npos * (size_t)Wp * 8) || !ctx->joint_list.ensure(ctx->joint_hlist.size() * 4) ||
        !ctx->joint_out.ensure((size_t)nunits * 2 * 8) || !ctx->joint_info.ensure((size_t)nunits * 4 * 8) ||
        (nblk[3] > 0 && (!ctx->joint_S.ensure((size_t)nblk[3] * (size_t)sslice * 8) || !ctx->joint_Y.ensure((size_t)nblk[3] * (size_t)yslice * 8))))
        return ctx->fail(FSNAP_E_NOMEM, "hipMalloc(joint) failed");
    FSNAP_HIP(hipMemcpyAsync(ctx->joint_F.p, ctx->joint_hF.data(), (size_t)(Kp * Wp) * 8, hipMemcpyHostToDevice, ctx->stream), "hipMemcpy(F)");
    FSNAP_HIP(hipMemcpyAsync(ctx->joint_B.p, ctx->joint_hB.data(), ctx->joint_hB.size() * 8, hipMemcpyHostToDevice, ctx->stream), "hipMemcpy(B)");
    FSNAP_HIP(hipMemcpyAsync(ctx->joint_list.p, ctx->joint_hlist.data(), ctx->joint_hlist.size() * 4, hipMemcpyHostToDevice, ctx->stream),
              "hipMemcpy(lists)");
    FSNAP_HIP(hipMemsetAsync(ctx->joint_out.p, 0xFF, (size_t)nunits * 16, ctx->stream), "hipMemset(out)");      // all-ones: NaN
    FSNAP_HIP(hipMemsetAsync(ctx->joint_info.p, 0xFF, (size_t)nunits * 32, ctx->stream), "hipMemset(info)");
    FSNAP_HIP(fsnap::launch_joint_rows(ctx->dA, ctx->lda, (int)K, (const int*)ctx->joint_idx.p, npos, (const double*)ctx->joint_om.p,
                                       (const double*)ctx->joint_F.p, (int)Wp, (double*)ctx->joint_ZP.p, ctx->stream),
              "launch fsnap_joint_rows_k");
    const auto launch = [&](int D, int nwg, size_t first, int ncl) {
        return fsnap::launch_joint_units(D, nwg, (const double*)ctx->joint_ZP.p, (int)Wp, (int)Jp, (int)J, (int)rp,
                                         (const double*)ctx->joint_B.p, tau, (const int64_t*)ctx->joint_off.p,
                                         (const int*)ctx->joint_list.p + first, ncl, (double*)ctx->joint_S.p, (int)dmax,
                                         (double*)ctx->joint_Y.p, (double*)ctx->joint_out.p, (double*)ctx->joint_info.p, ctx->stream);
    };
    FSNAP_HIP(launch_bins(bins, launch), "launch fsnap_joint_unit_k");
    ctx->joint_hout.resize((size_t)nunits * 2);
    ctx->joint_hinfo.resize((size_t)nunits * 4);
    FSNAP_HIP(hipMemcpyAsync(ctx->joint_hout.data(), ctx->joint_out.p, (size_t)nunits * 16, hipMemcpyDeviceToHost, ctx->stream), "hipMemcpy(out)");
    FSNAP_HIP(hipMemcpyAsync(ctx->joint_hinfo.data(), ctx->joint_info.p, (size_t)nunits * 32, hipMemcpyDeviceToHost, ctx->stream), "hipMemcpy(info)");
    FSNAP_HIP(hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");
    for (int64_t u = 0; u < nunits; ++u) {
        if (!ctx->joint_halive[(size_t)u]) continue;
        if (gain) gain[u] = ctx->joint_hout[(size_t)(2 * u)];
        if (reduction) reduction[u] = ctx->joint_hout[(size_t)(2 * u + 1)];
        if (info) std::memcpy(info + 4 * u, &ctx->joint_hinfo[(size_t)(4 * u)], 32);
    }
    return FSNAP_OK;
}

int fsnap_joint_retire(fsnap_ctx* ctx, int64_t unit) {
    if (!ctx) return FSNAP_E_ARG;
    int rc = joint_session(ctx, "fsnap_joint_retire");
    if (rc) return rc;
    if (unit < 0 || unit >= ctx->joint_nunits || !ctx->joint_halive[(size_t)unit])
        return ctx->fail(FSNAP_E_ARG, "fsnap_joint_retire: unit %lld is not alive", (long long)unit);
    ctx->joint_halive[(size_t)unit] = 0;
    return FSNAP_OK;
}

int fsnap_joint_end(fsnap_ctx* ctx) {
    if (!ctx) return FSNAP_E_ARG;
    ctx->joint_active = false;
    return FSNAP_OK;
}

// ---- robust M-estimator fits by IRLS: the step between two fits (kernels R0 - R3 of fsnap_robust.hip) --------------------

namespace {

int robust_session(fsnap_ctx* ctx, const char* who) {
    if (!ctx->rob_active)
        return ctx->fail(FSNAP_E_STATE, "%s: no robust session (fsnap_robust_begin; new rows or new weights end one)", who);
    return FSNAP_OK;
}

// r, w r and the per-class sums from the session's residuals (rows == false) or from the rows themselves (one launch)
int robust_weights(fsnap_ctx* ctx, const char* who, bool rows, int loss, double c, const double* scale, double* sums) {
    if (loss != FSNAP_ROBUST_HUBER && loss != FSNAP_ROBUST_BISQUARE && loss != FSNAP_ROBUST_CAUCHY)
        return ctx->fail(FSNAP_E_ARG, "%s: unknown loss %d", who, loss);
    if (!(c > 0.0) || !std::isfinite(c)) return ctx->fail(FSNAP_E_ARG, "%s: the tuning constant must be positive", who);
    if (!scale && !ctx->rob_have_scale) return ctx->fail(FSNAP_E_STATE, "%s: no scales yet (fsnap_robust_scale, or pass them)", who);
    if (!rows && !ctx->rob_have_e && ctx->rob_m > 0) return ctx->fail(FSNAP_E_STATE, "%s: no residuals yet (fsnap_robust_residuals)", who);
    const int ncat = ctx->rob_ncat;
    const int64_t m = ctx->rob_m;
    if (sums) std::memset(sums, 0, (size_t)ncat * 6 * 8);
    double* dscale = fsnap::robust_scale_ptr(ctx->rob_state.p, ncat);
    if (scale) {
        for (int g = 0; g < ncat; ++g)
            if (!(scale[g] >= 0.0)) return ctx->fail(FSNAP_E_ARG, "%s: scale[%d] is negative or NaN", who, g);
        FSNAP_HIP(hipMemcpyAsync(dscale, scale, (size_t)ncat * 8, hipMemcpyHostToDevice, ctx->stream), "hipMemcpy(scale)");
        ctx->rob_have_scale = true;
    }
    if (m > 0) {
        const int nb = fsnap::robust_num_blocks(m, (int)ctx->K);
        if (!ctx->rob_part.ensure((size_t)nb * ncat * 6 * 8) || !ctx->rob_sums.ensure((size_t)ncat * 6 * 8))
            return ctx->fail(FSNAP_E_NOMEM, "hipMalloc(robust partials) failed");
        FSNAP_HIP(hipEventRecord(ctx->ev[7], ctx->stream), "hipEventRecord");       // (the row pass's slot of fsnap_timing)
        FSNAP_HIP(fsnap::launch_robust_rows(ctx->dA, ctx->lda, (const double*)ctx->beta.p, m, (int)ctx->K, ctx->db, ctx->rob_dw,
                                            (const int*)ctx->rob_pcat.p, rows ? nullptr : (const double*)ctx->rob_e.p,
                                            (double*)ctx->rob_e.p, true, loss, c, dscale, (double*)ctx->rob_r.p,
                                            (double*)ctx->rob_wr.p, (double*)ctx->rob_part.p, (double*)ctx->rob_sums.p, ncat,
                                            ctx->stream),
                  "launch fsnap_robust_rows_k");
        FSNAP_HIP(hipEventRecord(ctx->ev[8], ctx->stream), "hipEventRecord");
        ctx->t_predict = true;
        if (rows) ctx->rob_have_e = true;
        if (sums) FSNAP_HIP(hipMemcpyAsync(sums, ctx->rob_sums.p, (size_t)ncat * 6 * 8, hipMemcpyDeviceToHost, ctx->stream), "hipMemcpy(sums)");
        // from here on the context's fits read w r
        ctx->dw = (const double*)ctx->rob_wr.p;
        ctx->wpack_valid = false;
        ctx->rob_pointed = true;
        ctx->rob_have_r = true;
    }
    FSNAP_HIP(hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");
    return FSNAP_OK;
}

int robust_check_beta(fsnap_ctx* ctx, const char* who, const double* beta, int64_t K) {
    if (!beta) return ctx->fail(FSNAP_E_ARG, "%s: beta is NULL", who);
    if (ctx->rob_m > 0 && K != ctx->K)
        return ctx->fail(FSNAP_E_ARG, "%s: K = %lld, the resident rows have %lld columns", who, (long long)K, (long long)ctx->K);
    if (K < 1) return ctx->fail(FSNAP_E_ARG, "%s: K = %lld", who, (long long)K);
    if (ctx->rob_m > 0) {
        if (!ctx->beta.ensure((size_t)K * 8)) return ctx->fail(FSNAP_E_NOMEM, "hipMalloc(beta) failed");
        FSNAP_HIP(hipMemcpyAsync(ctx->beta.p, beta, (size_t)K * 8, hipMemcpyHostToDevice, ctx->stream), "hipMemcpy(beta)");
    }
    return FSNAP_OK;
}

}  // namespace

int fsnap_robust_end(fsnap_ctx* ctx) {
    if (!ctx) return FSNAP_E_ARG;
    if (ctx->rob_active) {
        ctx->dw = ctx->rob_dw;
        ctx->dmask = ctx->rob_dmask;
        // the packed pairs in wpack are those of the base weights only if no fit of the session has rewritten them
        ctx->wpack_valid = ctx->rob_pointed ? false : ctx->rob_wpack_valid;
    }
    ctx->rob_active = false;
    ctx->rob_pointed = false;
    return FSNAP_OK;
}

int fsnap_robust_begin(fsnap_ctx* ctx, const int32_t* cat, int ncat) {
    if (!ctx) return FSNAP_E_ARG;
    const char* who = "fsnap_robust_begin";
    (void)fsnap_robust_end(ctx);
    if (ncat < 1 || ncat > FSNAP_ROBUST_MAX_CLASSES)
        return ctx->fail(FSNAP_E_ARG, "%s: ncat = %d, the kernels hold 1 ... %d classes", who, ncat, FSNAP_ROBUST_MAX_CLASSES);
    const bool have_rows = ctx->dA && ctx->db && ctx->m > 0;
    if (!have_rows && !ctx->comm) return check_rows(ctx);
    const int64_t m = have_rows ? ctx->m : 0;
    int rc;
    if (m > 0 && (rc = check_weights(ctx))) return rc;
    for (int64_t i = 0; cat && i < m; ++i)
        if (cat[i] < 0 || cat[i] >= ncat) return ctx->fail(FSNAP_E_ARG, "%s: class %d of row %lld is outside [0, %d)", who, cat[i], (long long)i, ncat);
    FSNAP_HIP(hipSetDevice(ctx->device), "hipSetDevice");
    const size_t mm = (size_t)std::max<int64_t>(m, 1);
    if (!ctx->rob_pcat.ensure(mm * 4) || !ctx->rob_e.ensure(mm * 8) || !ctx->rob_r.ensure(mm * 8) || !ctx->rob_wr.ensure(mm * 8) ||
        !ctx->rob_state.ensure(fsnap::robust_state_bytes(ncat)))
        return ctx->fail(FSNAP_E_NOMEM, "hipMalloc(robust session) failed");
    if (m > 0) {
        // the class ids travel through the session's residual vector (m x 4 bytes fit in its m x 8) and are folded with the
        // base weights and the mask into the participating class of every row
        const int* dcat = nullptr;
        if (cat) {
            FSNAP_HIP(hipMemcpyAsync(ctx->rob_e.p, cat, (size_t)m * 4, hipMemcpyHostToDevice, ctx->stream), "hipMemcpy(classes)");
            dcat = (const int*)ctx->rob_e.p;
        }
        FSNAP_HIP(fsnap::launch_robust_pcat(ctx->dw, ctx->dmask, dcat, m, (int*)ctx->rob_pcat.p, ctx->stream), "launch fsnap_robust_pcat_k");
    }
    FSNAP_HIP(hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");
    ctx->rob_dw = ctx->dw;
    ctx->rob_dmask = ctx->dmask;
    ctx->rob_wpack_valid = ctx->wpack_valid;
    ctx->rob_ncat = ncat;
    ctx->rob_m = m;
    ctx->rob_have_e = ctx->rob_have_r = ctx->rob_have_scale = ctx->rob_pointed = false;
    ctx->rob_active = true;
    return FSNAP_OK;
}

int fsnap_robust_residuals(fsnap_ctx* ctx, const double* beta, int64_t K) {
    if (!ctx) return FSNAP_E_ARG;
    const char* who = "fsnap_robust_residuals";
    int rc = robust_session(ctx, who);
    if (rc) return rc;
    FSNAP_HIP(hipSetDevice(ctx->device), "hipSetDevice");
    if ((rc = robust_check_beta(ctx, who, beta, K))) return rc;
    if (ctx->rob_m > 0) {
        FSNAP_HIP(hipEventRecord(ctx->ev[7], ctx->stream), "hipEventRecord");       // (the row pass's slot of fsnap_timing)
        FSNAP_HIP(fsnap::launch_robust_rows(ctx->dA, ctx->lda, (const double*)ctx->beta.p, ctx->rob_m, (int)K, ctx->db, ctx->rob_dw,
                                            (const int*)ctx->rob_pcat.p, nullptr, (double*)ctx->rob_e.p, false, 0, 1.0, nullptr,
                                            nullptr, nullptr, nullptr, nullptr, ctx->rob_ncat, ctx->stream),
                  "launch fsnap_robust_rows_k");
        FSNAP_HIP(hipEventRecord(ctx->ev[8], ctx->stream), "hipEventRecord");
        ctx->t_predict = true;
        FSNAP_HIP(hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");       // the caller's beta may be reused
    }
    ctx->rob_have_e = true;
    return FSNAP_OK;
}

int fsnap_robust_scale(fsnap_ctx* ctx, double* scale, int64_t* count) {
    if (!ctx) return FSNAP_E_ARG;
    const char* who = "fsnap_robust_scale";
    int rc = robust_session(ctx, who);
    if (rc) return rc;
    if (!ctx->rob_have_e && ctx->rob_m > 0) return ctx->fail(FSNAP_E_STATE, "%s: no residuals yet (fsnap_robust_residuals)", who);
    FSNAP_HIP(hipSetDevice(ctx->device), "hipSetDevice");
    const int ncat = ctx->rob_ncat;
    void* st = ctx->rob_state.p;
    FSNAP_HIP(hipMemsetAsync(st, 0, fsnap::robust_state_bytes(ncat), ctx->stream), "hipMemsetAsync(robust state)");
    for (int pass = 0; pass < 8; ++pass) {
        FSNAP_HIP(fsnap::launch_robust_hist((const double*)ctx->rob_e.p, (const int*)ctx->rob_pcat.p, ctx->rob_m, pass, ncat, st,
                                            ctx->stream),
                  "launch fsnap_robust_hist_k");
        if (ctx->comm) {
            FSNAP_HIP(fsnap::launch_robust_table_to_double(st, ncat, ctx->stream), "launch fsnap_robust_table_to_double_k");
            if ((rc = fsnap_allreduce_device(ctx, fsnap::robust_table_doubles(st, ncat), (int64_t)ncat * 512))) return rc;
        }
        FSNAP_HIP(fsnap::launch_robust_choose(st, pass, ncat, ctx->comm != nullptr, ctx->stream), "launch fsnap_robust_choose_k");
    }
    std::vector<double> hs((size_t)ncat);
    std::vector<long long> hn((size_t)ncat);
    FSNAP_HIP(hipMemcpyAsync(hs.data(), fsnap::robust_scale_ptr(st, ncat), (size_t)ncat * 8, hipMemcpyDeviceToHost, ctx->stream), "hipMemcpy(scale)");
    FSNAP_HIP(hipMemcpyAsync(hn.data(), fsnap::robust_count_ptr(st, ncat), (size_t)ncat * 8, hipMemcpyDeviceToHost, ctx->stream), "hipMemcpy(count)");
    if ((rc = fsnap::wait_stream(ctx, nullptr, "robust scale"))) return rc;
    for (int g = 0; g < ncat; ++g) {
        if (scale) scale[g] = hs[(size_t)g];
        if (count) count[g] = (int64_t)hn[(size_t)g];
    }
    ctx->rob_have_scale = true;
    return FSNAP_OK;
}

int fsnap_robust_reweight(fsnap_ctx* ctx, int loss, double c, const double* scale, double* sums) {
    if (!ctx) return FSNAP_E_ARG;
    const char* who = "fsnap_robust_reweight";
    int rc = robust_session(ctx, who);
    if (rc) return rc;
    FSNAP_HIP(hipSetDevice(ctx->device), "hipSetDevice");
    return robust_weights(ctx, who, false, loss, c, scale, sums);
}

int fsnap_robust_step(fsnap_ctx* ctx, const double* beta, int64_t K, int loss, double c, const double* scale, double* sums) {
    if (!ctx) return FSNAP_E_ARG;
    const char* who = "fsnap_robust_step";
    int rc = robust_session(ctx, who);
    if (rc) return rc;
    if (loss != FSNAP_ROBUST_HUBER && loss != FSNAP_ROBUST_BISQUARE && loss != FSNAP_ROBUST_CAUCHY)
        return ctx->fail(FSNAP_E_ARG, "%s: unknown loss %d", who, loss);
    FSNAP_HIP(hipSetDevice(ctx->device), "hipSetDevice");
    if ((rc = robust_check_beta(ctx, who, beta, K))) return rc;
    return robust_weights(ctx, who, true, loss, c, scale, sums);
}

int fsnap_robust_download(fsnap_ctx* ctx, double* e, double* r, double* wr) {
    if (!ctx) return FSNAP_E_ARG;
    const char* who = "fsnap_robust_download";
    // the vectors outlive fsnap_robust_end (diagnostics are fetched after the loop), not new rows or new weights
    if (!ctx->rob_active && !ctx->rob_have_e && !ctx->rob_have_r) return robust_session(ctx, who);
    const size_t m = (size_t)ctx->rob_m;
    if (m == 0) return FSNAP_OK;
    if (e && !ctx->rob_have_e) return ctx->fail(FSNAP_E_STATE, "%s: no residuals yet", who);
    if ((r || wr) && !ctx->rob_have_r) return ctx->fail(FSNAP_E_STATE, "%s: no weights yet (fsnap_robust_reweight)", who);
    FSNAP_HIP(hipSetDevice(ctx->device), "hipSetDevice");
    if (e) FSNAP_HIP(hipMemcpyAsync(e, ctx->rob_e.p, m * 8, hipMemcpyDeviceToHost, ctx->stream), "hipMemcpy(e)");
    if (r) FSNAP_HIP(hipMemcpyAsync(r, ctx->rob_r.p, m * 8, hipMemcpyDeviceToHost, ctx->stream), "hipMemcpy(r)");
    if (wr) FSNAP_HIP(hipMemcpyAsync(wr, ctx->rob_wr.p, m * 8, hipMemcpyDeviceToHost, ctx->stream), "hipMemcpy(wr)");
    FSNAP_HIP(hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");
    return FSNAP_OK;
}
