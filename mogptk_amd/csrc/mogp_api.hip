// mogp_api.hip -- the model-independent part of the C ABI of libmogp_hip.so (see include/mogp_hip.h): error state, contexts and their streams, model
// lifecycle and setters, input sorting and tile lists, the phases of the dense SPD workspace (spd_potrf / trtri / lauum) and ensure_system, mogp_gram*, the
// getters and the profiling switches.  The evaluations live in exact.hip (one GPU), shard.hip (sweep / sharded) and the sparse models' files.
#include "mogp_model.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <cstdlib>

namespace mogp {

static thread_local std::string g_err;
void set_error(const std::string& msg) { g_err = msg; }
int hip_fail(hipError_t e, const char* what, const char* file, int line) {
    g_err = std::string("HIP error '") + hipGetErrorString(e) + "' in " + what + " (" + file + ":" + std::to_string(line) + ")";
    return MOGP_EHIP;
}
int launch_potrf_trtri_tile(double* A, int64_t ld, int t, double* invd, double* logdet, unsigned long long* info, hipStream_t s,
                            long long info_base = 0, int store_L = 0);

int fail(int code, const std::string& msg) { g_err = msg; return code; }

int sort_inputs(const double* X, int64_t M, int D, int C, int64_t pad_to, SortedX& o) {
    o.M = M;
    o.Mpad = round_up(std::max<int64_t>(M, 1), pad_to);
    o.perm.resize(M);
    o.off.assign(C + 1, 0);
    std::vector<int> chan(M);
    for (int64_t r = 0; r < M; ++r) {
        const double c = X[r * (1 + D)];
        if (!(c >= 0.0) || c >= (double)C || c != std::floor(c))
            return fail(MOGP_EINVAL, "X must have integers in [0, output_dims) for the channel IDs in the first input dimension");
        chan[r] = (int)c;
        o.off[chan[r] + 1]++;
    }
    for (int c = 0; c < C; ++c) o.off[c + 1] += o.off[c];
    std::vector<int> cur(o.off.begin(), o.off.end() - 1);
    o.identity = true;
    for (int64_t r = 0; r < M; ++r) {
        const int64_t pos = cur[chan[r]]++;
        o.perm[pos] = r;
        if (pos != r) o.identity = false;
    }
    o.xs.assign((size_t)D * o.Mpad, 0.0);
    for (int64_t pos = 0; pos < M; ++pos)
        for (int d = 0; d < D; ++d) o.xs[(size_t)d * o.Mpad + pos] = X[o.perm[pos] * (1 + D) + 1 + d];
    return 0;
}

// tiles of the symmetric Gram (lower channel pairs, lower tiles inside diagonal channel blocks), grouped by pair
void tile_blocks(const std::vector<int>& off, int C, std::vector<int>& blk) {
    blk.clear();
    for (int c = 0; c < C; ++c)
        for (int b = 0; b * MOGP_GT < off[c + 1] - off[c]; ++b) {
            blk.push_back(off[c] + b * MOGP_GT);
            blk.push_back(std::min(MOGP_GT, off[c + 1] - off[c] - b * MOGP_GT));
        }
}
static std::vector<int> block_base(const std::vector<int>& off, int C) {         // index of channel c's first block
    std::vector<int> base(C + 1, 0);
    for (int c = 0; c < C; ++c) base[c + 1] = base[c] + (off[c + 1] - off[c] + MOGP_GT - 1) / MOGP_GT;
    return base;
}

void build_sym_tiles(const std::vector<int>& off, int C, std::vector<GTile>& tiles, std::vector<int>& pair_start) {
    tiles.clear();
    pair_start.assign(1, 0);
    const std::vector<int> rbase = block_base(off, C), cbase = rbase;
    for (int i = 0; i < C; ++i)
        for (int j = 0; j <= i; ++j) {
            const int ni = off[i + 1] - off[i], nj = off[j + 1] - off[j];
            for (int bi = 0; bi * MOGP_GT < ni; ++bi)
                for (int bj = 0; bj * MOGP_GT < nj; ++bj) {
                    if (i == j && bj > bi) continue;
                    GTile t;
                    t.r0 = off[i] + bi * MOGP_GT; t.c0 = off[j] + bj * MOGP_GT;
                    t.nr = std::min(MOGP_GT, ni - bi * MOGP_GT); t.nc = std::min(MOGP_GT, nj - bj * MOGP_GT);
                    t.pair = i * C + j;
                    t.flags = (i == j && bi == bj) ? GT_DIAG : GT_MIRROR;
                    t.rb = rbase[i] + bi; t.cb = cbase[j] + bj;
                    tiles.push_back(t);
                }
            pair_start.push_back((int)tiles.size());
        }
}

void build_rect_tiles(const std::vector<int>& offr, const std::vector<int>& offc, int C, std::vector<GTile>& tiles,
                      std::vector<int>* pair_start) {
    tiles.clear();
    if (pair_start) pair_start->assign(1, 0);
    const std::vector<int> rbase = block_base(offr, C), cbase = block_base(offc, C);
    for (int i = 0; i < C; ++i)
        for (int j = 0; j < C; ++j) {
            const int ni = offr[i + 1] - offr[i], nj = offc[j + 1] - offc[j];
            for (int bi = 0; bi * MOGP_GT < ni; ++bi)
                for (int bj = 0; bj * MOGP_GT < nj; ++bj) {
                    GTile t;
                    t.r0 = offr[i] + bi * MOGP_GT; t.c0 = offc[j] + bj * MOGP_GT;
                    t.nr = std::min(MOGP_GT, ni - bi * MOGP_GT); t.nc = std::min(MOGP_GT, nj - bj * MOGP_GT);
                    t.pair = i * C + j;
                    t.flags = 0;
                    t.rb = rbase[i] + bi; t.cb = cbase[j] + bj;
                    tiles.push_back(t);
                }
            if (pair_start) pair_start->push_back((int)tiles.size());
        }
}

}  // namespace mogp

namespace mogp {
int plan_cus(const mogp_ctx* ctx) {
    if (ctx && ctx->plan_ncu > 0) return ctx->plan_ncu;
    static const int ncu = []() { int dev = 0; hipDeviceProp_t pr; if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&pr, dev) != hipSuccess) return 256; return pr.multiProcessorCount; }();
    return ncu;
}

void plan_strip_tiles(const std::vector<GTile>& tiles, int maxrun, int slots, std::vector<GSeg>& segs, std::vector<GTile>& rest) {
    split_strip_tiles(tiles, maxrun, segs, rest);
    // The hardware hands out workgroups in index order as slots free up: the launch ends when its LAST runs end, so those should be short.  The runs
    // that would be dispatched last (the final `tail` tiles' worth) are cut into single tiles, the `tail` tiles before them into pairs; a list with
    // fewer runs than there are workgroup slots is cut into single tiles altogether (the head launch of the dataflow schedule: 8 column tiles a row).
    if (segs.empty()) return;
    const long tail = slots;
    long total = 0;
    for (const GSeg& g : segs) total += g.n;
    std::vector<GSeg> out;
    out.reserve(segs.size() * 2);
    long seen = 0;
    const bool all_single = (long)segs.size() < 2L * slots;
    for (const GSeg& g : segs) {
        const long left = total - seen;                      // tiles from this run to the end of the list
        const int cut = (all_single || left <= tail) ? 1 : (left <= 2 * tail ? 2 : maxrun);
        for (int o = 0; o < g.n; o += cut) {
            GSeg h = g;
            h.c0 = g.c0 + o * MOGP_GT; h.n = std::min(cut, g.n - o); h.diag = (o + cut >= g.n) ? g.diag : 0;
            out.push_back(h);
        }
        seen += g.n;
    }
    segs.swap(out);
}
}  // namespace mogp

using namespace mogp;

constexpr int kStripMaxRun = 8;    // tiles per run (round 6, with the graded tail and the one-barrier kernel: 103 us at 8 against 105 at 4 and 108 at 6, configs[1])

int StripTiles::build(const std::vector<GTile>& tiles, int ncu_) {
    plan_strip_tiles(tiles, kStripMaxRun, 2 * ncu_, segs, rest);
    ncu = ncu_;
    int rc;
    if ((rc = d_segs.ensure(std::max<size_t>(segs.size(), 1)))) return rc;
    if ((rc = d_rest.ensure(std::max<size_t>(rest.size(), 1)))) return rc;
    if (!segs.empty()) HIP_TRY(dev_upload(d_segs.p, segs.data(), segs.size() * sizeof(GSeg)));
    if (!rest.empty()) HIP_TRY(dev_upload(d_rest.p, rest.data(), rest.size() * sizeof(GTile)));
    return 0;
}

namespace mogp { int use_device(mogp_ctx* c) { HIP_TRY(hipSetDevice(c->device)); return 0; } }

// ---------------------------------------------------------------------------------------------------------------
extern "C" {

const char* mogp_version(void) { return "mogp_hip 0.1 (gfx950, fp64)"; }
const char* mogp_last_error(void) { return g_err.c_str(); }

int mogp_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int mogp_ctx_create(int device, mogp_ctx** out) {
    if (!out) return fail(MOGP_EINVAL, "mogp_ctx_create: out is null");
    int n = mogp_device_count();
    if (n <= 0) return fail(MOGP_ENODEVICE, "no HIP device visible: mogptk_amd has no CPU path");
    if (device < 0 || device >= n) return fail(MOGP_EINVAL, "mogp_ctx_create: device ordinal out of range");
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    mogp_ctx* c = new mogp_ctx();
    c->device = device;
    c->name = std::string(prop.name) + " (" + prop.gcnArchName + ")";
    {   // One device-to-host copy of more than 16 KB into pinned memory NOW.  The first such copy of a process sets something up inside the runtime, and when
        // that happened while the dataflow kernel and its chain kernels were running (the z^T z parts of a model with more than 8192 points: 18 KB), they
        // stalled until their waits gave up: every first evaluation above N = 8192 fell back to the stream schedule (tools/r4_first.py; 16 KB pieces do not
        // trigger it, a sleep in front of the copy avoids it).  Found in round 4 when the dataflow default went to 96 tile rows.
        // ON THIS CONTEXT'S DEVICE (whatever the calling thread's current device is -- if the set-up is per device, GPUs 1 .. n need it as well), on
        // that device's null stream (the context's own streams are created with its first model), and the caller's current device is restored.
        int prev = -1;
        hipError_t e = hipGetDevice(&prev); (void)e;
        if (hipSetDevice(device) == hipSuccess) {
            void* dsrc = nullptr; void* hdst = nullptr;
            const size_t nbytes = 32u << 20;                     // and at three sizes: the runtime picks its copy path by size (the prediction brings back 33 KB, a fetch 512 MB)
            if (hipMalloc(&dsrc, nbytes) == hipSuccess && hipHostMalloc(&hdst, nbytes, hipHostMallocDefault) == hipSuccess) {
                e = hipMemsetAsync(dsrc, 0, nbytes, nullptr); (void)e;
                for (size_t nb : {(size_t)64 << 10, (size_t)2 << 20, nbytes}) { e = hipMemcpyAsync(hdst, dsrc, nb, hipMemcpyDeviceToHost, nullptr); (void)e; }
                e = hipStreamSynchronize(nullptr); (void)e;
            }
            if (hdst) { e = hipHostFree(hdst); (void)e; }
            if (dsrc) { e = hipFree(dsrc); (void)e; }
            if (prev >= 0 && prev != device) { e = hipSetDevice(prev); (void)e; }
        }
    }
    *out = c;
    return MOGP_OK;
}

int mogp_ctx_destroy(mogp_ctx* ctx) {
    if (!ctx) return MOGP_OK;
    for (hipStream_t q : {ctx->st, ctx->st2, ctx->st2u, ctx->st3, ctx->st4, ctx->st5, ctx->st_priv}) if (q) { hipError_t e = hipStreamSynchronize(q); (void)e; e = hipStreamDestroy(q); (void)e; }
    for (auto& kv : ctx->sk) { kv.second.ws.release(); kv.second.flags.release(); }
    ctx->sk.clear();
    delete ctx;
    return MOGP_OK;
}

int mogp_ctx_device_name(mogp_ctx* ctx, char* buf, int buflen) {
    if (!ctx || !buf || buflen <= 0) return fail(MOGP_EINVAL, "mogp_ctx_device_name: bad argument");
    std::snprintf(buf, (size_t)buflen, "%s", ctx->name.c_str());
    return MOGP_OK;
}

}  // extern "C"

// ---- TRTRI level tasks ------------------------------------------------------------------------------------------
// Bottom-up pairing of tile ranges: at level l (block size s = 2^(l-1) tiles) node b owns tiles [2sb, 2sb+2s); its left
// half [lo, mid) and right half [mid, hi) are already inverted, and  W21 = -W22 * (L21 * W11)  fills the off-diagonal part.
namespace mogp { void build_trtri_levels(Spd& w) {
    const int nb = w.nb;
    const int64_t ld = w.Npad;
    w.levels.clear();
    for (int s = 1; s < nb; s *= 2) {
        TrtriLevel lv;
        for (int lo = 0; lo < nb; lo += 2 * s) {
            const int mid = lo + s, hi = std::min(lo + 2 * s, nb);
            if (mid >= hi) continue;
            for (int ti = mid; ti < hi; ++ti)
                for (int tj = lo; tj < mid; ++tj) {
                    GemmTask t1;      // T[ti][tj] = sum_{k = tj..mid} L21[ti][k] * W11[k][tj]      (W11 lower: k >= tj)
                    t1.a_off = (int64_t)ti * MOGP_TILE * ld + (int64_t)tj * MOGP_TILE;
                    t1.b_off = (int64_t)tj * MOGP_TILE * ld + (int64_t)tj * MOGP_TILE;
                    t1.c_off = (int64_t)ti * MOGP_TILE * ld + (int64_t)tj * MOGP_TILE;
                    t1.kt = (mid - tj) * (MOGP_TILE / 16); t1.pad = 0;
                    lv.h1.push_back(t1);
                    GemmTask t2;      // W21[ti][tj] = - sum_{k = mid..ti} W22[ti][k] * T[k][tj]   (W22 lower: k <= ti)
                    t2.a_off = (int64_t)ti * MOGP_TILE * ld + (int64_t)mid * MOGP_TILE;
                    t2.b_off = (int64_t)mid * MOGP_TILE * ld + (int64_t)tj * MOGP_TILE;
                    t2.c_off = t1.c_off;
                    t2.kt = (ti - mid + 1) * (MOGP_TILE / 16); t2.pad = 0;
                    lv.h2.push_back(t2);
                }
        }
        auto by_k = [](const GemmTask& a, const GemmTask& b) { return a.kt > b.kt; };
        std::stable_sort(lv.h1.begin(), lv.h1.end(), by_k);
        std::stable_sort(lv.h2.begin(), lv.h2.end(), by_k);
        for (auto& t : lv.h1) lv.flops1 += 2.0 * MOGP_TILE * MOGP_TILE * 16.0 * t.kt;
        for (auto& t : lv.h2) lv.flops2 += 2.0 * MOGP_TILE * MOGP_TILE * 16.0 * t.kt;
        w.levels.push_back(std::move(lv));
    }
}
}  // namespace mogp

// Stream-K form for the launches whose tile count sits badly on the workgroup slots of their stream (linalg.hip:k_gemm_sk).
// Measured inside the schedules (round 3, tools/r3_x2.sh): the wide triangular solves of the sparse models -- 782-tile updates that have the
// chip to themselves -- gain (configs[4] 49.5 -> 47.9 ms); the fused factorisation + inversion and the prediction LOSE (configs[1] 12.9 ->
// 13.9 ms, configs[3] 47.2 -> 50.4): next to other launches a partly filled round is filled by them anyway, and workgroups that hold their
// slots four tiles long delay the critical stream's launches.  So: only where the caller asks (GemmArgs::sk_hint), for launches of at least
// half the slots whose last round would be less than sk_fill percent full.
namespace mogp { static int stream_k_setup(mogp_model* m, GemmArgs& g, hipStream_t st) {
    constexpr int sk_min = 8;        // k blocks per span at least
    constexpr int sk_fill = 60;
    g.sk_spans = 0;
    if (!g.sk_hint || m->no_chain || g.small || g.ksplit > 1 || g.row_mod > 1 || g.K % 16) return 0;
    if (!(g.mode == GM_RECT || g.mode == GM_RECT_LOWER || g.mode == GM_LOWER || g.mode == GM_KHI_J || g.mode == GM_KLO_J)) return 0;
    mogp_ctx* ctx = m->ctx;
    const int ncu = ctx->ncu > 0 ? ctx->ncu : 256;
    int cus = ncu;
    if (ctx->st_priv) {
        if (st == ctx->st_priv) cus = ctx->ncu_reserved;
        else if (st == ctx->st2 || st == ctx->st3 || st == ctx->st4) cus = ncu - ctx->ncu_reserved;
    }
    const int slots = 2 * cus;
    const long long T = g.mode == GM_LOWER ? (long long)g.mt * (g.mt + 1) / 2 : (long long)g.mt * g.nt;
    long long tot;
    if (g.mode == GM_KHI_J || g.mode == GM_KLO_J) { long long row = 0; for (int tj = 0; tj < g.nt; ++tj) row += (g.mode == GM_KHI_J ? std::min<long long>(g.K, (long long)(tj + 1) * MOGP_TILE) : g.K - (long long)tj * MOGP_TILE) / 16; tot = row * g.mt; }
    else tot = T * (g.K / 16);
    if (tot <= 0 || tot >= (1ll << 31) || (long long)slots * slots >= (1ll << 31)) return 0;
    const long long last = T % slots;                           // tiles of the last round
    if (2 * T < slots || last == 0 || 100 * last >= (long long)sk_fill * slots) return 0;
    const long long spans = std::min<long long>(slots, tot / sk_min);
    if (spans < 2) return 0;
    mogp_ctx::SkWs& w = ctx->sk[st];
    if (w.flags.n < (size_t)slots) {
        HIP_TRY(hipStreamSynchronize(st));
        int rc;
        if ((rc = w.ws.ensure((size_t)slots * MOGP_TILE * MOGP_TILE))) return rc;
        if ((rc = w.flags.ensure((size_t)slots))) return rc;
        HIP_TRY(hipMemsetAsync(w.flags.p, 0, (size_t)slots * sizeof(unsigned), st));      // in stream order before the launch (the streams are non-blocking)
        w.epoch = 0;
    }
    g.sk_spans = (int)spans; g.sk_ws = w.ws.p; g.sk_flags = w.flags.p; g.sk_epoch = ++w.epoch; g.sk_info = m->d_info.p;
    return 0;
} }

namespace mogp { int gemm_call(mogp_model* m, const GemmArgs& g, double flops, hipStream_t st) {
    if (!st) st = m->st;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (m->profiling) {
        if (m->gemm_ev_used + 2 > m->gemm_ev.size()) {
            for (int i = 0; i < 64; ++i) { hipEvent_t e; HIP_TRY(hipEventCreate(&e)); m->gemm_ev.push_back(e); }
        }
        e0 = m->gemm_ev[m->gemm_ev_used++];
        e1 = m->gemm_ev[m->gemm_ev_used++];
        HIP_TRY(hipEventRecord(e0, st));
    }
    GemmArgs gs = g;
    { int r__ = stream_k_setup(m, gs, st); if (r__) return r__; }
    int rc = launch_gemm(gs, st);
    if (rc) return rc;
    if (m->profiling) HIP_TRY(hipEventRecord(e1, st));
    m->gemm_launches++;
    m->gemm_flops += flops;
    return 0;
}
}  // namespace mogp

namespace mogp { int mark(mogp_model* m, int idx) {
    if (!m->profiling) return 0;
    while ((int)m->ev.size() <= idx) { hipEvent_t e; HIP_TRY(hipEventCreate(&e)); m->ev.push_back(e); }
    HIP_TRY(hipEventRecord(m->ev[idx], m->st));
    return 0;
}
}  // namespace mogp

// Cholesky of w.A (lower) in place; w.invd gets the inverses of the diagonal 128-tiles, w.logdet the per-tile sums of
// log L_kk; a non-positive pivot is reported through m->d_info (atomicMin of the 1-based index).
namespace mogp { int spd_potrf(mogp_model* m, Spd& w, long long info_base) {
    int rc;
    hipStream_t cq = m->st;
    // Bulk stream: the one masked to everything but the reserved CUs while the serial chain matters -- the chain's small kernels (this
    // stream, all CUs) then find idle CUs instead of sharing one with GEMM waves: 15.9 vs 21.1 ms per evaluation at N = 8192, 74 vs 82 ms
    // for the N = 16384 prediction.  Once the work is flop-bound the 6 % of CUs matter more (sweep at N = 32768: 597 vs 638 ms): all CUs.
    hipStream_t bulk_q = (w.nb > MOGP_CHAIN_BOUND_TILES && m->st2u) ? m->st2u : m->st2;
    // ---- two-level blocked right-looking Cholesky with look-ahead.
    // Outer blocks of MOGP_OUTER tiles.  "chain(kb)" = for each 128-column of the block: leaf (factor + inverse) -> panel =
    // panel * inv(Lkk)^T for ALL rows below -> update of the block's remaining columns (64x64-tile GEMMs: latency-bound).
    // The trailing matrix gets one K = MOGP_OUTER*128 SYRK per outer block, split in two:
    //   A(kb): the next block's columns, on the critical stream (chain(kb+1) needs them);
    //   B(kb): everything to the right, on the bulk stream, overlapping chain(kb+1).
    // A(kb) and B(kb-1) accumulate into the same tiles, so A(kb) waits for B(kb-1).
    const int nb = w.nb;
    const int nouter = (nb + MOGP_OUTER - 1) / MOGP_OUTER;
    while ((int)w.sync_ev.size() < 2 * nouter + 2) {
        hipEvent_t e;
        HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        w.sync_ev.push_back(e);
    }
    int last_bulk = -1;
    if (w.want_row_ev)
        while ((int)w.row_ev.size() < nb) {
            hipEvent_t e;
            HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
            w.row_ev.push_back(e);
        }
    for (int kb = 0; kb < nouter; ++kb) {
        const int k0 = kb * MOGP_OUTER, k1 = std::min(k0 + MOGP_OUTER, nb);
        for (int k = k0; k < k1; ++k) {
            if ((rc = launch_potrf_trtri_tile(w.A.p, w.Npad, k, w.invd.p, w.logdet.p, m->d_info.p, cq, info_base, w.keep_L ? 1 : 0))) return rc;
            if (w.want_row_ev) HIP_TRY(hipEventRecord(w.row_ev[k], cq));      // block row k of L: the panels of the columns left of it are behind us on this stream, L_kk is this leaf's
            const int rem = nb - k - 1;
            if (rem <= 0) break;
            double* panel = w.A.p + (int64_t)(k + 1) * MOGP_TILE * w.Npad + (int64_t)k * MOGP_TILE;
            GemmArgs g{};
            g.A = panel; g.lda = w.Npad; g.a_kmajor = 0;
            g.B = w.invd.p + (int64_t)k * MOGP_TILE * MOGP_TILE; g.ldb = MOGP_TILE; g.b_kmajor = 0;
            g.C = panel; g.ldc = w.Npad; g.alpha = 1.0; g.beta = 0.0;
            g.mode = GM_RECT; g.small = 1; g.mt = 2 * rem; g.nt = 1; g.K = MOGP_TILE;      // 64x128 tiles: in place
            if (w.refine_panels) {            // keep the panel as it came: the residual below is taken against it
                if ((rc = w.pscr.ensure((size_t)w.Npad * MOGP_TILE))) return rc;
                if ((rc = launch_copy2d(w.pscr.p, MOGP_TILE, panel, w.Npad, (int64_t)rem * MOGP_TILE, MOGP_TILE, 1.0, cq))) return rc;
            }
            if ((rc = gemm_call(m, g, gemm_flops(g, nullptr), cq))) return rc;
            if (w.refine_panels) {
                // (round 5) P = A0 W^T is only as good as the explicit tile inverse: with L_kk of condition 4e4 (a 128-point stretch of the inducing
                // grid of configs[4]) the leaf's W has |I - L W| = 3e-11 and the factor a backward error |L L^T - A| / |A| = 1.3e-11 -- four orders
                // above LAPACK's, 5 % of the smallest eigenvalue of K_uu + jitter, and the reason dELBO/dZ sat twice as far from the 80-bit truth
                // as the reference (tools/titsias_stage_errors.py, tools/titsias_chol_residual.py).  One step of iterative refinement against
                // the factor itself, P += (A0 - P L_kk^T) W^T, brings the residual to 6e-16.  Two more small GEMMs per tile column; asked for by
                // the sparse models' K_uu only (Spd::refine_panels; needs keep_L: the diagonal tile of A holds L_kk).
                GemmArgs r1 = g;
                r1.A = panel; r1.lda = w.Npad; r1.B = w.A.p + (int64_t)k * MOGP_TILE * (w.Npad + 1); r1.ldb = w.Npad;
                r1.C = w.pscr.p; r1.ldc = MOGP_TILE; r1.alpha = -1.0; r1.beta = 1.0;
                if ((rc = gemm_call(m, r1, gemm_flops(r1, nullptr), cq))) return rc;
                GemmArgs r2 = g;
                r2.A = w.pscr.p; r2.lda = MOGP_TILE; r2.C = panel; r2.ldc = w.Npad; r2.alpha = 1.0; r2.beta = 1.0;
                if ((rc = gemm_call(m, r2, gemm_flops(r2, nullptr), cq))) return rc;
            }
            const int inner = k1 - k - 1;            // columns k+1 .. k1-1 of this outer block
            if (inner > 0) {
                GemmArgs u{};
                u.A = panel; u.lda = w.Npad; u.a_kmajor = 0; u.B = panel; u.ldb = w.Npad; u.b_kmajor = 0;
                u.C = w.A.p + (int64_t)(k + 1) * MOGP_TILE * (w.Npad + 1); u.ldc = w.Npad; u.alpha = -1.0; u.beta = 1.0;
                u.mode = GM_RECT_LOWER; u.small = 2; u.mt = 2 * rem; u.nt = 2 * inner; u.K = MOGP_TILE;
                if ((rc = gemm_call(m, u, gemm_flops(u, nullptr), cq))) return rc;
            }
        }
        const int rem = nb - k1;
        HIP_TRY(hipEventRecord(w.sync_ev[2 * kb], cq));                       // chain(kb) done
        if (rem <= 0) break;
        double* blockp = w.A.p + (int64_t)k1 * MOGP_TILE * w.Npad + (int64_t)k0 * MOGP_TILE;
        const int K = (k1 - k0) * MOGP_TILE;
        const int na = std::min(MOGP_OUTER, rem);      // tile columns of the next outer block
        if (rem > na) {                                                           // B(kb) on the bulk stream
            HIP_TRY(hipStreamWaitEvent(bulk_q, w.sync_ev[2 * kb], 0));
            double* bp = blockp + (int64_t)na * MOGP_TILE * w.Npad;
            GemmArgs u{};
            u.A = bp; u.lda = w.Npad; u.a_kmajor = 0; u.B = bp; u.ldb = w.Npad; u.b_kmajor = 0;
            u.C = w.A.p + (int64_t)(k1 + na) * MOGP_TILE * (w.Npad + 1); u.ldc = w.Npad; u.alpha = -1.0; u.beta = 1.0;
            u.mode = GM_LOWER; u.mt = rem - na; u.nt = rem - na; u.K = K;
            if ((rc = gemm_call(m, u, gemm_flops(u, nullptr), bulk_q))) return rc;
        }
        if (last_bulk >= 0) HIP_TRY(hipStreamWaitEvent(cq, w.sync_ev[2 * last_bulk + 1], 0));   // A(kb) after B(kb-1)
        if (rem > na) { HIP_TRY(hipEventRecord(w.sync_ev[2 * kb + 1], bulk_q)); last_bulk = kb; }
        {
            GemmArgs u{};                                                         // A(kb): columns k1 .. k1+na-1, rows >= column
            u.A = blockp; u.lda = w.Npad; u.a_kmajor = 0; u.B = blockp; u.ldb = w.Npad; u.b_kmajor = 0;
            u.C = w.A.p + (int64_t)k1 * MOGP_TILE * (w.Npad + 1); u.ldc = w.Npad; u.alpha = -1.0; u.beta = 1.0;
            u.mode = GM_RECT_LOWER; u.mt = rem; u.nt = na; u.K = K;
            if ((rc = gemm_call(m, u, gemm_flops(u, nullptr), cq))) return rc;
        }
    }
    if (last_bulk >= 0) HIP_TRY(hipStreamWaitEvent(cq, w.sync_ev[2 * last_bulk + 1], 0));
    return 0;
}
}  // namespace mogp

// w.A: L -> W = L^-1 (lower), level-batched; uses w.B as scratch
namespace mogp { int spd_trtri(mogp_model* m, Spd& w) {
    int rc;
    const int nb = w.nb;
    // ---- W = L^-1, level by level (all nodes of one level in one launch)
    if ((rc = launch_put_diag_tiles(w.A.p, w.Npad, nb, w.invd.p, m->st))) return rc;
    for (auto& lv : w.levels) {
        GemmArgs g{};
        g.A = w.A.p; g.lda = w.Npad; g.a_kmajor = 0; g.B = w.A.p; g.ldb = w.Npad; g.b_kmajor = 1;
        g.C = w.B.p; g.ldc = w.Npad; g.alpha = 1.0; g.beta = 0.0;
        g.mode = GM_TASKS; g.mt = g.nt = 0; g.K = 0; g.tasks = lv.d1.p; g.ntasks = (int)lv.h1.size();
        if ((rc = gemm_call(m, g, lv.flops1))) return rc;
        g.B = w.B.p; g.C = w.A.p; g.alpha = -1.0; g.tasks = lv.d2.p; g.ntasks = (int)lv.h2.size();
        if ((rc = gemm_call(m, g, lv.flops2))) return rc;
    }
    return 0;
}
}  // namespace mogp

// w.B (lower tiles, full diagonal tiles) = W^T W with W = w.A lower triangular: ONE LAUUM-mode GEMM launch
namespace mogp { int spd_lauum(mogp_model* m, Spd& w) {
    GemmArgs g{};
    g.A = w.A.p; g.lda = w.Npad; g.a_kmajor = 1; g.B = w.A.p; g.ldb = w.Npad; g.b_kmajor = 1;
    g.C = w.B.p; g.ldc = w.Npad; g.alpha = 1.0; g.beta = 0.0;
    if (m->kinv_sparse && &w == &m->k && !m->kinv_lauum_tasks.empty()) {          // only the tiles the gradient reads (kinv_plan), longest k range first
        g.mode = GM_TASKS; g.tasks = m->d_kinv_lauum.p; g.ntasks = (int)m->kinv_lauum_tasks.size(); g.mt = g.nt = 0; g.K = 0;
        double fl = 0.0;
        for (const GemmTask& t : m->kinv_lauum_tasks) fl += 2.0 * MOGP_TILE * MOGP_TILE * 16.0 * t.kt;
        return gemm_call(m, g, fl);
    }
    g.mode = GM_LAUUM; g.mt = g.nt = w.nb; g.K = (int)w.Npad;
    return gemm_call(m, g, gemm_flops(g, nullptr));
}
}  // namespace mogp

namespace mogp { int spd_alloc(Spd& w, int64_t Npad, int owned_rows_device) {
    if (w.Npad == Npad) return 0;
    w.release();
    w.Npad = Npad; w.nb = (int)(Npad / MOGP_TILE);
    int rc;
    bool owned = owned_rows_device >= 0;
    if (owned && w.Arows.reserve((size_t)Npad * Npad * sizeof(double), owned_rows_device)) {
        // a runtime without virtual memory management (or out of address space): the ordinary allocation -- the owned-rows code path does not care
        // whether the rows it never touches exist
        w.Arows.release();
        (void)hipGetLastError();
        owned = false;
    }
    if (owned) {
        // the work matrix of a sharded evaluation: the whole address range, physical memory only where mogp_shard_config asks for it; no B
        // (nothing of the sharded gradient evaluation uses it -- the sharded prediction allocates it when it comes)
        w.A.p = reinterpret_cast<double*>(w.Arows.base); w.A.n = (size_t)Npad * Npad; w.A.borrowed = true;
        w.owned_rows = true;
    } else {
        if ((rc = w.A.ensure((size_t)Npad * Npad))) return rc;
        if ((rc = w.B.ensure((size_t)Npad * Npad))) return rc;
    }
    if ((rc = w.invd.ensure((size_t)w.nb * MOGP_TILE * MOGP_TILE))) return rc;
    if ((rc = w.logdet.ensure(w.nb))) return rc;
    build_trtri_levels(w);
    for (auto& lv : w.levels) {
        if ((rc = lv.d1.ensure(std::max<size_t>(lv.h1.size(), 1)))) return rc;
        if ((rc = lv.d2.ensure(std::max<size_t>(lv.h2.size(), 1)))) return rc;
        HIP_TRY(dev_upload(lv.d1.p, lv.h1.data(), lv.h1.size() * sizeof(GemmTask)));
        HIP_TRY(dev_upload(lv.d2.p, lv.h2.data(), lv.h2.size() * sizeof(GemmTask)));
    }
    // nothing ever writes above the block diagonal of A / B; keep it finite (an owned-rows A is zeroed granule by granule as it is backed)
    if (owned) return 0;
    { int r__ = dev_fill_zero(w.A.p, (size_t)Npad * Npad * sizeof(double)); if (r__) return r__; }
    { int r__ = dev_fill_zero(w.B.p, (size_t)Npad * Npad * sizeof(double)); if (r__) return r__; }
    return 0;
}
int spd_make_whole(Spd& w) {
    int rc;
    if (!w.owned_rows) return 0;
    if ((rc = w.Arows.back(0, (size_t)w.Npad * w.Npad * sizeof(double)))) return rc;
    if (!w.B.p) {
        if ((rc = w.B.ensure((size_t)w.Npad * w.Npad))) return rc;
        if ((rc = dev_fill_zero(w.B.p, (size_t)w.Npad * w.Npad * sizeof(double)))) return rc;
    }
    w.owned_rows = false;
    return 0;
}
}  // namespace mogp

// diagonal value of channel block (c, c) implied by the table (Delta = Psi = 0 there for every kernel on the path)
namespace mogp { double table_diag(const mogp_model* m, int c) {
    const int D = m->D, W = m->Wt;
    const double* tab = m->table.data() + (size_t)(c * m->C + c) * m->T * W;
    if (m->radial && !m->hkind.empty()) {
        // kinds are set: every profile is 1 at zero distance, so a row's diagonal value is its amplitude; a product group's is the product
        // of its rows', and the diagonal is the sum over groups
        const int* kd = m->hkind.data() + (size_t)(c * m->C + c) * m->T;
        double s = 0.0, prod = 1.0;
        for (int t = 0; t < m->T; ++t) {
            prod *= tab[(size_t)t * W];
            if (t == m->T - 1 || !(kd[t] & MOGP_KIND_TIMES)) { s += prod; prod = 1.0; }
        }
        return s;
    }
    double s = 0.0;
    for (int t = 0; t < m->T; ++t) {
        const double* r = tab + (size_t)t * W;
        double arg = 0.0, ph = r[1];
        for (int d = 0; d < D; ++d) { arg += r[2 + d] * r[2 + 2 * D + d] * r[2 + 2 * D + d]; ph += r[2 + D + d] * r[2 + 2 * D + d]; }
        s += r[0] * std::exp(-0.5 * arg) * std::cos(2.0 * M_PI * ph);
    }
    return s;
}

const char* check_kinds(const int* kind, const double* shape, int C, int D, int T, bool* any) {
    *any = false;
    if (!kind) return nullptr;
    const size_t n = (size_t)C * C * T;
    for (size_t i = 0; i < n; ++i) {
        const int k = kind[i] & MOGP_KIND_MASK;
        if (kind[i] < 0 || (kind[i] & ~(MOGP_KIND_MASK | MOGP_KIND_TIMES)) || k > MOGP_KIND_WHITE) return "unknown kind";
        if (k == MOGP_KIND_GATE && D != 1) return "the gate row takes one input dimension";
        // a weighted-dot row stands over the model's own input columns AND the feature columns behind them: with one column there is no such
        // row (over a single input it would be the dot-product row of degree 1), and 9 stays the unknown kind it has always been there
        if (k == MOGP_KIND_WDOT && D < 2) return "unknown kind in one input dimension: a weighted-dot row takes the inputs and at least one feature column, D >= 2";
        *any |= kind[i] != MOGP_KIND_GAUSS;
    }
    if (!*any) return nullptr;
    if (!shape) return "shape is null";
    for (size_t i = 0; i < n; ++i) {
        if ((kind[i] & MOGP_KIND_MASK) == MOGP_KIND_RQ && !(shape[i] > 0.0 && std::isfinite(shape[i]))) return "the rational quadratic shape must be positive";
        if ((kind[i] & MOGP_KIND_MASK) == MOGP_KIND_DOT && !(shape[i] >= 1.0 && shape[i] <= (double)MOGP_DOT_DEGREE_MAX && shape[i] == std::floor(shape[i])))
            return "the degree of a dot-product row must be an integer from 1 to 8";
    }
    // product groups: at most MOGP_GROUP_MAX rows, closed by the end of the pair's table, and the same in every channel pair
    for (int p = 0; p < C * C; ++p) {
        const int* kd = kind + (size_t)p * T;
        int run = 0;
        for (int t = 0; t < T; ++t) {
            if ((kd[t] & MOGP_KIND_TIMES) != (kind[t] & MOGP_KIND_TIMES)) return "product groups must be the same in every channel pair";
            run = (kd[t] & MOGP_KIND_TIMES) ? run + 1 : 0;
            if (run >= MOGP_GROUP_MAX) return "a product group has more than 4 rows";
        }
        if (run) return "the last row of a pair's table multiplies with nothing";
    }
    return nullptr;
}
}  // namespace mogp

// sum over the points of `pts` of the kernel diagonal K(x, x) implied by the table: n_c table_diag(c) per channel, or -- with an envelope on
// the input midpoint (rows of width 2 + 5 D, MOHSM) -- sum_t A_t exp(-1/2 sum_d L_d (x_d - c_d)^2) point by point
namespace mogp { double table_diag_points(const mogp_model* m, const SortedX& pts) {
    const int D = m->D, W = m->Wt, C = m->C;
    double s = 0.0;
    if (W == 2 + 3 * D && m->radial && m->point_kinds) {
        // point rows: a dot-product row's diagonal value at the point x is (A |x|^2 + c)^n, a gate row's A h(x)^2, a weighted-dot row's
        // A sum_d V_d x_d^2 (its amplitude for every other row: the profiles are 1 at zero distance, a white row is A on the diagonal), a group's
        // the product of its rows', the diagonal the sum over groups.  A point's groups are added up on their own and the points with a
        // compensated sum: one running sum over every group of every point drifts (the profile groups add the same constant N times, and the
        // rounding of equal addends does not average out) -- 3e-14 relative at N = 1100, more than the 1e-14 the jitter is held to.
        double comp = 0.0;
        for (int c = 0; c < C; ++c) {
            const double* tab = m->table.data() + (size_t)(c * C + c) * m->T * W;
            const int* kd = m->hkind.data() + (size_t)(c * C + c) * m->T;
            const double* sh = m->hshape.data() + (size_t)(c * C + c) * m->T;
            for (int pos = pts.off[c]; pos < pts.off[c + 1]; ++pos) {
                double x2 = 0.0, prod = 1.0, pt = 0.0;
                for (int d = 0; d < D; ++d) { const double x = pts.xs[(size_t)d * pts.Mpad + pos]; x2 += x * x; }
                for (int t = 0; t < m->T; ++t) {
                    const double* r = tab + (size_t)t * W;
                    double v = r[0];
                    if ((kd[t] & MOGP_KIND_MASK) == MOGP_KIND_DOT) {
                        const double b = r[0] * x2 + r[1];
                        v = b;
                        for (int k = 1; k < (int)sh[t]; ++k) v *= b;
                    } else if ((kd[t] & MOGP_KIND_MASK) == MOGP_KIND_WDOT) {      // A sum_d V_d x_d^2
                        double q = 0.0;
                        for (int d = 0; d < D; ++d) { const double x = pts.xs[(size_t)d * pts.Mpad + pos]; q += r[2 + d] * x * x; }
                        v = r[0] * q;
                    } else if ((kd[t] & MOGP_KIND_MASK) == MOGP_KIND_GATE) {      // h = sigmoid(z) without overflow, as the staging forms it (D = 1)
                        const double z = r[2] * (pts.xs[pos] - r[3]), e = std::exp(-std::fabs(z));
                        const double h = z >= 0.0 ? 1.0 / (1.0 + e) : e / (1.0 + e);
                        v = r[0] * h * h;
                    }
                    prod *= v;
                    if (t == m->T - 1 || !(kd[t] & MOGP_KIND_TIMES)) { pt += prod; prod = 1.0; }
                }
                const double sum = s + pt;                  // Neumaier: the low part of every addition is kept
                comp += std::fabs(s) >= std::fabs(pt) ? (s - sum) + pt : (pt - sum) + s;
                s = sum;
            }
        }
        return s + comp;
    }
    if (W == 2 + 3 * D) {
        for (int c = 0; c < C; ++c) s += (double)(pts.off[c + 1] - pts.off[c]) * table_diag(m, c);
        return s;
    }
    for (int c = 0; c < C; ++c) {
        const double* tab = m->table.data() + (size_t)(c * C + c) * m->T * W;
        for (int pos = pts.off[c]; pos < pts.off[c + 1]; ++pos)
            for (int t = 0; t < m->T; ++t) {
                const double* r = tab + (size_t)t * W;
                double arg = 0.0, ph = r[1], env = 0.0;
                for (int d = 0; d < D; ++d) {
                    arg += r[2 + d] * r[2 + 2 * D + d] * r[2 + 2 * D + d];
                    ph += r[2 + D + d] * r[2 + 2 * D + d];
                    const double a = pts.xs[(size_t)d * pts.Mpad + pos] - r[2 + 4 * D + d];
                    env += r[2 + 3 * D + d] * a * a;
                }
                s += r[0] * std::exp(-0.5 * (arg + env)) * std::cos(2.0 * M_PI * ph);
            }
    }
    return s;
}
}  // namespace mogp

// every entry point that evaluates on this GPU alone: whatever a sharded evaluation of the same model left behind (row ownership: the moment pass,
// the alpha sums and the sweep's updates mask by it; the owned-rows form of the work matrix) no longer applies
namespace mogp { void one_gpu_call(mogp_model* m) { m->sh_n = 1; m->sh_rank = 0; m->sh_owned = false; } }

namespace mogp { int ensure_system(mogp_model* m) {
    int rc;
    const int ncu = plan_cus(m->ctx);
    if (!m->tiles.empty() && m->strip.ncu != ncu) {
        // mogp_ctx_plan_cus changed the count since the runs were cut: cut them again (a measurement / test path -- the kernels of an earlier
        // evaluation may still read the old lists, so every stream that takes a Gram launch is drained first)
        for (hipStream_t q : {m->st, m->st2}) if (q) HIP_TRY(hipStreamSynchronize(q));
        if ((rc = m->strip.build(m->tiles, ncu))) return rc;
        if (m->strip_head.ncu >= 0 && (rc = m->strip_head.build(m->tiles_head, ncu))) return rc;
        if (m->strip_tail.ncu >= 0 && (rc = m->strip_tail.build(m->tiles_tail, ncu))) return rc;
        if (m->strip_own.ncu >= 0 && (rc = m->strip_own.build(m->tiles_own, ncu))) return rc;
    }
    if (m->tiles.empty()) {
        build_sym_tiles(m->sx.off, m->C, m->tiles, m->pair_start);
        if ((rc = m->d_tiles.ensure(m->tiles.size()))) return rc;
        if ((rc = m->d_pair_start.ensure(m->pair_start.size()))) return rc;
        HIP_TRY(dev_upload(m->d_tiles.p, m->tiles.data(), m->tiles.size() * sizeof(GTile)));
        if ((rc = m->strip.build(m->tiles, ncu))) return rc;
        for (const GTile& t : m->tiles) (t.c0 < 4 * MOGP_TILE ? m->tiles_head : m->tiles_tail).push_back(t);
        if (!m->tiles_head.empty() && !m->tiles_tail.empty()) {
            if ((rc = m->d_tiles_head.ensure(m->tiles_head.size()))) return rc;
            if ((rc = m->d_tiles_tail.ensure(m->tiles_tail.size()))) return rc;
            HIP_TRY(dev_upload(m->d_tiles_head.p, m->tiles_head.data(), m->tiles_head.size() * sizeof(GTile)));
            HIP_TRY(dev_upload(m->d_tiles_tail.p, m->tiles_tail.data(), m->tiles_tail.size() * sizeof(GTile)));
            if ((rc = m->strip_head.build(m->tiles_head, ncu))) return rc;
            if ((rc = m->strip_tail.build(m->tiles_tail, ncu))) return rc;
        }
        HIP_TRY(dev_upload(m->d_pair_start.p, m->pair_start.data(), m->pair_start.size() * sizeof(int)));
    }
    if ((rc = m->d_partial.ensure(m->tiles.size() * (size_t)std::max(m->T, 1) * (size_t)std::max(m->Wt, 1)))) return rc;
    // a model whose FIRST evaluation is a sharded one gets its work matrix in the owned-rows form (mogp_shard_config backs the rows); the first
    // one-GPU call on such a model makes it whole
    if (m->k.Npad == m->Npad) return (m->k.owned_rows && !m->sh_owned) ? spd_make_whole(m->k) : 0;
    return spd_alloc(m->k, m->Npad, m->sh_owned ? m->ctx->device : -1);
} }

extern "C" {

// the context's streams: critical (high priority, all CUs), private (reserved CUs only), two bulk streams (everything else)
static int ctx_streams(mogp_ctx* ctx) {
    if (ctx->streams_ready) return 0;
    int lo_prio = 0;
    {
        int lo = 0, hi = 0;
        HIP_TRY(hipDeviceGetStreamPriorityRange(&lo, &hi));
        lo_prio = lo;
        HIP_TRY(hipStreamCreateWithPriority(&ctx->st, hipStreamNonBlocking, hi));
        // MOGP_RESERVE_CUS = R compute units of every XCD are kept for the latency-bound intra-block chain of the fused
        // factorisation + inversion (potri.hip): CU-mask bit i is CU (i / 8) of XCD (i % 8) on gfx950 (tools/micro/cumask.hip),
        // so the first 8 R bits are R CUs from each XCD.  st_priv runs ONLY there, the bulk streams everywhere else: a 1-workgroup
        // leaf that shares its CU with bulk GEMM waves runs 1.6-3x slower (measured), and the dispatcher does not avoid that by itself.
        const char* er = std::getenv("MOGP_RESERVE_CUS");
        const int reserve = er ? std::atoi(er) : 2;
        hipDeviceProp_t prop;
        HIP_TRY(hipGetDeviceProperties(&prop, ctx->device));
        const int ncu = prop.multiProcessorCount;
        const bool masked = reserve > 0 && 16 * reserve < ncu;
        ctx->ncu = ncu; ctx->ncu_reserved = masked ? 8 * reserve : 0;
        ctx->chain_ok = !masked || 8 * reserve >= 13;        // one 128 KB workgroup per CU: fewer reserved CUs than workgroups would never all be resident
        if (masked) {
            std::vector<uint32_t> bulk((ncu + 31) / 32, 0u), priv((ncu + 31) / 32, 0u);
            for (int i = 0; i < ncu; ++i) (i < 8 * reserve ? priv : bulk)[i / 32] |= 1u << (i % 32);
            HIP_TRY(hipExtStreamCreateWithCUMask(&ctx->st_priv, (uint32_t)priv.size(), priv.data()));
            HIP_TRY(hipExtStreamCreateWithCUMask(&ctx->st2, (uint32_t)bulk.size(), bulk.data()));
            HIP_TRY(hipExtStreamCreateWithCUMask(&ctx->st3, (uint32_t)bulk.size(), bulk.data()));
            HIP_TRY(hipExtStreamCreateWithCUMask(&ctx->st4, (uint32_t)bulk.size(), bulk.data()));
        } else {
            HIP_TRY(hipStreamCreateWithPriority(&ctx->st2, hipStreamNonBlocking, (lo + hi) / 2));
            HIP_TRY(hipStreamCreateWithPriority(&ctx->st3, hipStreamNonBlocking, lo));
            HIP_TRY(hipStreamCreateWithPriority(&ctx->st4, hipStreamNonBlocking, lo));
        }
    }
    {   // bulk stream over ALL CUs (full mask), used once an evaluation is flop-bound
        hipDeviceProp_t prop;
        HIP_TRY(hipGetDeviceProperties(&prop, ctx->device));
        std::vector<uint32_t> all((prop.multiProcessorCount + 31) / 32, 0u);
        for (int i = 0; i < prop.multiProcessorCount; ++i) all[i / 32] |= 1u << (i % 32);
        if (ctx->st_priv) HIP_TRY(hipExtStreamCreateWithCUMask(&ctx->st2u, (uint32_t)all.size(), all.data()));
        else HIP_TRY(hipStreamCreateWithPriority(&ctx->st2u, hipStreamNonBlocking, lo_prio));
    }
    ctx->streams_ready = true;
    return 0;
}

int mogp_model_create(mogp_ctx* ctx, int64_t N, int D, int C, const double* X, const double* y, mogp_model** out) {
    if (!ctx || !X || !y || !out) return fail(MOGP_EINVAL, "mogp_model_create: null argument");
    *out = nullptr;
    if (N <= 0 || D <= 0 || D > MOGP_MAXD || C <= 0) return fail(MOGP_EINVAL, "mogp_model_create: need N > 0, 0 < D <= 8, C > 0");
    int rc;
    if ((rc = use_device(ctx))) return rc;
    mogp_model* m = new mogp_model();
    m->ctx = ctx; m->N = N; m->D = D; m->C = C;
    if ((rc = sort_inputs(X, N, D, C, MOGP_TILE, m->sx))) { delete m; return rc; }
    m->Npad = m->sx.Mpad;
    m->nb = (int)(m->Npad / MOGP_TILE);
    const int64_t Npad = m->Npad;
    const int nchunks = (int)((Npad + 511) / 512);
#define TRY_RC(x) do { int r__ = (x); if (r__) { mogp_model_destroy(m); return r__; } } while (0)
#define TRY_HIP(x) do { hipError_t e__ = (x); if (e__ != hipSuccess) { int r__ = hip_fail(e__, #x, __FILE__, __LINE__); mogp_model_destroy(m); return r__; } } while (0)
    TRY_RC(ctx_streams(ctx));
    m->st = ctx->st; m->st2 = ctx->st2; m->st2u = ctx->st2u; m->st3 = ctx->st3; m->st4 = ctx->st4; m->st_priv = ctx->st_priv;
    // the N x N system (two Npad^2 matrices: 160 GB at N = 100 000), the tile lists over (X, X) and their partial-moment buffer (N^2 / 4096
    // tiles) are set up by the first call that needs them (ensure_system): the sparse and variational models never do
    TRY_RC(m->d_x.ensure((size_t)D * Npad));
    TRY_RC(m->d_y.ensure(Npad));
    TRY_RC(m->d_noise.ensure(C));
    TRY_RC(m->d_z.ensure(Npad));
    TRY_RC(m->d_alpha.ensure((size_t)(1 + nchunks) * Npad));
    TRY_RC(m->d_zz.ensure((Npad + 3) / 4));
    TRY_RC(m->d_diagG.ensure(C));
    TRY_RC(m->d_info.ensure(2));                      // [1]: the first factorisation's report of a sparse evaluation (launch_info_stash)
    TRY_RC(m->d_flag.ensure(1));
    TRY_RC(m->d_chan_off.ensure(C + 1));
    TRY_HIP(dev_upload(m->d_x.p, m->sx.xs.data(), (size_t)D * Npad * sizeof(double)));
    TRY_HIP(dev_upload(m->d_chan_off.p, m->sx.off.data(), (C + 1) * sizeof(int)));
    TRY_RC(mogp_model_set_y(m, y));
#undef TRY_RC
#undef TRY_HIP
    *out = m;                                   // only a fully built model is handed out (a failure above has destroyed it)
    return MOGP_OK;
}

int mogp_model_destroy(mogp_model* m) {
    if (!m) return MOGP_OK;
    if (m->ctx) { hipError_t e = hipSetDevice(m->ctx->device); (void)e; }
    if (m->st) { hipError_t e = hipStreamSynchronize(m->st); (void)e; }
    for (auto e : m->ev) { hipError_t r = hipEventDestroy(e); (void)r; }
    for (auto e : m->gemm_ev) { hipError_t r = hipEventDestroy(e); (void)r; }
    for (auto& e : m->pred_ev) if (e) { hipError_t r = hipEventDestroy(e); (void)r; e = nullptr; }
    for (hipStream_t q : {m->st2, m->st2u, m->st3, m->st4, m->ctx->st5, m->st_priv}) if (q) { hipError_t e = hipStreamSynchronize(q); (void)e; }
    m->k.release(); m->ws.release(); m->ws_tail.release();
    for (int b = 0; b < 2; ++b) { m->swU[b].release(); m->swUr[b].release(); m->swXr[b].release(); }
    for (auto e : m->sw_ev) { hipError_t r = hipEventDestroy(e); (void)r; }
    for (auto e : m->sh_prof) { hipError_t r = hipEventDestroy(e); (void)r; }
    m->d_symv.release(); m->sh_send.release(); m->sh_recv.release(); m->sh_send1.release(); m->sh_recv1.release(); m->sh_fact.release();
    for (auto e : m->sh_ev) { hipError_t r = hipEventDestroy(e); (void)r; }
    if (m->tw) { m->tw->release(); delete m->tw; m->tw = nullptr; }
    m->oa.release();
    m->loo.release();
    m->cv.release();
    m->fc.release();
    m->d_x.release(); m->d_y.release(); m->d_table.release(); m->d_kind.release(); m->d_shape.release();
    m->d_noise.release(); m->d_dvar.release(); m->d_z.release(); m->d_alpha.release(); m->d_zz.release();
    m->d_partial.release(); m->d_moments.release(); m->d_diagG.release(); m->d_tiles.release(); m->d_pair_start.release(); m->strip.release(); m->strip_own.release();
    m->d_tiles_head.release(); m->d_tiles_tail.release(); m->strip_head.release(); m->strip_tail.release();
    if (m->gram_ev) { hipError_t r = hipEventDestroy(m->gram_ev); (void)r; m->gram_ev = nullptr; }
    if (m->gram_tail_ev) { hipError_t r = hipEventDestroy(m->gram_tail_ev); (void)r; m->gram_tail_ev = nullptr; }
    m->d_chan_off.release(); m->d_flag.release(); m->d_info.release(); m->d_pivots.release(); m->acc_rhs.release();
    m->d_xs.release(); m->d_Ksf.release(); m->d_Vt.release(); m->d_mu.release(); m->d_var.release(); m->d_kdiag.release();
    m->d_Kss.release(); m->d_parts.release(); m->d_ptiles.release(); m->d_pred_tasks.release();
    m->ph_xx.release(); m->ph_sx.release(); m->ph_ss.release();
    if (m->h_pin) { hipError_t e = hipHostFree(m->h_pin); (void)e; m->h_pin = nullptr; }
    mean_release(m);

    delete m;
    return MOGP_OK;
}

int mogp_model_set_y(mogp_model* m, const double* y) {
    if (!m || !y) return fail(MOGP_EINVAL, "mogp_model_set_y: null argument");
    int rc;
    if ((rc = use_device(m->ctx))) return rc;
    std::vector<double> ys(m->Npad, 0.0);
    for (int64_t pos = 0; pos < m->N; ++pos) ys[pos] = y[m->sx.perm[pos]];
    if (m->mean_on) {                           // the raw targets change under a mean table: the residual follows (mean.hip)
        HIP_TRY(dev_upload(m->d_y0.p, ys.data(), m->Npad * sizeof(double)));
        m->hy0 = ys;
        m->mean_g_valid = m->mean_g_pending = false;
        return mean_apply(m);
    }
    HIP_TRY(dev_upload(m->d_y.p, ys.data(), m->Npad * sizeof(double)));
    m->hy = ys;
    return MOGP_OK;
}

int mogp_model_set_terms_ex(mogp_model* m, int T, int width, const double* table) {
    if (!m || !table || T <= 0) return fail(MOGP_EINVAL, "mogp_model_set_terms: bad argument");
    if (width != 2 + 3 * m->D && width != 2 + 5 * m->D) return fail(MOGP_EINVAL, "mogp_model_set_terms: the row width must be 2 + 3 D or 2 + 5 D");
    int rc;
    if ((rc = use_device(m->ctx))) return rc;
    const int W = width;
    const size_t n = (size_t)m->C * m->C * T * W;
    for (size_t i = 0; i < n; ++i)
        if (!std::isfinite(table[i])) return fail(MOGP_ENONFINITE, "spectral term table has non-finite entries (kernel parameters diverged)");
    if (T != m->T) { m->radial = m->point_kinds = false; m->gate_kinds = 0; }       // kinds belong to a table shape (mogp_model_set_kinds)
    m->T = T;
    m->Wt = W;
    if (m->tw) m->tw->pred_valid = false;       // mogp_sparse_predict_cov combines the last prediction's panels with the CURRENT table: a new table ends that
    m->table.assign(table, table + n);
    if ((rc = m->d_table.ensure(n))) return rc;
    if ((rc = m->d_moments.ensure((size_t)(m->C * (m->C + 1) / 2) * T * W))) return rc;
    HIP_TRY(hipMemcpyAsync(m->d_table.p, m->table.data(), n * sizeof(double), hipMemcpyHostToDevice, m->st));
    return MOGP_OK;
}

int mogp_model_set_terms(mogp_model* m, int T, const double* table) {
    if (!m) return fail(MOGP_EINVAL, "mogp_model_set_terms: bad argument");
    return mogp_model_set_terms_ex(m, T, 2 + 3 * m->D, table);
}

int mogp_model_set_kinds(mogp_model* m, int T, const int* kind, const double* shape) {
    if (!m) return fail(MOGP_EINVAL, "mogp_model_set_kinds: model is null");
    if (T != m->T || T <= 0) return fail(MOGP_EINVAL, "mogp_model_set_kinds: T must be that of the last mogp_model_set_terms");
    const size_t n = (size_t)m->C * m->C * T;
    bool any = false;
    if (const char* bad = check_kinds(kind, shape, m->C, m->D, T, &any)) return fail(MOGP_EINVAL, std::string("mogp_model_set_kinds: ") + bad);
    m->radial = false; m->point_kinds = false; m->gate_kinds = 0;
    if (!any) return MOGP_OK;                   // all Gaussian: as if never called
    if (m->Wt != 2 + 3 * m->D) return fail(MOGP_EINVAL, "mogp_model_set_kinds: radial profiles do not combine with enveloped term rows");
    m->hkind.assign(kind, kind + n);            // table_diag needs the groups on the host
    m->hshape.assign(shape, shape + n);
    for (size_t i = 0; i < n; ++i) {
        const int k = kind[i] & MOGP_KIND_MASK;
        m->point_kinds |= k == MOGP_KIND_DOT || k == MOGP_KIND_GATE || k == MOGP_KIND_WDOT;        // rows whose diagonal follows the point
    }
    m->gate_kinds = extra_rows(kind, n);
    int rc;
    if ((rc = use_device(m->ctx))) return rc;
    if ((rc = m->d_kind.ensure(n))) return rc;
    if ((rc = m->d_shape.ensure(n))) return rc;
    // (pageable sources: the copies are staged before the calls return)
    HIP_TRY(hipMemcpyAsync(m->d_kind.p, kind, n * sizeof(int), hipMemcpyHostToDevice, m->st));
    HIP_TRY(hipMemcpyAsync(m->d_shape.p, shape, n * sizeof(double), hipMemcpyHostToDevice, m->st));
    m->radial = true;
    return MOGP_OK;
}

int mogp_model_set_point_diag(mogp_model* m, const double* kdiag) {
    if (!m) return fail(MOGP_EINVAL, "mogp_model_set_point_diag: model is null");
    m->point_diag.clear();
    if (kdiag) {
        m->point_diag.resize(m->N);
        for (int64_t pos = 0; pos < m->N; ++pos) m->point_diag[pos] = kdiag[m->sx.perm[pos]];
    }
    return MOGP_OK;
}

int mogp_gram(mogp_ctx* ctx, int C, int D, int T, const double* table, int64_t M1, const double* X1,
              int64_t M2, const double* X2, double* K_out) {
    return mogp_gram_ex(ctx, C, D, T, 2 + 3 * D, table, M1, X1, M2, X2, K_out);
}

int mogp_gram_ex(mogp_ctx* ctx, int C, int D, int T, int width, const double* table, int64_t M1, const double* X1,
                 int64_t M2, const double* X2, double* K_out) {
    return mogp_gram_kinds(ctx, C, D, T, width, table, nullptr, nullptr, M1, X1, M2, X2, K_out);
}

int mogp_gram_kinds(mogp_ctx* ctx, int C, int D, int T, int width, const double* table, const int* kind, const double* shape,
                    int64_t M1, const double* X1, int64_t M2, const double* X2, double* K_out) {
    if (!ctx || !table || !X1 || !K_out || M1 <= 0 || T <= 0 || C <= 0 || D <= 0 || D > MOGP_MAXD || (width != 2 + 3 * D && width != 2 + 5 * D))
        return fail(MOGP_EINVAL, "mogp_gram: bad argument");
    bool radial = false;
    if (const char* bad = check_kinds(kind, shape, C, D, T, &radial)) return fail(MOGP_EINVAL, std::string("mogp_gram_kinds: ") + bad);
    if (radial && width != 2 + 3 * D) return fail(MOGP_EINVAL, "mogp_gram_kinds: kinds need shapes and rows of width 2 + 3 D");
    int rc;
    if ((rc = use_device(ctx))) return rc;
    const bool sym = (X2 == nullptr);
    SortedX s1, s2;
    if ((rc = sort_inputs(X1, M1, D, C, 1, s1))) return rc;
    if (!sym && (rc = sort_inputs(X2, M2, D, C, 1, s2))) return rc;
    const SortedX& sc = sym ? s1 : s2;
    const int64_t R = s1.M, Cc = sc.M;
    std::vector<GTile> tiles;
    std::vector<int> ps;
    if (sym) build_sym_tiles(s1.off, C, tiles, ps); else build_rect_tiles(s1.off, s2.off, C, tiles);
    const int W = width;
    DevBuf<double> dx1, dx2, dtab, dout;
    DevBuf<GTile> dt;
    DevBuf<int> dkind;
    DevBuf<double> dshape;
    PhaseWs ph;
    auto cleanup = [&]() { dx1.release(); dx2.release(); dtab.release(); dout.release(); dt.release(); dkind.release(); dshape.release(); ph.release(); };
#define G_TRY(x) do { int r__ = (x); if (r__) { cleanup(); return r__; } } while (0)
#define G_HIP(x) do { hipError_t e__ = (x); if (e__ != hipSuccess) { cleanup(); return hip_fail(e__, #x, __FILE__, __LINE__); } } while (0)
    G_TRY(dx1.ensure((size_t)D * s1.Mpad));
    G_TRY(dtab.ensure((size_t)C * C * T * W));
    G_TRY(dout.ensure((size_t)R * Cc));
    G_TRY(dt.ensure(std::max<size_t>(tiles.size(), 1)));
    G_HIP(dev_upload(dx1.p, s1.xs.data(), (size_t)D * s1.Mpad * sizeof(double)));
    if (!sym) {
        G_TRY(dx2.ensure((size_t)D * s2.Mpad));
        G_HIP(dev_upload(dx2.p, s2.xs.data(), (size_t)D * s2.Mpad * sizeof(double)));
    }
    G_HIP(dev_upload(dtab.p, table, (size_t)C * C * T * W * sizeof(double)));
    G_HIP(dev_upload(dt.p, tiles.data(), tiles.size() * sizeof(GTile)));
    GramArgs ga{};
    ga.tiles = dt.p; ga.xr = dx1.p; ga.ldxr = s1.Mpad; ga.xc = sym ? dx1.p : dx2.p; ga.ldxc = sc.Mpad; ga.nrows = R; ga.ncols = Cc;
    G_TRY(ph.prepare(s1.off, sc.off, C, T, s1.Mpad, sc.Mpad, nullptr, ga.ph));
    ga.table = dtab.p; ga.T = T; ga.D = D; ga.C = C; ga.W = W; ga.out = dout.p; ga.ldo = Cc;
    ga.noise = nullptr; ga.dvar = nullptr; ga.jitter_abs = 0.0; ga.mirror = 1;
    if (radial) {
        G_TRY(dkind.ensure((size_t)C * C * T));
        G_TRY(dshape.ensure((size_t)C * C * T));
        G_HIP(dev_upload(dkind.p, kind, (size_t)C * C * T * sizeof(int)));
        G_HIP(dev_upload(dshape.p, shape, (size_t)C * C * T * sizeof(double)));
        ga.kind = dkind.p; ga.shape = dshape.p;
    }
    G_TRY(launch_gram(plan_cus(ctx), ga, (int)tiles.size(), nullptr, radial ? extra_rows(kind, (size_t)C * C * T) : 0));
    G_HIP(hipDeviceSynchronize());
    if (s1.identity && sc.identity) {
        G_HIP(hipMemcpy(K_out, dout.p, (size_t)R * Cc * sizeof(double), hipMemcpyDeviceToHost));
    } else {
        std::vector<double> h((size_t)R * Cc);
        G_HIP(hipMemcpy(h.data(), dout.p, h.size() * sizeof(double), hipMemcpyDeviceToHost));
        for (int64_t a = 0; a < R; ++a)
            for (int64_t b = 0; b < Cc; ++b) K_out[s1.perm[a] * Cc + sc.perm[b]] = h[(size_t)a * Cc + b];
    }
    cleanup();
#undef G_TRY
#undef G_HIP
    return MOGP_OK;
}

int mogp_model_work_bytes(mogp_model* m, int64_t* backed, int64_t* whole) {
    if (!m || !backed || !whole) return fail(MOGP_EINVAL, "mogp_model_work_bytes: bad argument");
    const int64_t one = (int64_t)m->k.Npad * m->k.Npad * (int64_t)sizeof(double);
    *whole = one;
    *backed = m->k.Npad == 0 ? 0 : (m->k.owned_rows || m->k.Arows.base ? (int64_t)m->k.Arows.backed_bytes() : one);
    return MOGP_OK;
}

int mogp_model_set_accurate(mogp_model* m, int on) {
    if (!m) return fail(MOGP_EINVAL, "mogp_model_set_accurate: model is null");
    m->accurate = on != 0;
    return MOGP_OK;
}

int mogp_model_pivot_range(mogp_model* m, double* lmin, double* lmax) {
    if (!m || !lmin || !lmax) return fail(MOGP_EINVAL, "mogp_model_pivot_range: bad argument");
    *lmin = m->pivot_min; *lmax = m->pivot_max;
    return MOGP_OK;
}

int mogp_model_inverse_fraction(mogp_model* m, double* fraction) {
    if (!m || !fraction) return fail(MOGP_EINVAL, "mogp_model_inverse_fraction: bad argument");
    *fraction = m->kinv_sparse ? m->kinv_fraction : 1.0;
    return MOGP_OK;
}

int mogp_model_schedule(mogp_model* m, int* flags) {
    if (!m || !flags) return fail(MOGP_EINVAL, "mogp_model_schedule: null argument");
    *flags = (m->k.flow_used ? MOGP_SCHED_DATAFLOW : 0) | (chain_enabled(m) ? MOGP_SCHED_CHAIN_KERNEL : 0) |
             (m->no_flow ? MOGP_SCHED_DATAFLOW_FELL_BACK : 0) | (m->no_chain ? MOGP_SCHED_CHAIN_FELL_BACK : 0) |
             (std::min(m->flow_timeouts, 0xffff) << MOGP_SCHED_TIMEOUTS_SHIFT);
    return MOGP_OK;
}

int mogp_model_flow_replay(mogp_model* m, int on) {
    if (!m) return fail(MOGP_EINVAL, "mogp_model_flow_replay: null model");
    if (on && !(m->k.Wm.p && m->have_Kinv)) return fail(MOGP_EINVAL, "mogp_model_flow_replay: needs a completed gradient evaluation on this model first (its W_KK blocks are the replay's input)");
    m->replay_flow = on != 0;
    return MOGP_OK;
}

int mogp_ctx_plan_cus(mogp_ctx* ctx, int ncu) {
    if (!ctx || ncu < 0) return fail(MOGP_EINVAL, "mogp_ctx_plan_cus: need a context and ncu >= 0 (0: the device's count)");
    ctx->plan_ncu = ncu;                        // the models' strip lists follow with their next evaluation (ensure_system, sparse_tiles)
    return MOGP_OK;
}

int mogp_model_strip_runs(mogp_model* m, int which, int64_t* out4) {
    if (!m || !out4 || which < 0 || which > 4) return fail(MOGP_EINVAL, "mogp_model_strip_runs: bad argument");
    const StripTiles* lists[5] = {&m->strip, &m->strip_head, &m->strip_tail, &m->strip_own, m->tw ? &m->tw->strip_uf : nullptr};
    const StripTiles* s = lists[which];
    out4[0] = s ? s->ncu : -1; out4[1] = out4[2] = out4[3] = 0;
    if (!s || s->ncu < 0) return MOGP_OK;                  // never built (or released)
    out4[1] = (int64_t)s->segs.size(); out4[2] = (int64_t)s->rest.size();
    for (const GSeg& g : s->segs) out4[3] = std::max<int64_t>(out4[3], g.n);
    return MOGP_OK;
}

int mogp_strip_plan(int C, const int64_t* sizes, int ncu, int64_t* out, int64_t cap, int64_t* count) {
    if (C <= 0 || !sizes || ncu <= 0 || ncu > (1 << 20) || !count) return fail(MOGP_EINVAL, "mogp_strip_plan: bad argument");
    std::vector<int> off(C + 1, 0);
    for (int c = 0; c < C; ++c) {
        if (sizes[c] < 0 || sizes[c] > (1 << 24) || (int64_t)off[c] + sizes[c] > (1 << 24)) return fail(MOGP_EINVAL, "mogp_strip_plan: channel sizes out of range");
        off[c + 1] = off[c] + (int)sizes[c];
    }
    std::vector<GTile> tiles, rest;
    std::vector<int> ps;
    std::vector<GSeg> segs;
    build_sym_tiles(off, C, tiles, ps);
    plan_strip_tiles(tiles, kStripMaxRun, 2 * ncu, segs, rest);
    const int64_t W = 8, rows = (int64_t)segs.size() + (int64_t)rest.size();
    *count = rows;
    if (!out) return MOGP_OK;
    if (cap < rows * W) return fail(MOGP_EINVAL, "mogp_strip_plan: the output holds fewer than 8 * count numbers");
    int64_t* o = out;
    for (const GSeg& g : segs) { const int64_t r[8] = {1, g.r0, g.c0, g.n, g.pair, g.diag, MOGP_GT, MOGP_GT}; std::copy(r, r + W, o); o += W; }
    for (const GTile& t : rest) { const int64_t r[8] = {0, t.r0, t.c0, 1, t.pair, (t.flags & GT_DIAG) ? 1 : 0, t.nr, t.nc}; std::copy(r, r + W, o); o += W; }
    return MOGP_OK;
}

int mogp_model_flow_diag(mogp_model* m, unsigned* out8) {
    if (!m || !out8) return fail(MOGP_EINVAL, "mogp_model_flow_diag: null argument");
    int rc;
    if ((rc = use_device(m->ctx))) return rc;
    std::memset(out8, 0, 8 * sizeof(unsigned));
    if (!m->k.flow_diag.p) return MOGP_OK;
    HIP_TRY(hipStreamSynchronize(m->st));
    HIP_TRY(hipMemcpy(out8, m->k.flow_diag.p, FLOW_DIAG_WORDS * sizeof(unsigned), hipMemcpyDeviceToHost));
    return MOGP_OK;
}

int mogp_comm_selftest(mogp_ctx* ctx, int* ranks_seen, int* rank_sum) {
    if (!ctx || !ranks_seen || !rank_sum) return fail(MOGP_EINVAL, "mogp_comm_selftest: bad argument");
    int rc;
    if ((rc = use_device(ctx))) return rc;
    if ((rc = ctx_streams(ctx))) return rc;
    double h[2] = {1.0, (double)(ctx->comm.rank + 1)};
    double* d = nullptr;
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&d), sizeof(h)));
    hipError_t e = hipMemcpyAsync(d, h, sizeof(h), hipMemcpyHostToDevice, ctx->st);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->st);
    if (e == hipSuccess && (rc = comm_allreduce(ctx, d, 2, ctx->st)) == 0) {
        e = hipMemcpyAsync(h, d, sizeof(h), hipMemcpyDeviceToHost, ctx->st);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->st);
    }
    hipError_t e2 = hipFree(d); (void)e2;
    if (rc) return rc;
    HIP_TRY(e);
    *ranks_seen = (int)(h[0] + 0.5);
    *rank_sum = (int)(h[1] + 0.5);
    return MOGP_OK;
}

int mogp_dev_copy(void* dst, const void* src, int64_t bytes, int to_device) {
    if (!dst || !src || bytes < 0) return fail(MOGP_EINVAL, "mogp_dev_copy: bad argument");
    HIP_TRY(hipMemcpy(dst, src, (size_t)bytes, to_device ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost));
    if (to_device) HIP_TRY(hipStreamSynchronize(nullptr));          // see dev_upload
    return MOGP_OK;
}

int mogp_set_profiling(mogp_model* m, int on) {
    if (!m) return fail(MOGP_EINVAL, "mogp_set_profiling: model is null");
    m->profiling = on != 0;
    return MOGP_OK;
}

int mogp_stage_ms(mogp_model* m, double* ms, int64_t* gemm_launches, double* gemm_flops) {
    if (!m || !ms) return fail(MOGP_EINVAL, "mogp_stage_ms: bad argument");
    for (int i = 0; i < MOGP_ST_COUNT; ++i) ms[i] = m->ms[i];
    if (gemm_launches) *gemm_launches = m->gemm_launches;
    if (gemm_flops) *gemm_flops = m->gemm_flops;
    return MOGP_OK;
}

int mogp_model_fetch(mogp_model* m, int which, double* out) {
    if (!m || !out) return fail(MOGP_EINVAL, "mogp_model_fetch: bad argument");
    int rc;
    if ((rc = use_device(m->ctx))) return rc;
    const int64_t N = m->N, Npad = m->Npad;
    if (which == 3) {                           // dp/dr of the last gradient evaluation (Exact, Titsias, Snelson): what a user mean's backward needs
        if (!m->mean_w) return fail(MOGP_EINVAL, "mogp_model_fetch: dp/dr needs a gradient evaluation of the exact, Titsias or Snelson model as the last call on the handle");
        std::vector<double> h(Npad);
        HIP_TRY(hipMemcpy(h.data(), m->mean_w, Npad * sizeof(double), hipMemcpyDeviceToHost));
        for (int64_t pos = 0; pos < N; ++pos) out[m->sx.perm[pos]] = m->mean_w_scale * h[pos];
        return MOGP_OK;
    }
    if (which == 4) {                           // measurement: the two kernels of lfo.hip in the last profiled mogp_exact_cv(MOGP_EVAL_GRAD)
        if (!m->cv.timed) return fail(MOGP_EINVAL, "mogp_model_fetch: kernel times need a mogp_exact_cv with MOGP_EVAL_GRAD under mogp_model_set_profiling");
        float a = 0.f, b = 0.f;
        HIP_TRY(hipEventElapsedTime(&a, m->cv.ev[0], m->cv.ev[1]));
        HIP_TRY(hipEventElapsedTime(&b, m->cv.ev[2], m->cv.ev[3]));
        out[0] = a; out[1] = b;
        return MOGP_OK;
    }
    if (which == 2) {
        if (!m->have_W && !m->have_Kinv) return fail(MOGP_EINVAL, "mogp_model_fetch: no evaluation has completed yet");
        std::vector<double> h(Npad);
        HIP_TRY(hipMemcpy(h.data(), m->d_alpha.p, Npad * sizeof(double), hipMemcpyDeviceToHost));
        for (int64_t pos = 0; pos < N; ++pos) out[m->sx.perm[pos]] = h[pos];
        return MOGP_OK;
    }
    if (which == 0 && !m->have_W) return fail(MOGP_EINVAL, "mogp_model_fetch: no evaluation has completed yet");
    if (which == 1 && !m->have_Kinv) return fail(MOGP_EINVAL, "mogp_model_fetch: Kj^-1 needs an evaluation with MOGP_EVAL_GRAD");
    if (which != 0 && which != 1) return fail(MOGP_EINVAL, "mogp_model_fetch: which must be 0 .. 4");
    if (m->k.owned_rows) return fail(MOGP_EINVAL, "mogp_model_fetch: this rank of a sharded evaluation holds only its own tile rows of the matrix");
    if (which == 1 && m->kinv_sparse && !m->kinv_in_A) {
        // the evaluation formed only the tiles of Kj^-1 its gradient reads (kinv_plan): form all of them now, W^T W from the W it left
        m->kinv_sparse = false;
        GemmArgs g{};
        const double* Wp = m->w_in_Wm ? m->k.Wm.p : m->k.A.p;
        g.A = Wp; g.lda = Npad; g.a_kmajor = 1; g.B = Wp; g.ldb = Npad; g.b_kmajor = 1;
        g.C = m->k.B.p; g.ldc = Npad; g.alpha = 1.0; g.beta = 0.0;
        g.mode = GM_LAUUM; g.mt = g.nt = m->nb; g.K = (int)Npad;
        if ((rc = gemm_call(m, g, gemm_flops(g, nullptr)))) return rc;
        HIP_TRY(hipStreamSynchronize(m->st));
    }
    std::vector<double> h((size_t)Npad * Npad);
    const bool neg = (which == 1 && m->kinv_in_A);
    const double* src = which == 0 ? (m->w_in_Wm ? m->k.Wm.p : m->k.A.p) : (neg ? m->k.A.p : m->k.B.p);
    HIP_TRY(hipMemcpy(h.data(), src, h.size() * sizeof(double), hipMemcpyDeviceToHost));
    if (neg) for (auto& v : h) v = -v;
    for (int64_t a = 0; a < N; ++a)
        for (int64_t b = 0; b < N; ++b) {
            double v;
            if (which == 0) v = (b <= a) ? h[(size_t)a * Npad + b] : 0.0;                               // W = L^-1 (sorted order)
            else v = (b <= a) ? h[(size_t)a * Npad + b] : h[(size_t)b * Npad + a];                        // symmetric Kj^-1
            if (which == 0) out[a * N + b] = v;
            else out[m->sx.perm[a] * N + m->sx.perm[b]] = v;
        }
    return MOGP_OK;
}

}  // extern "C"
