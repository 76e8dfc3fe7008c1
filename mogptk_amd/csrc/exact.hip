// exact.hip -- the exact GP path on one GPU, per evaluation:
//   Gram (lower tiles, noise + jitter fused on the diagonal) -> blocked Cholesky -> level-batched triangular inverse
//   -> alpha / log-det -> LAUUM (K^-1) -> gradient-moment pass -> a few hundred doubles back to the host,
// and the prediction on the factor.  What the entry points share is written once: begin_call, exact_begin, test_side, report_not_pd (also used by shard.hip), PinLayout, FactorPlan, retry_on_streams,
// grad_enqueue / grad_collect (the gradient outputs' way home) and held_out_eval (the one schedule of mogp_exact_loo and mogp_exact_cv).
#include "mogp_model.h"
#include <cstdlib>
#include <limits>

using namespace mogp;

// The ONE wait of an evaluation.  hipStreamSynchronize sleeps on an interrupt; on a shared, loaded host the wake-up is what the wall clock
// of a 13 ms evaluation then waits for.  Polling the stream costs one busy core for the duration and returns within microseconds.
static int wait_stream(hipStream_t st) {
    static const bool spin = !(std::getenv("MOGP_SPIN_WAIT") && std::atoi(std::getenv("MOGP_SPIN_WAIT")) == 0);
    if (!spin) { HIP_TRY(hipStreamSynchronize(st)); return 0; }
    for (;;) {
        const hipError_t e = hipStreamQuery(st);
        if (e == hipSuccess) return 0;
        if (e != hipErrorNotReady) return hip_fail(e, "hipStreamQuery", __FILE__, __LINE__);
    }
}

// events 7 .. 10 bracket the Gram and the moment tile kernels alone (handed to the launchers)
static hipEvent_t prof_event(mogp_model* m, int idx) {
    if (!m->profiling) return nullptr;
    while ((int)m->ev.size() <= idx) { hipEvent_t e; if (hipEventCreate(&e) != hipSuccess) return nullptr; m->ev.push_back(e); }
    return m->ev[idx];
}

// ---- which tiles of Kj^-1 a gradient evaluation needs ------------------------------------------------------------------------------------
// The gradient is 1/2 sum_ab (alpha_a alpha_b - Kinv_ab) dK_ab/dtheta.  The moment kernel (gram.hip:k_moments) drops a term in a 64 x 64
// tile when the smallest exponent it can reach there is below -50 (the rule the Gram build uses for K itself: gram.hip:stage_item_compute),
// so where ALL terms of a tile are dropped the entries of Kj^-1 under it are never read -- and the accumulation Kj^-1 = W^T W need not
// form them.  For stationary kernels on long series that is most of the matrix: at BASELINE configs[1] (2048 points per channel over
// [0, 100], spectral variances ~0.03: a support of +-10) 65 % of the 128 x 128 tiles, i.e. 22 % of all flops of the evaluation.
// The plan is made on the host from the same numbers the device uses (block centres and half spans, the term table) with a stricter
// threshold (52 instead of 50), so it can only keep MORE tiles than the kernel reads.  Exact: the dropped terms are below 2e-22 of a
// tile's peak either way.  MOGP_FULL_INVERSE=1 forms every tile; mogp_model_fetch(which = 1) completes a planned inverse on demand.
static void kinv_block_ranges(mogp_model* m) {
    std::vector<int> blk;
    tile_blocks(m->sx.off, m->C, blk);
    const int nblk = (int)blk.size() / 2, D = m->D;
    m->blk_cen.assign((size_t)D * nblk, 0.0); m->blk_half.assign((size_t)D * nblk, 0.0);
    for (int b = 0; b < nblk; ++b)
        for (int d = 0; d < D; ++d) {
            const double* x = m->sx.xs.data() + (size_t)d * m->sx.Mpad + blk[2 * b];
            double lo = x[0], hi = x[0];
            for (int i = 1; i < blk[2 * b + 1]; ++i) { lo = std::fmin(lo, x[i]); hi = std::fmax(hi, x[i]); }
            m->blk_cen[(size_t)d * nblk + b] = 0.5 * (lo + hi); m->blk_half[(size_t)d * nblk + b] = 0.5 * (hi - lo);
        }
}

static int kinv_plan(mogp_model* m, bool want) {
    static const bool full = std::getenv("MOGP_FULL_INVERSE") && std::atoi(std::getenv("MOGP_FULL_INVERSE")) != 0;
    m->kinv_sparse = false; m->kinv_fraction = 1.0;
    if (!want || full || m->sh_n > 1 || m->tiles.empty() || m->radial) return 0;      // (the e^-50 rule is the Gaussian's: other profiles decay more slowly)
    const int nb = m->nb, D = m->D, T = m->T, W = m->Wt;
    const int64_t ld = m->Npad;
    if (m->blk_cen.empty()) kinv_block_ranges(m);
    const int nblk = (int)(m->blk_cen.size() / std::max(D, 1));
    std::vector<char> need((size_t)nb * nb, 0);
    for (const GTile& t : m->tiles) {
        const double* tab = m->table.data() + (size_t)t.pair * T * W;
        bool read = false;
        for (int k = 0; k < T && !read; ++k) {
            const double* row = tab + (size_t)k * W;
            double emin = 0.0;
            for (int d = 0; d < D; ++d) {
                const double sd = (m->blk_cen[(size_t)d * nblk + t.rb] - m->blk_cen[(size_t)d * nblk + t.cb]) + row[2 + 2 * D + d];
                const double mu = std::fmax(0.0, std::fabs(sd) - m->blk_half[(size_t)d * nblk + t.rb] - m->blk_half[(size_t)d * nblk + t.cb]);
                emin += row[2 + d] * mu * mu;
            }
            read = !(0.5 * emin > 52.0);                      // NaN -> read
        }
        if (!read) continue;
        const int i0 = t.r0 / MOGP_TILE, i1 = (t.r0 + t.nr - 1) / MOGP_TILE, j0 = t.c0 / MOGP_TILE, j1 = (t.c0 + t.nc - 1) / MOGP_TILE;
        for (int i = i0; i <= i1; ++i) for (int j = j0; j <= j1; ++j) if (j <= i) need[(size_t)i * nb + j] = 1;
    }
    for (int i = 0; i < nb; ++i) need[(size_t)i * nb + i] = 1;            // the diagonal tiles always (trace term)
    std::vector<GemmTask> acc, lau;
    std::vector<int> prefix(nb + 1, 0);
    for (int i = 0; i < nb; ++i) {
        for (int j = 0; j <= i; ++j) {
            if (!need[(size_t)i * nb + j]) continue;
            GemmTask a;
            a.a_off = (int64_t)i * MOGP_TILE; a.b_off = (int64_t)j * MOGP_TILE; a.c_off = (int64_t)i * MOGP_TILE * ld + (int64_t)j * MOGP_TILE;
            a.kt = 4 * MOGP_TILE / 16; a.pad = i + 1;
            acc.push_back(a);
            GemmTask l;                                                     // LAUUM: sum over k >= 128 i of W[k, i]^T W[k, j]  (both k-major)
            l.a_off = (int64_t)i * MOGP_TILE * ld + (int64_t)i * MOGP_TILE; l.b_off = (int64_t)i * MOGP_TILE * ld + (int64_t)j * MOGP_TILE;
            l.c_off = a.c_off; l.kt = (int)((ld - (int64_t)i * MOGP_TILE) / 16); l.pad = 0;
            lau.push_back(l);
        }
        prefix[i + 1] = (int)acc.size();
    }
    const double frac = (double)acc.size() / ((double)nb * (nb + 1) / 2);
    m->kinv_fraction = frac;
    if (frac > 0.85) return 0;                                              // little to gain: the dense launches
    const bool same = acc.size() == m->kinv_acc_tasks.size() && (acc.empty() || std::memcmp(acc.data(), m->kinv_acc_tasks.data(), acc.size() * sizeof(GemmTask)) == 0);
    if (!same || m->d_kinv_acc.n < acc.size()) {
        int rc;
        if ((rc = m->d_kinv_acc.ensure(std::max<size_t>(acc.size(), 1)))) return rc;
        if ((rc = m->d_kinv_lauum.ensure(std::max<size_t>(lau.size(), 1)))) return rc;
        // (pageable source: the copy is staged before the call returns, so the vectors may be replaced afterwards)
        HIP_TRY(hipMemcpyAsync(m->d_kinv_acc.p, acc.data(), acc.size() * sizeof(GemmTask), hipMemcpyHostToDevice, m->st));
        HIP_TRY(hipMemcpyAsync(m->d_kinv_lauum.p, lau.data(), lau.size() * sizeof(GemmTask), hipMemcpyHostToDevice, m->st));
        HIP_TRY(hipStreamSynchronize(m->st));
        m->kinv_acc_tasks.swap(acc); m->kinv_lauum_tasks.swap(lau);
    }
    m->kinv_prefix.swap(prefix);
    m->kinv_sparse = true;
    return 0;
}

static int pin_ensure(mogp_model* m, size_t n) {
    if (n <= m->h_pin_n) return 0;
    if (m->h_pin) { hipError_t e = hipHostFree(m->h_pin); (void)e; m->h_pin = nullptr; m->h_pin_n = 0; }
    HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&m->h_pin), n * sizeof(double), hipHostMallocDefault));
    m->h_pin_n = n;
    return 0;
}
// The pinned block of an evaluation's scalars, in doubles: [nb log-det parts | nzz z^T z parts | pivot report | P T W moments | C diagG | 2 pivots], and behind
// `total` the slots of a held-out evaluation (mogp_exact_loo / mogp_exact_cv): [score | mu, Npad | var, Npad | pivot word of the folds' factorisations].  The ONE
// place that knows the order: factorize sizes and fills the evaluation's own part, grad_enqueue adds the moments, held_out_eval sizes and fills the held-out
// slots, factorize_finish reads the block behind the evaluation's one stream sync.
struct PinLayout {
    size_t nzz, logdet = 0, zz, info, moments, diagG, pivots, total, score, mu, var, fold_info;
    PinLayout(int nb, int64_t Npad, int C, int T, int Wt) : nzz((size_t)((Npad + 3) / 4)) {
        zz = (size_t)nb; info = zz + nzz; moments = info + 1; diagG = moments + (size_t)(C * (C + 1) / 2) * T * Wt; pivots = diagG + C; total = pivots + 2;
        score = total; mu = score + 1; var = mu + (size_t)Npad; fold_info = var + (size_t)Npad;
    }
    explicit PinLayout(const mogp_model* m) : PinLayout(m->nb, m->Npad, m->C, m->T, m->Wt) {}
    size_t held_out_total(bool folds) const { return fold_info + (folds ? 1 : 0); }      // (leave-one-out has no folds to report on)
};

namespace mogp {
int begin_call(mogp_model* m, int64_t* info, bool one_gpu) {
    m->mean_w = nullptr;
    if (int rc = use_device(m->ctx)) return rc;
    if (info) *info = 0;
    if (one_gpu) one_gpu_call(m);
    return 0;
}

int exact_begin(mogp_model* m, const double* noise_var, const double* data_var, double jitter, GramArgs& ga, double& jabs) {
    const int C = m->C;
    const int64_t N = m->N, Npad = m->Npad;
    if (m->T <= 0) return fail(MOGP_EINVAL, "mogp_model_set_terms must be called before an evaluation");
    if (!noise_var) return fail(MOGP_EINVAL, "noise_var is null");
    { int r__ = ensure_system(m); if (r__) return r__; }
    m->have_W = m->have_Kinv = false;
    m->gemm_ev_used = 0; m->gemm_launches = 0; m->gemm_flops = 0.0;

    // host scalars: mean of the diagonal for the relative jitter (reference gpr/model.py:244)
    double dsum = 0.0;
    if (!m->point_diag.empty()) {       // non-stationary kernels: the caller supplied K_diag per point (mogp_model_set_point_diag)
        for (int c = 0; c < C; ++c)
            for (int k = m->sx.off[c]; k < m->sx.off[c + 1]; ++k) dsum += m->point_diag[k] + noise_var[c];
    } else if (m->radial && m->point_kinds) {      // dot-product or gate rows and no diagonal from the caller: from the table and the kinds, point by point
        dsum = table_diag_points(m, m->sx);
        for (int c = 0; c < C; ++c) dsum += (double)(m->sx.off[c + 1] - m->sx.off[c]) * noise_var[c];
    } else
    for (int c = 0; c < C; ++c) dsum += (double)(m->sx.off[c + 1] - m->sx.off[c]) * (table_diag(m, c) + noise_var[c]);
    if (data_var) {
        std::vector<double> dv(Npad, 0.0);
        for (int64_t pos = 0; pos < N; ++pos) { dv[pos] = data_var[m->sx.perm[pos]]; dsum += dv[pos]; }
        { int r__ = m->d_dvar.ensure(Npad); if (r__) return r__; }
        HIP_TRY(hipMemcpyAsync(m->d_dvar.p, dv.data(), Npad * sizeof(double), hipMemcpyHostToDevice, m->st));      // (pageable source: staged before the call returns)
    }
    jabs = jitter * dsum / (double)N;
    HIP_TRY(hipMemcpyAsync(m->d_noise.p, noise_var, C * sizeof(double), hipMemcpyHostToDevice, m->st));
    static const unsigned long long big = std::numeric_limits<unsigned long long>::max();
    HIP_TRY(hipMemcpyAsync(m->d_info.p, &big, sizeof(big), hipMemcpyHostToDevice, m->st));
    int rc;
    if ((rc = mark(m, 0))) return rc;
    ga = GramArgs{};
    ga.tiles = m->d_tiles.p; ga.xr = m->d_x.p; ga.xc = m->d_x.p; ga.ldxr = ga.ldxc = Npad; ga.nrows = ga.ncols = N;
    if ((rc = m->ph_xx.prepare(m->sx.off, m->sx.off, C, m->T, Npad, Npad, m->st, ga.ph))) return rc;
    ga.table = m->d_table.p; ga.T = m->T; ga.D = m->D; ga.C = C; ga.W = m->Wt;
    ga.out = m->k.A.p; ga.ldo = Npad; ga.noise = m->d_noise.p; ga.dvar = data_var ? m->d_dvar.p : nullptr;
    ga.jitter_abs = jabs; ga.mirror = 0;
    if (m->radial) { ga.kind = m->d_kind.p; ga.shape = m->d_shape.p; }
    return 0;
}
}  // namespace mogp

// A hand-off inside the persistent chain kernel (chain.hip) timed out: its 13 workgroups were not all resident -- another process sharing the
// GPU holds part of the reserved CUs with its own chain kernel (two such kernels can each hold some of the 16 CUs and wait for the rest).
// Nothing is wrong with the data: drain the streams and repeat the evaluation on the launch-per-step chain, which this model keeps from now on.
namespace mogp { int chain_fallback(mogp_model* m) {
    if (m->flow_ran) {                           // the dataflow schedule (flow.hip) was on: drop IT first, the chain kernel stays
        // (round 5) ... for a while, not for good: a soak of configs[1] (tools/flow_soak.py) sees one stall of 60 - 900 ms in 2000 - 4000 evaluations on an
        // otherwise idle box -- every workgroup of every kernel of the process standing still, then going on -- and a model that stayed on the stream schedule
        // from its first time-out on trained 20 % slower for the rest of its life.  The stream schedule for the next `flow_backoff` evaluations, four times
        // as many after every further time-out (64, 256, ... 16384): a GPU that really is shared ends up there for good, a hiccup costs one repeated evaluation.
        m->no_flow = true; m->flow_ran = false;
        m->flow_timeouts++;
        m->flow_retry_at = m->n_fact + m->flow_backoff;
        m->flow_backoff = std::min(m->flow_backoff * 4, 16384);
        for (hipStream_t q : {m->st, m->st2, m->st3, m->st4, m->ctx->st5, m->st_priv}) if (q) HIP_TRY(hipStreamSynchronize(q));
        static bool said_flow = false;
        if (!said_flow) {
            said_flow = true;
            unsigned code = 0;                       // which wait gave up: 0x700 an idle workgroup of the dataflow kernel, 0x800 + k a hook of a private-stream launch, else a chain kernel's
            if (m->k.flow_flags.p && m->k.flow_cur && m->k.flow_cur->base_err > 0) { hipError_t e = hipMemcpy(&code, m->k.flow_flags.p + m->k.flow_cur->base_err, sizeof(code), hipMemcpyDeviceToHost); (void)e; }
            fprintf(stderr, "mogp: the dataflow kernel timed out (wait 0x%x; GPU shared with another process?); using the stream schedule for the next %d evaluations (said once)\n", code, (int)(m->flow_retry_at - m->n_fact));
            fprintf(stderr, "mogp: the host enqueued that evaluation in %.0f us (longest so far %.0f us)\n", m->flow_enqueue_us, m->flow_enqueue_us_max);
        }
        if (std::getenv("MOGP_FLOW_DEBUG")) { fprintf(stderr, "mogp: dataflow time-out %d of this model\n", m->flow_timeouts); flow_debug_dump(m); }
        return 0;
    }
    if (m->no_chain) return fail(MOGP_EHIP, "chain kernel: a hand-off timed out although the model is on the launch-per-step chain");
    m->no_chain = true;
    for (hipStream_t q : {m->st, m->st2, m->st3, m->st4, m->ctx->st5, m->st_priv}) if (q) HIP_TRY(hipStreamSynchronize(q));
    static bool said = false;
    if (!said) { said = true; fprintf(stderr, "mogp: the persistent chain kernel timed out (GPU shared with another process?); using the launch-per-step chain\n"); }
    return 0;
} }

// rc of an evaluation step; MOGP_RETRY_NO_CHAIN: a hand-off timed out -- chain_fallback drops the schedule that waited, then `again` repeats the entry point on streams
template <typename F> static int retry_on_streams(mogp_model* m, int rc, F again) {
    if (rc != MOGP_RETRY_NO_CHAIN) return rc;
    if ((rc = chain_fallback(m))) return rc;
    return again();
}

namespace mogp { int report_not_pd(unsigned long long hinfo, int64_t* info) {
    if (info) *info = (int64_t)hinfo;
    return fail(MOGP_ENOTPD, "linalg.cholesky: The factorization could not be completed because the input is not "
                             "positive-definite (the leading minor of order " + std::to_string(hinfo) + " is not positive-definite).");
} }

static int factorize_finish(mogp_model* m, const GramArgs& ga, double* lml, int64_t* info) {
    const int64_t N = m->N, Npad = m->Npad;
    const PinLayout pl(m);
    const unsigned long long big = std::numeric_limits<unsigned long long>::max();
    unsigned long long hinfo = 0;
    std::memcpy(&hinfo, m->h_pin + pl.info, sizeof(hinfo));
    int rc;
    if (hinfo == MOGP_INFO_CHAIN_TIMEOUT) return MOGP_RETRY_NO_CHAIN;      // the caller repeats the evaluation on the launch-per-step chain
    if (hinfo != big) {
        if (info) *info = (int64_t)hinfo;
        // distinguish NaN / Inf in the Gram from a plain indefinite matrix (reference prints which, gpr/model.py:249-252)
        int flag = 0;
        HIP_TRY(hipMemsetAsync(m->d_flag.p, 0, sizeof(int), m->st));
        if ((rc = launch_gram(plan_cus(m->ctx), ga, (int)m->tiles.size(), m->st, m->radial ? m->gate_kinds : 0))) return rc;
        if ((rc = launch_nonfinite_scan(m->k.A.p, Npad, N, m->d_flag.p, m->st))) return rc;
        HIP_TRY(hipMemcpyAsync(&flag, m->d_flag.p, sizeof(int), hipMemcpyDeviceToHost, m->st));
        HIP_TRY(hipStreamSynchronize(m->st));
        if (flag & 1) return fail(MOGP_ENONFINITE, "linalg.cholesky: kernel matrix has NaNs!");
        if (flag & 2) return fail(MOGP_ENONFINITE, "linalg.cholesky: kernel matrix has infinities!");
        return report_not_pd(hinfo, info);
    }
    m->pivot_min = m->h_pin[pl.pivots]; m->pivot_max = m->h_pin[pl.pivots + 1];
    double logdet = 0.0, zz = 0.0;
    for (int i = 0; i < m->nb; ++i) logdet += m->h_pin[pl.logdet + i];
    for (size_t i = 0; i < pl.nzz; ++i) zz += m->h_pin[pl.zz + i];
    if (lml) *lml = -0.5 * (double)N * std::log(2.0 * M_PI) - logdet - 0.5 * zz;
    m->have_W = !m->factor_only && !m->accurate_ran;     // (the accurate form keeps L, not W = L^-1)
    return 0;
}

// What a factorize() call is asked for.  Fused: the inverse streamed behind the Cholesky chain (potri.hip), as tile dataflow where available (flow.hip: also z and
// alpha).  Phases: POTRF, then TRTRI (the caller adds LAUUM) -- or, under mogp_model_set_accurate, the refined factor and substitutions.  FactorOnly: L alone; the
// caller (prediction) solves with L itself and the LML is not formed.
struct FactorPlan {
    enum Schedule { Fused, Phases, FactorOnly } schedule = Phases;
    bool defer = false;             // enqueue only -- the scalars travel to the pinned block asynchronously; factorize_finish() (after the caller's ONE stream sync) makes the LML / the failure report of them
    bool want_inverse = true;       // the accurate form: Kj^-1 too (an LML-only evaluation needs L, z and the log-determinant: not the N^2 fill and the N^3 solve nothing would read)
    bool refine = false;            // the factorisation keeps L's diagonal tiles and refines every panel against L_kk (Spd::keep_L, refine_panels); the accurate form implies it
    const int* gather = nullptr;    // the forecast (forecast.hip): device map [Npad], time position -> storage position -- Kj is factored in THAT order (FactorOnly, refine, no rhs_job; k.B is the scratch of the permutation)
};

// Gram + factorisation + inverse factor + alpha.  On return d_A holds W = L^-1, d_alpha = Kj^-1 y.
static int factorize(mogp_model* m, const double* noise_var, const double* data_var, double jitter, const FactorPlan& plan,
                     double* lml, double* jitter_abs, int64_t* info, GramArgs* ga_out = nullptr) {
    const bool fuse_inverse = plan.schedule == FactorPlan::Fused, factor_only = plan.schedule == FactorPlan::FactorOnly;
    const int64_t N = m->N, Npad = m->Npad;
    GramArgs ga{};
    double jabs = 0.0;
    int rc = exact_begin(m, noise_var, data_var, jitter, ga, jabs);
    if (rc) return rc;
    if (jitter_abs) *jitter_abs = jabs;
    m->n_fact++;
    if (m->no_flow && m->n_fact >= m->flow_retry_at) m->no_flow = false;        // the dataflow schedule gets another try (chain_fallback)
    m->factor_only = factor_only;
    ga.ev0 = prof_event(m, 7); ga.ev1 = prof_event(m, 8);
    m->strip.attach(ga);
    // Dataflow schedule: the first chain kernel and the first panel read the first 512 columns only, so the Gram matrix is built in two
    // launches -- those columns on this stream, the rest on the bulk stream in front of the dataflow kernel, i.e. UNDERNEATH the first chain
    // kernel (whose 240 us every workgroup of the dataflow kernel used to sit out after the whole Gram build).
    // (the prediction's dataflow schedule gains nothing from the split: 45.55 vs 45.59 ms at configs[3], it is throughput-bound)
    const bool split = fuse_inverse && flow_enabled(m, m->k) && !m->tiles_head.empty() && !m->tiles_tail.empty() && m->st2;
    if (split) {
        GramArgs gh = ga, gt = ga;
        gh.tiles = m->d_tiles_head.p; m->strip_head.attach(gh); gh.ev1 = nullptr;
        gt.tiles = m->d_tiles_tail.p; m->strip_tail.attach(gt); gt.ev0 = nullptr; gt.phases_ready = 1;
        if ((rc = launch_gram(plan_cus(m->ctx), gh, (int)m->tiles_head.size(), m->st, m->radial ? m->gate_kinds : 0))) return rc;
        if ((rc = launch_pad_identity(m->k.A.p, Npad, N, Npad, m->st))) return rc;
        if (!m->gram_ev) HIP_TRY(hipEventCreateWithFlags(&m->gram_ev, hipEventDisableTiming));
        HIP_TRY(hipEventRecord(m->gram_ev, m->st));
        HIP_TRY(hipStreamWaitEvent(m->st2, m->gram_ev, 0));
        if ((rc = launch_gram(plan_cus(m->ctx), gt, (int)m->tiles_tail.size(), m->st2, m->radial ? m->gate_kinds : 0))) return rc;       // spd_potri_flow enqueues the dataflow kernel behind it
        // ... and makes the private stream wait for this event before the first launch that reads beyond the first 512 columns (round 4: with
        // four processes on one GPU the next-diagonal update of block 0 ran BEFORE this launch had written its block: "not positive definite")
        if (!m->gram_tail_ev) HIP_TRY(hipEventCreateWithFlags(&m->gram_tail_ev, hipEventDisableTiming));
        HIP_TRY(hipEventRecord(m->gram_tail_ev, m->st2));
        m->k.tail_ready = m->gram_tail_ev;
    } else {
        if ((rc = launch_gram(plan_cus(m->ctx), ga, (int)m->tiles.size(), m->st, m->radial ? m->gate_kinds : 0))) return rc;
        if ((rc = launch_pad_identity(m->k.A.p, Npad, N, Npad, m->st))) return rc;
        if (plan.gather) {              // Kj into time order: A -> B through the map, the lower block triangle back into A; spd_potrf then runs as it stands
            if (!factor_only || !plan.refine || m->rhs_job) return fail(MOGP_EINVAL, "factorize: a gathered factorisation is the refined factor alone, on streams");
            if ((rc = launch_sym_gather(m->k.A.p, m->k.B.p, Npad, m->nb, N, plan.gather, m->st))) return rc;
            if ((rc = launch_sym_gather(m->k.B.p, m->k.A.p, Npad, m->nb, N, nullptr, m->st))) return rc;
            if ((rc = launch_pad_identity(m->k.A.p, Npad, N, Npad, m->st))) return rc;
        }
    }
    ga.ev0 = ga.ev1 = nullptr;
    if ((rc = mark(m, 1))) return rc;

    // every allocation of this evaluation BEFORE the co-operating kernels are enqueued
    // (the two pivot doubles and the accurate form's right-hand-side block included: a hipHostMalloc / hipMalloc behind the enqueue of kernels that
    // wait for each other is the stall mogp_ctx_create's comment describes)
    const PinLayout pl(m);
    if ((rc = pin_ensure(m, pl.total))) return rc;
    if ((rc = m->d_pivots.ensure(2))) return rc;
    if ((m->accurate || plan.gather) && (rc = m->acc_rhs.ensure((size_t)Npad * MOGP_TILE))) return rc;
    m->k.flow_used = false;                           // (mogp_model_schedule reports the LAST evaluation: set again by spd_potri_flow)
    m->flow_ran = false;                              // ... and chain_fallback decides from THIS evaluation which schedule to drop, not from an earlier one
    m->k.want_vec = fuse_inverse;                     // the dataflow schedule (flow.hip) also forms z = W y and alpha = W^T z
    m->k.vec_y = m->d_y.p; m->k.vec_z = m->d_z.p; m->k.vec_zz = m->d_zz.p; m->k.vec_part = m->d_alpha.p + Npad;
    // (round 6, measured and dropped -- profiles/r6_exact_illcond.txt: the refined factorisation followed by the phases schedule's TRTRI / LAUUM products instead of
    // the two substitutions repairs the LML (2e-10 at cond 7e7) but NOT the gradient (2.8e-4, the fast schedules' 2.0e-4; the substitutions: 5.9e-6): it is the
    // inverse formed through explicit block inverses that costs the gradient its digits, so Kj^-1 stays with trsm.hip here)
    const bool accurate = m->accurate && plan.schedule == FactorPlan::Phases;
    m->accurate_ran = accurate;
    m->k.keep_L = m->k.refine_panels = plan.refine || accurate;      // read by spd_potrf, for this factorisation only
    if (factor_only && m->rhs_job && flow_enabled(m, m->k)) rc = spd_potri_flow(m, m->k, m->rhs_job);      // the prediction: factor + substitute as dataflow
    else rc = fuse_inverse ? spd_potri_fused(m, m->k) : spd_potrf(m, m->k);
    m->k.keep_L = m->k.refine_panels = false;
    m->k.want_vec = false; m->k.tail_ready = nullptr;
    if (rc) return rc;
    if ((rc = mark(m, 2))) return rc;
    if (accurate) {
        // (round 5) The backward-stable form, for matrices outside the envelope of the fast schedules: the launch-per-step Cholesky with
        // every panel refined against L_kk (Spd::refine_panels), then Kj^-1 = L^-T (L^-1 I) by two blocked SUBSTITUTIONS (trsm.hip) instead of
        // products with explicit block inverses, z and alpha by the same substitution on a 128-column block.  2 1/3 N^3 flop at the solves' rate
        // instead of N^3 at the products', behind a launch-per-step factorisation: 43 ms against 10 at N = 8192 (12 factorisation, 24 the two solves in their triangular form, 10 the two vector solves).  mogp_model_set_accurate; the host side switches to it when the pivot range says so.
        // Round 6: (i) the matrix solve and the two vector solves (128 dependent leaf + update steps, ~10 ms at N = 8192, latency-bound) overlap -- the SMALL launches stay
        // on the main stream (highest priority), the matrix solve goes to the all-CU stream of normal priority: the other way round a 4-workgroup leaf waits until the
        // large launch's queued workgroups have drained (titsias.hip found the same in configs[4]); (ii) Kj^-1 = W^T W with W = L^-1 from ONE substitution (every column a
        // backward-stable solve) and one LAUUM-mode product at the matrix cores' rate, instead of a second substitution L^-T W.  42.7 -> 25 ms (profiles/r6_exact_illcond.txt).
        hipStream_t ms = (plan.want_inverse && m->st2u) ? m->st2u : m->st;
        if (plan.want_inverse) {
            if (ms != m->st) {
                while ((int)m->k.inv_ev.size() < 4) { hipEvent_t e; HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming)); m->k.inv_ev.push_back(e); }
                HIP_TRY(hipEventRecord(m->k.inv_ev[0], m->st));                  // the factor is complete
                HIP_TRY(hipStreamWaitEvent(ms, m->k.inv_ev[0], 0));
            }
            if ((rc = m->k.Wm.ensure((size_t)Npad * Npad))) return rc;
            HIP_TRY(hipMemsetAsync(m->k.Wm.p, 0, (size_t)Npad * Npad * sizeof(double), ms));      // (above its block diagonal W stays zero: flow.hip relies on it)
            if ((rc = launch_add_diag(m->k.Wm.p, Npad, Npad, 1.0, ms))) return rc;
            if ((rc = trsm_lower(m, m->k.A.p, Npad, m->nb, m->k.Wm.p, Npad, Npad, false, ms, true))) return rc;      // W = L^-1 I, lower block triangle only (trsm.hip: tri)
            GemmArgs g{};
            g.A = m->k.Wm.p; g.lda = Npad; g.a_kmajor = 1; g.B = m->k.Wm.p; g.ldb = Npad; g.b_kmajor = 1;
            g.C = m->k.B.p; g.ldc = Npad; g.alpha = 1.0; g.beta = 0.0; g.mode = GM_LAUUM; g.mt = g.nt = m->nb; g.K = (int)Npad;
            if ((rc = gemm_call(m, g, gemm_flops(g, nullptr), ms))) return rc;
            if (ms != m->st) HIP_TRY(hipEventRecord(m->k.inv_ev[1], ms));
        }
        HIP_TRY(hipMemsetAsync(m->acc_rhs.p, 0, (size_t)Npad * MOGP_TILE * sizeof(double), m->st));
        if ((rc = launch_copy2d(m->acc_rhs.p, MOGP_TILE, m->d_y.p, 1, Npad, 1, 1.0, m->st))) return rc;
        if ((rc = trsm_lower(m, m->k.A.p, Npad, m->nb, m->acc_rhs.p, MOGP_TILE, MOGP_TILE, false))) return rc;
        if ((rc = launch_copy2d(m->d_z.p, 1, m->acc_rhs.p, MOGP_TILE, Npad, 1, 1.0, m->st))) return rc;
        HIP_TRY(hipMemsetAsync(m->d_zz.p, 0, pl.nzz * sizeof(double), m->st));
        if ((rc = launch_gemv_rows(m->d_z.p, Npad, 1, Npad, m->d_z.p, m->d_zz.p, m->st))) return rc;       // z^T z into the first part
        if ((rc = trsm_lower(m, m->k.A.p, Npad, m->nb, m->acc_rhs.p, MOGP_TILE, MOGP_TILE, true))) return rc;
        if ((rc = launch_copy2d(m->d_alpha.p, 1, m->acc_rhs.p, MOGP_TILE, Npad, 1, 1.0, m->st))) return rc;
        if (plan.want_inverse && ms != m->st) HIP_TRY(hipStreamWaitEvent(m->st, m->k.inv_ev[1], 0));
    } else if (plan.schedule == FactorPlan::Phases && (rc = spd_trtri(m, m->k))) return rc;
    if ((rc = mark(m, 3))) return rc;

    // ---- z = W y, alpha = W^T z   (factor_only: the caller solves with L itself; the LML is not formed)
    if (factor_only) {
        HIP_TRY(hipMemsetAsync(m->d_zz.p, 0, pl.nzz * sizeof(double), m->st));
    } else if (!accurate) {
        const double* Wp = fuse_inverse ? m->k.Wm.p : m->k.A.p;
        m->w_in_Wm = fuse_inverse;
        if (fuse_inverse && m->k.flow_used && m->k.vec_done) {
            if ((rc = launch_flow_alpha_sum(m->k, m->d_alpha.p, m->st))) return rc;
        } else {
            if ((rc = launch_trmv_lower(Wp, Npad, Npad, m->d_y.p, m->d_z.p, m->d_zz.p, m->st))) return rc;
            if ((rc = launch_trmv_lower_t(Wp, Npad, Npad, m->d_z.p, m->d_alpha.p, m->st))) return rc;
        }
    }
    if (fuse_inverse && (rc = spd_potri_fused_finish(m, m->k))) return rc;
    if ((rc = mark(m, 4))) return rc;
    {   // test hook (tests/test_gpu_parity.py: the detour test): every dataflow evaluation reports a hand-off time-out, as if one of its waits had given up
        static const bool fault = std::getenv("MOGP_FLOW_FAULT") && std::atoi(std::getenv("MOGP_FLOW_FAULT")) != 0;
        static const unsigned long long timed_out = MOGP_INFO_CHAIN_TIMEOUT;
        if (fault && m->k.flow_used) HIP_TRY(hipMemcpyAsync(m->d_info.p, &timed_out, sizeof(timed_out), hipMemcpyHostToDevice, m->st));
    }

    // scalars back: [nb log-det parts][nzz z^T z parts][pivot report] through the pinned block (PinLayout), the factor's smallest and largest diagonal entry with them
    const int nzz = (int)pl.nzz;
    if ((rc = launch_pivot_range(m->k.invd.p, N, m->d_pivots.p, m->st))) return rc;
    HIP_TRY(hipMemcpyAsync(m->h_pin + pl.pivots, m->d_pivots.p, 2 * sizeof(double), hipMemcpyDeviceToHost, m->st));
    HIP_TRY(hipMemcpyAsync(m->h_pin + pl.logdet, m->k.logdet.p, m->nb * sizeof(double), hipMemcpyDeviceToHost, m->st));
    constexpr int zz_piece = 2048;
    for (int o = 0; o < nzz; o += zz_piece)               // in pieces of 16 KB: see mogp_ctx_create on larger device-to-host copies next to running co-operating kernels
        HIP_TRY(hipMemcpyAsync(m->h_pin + pl.zz + o, m->d_zz.p + o, std::min(zz_piece, nzz - o) * sizeof(double), hipMemcpyDeviceToHost, m->st));
    HIP_TRY(hipMemcpyAsync(m->h_pin + pl.info, m->d_info.p, sizeof(unsigned long long), hipMemcpyDeviceToHost, m->st));
    if (ga_out) *ga_out = ga;
    if (plan.defer) return 0;
    HIP_TRY(hipStreamSynchronize(m->st));
    return factorize_finish(m, ga, lml, info);
}

namespace mogp { void collect_timing(mogp_model* m, int last_mark) {
    if (!m->profiling) return;
    auto el = [&](int a, int b) { float t = 0.f; if (hipEventElapsedTime(&t, m->ev[a], m->ev[b]) != hipSuccess) t = 0.f; return (double)t; };
    std::fill(m->ms, m->ms + MOGP_ST_COUNT, 0.0);
    m->ms[MOGP_ST_GRAM] = el(0, 1);
    m->ms[MOGP_ST_POTRF] = el(1, 2);
    m->ms[MOGP_ST_TRTRI] = el(2, 3);
    m->ms[MOGP_ST_SOLVE] = el(3, 4);
    if (last_mark >= 6) { m->ms[MOGP_ST_LAUUM] = el(4, 5); m->ms[MOGP_ST_MOMENTS] = el(5, 6); }
    m->ms[MOGP_ST_TOTAL] = el(0, last_mark);
    if ((int)m->ev.size() > 8) m->ms[MOGP_ST_GRAM_KERNEL] = el(7, 8);
    if (last_mark >= 6 && (int)m->ev.size() > 10) m->ms[MOGP_ST_MOMENT_KERNEL] = el(9, 10);
    double gsum = 0.0;
    for (size_t i = 0; i + 1 < m->gemm_ev_used; i += 2) {
        float t = 0.f;
        if (hipEventElapsedTime(&t, m->gemm_ev[i], m->gemm_ev[i + 1]) == hipSuccess) gsum += t;
    }
    m->ms[MOGP_ST_GEMM_KERNEL] = gsum;
}

// gradient-moment pass over this rank's rows of Kj^-1 (all rows when not sharded): results in m->d_moments / m->d_diagG
int moment_pass_device(mogp_model* m, const double* kinv, double ksign) {
    const int C = m->C, D = m->D, W = m->Wt, T = m->T, P = C * (C + 1) / 2;
    const int64_t Npad = m->Npad;
    const int rm = m->sh_n > 1 ? m->sh_n : 0;
    const bool own = m->sh_n > 1 && m->own_n == m->sh_n && m->own_rank == m->sh_rank;
    int rc;
    MomentArgs ma{};
    ma.tiles = own ? m->d_tiles_own.p : m->d_tiles.p; ma.ntiles = (int)(own ? m->tiles_own.size() : m->tiles.size());
    ma.x = m->d_x.p; ma.ldx = Npad; ma.nrows = ma.ncols = m->N;
    if ((rc = m->ph_xx.prepare(m->sx.off, m->sx.off, C, T, Npad, Npad, m->st, ma.ph))) return rc;
    ma.table = m->d_table.p; ma.T = T; ma.D = D; ma.C = C; ma.W = W; ma.kinv = kinv; ma.kinv_sign = ksign; ma.ld = Npad; ma.alpha = m->d_alpha.p;
    ma.row_mod = rm; ma.row_rem = m->sh_rank;
    if (m->radial) { ma.kind = m->d_kind.p; ma.shape = m->d_shape.p; }
    ma.partial = m->d_partial.p;
    ma.phases_ready = 1;                       // ph_xx was filled by this evaluation's Gram launch: same inputs, same table
    ma.ev0 = prof_event(m, 9); ma.ev1 = prof_event(m, 10);
    if ((rc = launch_moments(plan_cus(m->ctx), ma, m->st, m->radial ? m->gate_kinds : 0))) return rc;
    if ((rc = launch_moment_reduce(m->d_partial.p, own ? m->d_pair_start_own.p : m->d_pair_start.p, P, T, W, D, m->d_moments.p, m->st))) return rc;
    if ((rc = launch_diagG(kinv, Npad, m->d_alpha.p, m->d_chan_off.p, C, m->d_diagG.p, m->st, ksign, rm, m->sh_rank))) return rc;
    if ((rc = mean_grad_enqueue(m, m->d_alpha.p, -1.0))) return rc;            // dp/dr = -alpha (nothing is launched without a mean table)
    return mark(m, 6);
}

int moment_pass(mogp_model* m, const double* kinv, double ksign, double* moments, double* diagG) {
    const int C = m->C, W = m->Wt, T = m->T, P = C * (C + 1) / 2;
    int rc;
    if ((rc = moment_pass_device(m, kinv, ksign))) return rc;
    HIP_TRY(hipMemcpyAsync(moments, m->d_moments.p, (size_t)P * T * W * sizeof(double), hipMemcpyDeviceToHost, m->st));
    HIP_TRY(hipMemcpyAsync(diagG, m->d_diagG.p, C * sizeof(double), hipMemcpyDeviceToHost, m->st));
    HIP_TRY(hipStreamSynchronize(m->st));
    return 0;
}

int test_side(mogp_model* m, int64_t S, const double* Xs, const double* kss_diag, int64_t extra_rows, hipStream_t st, TestSide& ts, GramArgs& ga, int R, bool point_diag) {
    const int C = m->C, D = m->D;
    const int64_t Npad = m->Npad;
    SortedX& ss = ts.ss;
    int rc;
    if ((rc = sort_inputs(Xs, S, D, C, MOGP_TILE, ss))) return rc;
    const int64_t Spad = ts.Spad = ss.Mpad, Srow = R * Spad + extra_rows;      // R row blocks of Spad rows each over ONE sorted copy of Xs (R = 1: a plain prediction)
    std::vector<GTile> pt;
    build_rect_tiles(ss.off, m->sx.off, C, pt);
    ts.ntiles = (int)pt.size();
    if ((rc = m->d_xs.ensure((size_t)D * Spad))) return rc;
    if ((rc = m->d_Ksf.ensure((size_t)Srow * Npad))) return rc;
    if ((rc = m->d_mu.ensure((size_t)R * Spad))) return rc;
    if ((rc = m->d_kdiag.ensure((size_t)R * Spad))) return rc;
    if ((rc = m->d_ptiles.ensure(std::max<size_t>(pt.size(), 1)))) return rc;
    std::vector<double> kd((size_t)R * Spad, 0.0);
    const bool per_point = point_diag || m->Wt > 2 + 3 * D || (m->radial && m->point_kinds);      // terms with an envelope, dot-product or gate rows (or the caller says so): kss_diag holds one value per test point (caller order)
    for (int r = 0; r < R; ++r) {                                                   // (block r's diagonal: row r of kss_diag, C or S values)
        const double* kr = kss_diag + (size_t)r * (per_point ? S : C);
        for (int c = 0; c < C; ++c)
            for (int pos = ss.off[c]; pos < ss.off[c + 1]; ++pos) kd[(size_t)r * Spad + pos] = per_point ? kr[ss.perm[pos]] : kr[c];
    }
    HIP_TRY(hipMemcpyAsync(m->d_xs.p, ss.xs.data(), (size_t)D * Spad * sizeof(double), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(m->d_kdiag.p, kd.data(), (size_t)R * Spad * sizeof(double), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(m->d_ptiles.p, pt.data(), pt.size() * sizeof(GTile), hipMemcpyHostToDevice, st));
    // padded rows/columns of Ksf must be zero: rows >= S and columns >= N are never written by the Gram kernel
    HIP_TRY(hipMemsetAsync(m->d_Ksf.p, 0, (size_t)Srow * Npad * sizeof(double), st));
    // K_sf = K(Xs, X)   (rows: test points, columns: training points; all C*C pairs, reference kernel.py:468-479 transposed)
    ga = GramArgs{};
    ga.tiles = m->d_ptiles.p; ga.xr = m->d_xs.p; ga.ldxr = Spad; ga.xc = m->d_x.p; ga.ldxc = Npad; ga.nrows = S; ga.ncols = m->N;
    if ((rc = m->ph_sx.prepare(ss.off, m->sx.off, C, m->T, Spad, Npad, st, ga.ph))) return rc;
    ga.table = m->d_table.p; ga.T = m->T; ga.D = D; ga.C = C; ga.W = m->Wt; ga.out = m->d_Ksf.p; ga.ldo = Npad;
    ga.noise = nullptr; ga.dvar = nullptr; ga.jitter_abs = 0.0; ga.mirror = 0;
    if (m->radial) { ga.kind = m->d_kind.p; ga.shape = m->d_shape.p; }
    return 0;
}
}  // namespace mogp

static const std::string& grad_path_env() {
    static const std::string grad_path = []() { const char* e = std::getenv("MOGP_GRAD_PATH"); return std::string(e ? e : ""); }();
    return grad_path;
}

// The factorisation of an evaluation on the POTRF path, and with `inverse` Kj^-1 (lower tiles, full diagonal tiles) in k.B behind it -- then
// ENQUEUED only: the caller adds its own passes, waits once and calls factorize_finish.  Three schedules of the same arithmetic
// (MOGP_GRAD_PATH = fused | phases overrides the choice; sweep is mogp_exact_eval's own):
//   fused   potri.hip: the inverse streamed behind the Cholesky chain.  Wins while the serial chain dominates: 15.1 vs 15.9 ms at
//           N = 8192, 20.1 vs 21.1 ms at N = 9216, even at N = 10240 -- the default up to 80 tile rows (112 as dataflow, below).
//   phases  POTRF, TRTRI, LAUUM one after the other: fewer, larger GEMM launches.  Wins once the evaluation is flop-bound
//           (38.8 vs 41.8 ms at N = 12288, 80.6 vs 90.1 ms at N = 16384, 569 vs 657 ms at N = 32768) -- the default above.
//   sweep   sweep.hip: single-sweep blocked inversion; slower on one GPU (47 evals/s at N = 8192) but with one panel
//           exchange per pivot block, which is what the sharded multi-GPU evaluation (mogp_shard_*) is built on.
// banded: the inverse may stop at the tiles the marginal likelihood's gradient reads (kinv_plan); a caller that reads every tile says false.
static int enqueue_inverse(mogp_model* m, const double* noise_var, const double* data_var, double jitter, bool inverse, bool banded,
                           double* lml, double* jitter_abs, int64_t* info, GramArgs& ga) {
    const std::string& grad_path = grad_path_env();
    int rc;
    if ((rc = ensure_system(m))) return rc;
    if ((rc = kinv_plan(m, inverse && banded && !m->accurate))) return rc;
    // round 4: as tile dataflow (flow.hip) the fused schedule also beats the phases at 81 .. 112 tile rows (configs[1]'s kernel, tools/r4_sizes.sh:
    // 19.3 vs 22.4 ms at N = 10240, 32.5 vs 35.9 at 12288, 41.0 vs 43.8 at 13312, 50.7 vs 53.0 at 14336; 76.6 vs 75.8 the other way at 16384); where
    // the dataflow kernel is not available (switched off, fallen back, a planned inverse) the stream form keeps its 80
    const int fused_max = flow_enabled(m, m->k) ? 112 : 80;
    const bool fused = inverse && !m->accurate && (grad_path == "fused" || (grad_path != "phases" && m->nb <= fused_max));
    FactorPlan plan;
    plan.schedule = fused ? FactorPlan::Fused : FactorPlan::Phases; plan.defer = inverse; plan.want_inverse = inverse;
    if ((rc = factorize(m, noise_var, data_var, jitter, plan, lml, jitter_abs, info, &ga))) return rc;
    if (!inverse) return 0;
    if (!fused && !m->accurate_ran && (rc = spd_lauum(m, m->k))) return rc;          // (the accurate form left Kj^-1 itself in k.B)
    return mark(m, 5);
}

// The gradient outputs of an evaluation on their way home.  grad_enqueue: d_moments and d_diagG into the pinned block, behind whatever pass filled them and in
// front of the evaluation's one wait.  grad_finish, after that wait: the trace in channel order, dp/dr for the mean table, the stage times up to mark 6;
// grad_collect: the two results out of the pinned block first.
static int grad_enqueue(mogp_model* m, const PinLayout& pl) {
    HIP_TRY(hipMemcpyAsync(m->h_pin + pl.moments, m->d_moments.p, (pl.diagG - pl.moments) * sizeof(double), hipMemcpyDeviceToHost, m->st));
    HIP_TRY(hipMemcpyAsync(m->h_pin + pl.diagG, m->d_diagG.p, m->C * sizeof(double), hipMemcpyDeviceToHost, m->st));
    return 0;
}
static void grad_finish(mogp_model* m, const double* diagG, double* trG) {
    double tr = 0.0;
    for (int c = 0; c < m->C; ++c) tr += diagG[c];
    *trG = tr;
    mean_grad_collect(m);
    collect_timing(m, 6);
}
static void grad_collect(mogp_model* m, const PinLayout& pl, double* moments, double* diagG, double* trG) {
    std::memcpy(moments, m->h_pin + pl.moments, (pl.diagG - pl.moments) * sizeof(double));
    std::memcpy(diagG, m->h_pin + pl.diagG, m->C * sizeof(double));
    grad_finish(m, diagG, trG);
}

// The held-out scores of the exact path are ONE schedule: the COMPLETE inverse of a gradient evaluation (the adjoint Kj^-1 E Kj^-1 reads every tile), the
// score's points pass, with gradients its adjoint where G = 1/2 (alpha alpha^T - Kj^-1) stands for the marginal likelihood (rho, S, -S S^T, the rank-two term;
// loo.hip) and the moment pass in the marginal likelihood's layout -- and score, mu, var and the gradient outputs home through the pinned block behind ONE wait.
// fold null: leave-one-out (loo.hip).  fold, the caller's labels: leave-fold-out (lfo.hip), which adds the fold lists to the workspace, the pivot word as it
// stands BEHIND the folds' own factorisations, and NaN for the points in no fold.  The two entry points have checked their arguments.
static int held_out_eval(mogp_model* m, const double* noise_var, const double* data_var, double jitter, int flags, const int32_t* fold, int64_t nfolds,
                         double* score, double* mu, double* var, double* moments, double* diagG, double* trG, double* jitter_abs, int64_t* info) {
    const bool grad = (flags & MOGP_EVAL_GRAD) != 0, folds = fold != nullptr;
    int rc;
    if ((rc = begin_call(m, info, true))) return rc;
    auto again = [&]() {                                      // the public entry point, with the same arguments
        return folds ? mogp_exact_cv(m, noise_var, data_var, jitter, flags, fold, nfolds, score, mu, var, moments, diagG, trG, jitter_abs, info)
                     : mogp_exact_loo(m, noise_var, data_var, jitter, flags, score, mu, var, moments, diagG, trG, jitter_abs, info);
    };
    // every allocation (and the fold lists) before the co-operating kernels are enqueued (see factorize): the score's workspace, and the pinned block with the
    // held-out slots behind the evaluation's own scalars
    if ((rc = ensure_system(m))) return rc;
    if ((rc = folds ? cv_workspace(m, fold, nfolds, grad) : loo_workspace(m, grad))) return rc;
    const PinLayout pl(m);
    if ((rc = pin_ensure(m, pl.held_out_total(folds)))) return rc;
    const int64_t N = m->N, Npad = m->Npad;
    GramArgs ga{};
    if ((rc = enqueue_inverse(m, noise_var, data_var, jitter, true, /*banded=*/false, nullptr, jitter_abs, info, ga))) return retry_on_streams(m, rc, again);
    if ((rc = held_out_points(m, m->k.B.p, folds, grad))) return rc;
    if (grad) {
        // S goes where the factorisation's own matrix was (k.A: the Gram matrix, then L or W): nothing reads it after alpha, and the next evaluation
        // builds it anew -- so the handle no longer holds W for mogp_model_fetch(0)
        m->have_W = false;
        if ((rc = held_out_adjoint(m, m->k.B.p, m->k.A.p, folds))) return rc;
        if ((rc = loo_moment_pass(m))) return rc;
        if ((rc = grad_enqueue(m, pl))) return rc;
    }
    const double* v = m->loo.vec.p;
    double* h = m->h_pin;
    HIP_TRY(hipMemcpyAsync(h + pl.score, v + LOO_SUM * Npad, sizeof(double), hipMemcpyDeviceToHost, m->st));
    HIP_TRY(hipMemcpyAsync(h + pl.mu, v + LOO_MU * Npad, N * sizeof(double), hipMemcpyDeviceToHost, m->st));
    HIP_TRY(hipMemcpyAsync(h + pl.var, v + LOO_VAR * Npad, N * sizeof(double), hipMemcpyDeviceToHost, m->st));
    if (folds) HIP_TRY(hipMemcpyAsync(h + pl.fold_info, m->d_info.p, sizeof(unsigned long long), hipMemcpyDeviceToHost, m->st));
    if ((rc = wait_stream(m->st))) return rc;
    if ((rc = factorize_finish(m, ga, nullptr, info))) return retry_on_streams(m, rc, again);
    if (grad) m->have_W = false;                              // (factorize_finish set it: k.A holds S now)
    if (folds) {
        unsigned long long finfo = 0;
        std::memcpy(&finfo, h + pl.fold_info, sizeof(finfo));
        if (finfo != std::numeric_limits<unsigned long long>::max()) {          // Kj itself factored: a fold's block of its inverse did not
            if (info) *info = (int64_t)(finfo - 1) / 256;
            return fail(MOGP_ENOTPD, "mogp_exact_cv: the block of Kj^-1 over fold " + std::to_string((finfo - 1) / 256) + " is not positive definite (pivot " +
                                     std::to_string((finfo - 1) % 256 + 1) + " of its factorisation): Kj is too ill-conditioned for this fold");
        }
        for (int64_t pos = 0; pos < N; ++pos)                 // a point in no fold has no prediction
            if (m->cv.label[pos] < 0) h[pl.mu + pos] = h[pl.var + pos] = std::numeric_limits<double>::quiet_NaN();
    }
    *score = h[pl.score];
    scatter_by_perm(m->sx, h + pl.mu, mu);
    scatter_by_perm(m->sx, h + pl.var, var);
    m->have_Kinv = true;                                      // complete and mirrored: mogp_model_fetch(1) copies it as it is
    m->kinv_in_A = false;
    if (!grad) { collect_timing(m, 5); return MOGP_OK; }
    grad_collect(m, pl, moments, diagG, trG);
    return MOGP_OK;
}

extern "C" {

int mogp_exact_eval(mogp_model* m, const double* noise_var, const double* data_var, double jitter, int flags,
                    double* lml, double* moments, double* diagG, double* trG, double* jitter_abs, int64_t* info) {
    if (!m) return fail(MOGP_EINVAL, "mogp_exact_eval: model is null");
    int rc;
    if ((rc = begin_call(m, info, true))) return rc;
    const std::string& grad_path = grad_path_env();
    const bool sweep = grad_path == "sweep" && (flags & MOGP_EVAL_GRAD);
    const bool grad = (flags & MOGP_EVAL_GRAD) != 0;
    GramArgs ga{};
    auto again = [&]() { return mogp_exact_eval(m, noise_var, data_var, jitter, flags, lml, moments, diagG, trG, jitter_abs, info); };
    if (grad && (!moments || !diagG || !trG)) return fail(MOGP_EINVAL, "mogp_exact_eval: gradient outputs are null");
    if (sweep) {
        if ((rc = ensure_system(m))) return rc;
        if ((rc = kinv_plan(m, false))) return rc;
        m->pivot_min = m->pivot_max = 0.0;                     // (the sweep reports no pivot range)
        if ((rc = eval_sweep(m, noise_var, data_var, jitter, lml, jitter_abs, info))) return retry_on_streams(m, rc, again);
    }
    else if ((rc = enqueue_inverse(m, noise_var, data_var, jitter, grad, /*banded=*/true, lml, jitter_abs, info, ga))) return retry_on_streams(m, rc, again);
    if (!grad) { collect_timing(m, 4); return MOGP_OK; }

    // K^-1: the sweep left -Kj^-1 in k.A; the POTRF path W^T W (lower tiles, full diagonal tiles) in k.B
    const double* kinv = sweep ? m->k.A.p : m->k.B.p;
    const double ksign = sweep ? -1.0 : 1.0;
    const PinLayout pl(m);
    if (sweep && (rc = mark(m, 5))) return rc;
    if (sweep) {
        if ((rc = moment_pass(m, kinv, ksign, moments, diagG))) return rc;
    } else {
        // everything of this evaluation is enqueued before the host waits ONCE: scalars and moments come back through the pinned block
        if ((rc = moment_pass_device(m, kinv, ksign))) return rc;
        if ((rc = grad_enqueue(m, pl))) return rc;
        if ((rc = wait_stream(m->st))) return rc;
        if ((rc = factorize_finish(m, ga, lml, info))) return retry_on_streams(m, rc, again);
    }
    m->have_Kinv = true;
    m->kinv_in_A = sweep;
    if (sweep) grad_finish(m, diagG, trG);
    else grad_collect(m, pl, moments, diagG, trG);
    return MOGP_OK;
}

// Kj as factorize() builds it in its unsplit branch -- the strip runs of m->strip on k_gram_strip2, the rest on k_gram<1>, the padding's identity --
// read back before anything factors it: numerics diagnostics (tests/test_spectral_sweep_gpu.py), no reference seam
int mogp_model_gram(mogp_model* m, const double* noise_var, const double* data_var, double jitter, double* K_out) {
    if (!m || !K_out) return fail(MOGP_EINVAL, "mogp_model_gram: null argument");
    int rc;
    if ((rc = begin_call(m, nullptr, true))) return rc;
    const int64_t N = m->N, Npad = m->Npad;
    GramArgs ga{};
    double jabs = 0.0;
    if ((rc = exact_begin(m, noise_var, data_var, jitter, ga, jabs))) return rc;
    m->strip.attach(ga);
    if ((rc = launch_gram(plan_cus(m->ctx), ga, (int)m->tiles.size(), m->st, m->radial ? m->gate_kinds : 0))) return rc;
    if ((rc = launch_pad_identity(m->k.A.p, Npad, N, Npad, m->st))) return rc;
    std::vector<double> h((size_t)Npad * Npad);
    HIP_TRY(hipMemcpyAsync(h.data(), m->k.A.p, h.size() * sizeof(double), hipMemcpyDeviceToHost, m->st));
    HIP_TRY(hipStreamSynchronize(m->st));
    for (int64_t a = 0; a < N; ++a)
        for (int64_t b = 0; b < N; ++b) K_out[a * N + b] = b <= a ? h[(size_t)a * Npad + b] : 0.0;
    return MOGP_OK;
}

int mogp_exact_loo(mogp_model* m, const double* noise_var, const double* data_var, double jitter, int flags,
                   double* loo, double* mu, double* var, double* moments, double* diagG, double* trG, double* jitter_abs, int64_t* info) {
    if (!m) return fail(MOGP_EINVAL, "mogp_exact_loo: model is null");
    if (!loo || !mu || !var) return fail(MOGP_EINVAL, "mogp_exact_loo: loo, mu or var is null");
    if ((flags & MOGP_EVAL_GRAD) && (!moments || !diagG || !trG)) return fail(MOGP_EINVAL, "mogp_exact_loo: gradient outputs are null");
    return held_out_eval(m, noise_var, data_var, jitter, flags, nullptr, 0, loo, mu, var, moments, diagG, trG, jitter_abs, info);
}

int mogp_exact_cv(mogp_model* m, const double* noise_var, const double* data_var, double jitter, int flags, const int32_t* fold, int64_t nfolds,
                  double* cv, double* mu, double* var, double* moments, double* diagG, double* trG, double* jitter_abs, int64_t* info) {
    if (!m) return fail(MOGP_EINVAL, "mogp_exact_cv: model is null");
    if (!fold || !cv || !mu || !var) return fail(MOGP_EINVAL, "mogp_exact_cv: fold, cv, mu or var is null");
    if ((flags & MOGP_EVAL_GRAD) && (!moments || !diagG || !trG)) return fail(MOGP_EINVAL, "mogp_exact_cv: gradient outputs are null");
    return held_out_eval(m, noise_var, data_var, jitter, flags, fold, nfolds, cv, mu, var, moments, diagG, trG, jitter_abs, info);
}

int mogp_model_loo_bytes(mogp_model* m, int64_t* bytes) {
    if (!m || !bytes) return fail(MOGP_EINVAL, "mogp_model_loo_bytes: bad argument");
    *bytes = (int64_t)((m->loo.G.n + m->loo.vec.n) * sizeof(double) + cv_bytes(m));
    return MOGP_OK;
}

// The rolling-origin forecast: Kj gathered into time order and factored once in the refined form (FactorPlan::gather), r gathered the same way,
// z = L^-1 r by substitution on a 128-column block as the accurate form has it, ONE pass over the rows of L for every cut (forecast.hip) and the 2 H N sums home
// through the pinned block behind the call's one wait.  The scores are added up here, in time order.
int mogp_exact_forecast(mogp_model* m, const double* noise_var, const double* data_var, double jitter, const int64_t* order, int H, const int64_t* cut,
                        double* score, double* mu, double* var, double* jitter_abs, int64_t* info) {
    if (!m) return fail(MOGP_EINVAL, "mogp_exact_forecast: model is null");
    if (!order || !cut || !score || !mu || !var) return fail(MOGP_EINVAL, "mogp_exact_forecast: order, cut, score, mu or var is null");
    if (H < 1 || H > MOGP_FORECAST_MAXH) return fail(MOGP_EINVAL, "mogp_exact_forecast: H = " + std::to_string(H) + " cuts per point, and a call takes 1 .. " + std::to_string(MOGP_FORECAST_MAXH));
    if (m->ctx->comm.kind != MOGP_COMM_NONE && m->ctx->comm.n > 1) return fail(MOGP_EINVAL, "mogp_exact_forecast: not sharded (the handle's context has a communicator of more than one rank)");
    const int64_t N = m->N, Npad = m->Npad;
    std::vector<int> storage(N, -1), map(Npad, -1);             // caller's row -> storage position; time position -> storage position
    for (int64_t pos = 0; pos < N; ++pos) storage[m->sx.perm[pos]] = (int)pos;
    std::vector<char> seen(N, 0);
    for (int64_t p = 0; p < N; ++p) {
        if (order[p] < 0 || order[p] >= N || seen[order[p]])
            return fail(MOGP_EINVAL, "mogp_exact_forecast: order is not a permutation of 0 .. N - 1: order[" + std::to_string(p) + "] = " + std::to_string(order[p]) +
                                     (order[p] < 0 || order[p] >= N ? " is out of range" : " appears twice"));
        seen[order[p]] = 1;
        map[p] = storage[order[p]];
    }
    std::vector<int> hcut((size_t)H * N);
    for (int h = 0; h < H; ++h)
        for (int64_t p = 0; p < N; ++p) {
            const int64_t c = cut[(size_t)h * N + p];
            if (c < -1 || c > p)
                return fail(MOGP_EINVAL, "mogp_exact_forecast: cut[h = " + std::to_string(h) + ", p = " + std::to_string(p) + "] = " + std::to_string(c) + ", and a cut is -1 (skipped) or 0 .. p");
            hcut[(size_t)h * N + p] = (int)c;
        }
    int rc;
    if ((rc = begin_call(m, info, true))) return rc;
    auto again = [&]() { return mogp_exact_forecast(m, noise_var, data_var, jitter, order, H, cut, score, mu, var, jitter_abs, info); };
    // every allocation and upload before the factorisation is enqueued (see factorize); the sums travel behind the evaluation's own scalars in the pinned block
    if ((rc = ensure_system(m))) return rc;
    const PinLayout pl(m);
    const size_t HN = (size_t)H * N;
    if ((rc = pin_ensure(m, pl.total + 2 * HN))) return rc;
    ForecastWork& f = m->fc;
    if ((rc = f.map.ensure(Npad))) return rc;
    if ((rc = f.cut.ensure((size_t)MOGP_FORECAST_MAXH * N))) return rc;
    if ((rc = f.sums.ensure((size_t)2 * MOGP_FORECAST_MAXH * N))) return rc;
    HIP_TRY(hipMemcpyAsync(f.map.p, map.data(), Npad * sizeof(int), hipMemcpyHostToDevice, m->st));          // (pageable sources: staged before the call returns)
    HIP_TRY(hipMemcpyAsync(f.cut.p, hcut.data(), HN * sizeof(int), hipMemcpyHostToDevice, m->st));
    GramArgs ga{};
    FactorPlan plan;
    plan.schedule = FactorPlan::FactorOnly; plan.defer = true; plan.refine = true; plan.gather = f.map.p;
    if ((rc = factorize(m, noise_var, data_var, jitter, plan, nullptr, jitter_abs, info, &ga))) return rc;
    // z = L^-1 r with L itself, r in time order
    HIP_TRY(hipMemsetAsync(m->acc_rhs.p, 0, (size_t)Npad * MOGP_TILE * sizeof(double), m->st));
    if ((rc = launch_gather_vec(m->d_y.p, m->d_z.p, N, Npad, f.map.p, m->st))) return rc;
    if ((rc = launch_copy2d(m->acc_rhs.p, MOGP_TILE, m->d_z.p, 1, Npad, 1, 1.0, m->st))) return rc;
    if ((rc = trsm_lower(m, m->k.A.p, Npad, m->nb, m->acc_rhs.p, MOGP_TILE, MOGP_TILE, false))) return rc;
    if ((rc = launch_copy2d(m->d_z.p, 1, m->acc_rhs.p, MOGP_TILE, Npad, 1, 1.0, m->st))) return rc;
    if ((rc = launch_forecast_rows(m->k.A.p, Npad, N, m->d_z.p, f.cut.p, H, f.sums.p, f.sums.p + HN, m->st))) return rc;
    double* hs = m->h_pin + pl.total;
    HIP_TRY(hipMemcpyAsync(hs, f.sums.p, 2 * HN * sizeof(double), hipMemcpyDeviceToHost, m->st));
    if ((rc = mark(m, 5))) return rc;
    if ((rc = wait_stream(m->st))) return rc;
    if ((rc = factorize_finish(m, ga, nullptr, info))) return retry_on_streams(m, rc, again);      // the pivot report: in time order
    collect_timing(m, 5);
    // y as the caller gave it: under a mean table hy0 holds it and hy the residual, so m_p = hy0 - hy
    const double nan = std::numeric_limits<double>::quiet_NaN();
    for (int h = 0; h < H; ++h) {
        double sum = 0.0;
        for (int64_t p = 0; p < N; ++p) {
            const size_t i = (size_t)h * N + p, o = (size_t)h * N + order[p];
            if (hcut[i] < 0) { mu[o] = var[o] = nan; continue; }
            const int s = map[p];
            const double r = m->hy[s], e = r - hs[i], v = hs[HN + i];
            mu[o] = (m->mean_on ? m->hy0[s] - r : 0.0) + hs[i];
            var[o] = v;
            sum += -0.5 * std::log(2.0 * M_PI * v) - 0.5 * e * e / v;
        }
        score[h] = sum;
    }
    return MOGP_OK;
}

// mean_w (caller order, may be null): the predictive mean is K_sf mean_w instead of K_sf Kj^-1 y (the Opper-Archambeau model, whose mean
// weights are variational parameters; its variance is the exact one with the per-point variances 1 / lambda^2)
// parts (may be null: ONE row block built from the model's own table, a plain prediction): R amplitude-masked tables (host, R x C x C x T x W; checked by
// mogp_exact_predict_parts) -- block p of [K_sf ; y^T] is K_p(Xs, X) from table p, the R blocks share the sorted Xs, the tile list, the factorisation and the ONE
// substitution; kss_diag, mu and var then hold R rows.  psi_same[p] (p >= 1): table p has the Psi column of table p - 1, so its launch keeps the phase tables.
// The row blocks of a call are one of two descriptions.  tables != null: block p is the Gram from table p (above).  jacobian (mogp_exact_predict_grad):
// block d is the Jacobian dK(Xs, X)/dx*_d of the model's OWN table in input dimension d, R = D, all blocks written by ONE launch (gram.hip:k_gram_dx); kss_diag
// then holds one value per block and test point whatever the table (D x S, caller order).  `full` with Jacobian blocks (mogp_exact_predict_grad_cov):
// `var` is the joint covariance of all D S derivatives, H - V V^T over the D Spad stacked rows, index ((a D + d) S + b) D + e; kss_diag is then not read
// by the result (the diagonal comes from the device's own H).
struct RowBlocks { int R; const double* tables; const char* psi_same; bool jacobian; };
static int predict_core(mogp_model* m, const double* noise_var, const double* data_var, double jitter,
                        const double* kss_diag, int64_t S, const double* Xs, int full,
                        double* mu, double* var, int64_t* info, const double* mean_w, const RowBlocks* blocks = nullptr) {
    int rc;
    if ((rc = begin_call(m, info, true))) return rc;
    const int R = blocks ? blocks->R : 1;
    const bool jac = blocks && blocks->jacobian;
    const RowBlocks* parts = blocks && blocks->tables ? blocks : nullptr;      // blocks that bring tables of their own
    if (jac && mean_w) return fail(MOGP_EINVAL, "predict_core: Jacobian row blocks have no mean weights");
    const size_t tab_n = (size_t)m->C * m->C * m->T * m->Wt;
    // Cholesky factor only: the predictive equations need V = L^-1 K_fs and z = L^-1 y, never L^-1 itself (reference gpr/model.py:470-472 solves).
    // Round 1 / 2a formed W = L^-1 (N^3/3 flop) and multiplied; here [V | z] comes from ONE blocked forward substitution, N^2 (S+1) flop,
    // streamed behind the factorisation: block column K is solved as soon as the factorisation's chain has finished block K.
    const int C = m->C, nb = m->nb;
    const int64_t Npad = m->Npad;
    hipStream_t sv = m->st3 ? m->st3 : m->st;                       // test Gram + substitution (bulk CUs, lowest priority)
    for (auto& e : m->pred_ev) if (!e) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    HIP_TRY(hipEventRecord(m->pred_ev[0], m->st));                  // whatever the model's stream still holds comes first
    HIP_TRY(hipStreamWaitEvent(sv, m->pred_ev[0], 0));
    TestSide ts; GramArgs ga{};
    if ((rc = test_side(m, S, Xs, kss_diag, MOGP_TILE, sv, ts, ga, R, jac))) return rc;   // one more tile row of K_sf: its first row carries y^T through the same solve
    const SortedX& ss = ts.ss;
    const int64_t Spad = ts.Spad, Sall = R * Spad, Srow = Sall + MOGP_TILE;          // R row blocks, the y^T tile row last
    if ((rc = m->d_Vt.ensure((size_t)Srow * Npad))) return rc;
    if ((rc = m->d_var.ensure(Sall))) return rc;
    if (parts) {
        if ((rc = m->d_parts.ensure(R * tab_n))) return rc;
        HIP_TRY(hipMemcpyAsync(m->d_parts.p, parts->tables, R * tab_n * sizeof(double), hipMemcpyHostToDevice, sv));      // (pageable source: staged before the call returns)
    }
    HIP_TRY(hipMemcpyAsync(m->d_Ksf.p + Sall * Npad, m->d_y.p, Npad * sizeof(double), hipMemcpyDeviceToDevice, sv));
    if (jac) {                                                       // block d: dK(Xs, X)/dx*_d, every block from the one launch
        if ((rc = launch_gram_dx(ga, ts.ntiles, Spad * Npad, sv))) return rc;
    } else
    for (int p = 0; p < R; ++p) {                                    // block p: K_p(Xs, X) from table p into its Spad rows
        GramArgs gp = ga;
        if (parts) { gp.table = m->d_parts.p + p * tab_n; gp.out = m->d_Ksf.p + (int64_t)p * Spad * Npad; gp.phases_ready = p > 0 && parts->psi_same[p]; }
        if ((rc = launch_gram(plan_cus(m->ctx), gp, ts.ntiles, sv, m->radial ? m->gate_kinds : 0))) return rc;
    }
    if (mean_w) {                                                    // mu = K_sf w, before the substitution consumes K_sf
        std::vector<double> hw(Npad, 0.0);
        for (int64_t pos = 0; pos < m->N; ++pos) hw[pos] = mean_w[m->sx.perm[pos]];
        if ((rc = m->d_z.ensure(Npad))) return rc;
        HIP_TRY(dev_upload(m->d_z.p, hw.data(), Npad * sizeof(double)));
        if ((rc = launch_gemv_rows(m->d_Ksf.p, Npad, Spad, Npad, m->d_z.p, m->d_mu.p, sv))) return rc;
    }

    // Round 4: factorisation AND substitution as ONE tile-dataflow schedule (flow.hip, the prediction's plan: panels, Schur updates, the solved block
    // X[:, K] = T[:, K] W_KK^T and the updates T[:, > K] -= X[:, K] L[> K, K]^T as tasks of the resident kernel, the chain kernels as producers) where the
    // dataflow kernel is available: the two sets of rank-512 launches on their streams got in each other's way like those of round 3's gradient schedule.
    // MOGP_FLOW_PREDICT=0: the stream form below.
    // From 48 tile rows on (CSM, S = N / 4, tools/r4_predict_sizes.py: N = 4096 3.9 vs 3.5 ms -- below, the chain sets the pace and the launch-per-step
    // chain of the stream form is the shorter one -- 8192 8.6 vs 9.5, 12288 21.1 vs 22.8, 16384 45.6 vs 47.8, 20480 86.3 vs 90.3).
    if ((rc = ensure_system(m))) return rc;                                                 // (flow_enabled looks at the system's tile count: a model's first call may be a prediction)
    const char* fpe = std::getenv("MOGP_FLOW_PREDICT");                                     // "0": never; "lo:hi": the range of tile rows (read per call: tests)
    int fp_lo = 48, fp_hi = 160;
    if (fpe && std::strchr(fpe, ':')) { fp_lo = std::atoi(fpe); fp_hi = std::atoi(std::strchr(fpe, ':') + 1); }
    else if (fpe) fp_hi = std::atoi(fpe);
    // mogp_model_set_accurate: the stream form with every panel of the factorisation and every solved block column refined once against L itself
    const bool acc = m->accurate;
    const bool as_flow = !acc && fp_hi > 0 && nb >= fp_lo && nb <= fp_hi && Srow / MOGP_TILE <= 4096 && flow_enabled(m, m->k) && !m->kinv_sparse;
    FlowRhs job{m->d_Ksf.p, m->d_Vt.p, (int)(Srow / MOGP_TILE), nullptr};
    if (as_flow) {
        HIP_TRY(hipEventRecord(m->pred_ev[1], sv));           // K_sf (and y^T in its last tile row) are in place
        job.ready = m->pred_ev[1];
        m->rhs_job = &job;
    }
    // the factorisation: enqueued on the model's streams, not waited for
    GramArgs gaK{};
    FactorPlan plan;
    plan.schedule = FactorPlan::FactorOnly; plan.defer = true; plan.refine = acc;
    rc = factorize(m, noise_var, data_var, jitter, plan, nullptr, nullptr, info, &gaK);
    m->rhs_job = nullptr;
    if (rc) return rc;
    const bool flowed = as_flow && m->k.flow_used;

    // X L^T = [K_sf ; y^T]  by block columns of 512 (right-looking):  X[:, K] = T[:, K] W_KK^T,  T[:, > K] -= X[:, K] L[> K, K]^T.
    // W_KK = L_KK^-1 of the 512 x 512 diagonal blocks comes from the tile inverses the factorisation leaves behind (wkk.hip).
    if (!flowed) {
        // The factorisation behind this branch is spd_potrf's (factorize takes the dataflow form only with m->rhs_job set, i.e. as_flow, and
        // spd_potri_flow sets flow_used wherever it succeeds): its outer blocks are these blocks and it has recorded sync_ev[2 kb] for every one.
        constexpr int OB = MOGP_OUTER, KD = OB * MOGP_TILE;
        const int nouter = (nb + OB - 1) / OB, mt = (int)(Srow / MOGP_TILE);
        Spd& w = m->k;
        if (w.Wd.n < (size_t)nouter * KD * KD) {             // tiles above the diagonal of a W_KK are never written and must be zero
            if ((rc = w.Wd.ensure((size_t)nouter * KD * KD))) return rc;
            HIP_TRY(hipMemsetAsync(w.Wd.p, 0, (size_t)nouter * KD * KD * sizeof(double), sv));
        }
        for (int kb = 0; kb < nouter; ++kb) {
            const int k0 = kb * OB, nk = std::min(OB, nb - k0), k1 = k0 + nk, rem = nb - k1;
            const int64_t c0 = (int64_t)k0 * MOGP_TILE;
            HIP_TRY(hipStreamWaitEvent(sv, w.sync_ev[2 * kb], 0));            // chain(kb): L[>= K, K] and the tile inverses of block K are final
            double* Wk = w.Wd.p + (int64_t)kb * KD * KD;
            if ((rc = launch_wkk(w.A.p + c0 * (Npad + 1), Npad, w.invd.p + (int64_t)k0 * MOGP_TILE * MOGP_TILE, nk, Wk, KD, sv))) return rc;
            GemmArgs g{};
            g.A = m->d_Ksf.p + c0; g.lda = Npad; g.a_kmajor = 0; g.B = Wk; g.ldb = KD; g.b_kmajor = 0;
            g.C = m->d_Vt.p + c0; g.ldc = Npad; g.alpha = 1.0; g.beta = 0.0;
            g.mode = GM_KHI_J; g.small = 1; g.mt = 2 * mt; g.nt = nk; g.K = nk * MOGP_TILE;        // 64 x 128 tiles: twice the workgroups of a launch that fills a quarter of the chip
            if ((rc = gemm_call(m, g, gemm_flops(g, nullptr), sv))) return rc;
            if (acc) {                 // X += (T - X L_KK^T) W_KK^T: the product with the explicit W_KK is only a first approximation of the solve (spd_potrf does the same to its panels)
                GemmArgs r1 = g;
                r1.A = m->d_Vt.p + c0; r1.B = w.A.p + c0 * (Npad + 1); r1.ldb = Npad; r1.C = m->d_Ksf.p + c0; r1.alpha = -1.0; r1.beta = 1.0;
                if ((rc = gemm_call(m, r1, gemm_flops(r1, nullptr), sv))) return rc;
                GemmArgs r2 = g;
                r2.A = m->d_Ksf.p + c0; r2.C = m->d_Vt.p + c0; r2.alpha = 1.0; r2.beta = 1.0;
                if ((rc = gemm_call(m, r2, gemm_flops(r2, nullptr), sv))) return rc;
            }
            if (rem > 0) {
                GemmArgs u{};
                u.A = m->d_Vt.p + c0; u.lda = Npad; u.a_kmajor = 0;
                u.B = w.A.p + (int64_t)k1 * MOGP_TILE * Npad + c0; u.ldb = Npad; u.b_kmajor = 0;
                u.C = m->d_Ksf.p + (int64_t)k1 * MOGP_TILE; u.ldc = Npad; u.alpha = -1.0; u.beta = 1.0;
                u.mode = GM_RECT; u.mt = mt; u.nt = rem; u.K = nk * MOGP_TILE;
                if ((rc = gemm_call(m, u, gemm_flops(u, nullptr), sv))) return rc;
            }
        }
        HIP_TRY(hipEventRecord(m->pred_ev[1], sv));
        HIP_TRY(hipStreamWaitEvent(m->st, m->pred_ev[1], 0));
    }
    // mu = V^T z: the rows of X against its last row (z^T)
    if (!mean_w && (rc = launch_gemv_rows(m->d_Vt.p, Npad, Sall, Npad, m->d_Vt.p + Sall * Npad, m->d_mu.p, m->st))) return rc;

    std::vector<double> hmu(Sall);
    HIP_TRY(hipMemcpyAsync(hmu.data(), m->d_mu.p, Sall * sizeof(double), hipMemcpyDeviceToHost, m->st));
    // a hand-off of the dataflow schedule timed out: again, on streams
    auto again = [&]() { return predict_core(m, noise_var, data_var, jitter, kss_diag, S, Xs, full, mu, var, info, mean_w, blocks); };
    if (!full) {
        if ((rc = launch_row_sqnorm_sub(m->d_Vt.p, Npad, Sall, Npad, m->d_kdiag.p, m->d_var.p, m->st))) return rc;
        std::vector<double> hv(Sall);
        HIP_TRY(hipMemcpyAsync(hv.data(), m->d_var.p, Sall * sizeof(double), hipMemcpyDeviceToHost, m->st));
        if ((rc = mark(m, 5))) return rc;                      // (profiling: MOGP_ST_TOTAL of a prediction is the device's span of the whole call)
        HIP_TRY(hipStreamSynchronize(m->st));
        if ((rc = factorize_finish(m, gaK, nullptr, info))) return retry_on_streams(m, rc, again);      // the pivot report of the factorisation
        collect_timing(m, 5);
        for (int p = 0; p < R; ++p) { scatter_by_perm(ss, hmu.data() + p * Spad, mu + p * S); scatter_by_perm(ss, hv.data() + p * Spad, var + p * S); }
        return MOGP_OK;
    }
    // full covariance: K_ss - V^T V   (reference gpr/model.py:476-478), block by block
    std::vector<GTile> st_tiles;
    std::vector<int> ps;
    build_sym_tiles(ss.off, C, st_tiles, ps);
    if (jac) {
        // the joint covariance of the derivative: H (every (d, e) block from ONE launch of k_gram_dxdx) less ONE product V V^T over all D Spad rows
        const size_t HH = (size_t)Sall * Sall;
        if ((rc = m->d_Kss.ensure(HH))) return rc;
        if ((rc = m->d_ptiles.ensure(st_tiles.size()))) return rc;
        HIP_TRY(hipMemsetAsync(m->d_Kss.p, 0, HH * sizeof(double), m->st));
        HIP_TRY(hipMemcpyAsync(m->d_ptiles.p, st_tiles.data(), st_tiles.size() * sizeof(GTile), hipMemcpyHostToDevice, m->st));
        ga.tiles = m->d_ptiles.p; ga.xc = m->d_xs.p; ga.ldxc = Spad; ga.ncols = S; ga.out = m->d_Kss.p; ga.ldo = Sall; ga.mirror = 0;
        if ((rc = m->ph_ss.prepare(ss.off, ss.off, C, m->T, Spad, Spad, m->st, ga.ph))) return rc;
        if ((rc = launch_gram_dxdx(ga, (int)st_tiles.size(), Spad, m->st))) return rc;
        GemmArgs c{};
        c.A = m->d_Vt.p; c.lda = Npad; c.a_kmajor = 0; c.B = c.A; c.ldb = Npad; c.b_kmajor = 0;
        c.C = m->d_Kss.p; c.ldc = Sall; c.alpha = -1.0; c.beta = 1.0;
        c.mode = GM_RECT; c.mt = c.nt = (int)(Sall / MOGP_TILE); c.K = (int)Npad; c.tasks = nullptr; c.ntasks = 0;
        if ((rc = gemm_call(m, c, gemm_flops(c, nullptr)))) return rc;
        std::vector<double> hc(HH);
        HIP_TRY(hipMemcpyAsync(hc.data(), m->d_Kss.p, HH * sizeof(double), hipMemcpyDeviceToHost, m->st));
        if ((rc = mark(m, 5))) return rc;
        HIP_TRY(hipStreamSynchronize(m->st));
        if ((rc = factorize_finish(m, gaK, nullptr, info))) return retry_on_streams(m, rc, again);
        collect_timing(m, 5);
        for (int d = 0; d < R; ++d) {
            scatter_by_perm(ss, hmu.data() + d * Spad, mu + d * S);
            for (int64_t a = 0; a < S; ++a)
                for (int e = 0; e < R; ++e) {
                    const double* row = hc.data() + ((size_t)d * Spad + a) * Sall + (size_t)e * Spad;
                    double* out = var + ((size_t)ss.perm[a] * R + d) * S * R + e;
                    for (int64_t b = 0; b < S; ++b) out[(size_t)ss.perm[b] * R] = row[b];
                }
        }
        return MOGP_OK;
    }
    const size_t SS = (size_t)Spad * Spad;
    if ((rc = m->d_Kss.ensure(R * SS))) return rc;
    if ((rc = m->d_ptiles.ensure(st_tiles.size()))) return rc;
    HIP_TRY(hipMemsetAsync(m->d_Kss.p, 0, R * SS * sizeof(double), m->st));
    HIP_TRY(hipMemcpyAsync(m->d_ptiles.p, st_tiles.data(), st_tiles.size() * sizeof(GTile), hipMemcpyHostToDevice, m->st));
    ga.tiles = m->d_ptiles.p; ga.xc = m->d_xs.p; ga.ldxc = Spad; ga.ncols = S; ga.out = m->d_Kss.p; ga.ldo = Spad; ga.mirror = 1;
    if ((rc = m->ph_ss.prepare(ss.off, ss.off, C, m->T, Spad, Spad, m->st, ga.ph))) return rc;
    for (int p = 0; p < R; ++p) {
        GramArgs gp = ga;
        if (parts) { gp.table = m->d_parts.p + p * tab_n; gp.out = m->d_Kss.p + p * SS; gp.phases_ready = p > 0 && parts->psi_same[p]; }
        if ((rc = launch_gram(plan_cus(m->ctx), gp, (int)st_tiles.size(), m->st, m->radial ? m->gate_kinds : 0))) return rc;
        GemmArgs c{};
        c.A = m->d_Vt.p + (int64_t)p * Spad * Npad; c.lda = Npad; c.a_kmajor = 0; c.B = c.A; c.ldb = Npad; c.b_kmajor = 0;
        c.C = m->d_Kss.p + p * SS; c.ldc = Spad; c.alpha = -1.0; c.beta = 1.0;
        c.mode = GM_RECT; c.mt = c.nt = (int)(Spad / MOGP_TILE); c.K = (int)Npad; c.tasks = nullptr; c.ntasks = 0;
        if ((rc = gemm_call(m, c, gemm_flops(c, nullptr)))) return rc;
    }
    std::vector<double> hc(R * SS);
    HIP_TRY(hipMemcpyAsync(hc.data(), m->d_Kss.p, hc.size() * sizeof(double), hipMemcpyDeviceToHost, m->st));
    if ((rc = mark(m, 5))) return rc;
    HIP_TRY(hipStreamSynchronize(m->st));
    if ((rc = factorize_finish(m, gaK, nullptr, info))) return retry_on_streams(m, rc, again);
    collect_timing(m, 5);
    for (int p = 0; p < R; ++p) {
        scatter_by_perm(ss, hmu.data() + p * Spad, mu + p * S);
        for (int64_t a = 0; a < S; ++a)
            for (int64_t b = 0; b < S; ++b) var[(size_t)p * S * S + ss.perm[a] * S + ss.perm[b]] = hc[p * SS + (size_t)a * Spad + b];
    }
    return MOGP_OK;
}

int mogp_exact_predict(mogp_model* m, const double* noise_var, const double* data_var, double jitter,
                       const double* kss_diag, int64_t S, const double* Xs, int full,
                       double* mu, double* var, int64_t* info) {
    if (!m || !Xs || !mu || !var || !kss_diag || S <= 0) return fail(MOGP_EINVAL, "mogp_exact_predict: bad argument");
    return predict_core(m, noise_var, data_var, jitter, kss_diag, S, Xs, full, mu, var, info, nullptr);
}

// The posterior of every addend of the model's covariance behind ONE factorisation and ONE substitution: predict_core with P row blocks.
int mogp_exact_predict_parts(mogp_model* m, const double* noise_var, const double* data_var, double jitter, int P, const double* part_tables,
                             const double* kss_diag, int64_t S, const double* Xs, int full, double* mu, double* var, int64_t* info) {
    if (!m || !part_tables || !Xs || !mu || !var || !kss_diag || S <= 0 || P <= 0) return fail(MOGP_EINVAL, "mogp_exact_predict_parts: bad argument (null pointer, S <= 0 or P <= 0)");
    if (m->T <= 0) return fail(MOGP_EINVAL, "mogp_model_set_terms must be called before an evaluation");
    if (m->ctx->comm.kind != MOGP_COMM_NONE && m->ctx->comm.n > 1) return fail(MOGP_EINVAL, "mogp_exact_predict_parts: not sharded (the handle's context has a communicator of more than one rank)");
    // a part's table is the model's but for the amplitudes and the bias of dot-product rows (their Psi slot): everything the phase tables, the kinds and the
    // shapes depend on is the model's own
    const int C = m->C, T = m->T, W = m->Wt;
    const size_t n = (size_t)C * C * T * W;
    std::vector<char> psi_same(P, 0);
    for (int p = 0; p < P; ++p) {
        const double* tp = part_tables + p * n;
        bool same = p > 0;
        for (int pair = 0; pair < C * C; ++pair)
            for (int t = 0; t < T; ++t) {
                const size_t row = ((size_t)pair * T + t) * W;
                const bool dot = m->radial && (m->hkind[(size_t)pair * T + t] & MOGP_KIND_MASK) == MOGP_KIND_DOT;
                if (!std::isfinite(tp[row])) return fail(MOGP_ENONFINITE, "mogp_exact_predict_parts: part " + std::to_string(p) + " has a non-finite amplitude");
                if (p > 0 && std::memcmp(tp + row + 1, tp - n + row + 1, sizeof(double)) != 0) same = false;
                for (int w = 1; w < W; ++w) {
                    if (w == 1 && dot) { if (!std::isfinite(tp[row + 1])) return fail(MOGP_ENONFINITE, "mogp_exact_predict_parts: part " + std::to_string(p) + " has a non-finite bias"); continue; }
                    if (std::memcmp(tp + row + w, m->table.data() + row + w, sizeof(double)) != 0)
                        return fail(MOGP_EINVAL, "mogp_exact_predict_parts: part " + std::to_string(p) + " differs from the model's table at pair (" + std::to_string(pair / C) + ", " +
                                                 std::to_string(pair % C) + "), row " + std::to_string(t) + ", column " + std::to_string(w) +
                                                 ": only amplitudes and the bias of dot-product rows may differ");
                }
            }
        psi_same[p] = same;
    }
    const RowBlocks parts{P, part_tables, psi_same.data(), false};
    return predict_core(m, noise_var, data_var, jitter, kss_diag, S, Xs, full, mu, var, info, nullptr, &parts);
}

// The posterior of df/dx_d at the test points: predict_core over D Jacobian row blocks [J_1 ; .. ; J_D ; y^T], J_d = dK(Xs, X)/dx*_d.
int mogp_exact_predict_grad(mogp_model* m, const double* noise_var, const double* data_var, double jitter,
                            const double* dkss_diag, int64_t S, const double* Xs, double* dmu, double* dvar, int64_t* info) {
    if (!m || !dkss_diag || !Xs || !dmu || !dvar || S <= 0) return fail(MOGP_EINVAL, "mogp_exact_predict_grad: bad argument (null pointer or S <= 0)");
    if (m->T <= 0) return fail(MOGP_EINVAL, "mogp_model_set_terms must be called before an evaluation");
    if (m->ctx->comm.kind != MOGP_COMM_NONE && m->ctx->comm.n > 1) return fail(MOGP_EINVAL, "mogp_exact_predict_grad: not sharded (the handle's context has a communicator of more than one rank)");
    if (m->radial)
        for (size_t k = 0; k < (size_t)m->C * m->C * m->T; ++k) {
            const int kd = m->hkind[k] & MOGP_KIND_MASK;
            const std::string row = "row " + std::to_string(k % m->T) + " of pair (" + std::to_string(k / m->T / m->C) + ", " + std::to_string(k / m->T % m->C) + ") is ";
            if (kd == MOGP_KIND_MATERN12) return fail(MOGP_EINVAL, "mogp_exact_predict_grad: " + row + "a Matern 1/2 (exponential) row (kind 2): its sample paths are not differentiable");
            if (kd == MOGP_KIND_WHITE) return fail(MOGP_EINVAL, "mogp_exact_predict_grad: " + row + "a white row (kind 10): its sample paths are not differentiable");
            if (kd == MOGP_KIND_GATE) return fail(MOGP_EINVAL, "mogp_exact_predict_grad: " + row + "a gate row (kind 8): its input derivative is not yet carried on the device");
            if (kd == MOGP_KIND_WDOT) return fail(MOGP_EINVAL, "mogp_exact_predict_grad: " + row + "a weighted-dot row (kind 9): its input derivative is not yet carried on the device");
        }
    const RowBlocks blocks{m->D, nullptr, nullptr, true};
    return predict_core(m, noise_var, data_var, jitter, dkss_diag, S, Xs, 0, dmu, dvar, info, nullptr, &blocks);
}

// The joint posterior covariance of df/dx over all test points and dimensions: mogp_exact_predict_grad's row blocks, factorisation and substitution,
// then H = d^2 K(Xs, Xs)/dx dx' from one launch of k_gram_dxdx less one product V V^T.  No dkss_diag: the diagonal is the device's own H at coincident inputs.
int mogp_exact_predict_grad_cov(mogp_model* m, const double* noise_var, const double* data_var, double jitter,
                                int64_t S, const double* Xs, double* dmu, double* dcov, int64_t* info) {
    if (!m || !Xs || !dmu || !dcov || S <= 0) return fail(MOGP_EINVAL, "mogp_exact_predict_grad_cov: bad argument (null pointer or S <= 0)");
    if (m->T <= 0) return fail(MOGP_EINVAL, "mogp_model_set_terms must be called before an evaluation");
    if (m->ctx->comm.kind != MOGP_COMM_NONE && m->ctx->comm.n > 1) return fail(MOGP_EINVAL, "mogp_exact_predict_grad_cov: not sharded (the handle's context has a communicator of more than one rank)");
    if ((int64_t)m->D * S > MOGP_GRAD_COV_ROWS)
        return fail(MOGP_EINVAL, "mogp_exact_predict_grad_cov: D * S = " + std::to_string((int64_t)m->D * S) + " stacked rows, and the joint covariance is limited to " +
                                 std::to_string(MOGP_GRAD_COV_ROWS) + " (half a gigabyte on the device and again on the host)");
    if (m->radial)                                                     // the refusals of mogp_exact_predict_grad, row by row
        for (size_t k = 0; k < (size_t)m->C * m->C * m->T; ++k) {
            const int kd = m->hkind[k] & MOGP_KIND_MASK;
            const std::string row = "row " + std::to_string(k % m->T) + " of pair (" + std::to_string(k / m->T / m->C) + ", " + std::to_string(k / m->T % m->C) + ") is ";
            if (kd == MOGP_KIND_MATERN12) return fail(MOGP_EINVAL, "mogp_exact_predict_grad_cov: " + row + "a Matern 1/2 (exponential) row (kind 2): its sample paths are not differentiable");
            if (kd == MOGP_KIND_WHITE) return fail(MOGP_EINVAL, "mogp_exact_predict_grad_cov: " + row + "a white row (kind 10): its sample paths are not differentiable");
            if (kd == MOGP_KIND_GATE) return fail(MOGP_EINVAL, "mogp_exact_predict_grad_cov: " + row + "a gate row (kind 8): its input derivative is not yet carried on the device");
            if (kd == MOGP_KIND_WDOT) return fail(MOGP_EINVAL, "mogp_exact_predict_grad_cov: " + row + "a weighted-dot row (kind 9): its input derivative is not yet carried on the device");
        }
    const std::vector<double> kappa((size_t)m->D * S, 0.0);            // (test_side uploads a prior diagonal per block; the full covariance does not read it)
    const RowBlocks blocks{m->D, nullptr, nullptr, true};
    return predict_core(m, noise_var, data_var, jitter, kappa.data(), S, Xs, 1, dmu, dcov, info, nullptr, &blocks);
}

// OpperArchambeau.predict_f (reference gpr/model.py:640-668):  mu = K_sf nu,  var = K_ss - K_sf (K + diag(1 / lambda^2))^-1 K_fs, no jitter
int mogp_oa_predict(mogp_model* m, const double* q_nu, const double* q_lambda, const double* kss_diag, int64_t S, const double* Xs, int full,
                    double* mu, double* var, int64_t* info) {
    if (!m || !q_nu || !q_lambda || !Xs || !mu || !var || !kss_diag || S <= 0) return fail(MOGP_EINVAL, "mogp_oa_predict: bad argument");
    std::vector<double> dv(m->N), zero(m->C, 0.0);
    for (int64_t i = 0; i < m->N; ++i) {
        if (!(q_lambda[i] > 0.0)) return fail(MOGP_EINVAL, "mogp_oa_predict: q_lambda must be positive");
        dv[i] = 1.0 / (q_lambda[i] * q_lambda[i]);
    }
    return predict_core(m, zero.data(), dv.data(), 0.0, kss_diag, S, Xs, full, mu, var, info, q_nu);
}

}  // extern "C"
