// shard.hip -- the exact GP path on the sweep inversion (sweep.hip): the one-GPU sweep schedule of mogp_exact_eval and the evaluation and prediction sharded
// over the ranks of a communicator (comm.hip), as one call or as the staged mogp_shard_* protocol.  The prologue, the test side of a prediction and the
// not-positive-definite report are the exact path's (exact.hip).
#include "mogp_model.h"
#include <cstdlib>
#include <limits>

using namespace mogp;

// ---- gradient evaluation on the sweep inversion: Gram -> A = -Kj^-1 (one sweep) -> alpha, LML -------------------------
// sweep_eval_begin: uploads, Gram (lower, noise + jitter on the diagonal), padding.  m->sh_jabs keeps the absolute jitter.
static int sweep_eval_begin(mogp_model* m, const double* noise_var, const double* data_var, double jitter) {
    const int64_t N = m->N, Npad = m->Npad;
    GramArgs ga{};
    int rc = exact_begin(m, noise_var, data_var, jitter, ga, m->sh_jabs);
    if (rc) return rc;
    m->sh_dvar = data_var != nullptr;
    if (m->radial) return fail(MOGP_EINVAL, "the sweep / sharded evaluation does not take radial kinds (mogp_model_set_kinds)");
    const bool own = m->sh_n > 1 && m->own_n == m->sh_n && m->own_rank == m->sh_rank;
    if (own) ga.tiles = m->d_tiles_own.p;
    (own ? m->strip_own : m->strip).attach(ga);
    if ((rc = launch_gram(plan_cus(m->ctx), ga, (int)(own ? m->tiles_own.size() : m->tiles.size()), m->st))) return rc;
    // (owned-rows form: the padding rows lie in the last tile row -- its owner's business; everybody else gets them with the pivot block)
    if (!(m->sh_owned && m->sh_n > 1 && (m->nb - 1) % m->sh_n != m->sh_rank))
        if ((rc = launch_pad_identity(m->k.A.p, Npad, N, Npad, m->st))) return rc;
    return mark(m, 1);
}

// alpha (or this rank's partial sums of it) = -A y into m->d_alpha
static int sweep_eval_alpha(mogp_model* m) {
    const int64_t Npad = m->Npad;
    int rc;
    if ((rc = mark(m, 2))) return rc;
    if ((rc = mark(m, 3))) return rc;
    const int nchunks = (int)((Npad + 511) / 512);
    if ((rc = m->d_symv.ensure((size_t)(4 + nchunks) * Npad))) return rc;
    const int rm = m->sh_n > 1 ? m->sh_n : 0;
    if ((rc = launch_symv_lower(m->k.A.p, Npad, Npad, m->d_y.p, m->d_alpha.p, m->d_symv.p, -1.0, m->st, rm, m->sh_rank))) return rc;
    return mark(m, 4);
}

// scalars back: failure report, log-det (every rank factors every pivot block, so it is complete everywhere), y^T alpha
static int sweep_eval_scalars(mogp_model* m, double* lml, int64_t* info) {
    const int64_t N = m->N, Npad = m->Npad;
    const int nb = m->nb;
    const unsigned long long big = std::numeric_limits<unsigned long long>::max();
    std::vector<double> hl(nb), ha(Npad);
    unsigned long long hinfo = 0;
    HIP_TRY(hipMemcpyAsync(hl.data(), m->k.logdet.p, nb * sizeof(double), hipMemcpyDeviceToHost, m->st));
    HIP_TRY(hipMemcpyAsync(ha.data(), m->d_alpha.p, Npad * sizeof(double), hipMemcpyDeviceToHost, m->st));
    HIP_TRY(hipMemcpyAsync(&hinfo, m->d_info.p, sizeof(hinfo), hipMemcpyDeviceToHost, m->st));
    HIP_TRY(hipStreamSynchronize(m->st));
    if (hinfo == MOGP_INFO_CHAIN_TIMEOUT) return MOGP_RETRY_NO_CHAIN;
    if (hinfo != big) return report_not_pd(hinfo, info);
    double logdet = 0.0, ya = 0.0;
    for (double v : hl) logdet += v;
    for (int64_t i = 0; i < N; ++i) ya += m->hy[i] * ha[i];
    if (lml) *lml = -0.5 * (double)N * std::log(2.0 * M_PI) - logdet - 0.5 * ya;
    return 0;
}

namespace mogp { int eval_sweep(mogp_model* m, const double* noise_var, const double* data_var, double jitter, double* lml, double* jitter_abs, int64_t* info) {
    int rc;
    if ((rc = sweep_eval_begin(m, noise_var, data_var, jitter))) return rc;
    if (jitter_abs) *jitter_abs = m->sh_jabs;
    if ((rc = spd_sweep(m, m->k))) return rc;
    if ((rc = sweep_eval_alpha(m))) return rc;
    return sweep_eval_scalars(m, lml, info);
} }

extern "C" {

// A chain-kernel time-out inside a sharded evaluation cannot be repeated here (the other ranks are past their collectives).  One GPU per
// rank means nothing else competes for the reserved CUs, so it is not expected; the rank switches to the launch-per-step chain and reports.
static int sharded_rc(mogp_model* m, int rc) {
    if (rc != MOGP_RETRY_NO_CHAIN) return rc;
    if ((rc = chain_fallback(m))) return rc;
    return fail(MOGP_EHIP, "chain kernel: a hand-off timed out inside a sharded evaluation; this rank uses the launch-per-step chain from now on -- repeat the call on every rank");
}

// ---- sharded evaluation (one process per GPU; collectives are issued by the caller between these calls) --------------------
int mogp_shard_config(mogp_model* m, int rank, int nranks) {
    if (!m || nranks < 1 || rank < 0 || rank >= nranks) return fail(MOGP_EINVAL, "mogp_shard_config: bad argument");
    m->sh_rank = rank; m->sh_n = nranks;
    // MOGP_SHARD_OWNED: 1 (default) the owned-rows form for every group of more than one rank, 0 the replicated-matrix form of rounds 1-5,
    // 2 the owned-rows form for a one-rank group as well (its code path on one GPU: tests)
    static const int owned_mode = []() { const char* e = std::getenv("MOGP_SHARD_OWNED"); return e ? std::atoi(e) : 1; }();
    m->sh_owned = (owned_mode >= 1 && nranks > 1) || owned_mode >= 2;
    { int r__ = use_device(m->ctx); if (r__) return r__; r__ = ensure_system(m); if (r__) return r__; }
    if (nranks > 1 && (m->own_rank != rank || m->own_n != nranks)) {
        // each rank generates exactly the Gram / moment tiles it owns: a 64-row tile is kept if one of the (at most two)
        // 128-row tile rows it touches belongs to this rank; nothing else of the work matrix is ever read on this rank (sweep.hip)
        int rc;
        if ((rc = use_device(m->ctx))) return rc;
        m->tiles_own.clear();
        m->pair_start_own.assign(1, 0);
        for (size_t p = 0; p + 1 < m->pair_start.size(); ++p) {
            for (int t = m->pair_start[p]; t < m->pair_start[p + 1]; ++t) {
                const GTile& g = m->tiles[t];
                const int a = g.r0 / MOGP_TILE, b = (g.r0 + g.nr - 1) / MOGP_TILE;
                if (a % nranks == rank || b % nranks == rank) m->tiles_own.push_back(g);
            }
            m->pair_start_own.push_back((int)m->tiles_own.size());
        }
        if ((rc = m->d_tiles_own.ensure(std::max<size_t>(m->tiles_own.size(), 1)))) return rc;
        if ((rc = m->d_pair_start_own.ensure(m->pair_start_own.size()))) return rc;
        HIP_TRY(dev_upload(m->d_tiles_own.p, m->tiles_own.data(), m->tiles_own.size() * sizeof(GTile)));
        if ((rc = m->strip_own.build(m->tiles_own, plan_cus(m->ctx)))) return rc;
        HIP_TRY(dev_upload(m->d_pair_start_own.p, m->pair_start_own.data(), m->pair_start_own.size() * sizeof(int)));
        m->own_rank = rank; m->own_n = nranks;
    }
    if (m->k.owned_rows && (m->backed_rank != rank || m->backed_n != nranks)) {
        // physical memory under this rank's part of the work matrix: its tile rows (i % nranks == rank) and, where a channel does not start on a
        // 128-row boundary, the rows of a neighbouring tile row that one of its 64-row Gram tiles reaches into
        int rc;
        const size_t row_bytes = (size_t)m->Npad * sizeof(double);
        for (int i = rank; i < m->nb; i += nranks)
            if ((rc = m->k.Arows.back((size_t)i * MOGP_TILE * row_bytes, (size_t)MOGP_TILE * row_bytes))) return rc;
        if (nranks > 1)
            for (const GTile& g : m->tiles_own)
                if ((rc = m->k.Arows.back((size_t)g.r0 * row_bytes, (size_t)g.nr * row_bytes))) return rc;
        m->backed_rank = rank; m->backed_n = nranks;
    }
    return MOGP_OK;
}

int mogp_shard_begin(mogp_model* m, const double* noise_var, const double* data_var, double jitter, double* jitter_abs, int* nblocks) {
    if (!m || !nblocks) return fail(MOGP_EINVAL, "mogp_shard_begin: bad argument");
    int rc;
    if ((rc = begin_call(m, nullptr, false))) return rc;
    if ((rc = sweep_eval_begin(m, noise_var, data_var, jitter))) return rc;
    if ((rc = sweep_prepare(m, m->k))) return rc;
    if (jitter_abs) *jitter_abs = m->sh_jabs;
    *nblocks = sweep_nblocks(m->k);
    return MOGP_OK;
}

int mogp_shard_pack(mogp_model* m, int kb, void** send, void** recv, int64_t* count) {
    if (!m || !send || !recv || !count) return fail(MOGP_EINVAL, "mogp_shard_pack: bad argument");
    int rc;
    if ((rc = use_device(m->ctx))) return rc;
    double *s = nullptr, *r = nullptr;
    if ((rc = shard_pack(m, m->k, kb, &s, &r, count))) return rc;
    HIP_TRY(hipStreamSynchronize(m->st));           // the caller's collective runs outside this stream; the bulk stream keeps running
    *send = s; *recv = r;
    return MOGP_OK;
}

int mogp_shard_unpack(mogp_model* m, int kb) {
    if (!m) return fail(MOGP_EINVAL, "mogp_shard_unpack: bad argument");
    int rc;
    if ((rc = use_device(m->ctx))) return rc;
    return shard_unpack(m, m->k, kb);
}

int mogp_shard_block(mogp_model* m, int kb) {
    if (!m) return fail(MOGP_EINVAL, "mogp_shard_block: bad argument");
    int rc;
    if ((rc = use_device(m->ctx))) return rc;
    return sweep_block(m, m->k, kb);
}

int mogp_shard_alpha(mogp_model* m, void** vec, int64_t* count) {
    if (!m || !vec || !count) return fail(MOGP_EINVAL, "mogp_shard_alpha: bad argument");
    int rc;
    if ((rc = use_device(m->ctx))) return rc;
    if ((rc = sweep_finish(m, m->k))) return rc;
    if ((rc = sweep_eval_alpha(m))) return rc;
    HIP_TRY(hipStreamSynchronize(m->st));
    *vec = m->d_alpha.p; *count = m->Npad;
    return MOGP_OK;
}

int mogp_shard_finish(mogp_model* m, double* lml, double* moments, double* diagG, int64_t* info) {
    if (!m || !lml || !moments || !diagG) return fail(MOGP_EINVAL, "mogp_shard_finish: bad argument");
    int rc;
    if ((rc = use_device(m->ctx))) return rc;
    if (info) *info = 0;
    if ((rc = sweep_eval_scalars(m, lml, info))) return sharded_rc(m, rc);
    if ((rc = mark(m, 5))) return rc;
    if ((rc = moment_pass(m, m->k.A.p, -1.0, moments, diagG))) return rc;
    m->have_Kinv = true; m->kinv_in_A = true;
    return MOGP_OK;
}

// ---- the sharded evaluation as ONE call: the collectives are issued here, on the model's critical stream (comm.hip) ---------------------
static int sharded_inverse(mogp_model* m, const double* noise_var, const double* data_var, double jitter, double* jitter_abs) {
    mogp_comm& c = m->ctx->comm;
    int rc;
    if ((rc = mogp_shard_config(m, c.rank, c.n))) return rc;
    if ((rc = sweep_eval_begin(m, noise_var, data_var, jitter))) return rc;
    if ((rc = sweep_prepare(m, m->k))) return rc;
    if (jitter_abs) *jitter_abs = m->sh_jabs;
    const int nblocks = sweep_nblocks(m->k);
    m->sh_prof_blocks = 0;
    // Round 5: the exchange of a pivot block in TWO messages.  The serial part (Schur block inversion, 0.3 ms, repeated on every rank) needs the pivot
    // block's own tile rows only: 4 tiles of 128 x 512, 2 MB.  The rest of the panel -- the column part below the block and the row part left of it,
    // up to 134 MB at configs[2] -- is needed by the panel products behind it.  So: small message on the critical stream, large message on a
    // communication stream of its own (the context's third stream, idle in this schedule) UNDERNEATH the serial part; the critical stream waits
    // for it only where the panels start.  Both are collectives of the same communicator issued in the same order on every rank.
    // MOGP_SHARD_SPLIT=0: one message on the critical stream, as in rounds 1-4.  (A group of ONE rank runs the same schedule -- its messages are
    // copies -- so that the one-rank time measures what the schedule costs a rank, not a schedule of its own.)
    { const char* e = std::getenv("MOGP_SHARD_SPLIT"); m->sh_split = m->st3 && !(e && std::atoi(e) == 0); }
    { const char* e = std::getenv("MOGP_SHARD_FACTOR_ONCE"); m->sh_factor_once = c.n > 1 && e && std::atoi(e) != 0; }
    const int PEV = 10;                                  // timing events per pivot block
    if (m->profiling) {
        while ((int)m->sh_prof.size() < PEV * nblocks) { hipEvent_t e; HIP_TRY(hipEventCreate(&e)); m->sh_prof.push_back(e); }
        m->sh_prof_blocks = nblocks;
    }
    while ((int)m->sh_ev.size() < 2 * nblocks) { hipEvent_t e; HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming)); m->sh_ev.push_back(e); }
    hipStream_t qc = m->st3;
    for (int kb = 0; kb < nblocks; ++kb) {
        int64_t count = 0;
        hipEvent_t* pe = m->profiling ? m->sh_prof.data() + PEV * kb : nullptr;
        if (pe) HIP_TRY(hipEventRecord(pe[0], m->st));
        if (!m->sh_split) {
            double *send = nullptr, *recv = nullptr;
            if ((rc = shard_pack(m, m->k, kb, &send, &recv, &count))) return rc;
            if ((rc = comm_allgather(m->ctx, send, recv, count, m->st))) return rc;       // stream ordered: no host round trip with RCCL
            if ((rc = shard_unpack(m, m->k, kb))) return rc;
            if (pe) HIP_TRY(hipEventRecord(pe[1], m->st));
            if ((rc = sweep_block(m, m->k, kb, pe ? pe + 2 : nullptr))) return rc;
            continue;
        }
        hipEvent_t packed = m->sh_ev[2 * kb], rest_in = m->sh_ev[2 * kb + 1];
        int64_t count2 = 0;
        if ((rc = shard_pack_part(m, m->k, kb, 1, m->sh_send1, m->sh_recv1, &count, m->st))) return rc;
        if ((rc = shard_pack_part(m, m->k, kb, 2, m->sh_send, m->sh_recv, &count2, m->st))) return rc;     // (both read what the previous block's next-columns update left: this stream)
        HIP_TRY(hipEventRecord(packed, m->st));
        if ((rc = comm_allgather(m->ctx, m->sh_send1.p, m->sh_recv1.p, count, m->st))) return rc;
        if ((rc = shard_unpack_part(m, m->k, kb, 1, m->sh_recv1, m->st))) return rc;
        if (pe) HIP_TRY(hipEventRecord(pe[1], m->st));
        HIP_TRY(hipStreamWaitEvent(qc, packed, 0));
        if (pe) HIP_TRY(hipEventRecord(pe[6], qc));
        if ((rc = comm_allgather(m->ctx, m->sh_send.p, m->sh_recv.p, count2, qc))) return rc;
        if ((rc = shard_unpack_part(m, m->k, kb, 2, m->sh_recv, qc))) return rc;            // other ranks' rows only: nothing this rank's streams touch
        if (pe) HIP_TRY(hipEventRecord(pe[7], qc));
        HIP_TRY(hipEventRecord(rest_in, qc));
        if ((rc = sweep_block(m, m->k, kb, pe ? pe + 2 : nullptr, rest_in, pe ? pe + 8 : nullptr))) return rc;
    }
    if ((rc = sweep_finish(m, m->k))) return rc;
    if ((rc = sweep_eval_alpha(m))) return rc;                                         // owned-row partial sums of alpha
    return comm_allreduce(m->ctx, m->d_alpha.p, m->Npad, m->st);
}

int mogp_exact_eval_sharded(mogp_model* m, const double* noise_var, const double* data_var, double jitter,
                            double* lml, double* moments, double* diagG, double* trG, double* jitter_abs, int64_t* info) {
    if (!m || !lml || !moments || !diagG || !trG) return fail(MOGP_EINVAL, "mogp_exact_eval_sharded: bad argument");
    int rc;
    if ((rc = begin_call(m, info, false))) return rc;
    const int C = m->C, W = m->Wt, T = m->T, P = C * (C + 1) / 2;
    m->pivot_min = m->pivot_max = 0.0;
    if ((rc = sharded_inverse(m, noise_var, data_var, jitter, jitter_abs))) return rc;
    if ((rc = mark(m, 5))) return rc;
    if ((rc = moment_pass_device(m, m->k.A.p, -1.0))) return rc;                       // owned rows only
    if ((rc = comm_allreduce(m->ctx, m->d_moments.p, (int64_t)P * T * W, m->st))) return rc;
    if ((rc = comm_allreduce(m->ctx, m->d_diagG.p, C, m->st))) return rc;
    HIP_TRY(hipMemcpyAsync(moments, m->d_moments.p, (size_t)P * T * W * sizeof(double), hipMemcpyDeviceToHost, m->st));
    HIP_TRY(hipMemcpyAsync(diagG, m->d_diagG.p, C * sizeof(double), hipMemcpyDeviceToHost, m->st));
    if ((rc = sweep_eval_scalars(m, lml, info))) return sharded_rc(m, rc);             // syncs the stream
    if (m->sh_prof_blocks > 0) {
        for (hipStream_t q : {m->st2, m->st2u}) if (q) HIP_TRY(hipStreamSynchronize(q));
        if (m->st3) HIP_TRY(hipStreamSynchronize(m->st3));
        double acc6[6] = {0, 0, 0, 0, 0, 0};
        for (int kb = 0; kb < m->sh_prof_blocks; ++kb) {
            hipEvent_t* pe = m->sh_prof.data() + 10 * kb;
            // exchange on the critical stream | serial part (inversion + panels) | next-block columns | bulk | exchange on the communication stream | the critical stream's wait for it
            const int a_[6] = {0, 1, 2, 4, 6, 8}, b_[6] = {1, 2, 3, 5, 7, 9};
            for (int i = 0; i < 6; ++i) {
                if (i >= 4 && !m->sh_split) continue;
                float t = 0.f;
                if (hipEventElapsedTime(&t, pe[a_[i]], pe[b_[i]]) == hipSuccess) acc6[i] += t;
            }
        }
        for (int i = 0; i < 6; ++i) m->sh_ms[i] = acc6[i];
    }
    double tr = 0.0;
    for (int c = 0; c < C; ++c) tr += diagG[c];
    *trG = tr;
    m->have_Kinv = true; m->kinv_in_A = true;
    collect_timing(m, 6);
    return MOGP_OK;
}

// part[s] = sum over this rank's tile rows j (T[s][j*128 + k], the rows' share of K_s. Kj^-1) and k of Ksf[s][row(j)*128 + k] * T[s][j*128 + k]
// (one wave per test point; rows: the tile rows i = rank, rank + P, ...)
__global__ __launch_bounds__(256) void k_owned_quadform(const double* __restrict__ Ksf, int64_t ldk, const double* __restrict__ T, int64_t ldt, int64_t S,
                                                        int nown, int P, int rank, double* __restrict__ part) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t s = (int64_t)blockIdx.x * 4 + wave;
    if (s >= S) return;
    double acc = 0.0;
    for (int j = 0; j < nown; ++j) {
        const double* kr = Ksf + s * ldk + (int64_t)(rank + j * P) * MOGP_TILE;
        const double* tr = T + s * ldt + (int64_t)j * MOGP_TILE;
        acc = fma(kr[lane], tr[lane], acc);
        acc = fma(kr[lane + 64], tr[lane + 64], acc);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
    if (lane == 0) part[s] = acc;
}
__global__ void k_var_finish(const double* __restrict__ kdiag, const double* __restrict__ part, int64_t S, double* __restrict__ var) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < S) var[i] = kdiag[i] + part[i];               // (the work matrix holds MINUS Kj^-1)
}

int mogp_exact_predict_sharded(mogp_model* m, const double* noise_var, const double* data_var, double jitter,
                               const double* kss_diag, int64_t S, const double* Xs, double* mu, double* var, int64_t* info) {
    if (!m || !Xs || !mu || !var || !kss_diag || S <= 0) return fail(MOGP_EINVAL, "mogp_exact_predict_sharded: bad argument");
    int rc;
    if ((rc = begin_call(m, info, false))) return rc;
    mogp_comm& cm = m->ctx->comm;
    const int P = cm.n, rank = cm.rank, nb = m->nb;
    const int64_t Npad = m->Npad;
    // 1. the inversion, sharded exactly like the gradient evaluation: owned tile rows of -Kj^-1 (lower tiles, whole diagonal tiles) in k.A, alpha complete on every rank
    if ((rc = sharded_inverse(m, noise_var, data_var, jitter, nullptr))) return rc;
    double lml = 0.0;
    if ((rc = sweep_eval_scalars(m, &lml, info))) return sharded_rc(m, rc);            // failure report (not positive definite)
    // 2. Round 6: the predictive variance FROM THE OWNED ROWS, no all-gather of Kj^-1 (N^2 doubles, and the whole inverse on every rank, in rounds 3 - 5).
    //    k_ss - K_s. Kj^-1 K_.s is a quadratic form: with the rows a of Kj^-1 dealt out to the ranks,
    //        sum_ab K_sa Kinv_ab K_sb = sum over ranks, over their tile rows i, of  sum_{a in i} K_sa ( 2 sum_{b left of tile i} Kinv_ab K_sb + sum_{b in tile i} Kinv_ab K_sb )
    //    -- the strictly lower tiles count twice, the diagonal tile (held whole) once.  Every rank: the test Gram K_sf for ALL test points, one task-list GEMM
    //    T[:, tile row] = K_sf[:, left of it] A[row, left of it]^T (x 2) behind one for the diagonal tiles, a row-wise dot, and ONE all-reduce of S doubles.
    TestSide ts; GramArgs ga{};
    if ((rc = test_side(m, S, Xs, kss_diag, 0, m->st, ts, ga))) return rc;
    const SortedX& ss = ts.ss;
    const int64_t Spad = ts.Spad;
    const int st = (int)(Spad / MOGP_TILE);
    const int nown = rank < nb ? (nb - rank + P - 1) / P : 0;                          // tile rows rank, rank + P, ...
    const int64_t ldt = (int64_t)std::max(nown, 1) * MOGP_TILE;
    if ((rc = m->d_Vt.ensure((size_t)Spad * ldt))) return rc;
    if ((rc = m->d_var.ensure(2 * Spad))) return rc;                                   // [variance | this rank's share of the quadratic form]
    // the two task lists: [diagonal tiles | strictly lower parts], longest k range first within each
    std::vector<GemmTask> tasks;
    for (int j = 0; j < nown; ++j)
        for (int t = 0; t < st; ++t) {
            const int64_t i = rank + (int64_t)j * P;
            GemmTask g{};
            g.a_off = (int64_t)t * MOGP_TILE * Npad + i * MOGP_TILE; g.b_off = i * MOGP_TILE * Npad + i * MOGP_TILE;
            g.c_off = (int64_t)t * MOGP_TILE * ldt + (int64_t)j * MOGP_TILE; g.kt = MOGP_TILE / 16; g.pad = 0;
            tasks.push_back(g);
        }
    const size_t ndiag = tasks.size();
    for (int j = nown - 1; j >= 0; --j)
        for (int t = 0; t < st; ++t) {
            const int64_t i = rank + (int64_t)j * P;
            if (i == 0) continue;
            GemmTask g{};
            g.a_off = (int64_t)t * MOGP_TILE * Npad; g.b_off = i * MOGP_TILE * Npad;
            g.c_off = (int64_t)t * MOGP_TILE * ldt + (int64_t)j * MOGP_TILE; g.kt = (int)(i * MOGP_TILE / 16); g.pad = 0;
            tasks.push_back(g);
        }
    if ((rc = m->d_pred_tasks.ensure(std::max<size_t>(tasks.size(), 1)))) return rc;
    if (!tasks.empty()) HIP_TRY(hipMemcpyAsync(m->d_pred_tasks.p, tasks.data(), tasks.size() * sizeof(GemmTask), hipMemcpyHostToDevice, m->st));
    HIP_TRY(hipMemsetAsync(m->d_var.p, 0, 2 * Spad * sizeof(double), m->st));
    if ((rc = launch_gram(plan_cus(m->ctx), ga, ts.ntiles, m->st, m->radial ? m->gate_kinds : 0))) return rc;
    if ((rc = launch_gemv_rows(m->d_Ksf.p, Npad, Spad, Npad, m->d_alpha.p, m->d_mu.p, m->st))) return rc;            // mu = K_sf alpha (alpha is complete on every rank)
    if (nown > 0) {
        GemmArgs g{};
        g.A = m->d_Ksf.p; g.lda = Npad; g.a_kmajor = 0; g.B = m->k.A.p; g.ldb = Npad; g.b_kmajor = 0;
        g.C = m->d_Vt.p; g.ldc = ldt; g.mode = GM_TASKS; g.mt = g.nt = 0; g.K = 0;
        g.alpha = 1.0; g.beta = 0.0; g.tasks = m->d_pred_tasks.p; g.ntasks = (int)ndiag;
        if ((rc = gemm_call(m, g, 2.0 * MOGP_TILE * MOGP_TILE * MOGP_TILE * (double)ndiag))) return rc;
        if (tasks.size() > ndiag) {
            double fl = 0.0;
            for (size_t k = ndiag; k < tasks.size(); ++k) fl += 2.0 * MOGP_TILE * MOGP_TILE * 16.0 * tasks[k].kt;
            g.alpha = 2.0; g.beta = 1.0; g.tasks = m->d_pred_tasks.p + ndiag; g.ntasks = (int)(tasks.size() - ndiag);
            if ((rc = gemm_call(m, g, fl))) return rc;
        }
        hipLaunchKernelGGL(k_owned_quadform, dim3((unsigned)((Spad + 3) / 4)), dim3(256), 0, m->st, m->d_Ksf.p, Npad, m->d_Vt.p, ldt, Spad, nown, P, rank,
                           m->d_var.p + Spad);
        HIP_TRY(hipGetLastError());
    }
    // 3. the ranks' shares of the quadratic form: one sum of S doubles
    if ((rc = comm_allreduce(m->ctx, m->d_var.p + Spad, Spad, m->st))) return rc;
    hipLaunchKernelGGL(k_var_finish, dim3((unsigned)((Spad + 255) / 256)), dim3(256), 0, m->st, m->d_kdiag.p, m->d_var.p + Spad, Spad, m->d_var.p);
    HIP_TRY(hipGetLastError());
    std::vector<double> hmu(Spad), hv(Spad);
    HIP_TRY(hipMemcpyAsync(hmu.data(), m->d_mu.p, Spad * sizeof(double), hipMemcpyDeviceToHost, m->st));
    HIP_TRY(hipMemcpyAsync(hv.data(), m->d_var.p, Spad * sizeof(double), hipMemcpyDeviceToHost, m->st));
    HIP_TRY(hipStreamSynchronize(m->st));
    scatter_by_perm(ss, hmu.data(), mu); scatter_by_perm(ss, hv.data(), var);
    m->have_Kinv = false; m->have_W = false;
    return MOGP_OK;
}

int mogp_shard_stage_ms(mogp_model* m, double* ms) {
    if (!m || !ms) return fail(MOGP_EINVAL, "mogp_shard_stage_ms: bad argument");
    for (int i = 0; i < 6; ++i) ms[i] = m->sh_ms[i];
    return MOGP_OK;
}

}  // extern "C"
