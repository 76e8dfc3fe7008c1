// titsias.hip -- the Titsias sparse variational bound and its gradient on the device (BASELINE.json configs[4]).
// Reference: gpr/model.py:700-724 (elbo), :730-765 (predict_f); the gradient replaces autograd through that code.
//
// Whitened, cancellation-free forms (A = Kuu + jitter mean(diag Kuu) I = L L^T, B = Kuf, s2 = sigma^2):
//   v = L^-1 B,  Qs = v v^T / s2 + I = Lq Lq^T,  Pq = Qs^-1,  t1 = Pq (v y),  beta = L^-T t1
//   ELBO      = -N/2 log 2pi - sum log Lq_kk - N log sigma - y^T y /(2 s2) + t1.(v y) /(2 s2^2) - (sum Kff_diag - tr Q)/(2 s2)
//   dELBO/dB  = L^-T (I - Pq) v / s2 + beta (y / s2^2 - B^T beta / s2^3)^T
//   dELBO/dA  = 1/2 L^-T (2 I - Pq - Qs) L^-1 - 1/2 beta beta^T / s2^2
// Everything that goes through K_uu^-1 is a triangular SOLVE with L (trsm.hip: blocked substitution, as the reference's
// solve_triangular at gpr/model.py:711,715): K_uu has condition number ~1e11 at configs[4] and products with an explicit L^-1 lose
// dELBO/dZ (12-19 % error; 4e-5 with solves -- tools/titsias_numerics.py).  The inner system Qs = I + v v^T / s2 is well conditioned:
// its inverse Pq is formed explicitly (Cholesky, triangular inverse, W^T W on the MFMA GEMM).  The two adjoints are contracted with
// the kernel derivatives by the dense-mode moment kernel, which also accumulates the gradient w.r.t. the inducing inputs.
#include "mogp_model.h"

#include <cmath>
#include <cstdlib>
#include <cstring>
#include <limits>

using namespace mogp;

#define RC(x) do { int r__ = (x); if (r__) return r__; } while (0)

// Common front end: sort Z, build tiles, Kuu -> W (in tw.a.A), Kuf -> tw.B, v -> tw.v, Qs -> tw.Qs, Wq (tw.q.A), Pq (tw.q.B, full),
// vy, t1 in tw.vec[0 : Mpad], tw.vec[Mpad : 2 Mpad].  Host scalars through `sc`.
struct TitsiasScalars { double logdet_q, yy, t1vy, t1t1, trPq, trQs, jit, ntot, kff; };

// sharded: this handle holds ONE SHARD of the training points (the ranks of the context's communicator hold the others; Z, sigma and the
// terms are the same everywhere).  Everything that sums over data points -- v v^T, v y, y^T y, N, sum K_ff,nn -- is all-reduced, after which
// every M x M quantity is the full model's on every rank (two collectives: Mpad^2 doubles and Mpad + 3).
static int titsias_front(mogp_model* m, int64_t M, const double* Z, double sigma, double jitter, SortedX& sz, TitsiasScalars& sc, int64_t* info,
                         bool sharded = false, const double* kff_diag = nullptr) {
    if (!(sigma > 0.0)) return fail(MOGP_EINVAL, "sigma must be positive");
    RC(sparse_kuu(m, M, Z, jitter, true, sz, &sc.jit));
    TitsiasWork& t = *m->tw;
    const int C = m->C;
    const bool env = m->Wt > 2 + 3 * m->D;                     // terms with an envelope on the input midpoint (MOHSM)
    const int64_t Mpad = t.Mpad, Npad = m->Npad;
    const int mt = (int)(Mpad / MOGP_TILE);
    // Kuf and its working copy on the side stream, underneath the (chain-bound) factorisation of Kuu
    hipStream_t side;
    RC(side_fork(m, t, &side));
    RC(sparse_kuf(m, t, sz, side, true, t.v.p));                                // t.v: the copy the solve below works in, written by the same kernel
    // (round 5, measured and dropped: the chain of this factorisation on the CU-masked private stream, so that its one-workgroup kernels do not share
    // a CU with the K_uf Gram waves -- configs[4] 39.7-39.9 vs 39.3-39.5 ms, bit-identical: the panel and next-column products of the chain are
    // slower on 16 CUs than the leaves gain)
    // Round 6: v = L^-1 B FOLLOWS the factorisation block row by block row instead of waiting for all of it.  Block row i of L is final behind the leaf of
    // tile column i (right-looking: the panels left of it were finished by the columns before), and the left-looking substitution needs exactly that row for
    // its step i -- so the substitution (M^2 N flop, 9.3 ms at configs[4]) runs on the side stream behind the K_uf Gram, waiting per step for the event the
    // factorisation records, and the factorisation's 16 x 7 dependent small launches (3.6 ms by themselves) run underneath it: the side stream is masked off
    // the reserved CUs, so the chain's one-workgroup kernels always find a free CU.  Measured at configs[4] (profiles/r6_cfg5_follow.txt): 38.3 against 39.7 ms
    // per step, ELBO and kernel gradients unchanged -- but NOT the default: on the masked stream the substitution's stream-K products split their k range over
    // 480 workgroups instead of 512, a different summation order, and dELBO/dZ -- which sits at the rounding floor of this conditioning (cond K_uu ~ 1e11) --
    // lands 2.62e-3 of the tensor from the 80-bit truth instead of 1.59e-3 (the reference's two runs: 1.44e-3, 1.93e-3).  Both are inside the scatter of the
    // reference itself; the test holds the device to "no further away than the reference", so the schedule that is there stays.  MOGP_TITSIAS_FOLLOW=1 switches this on.
    static const bool follow = std::getenv("MOGP_TITSIAS_FOLLOW") && std::atoi(std::getenv("MOGP_TITSIAS_FOLLOW")) != 0;
    const bool fl = follow && side != m->st && Npad / MOGP_TILE > 32;
    t.a.want_row_ev = fl;
    RC(spd_potrf(m, t.a));                                                      // its pivot report is read with the scalars at the end of this function
    t.a.want_row_ev = false;
    const double s2 = sigma * sigma;
    if (fl) {
        RC(trsm_lower(m, t.a.A.p, Mpad, mt, t.v.p, Npad, Npad, false, side, false, t.a.row_ev.data()));
        RC(side_join(m, t, side));
    } else {
        RC(side_join(m, t, side));
        RC(trsm_lower(m, t.a.A.p, Mpad, mt, t.v.p, Npad, Npad, false));          // v = L^-1 B   (reference gpr/model.py:711)
    }
    // Qs = v v^T / s2 + I, with v y (one memory-bound pass over v) underneath the compute-bound product
    double* vy = t.vec.p;
    RC(side_fork(m, t, &side));
    RC(launch_gemv_rows(t.v.p, Npad, Mpad, Npad, m->d_y.p, vy, side));
    RC(mm_lower_splitk(m, t, t.v.p, t.v.p, t.q.A.p, mt, Mpad, Npad, Npad, 1.0 / s2));
    RC(side_join(m, t, side));
    sc.yy = 0.0; for (int64_t i = 0; i < m->N; ++i) sc.yy += m->hy[i] * m->hy[i];
    sc.ntot = (double)m->N;
    sc.kff = 0.0;
    if (kff_diag && env) for (int64_t i = 0; i < m->N; ++i) sc.kff += kff_diag[i];                  // per training point
    else if (kff_diag) for (int c = 0; c < C; ++c) sc.kff += (double)(m->sx.off[c + 1] - m->sx.off[c]) * kff_diag[c];
    if (sharded) {
        RC(comm_allreduce(m->ctx, t.q.A.p, Mpad * Mpad, m->st));
        double hs[3] = {sc.yy, sc.ntot, sc.kff};
        RC(allreduce_vec_scalars(m, t, vy, Mpad, hs, 3));
        sc.yy = hs[0]; sc.ntot = hs[1]; sc.kff = hs[2];
    }
    RC(launch_add_diag(t.q.A.p, Mpad, Mpad, 1.0, m->st));
    HIP_TRY(hipMemcpyAsync(t.Qs.p, t.q.A.p, (size_t)Mpad * Mpad * sizeof(double), hipMemcpyDeviceToDevice, m->st));
    RC(launch_info_stash(m->d_info.p, m->st));              // Kuu's report (and a time-out of the wide solve above) -> info[1]; info[0] armed for Qs
    RC(spd_invert(m, t.q, "Q/sigma^2 + I", info, &t.Wq, true));                 // t.Wq = Lq^-1, t.q.B = Pq (lower)
    RC(launch_symmetrize(t.q.B.p, Mpad, Mpad, m->st));
    double* t1 = t.vec.p + Mpad;
    double* dg = t.vec.p + 2 * Mpad;                                            // diag Pq, diag Qs
    // t1 = Pq (v y): the explicit inverse plus ONE step of iterative refinement against Qs (see refined_apply)
    RC(launch_symmetrize(t.Qs.p, Mpad, Mpad, m->st));
    RC(refined_apply(m, t, t.q.B.p, t.Qs.p, vy, t1));
    RC(launch_get_diag(t.q.B.p, Mpad, Mpad, dg, m->st));
    RC(launch_get_diag(t.Qs.p, Mpad, Mpad, dg + Mpad, m->st));
    const int nbq = t.q.nb;
    std::vector<double> hv((size_t)4 * Mpad), hl(nbq);
    HIP_TRY(hipMemcpyAsync(hv.data(), t.vec.p, (size_t)4 * Mpad * sizeof(double), hipMemcpyDeviceToHost, m->st));
    HIP_TRY(hipMemcpyAsync(hl.data(), t.q.logdet.p, nbq * sizeof(double), hipMemcpyDeviceToHost, m->st));
    unsigned long long hinfo[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(hinfo, m->d_info.p, sizeof(hinfo), hipMemcpyDeviceToHost, m->st));
    HIP_TRY(hipStreamSynchronize(m->st));
    RC(spd_info_verdict(m, "Kuu", hinfo[1], info));                             // the one synchronisation of the forward part: both factorisations' reports
    RC(spd_info_verdict(m, "Q/sigma^2 + I", hinfo[0], info));
    sc.logdet_q = 0.0; for (double x : hl) sc.logdet_q += x;
    sc.t1vy = sc.t1t1 = sc.trPq = sc.trQs = 0.0;
    for (int64_t i = 0; i < M; ++i) {
        sc.t1vy += hv[Mpad + i] * hv[i]; sc.t1t1 += hv[Mpad + i] * hv[Mpad + i];
        sc.trPq += hv[2 * Mpad + i]; sc.trQs += hv[3 * Mpad + i];
    }
    return 0;
}

static int titsias_eval_impl(mogp_model* m, int64_t M, const double* Z, double sigma, double jitter, const double* kff_diag, int flags,
                             double* elbo, double* mom_uu, double* mom_uf, double* gZ, double* trGA, double* dsigma,
                             double* jitter_abs, int64_t* info, bool sharded) {
    if (m) m->mean_w = nullptr;                 // dp/dr of an earlier gradient evaluation: this call may overwrite or regrow its buffer (mogp_model_fetch 3)
    if (!m || !Z || !kff_diag || !elbo || M <= 0) return fail(MOGP_EINVAL, "mogp_titsias_eval: bad argument");
    RC(use_device(m->ctx));
    if (info) *info = 0;
    const int C = m->C, D = m->D, W = m->Wt, T = m->T, P = C * (C + 1) / 2;
    const int64_t Npad = m->Npad;
    const bool grad = (flags & MOGP_EVAL_GRAD) != 0;
    SortedX sz;
    TitsiasScalars sc;
    RC(titsias_front(m, M, Z, sigma, jitter, sz, sc, info, sharded, kff_diag));
    TitsiasWork& t = *m->tw;
    const int64_t Mpad = t.Mpad;
    const int mt = (int)(Mpad / MOGP_TILE), nt = (int)(Npad / MOGP_TILE);
    const double s2 = sigma * sigma;
    const double kff = sc.kff, Ntot = sc.ntot;                   // sums over ALL data points (all-reduced when the data is sharded)
    const double trQ = s2 * (sc.trQs - (double)M);
    *elbo = -0.5 * Ntot * std::log(2.0 * M_PI) - sc.logdet_q - Ntot * std::log(sigma) - 0.5 * sc.yy / s2
            + 0.5 * sc.t1vy / (s2 * s2) - 0.5 * (kff - trQ) / s2;
    if (jitter_abs) *jitter_abs = sc.jit;
    if (!grad) return sparse_timeout_check(m);
    if (!mom_uu || !mom_uf || !gZ || !trGA || !dsigma) return fail(MOGP_EINVAL, "mogp_titsias_eval: gradient outputs are null");

    // d ELBO / d s2, then d sigma  (tr(Pq Q) = s2 (M - tr Pq);  vy^T Pq Q Pq vy = s2 (t1.vy - t1.t1))
    const double ds2 = -0.5 * Ntot / s2 + 0.5 * ((double)M - sc.trPq) / s2 + 0.5 * sc.yy / (s2 * s2) - sc.t1vy / (s2 * s2 * s2)
                       + 0.5 * (sc.t1vy - sc.t1t1) / (s2 * s2 * s2) + 0.5 * (kff - trQ) / (s2 * s2);
    *dsigma = 2.0 * sigma * ds2;

    RC(t.GB.ensure((size_t)Mpad * Npad)); RC(t.E.ensure((size_t)Mpad * Mpad)); RC(t.R.ensure((size_t)Mpad * Mpad));
    RC(t.GA.ensure((size_t)Mpad * Mpad));
    double* t1 = t.vec.p + Mpad;
    double* beta = t.vec.p + 4 * Mpad;            // [Mpad] (+ chunk scratch behind it, see launch_trmv_lower_t)
    double* dga = t.vec.p + 2 * Mpad;             // reuse: diag of GA
    double* btb = t.vec.p + 8 * Mpad;             // [Npad]
    double* r = btb + Npad;                       // [Npad]
    // GA = 1/2 L^-T E L^-1 (symmetric), E = 2I - Pq - Qs: T1 = L^-T E in place, then L^-T T1^T, then the lower triangle of the symmetrised half.
    // M x M only, on the side stream underneath the M x N work below.  Round 6, measured and removed: the adjoint chain (~70 launches of 4 .. 200
    // workgroups) on the MAIN stream (highest priority) and the M x M x N product on the all-CU stream of normal priority -- on the lower-priority side
    // stream a 4-workgroup leaf that arrives while the product's 12 000 workgroups are queued is not dispatched until the product has drained, 12.8 ms for
    // a 67 us kernel in every configs[4] evaluation (profiles/r5_cfg5_bench_kernel_stats.csv), i.e. the chain runs BEHIND the product, not under it: 42.8 vs
    // 40.0 ms -- the chain is hidden, the product and the memory-bound passes behind the chain slow each other by more.  And the two on DISJOINT CUs (the
    // product masked off the reserved CUs, the chain on them alone; same tiles, same bits): 40.6 vs 40.4 ms, no gain.
    hipStream_t side;
    RC(side_fork(m, t, &side));
    // GB = L^-T (R v) / s2.  The large product is ENQUEUED before the side chain's ~70 launches, so that a slow host does not hold it back.
    RC(launch_combine(t.R.p, t.q.B.p, nullptr, Mpad, Mpad, 1.0, 1.0, 0.0, m->st));           // R = I - Pq
    // Round 4: GB = (L^-T R) v / s2 -- the M x M solve FIRST (16 block rows of a 2048-column right-hand side), then ONE M x M x N product, instead of
    // the product followed by the M x N solve (8.6 of configs[4]'s 45 ms; removed).  This is not the explicit-inverse product that cost round 1 its dELBO/dZ:
    // L^-T R comes from a backward-stable substitution, v is the accurately solved L^-1 B, and the product is the LAST step before the contraction
    // with the kernel derivatives -- no solve behind it amplifies its rounding.  Against the 80-bit truth dELBO/dZ is 2.17e-3 of the tensor off
    // (M x N solve: 2.37e-3, the reference's fp64: 2.40e-3); kernel gradients 9.6e-9 (9.2e-9).
    RC(trsm_lower(m, t.a.A.p, Mpad, mt, t.R.p, Mpad, Mpad, true));
    GemmArgs g = make_gemm(t.R.p, Mpad, 0, t.v.p, Npad, 1, t.GB.p, Npad, 1.0 / s2, GM_RECT, mt, nt, Mpad);
    // tiles down the columns: the 64 workgroups an XCD holds are then 64 / mt column blocks of v against all of R (M x M: cache-resident), and v comes
    // in from memory once -- row by row it came in mt times (27 GB fetched at configs[4] for a 1.6 GB panel)
    g.col_major = 1;
    RC(gemm_call(m, g, gemm_flops(g, nullptr)));
    RC(launch_combine(t.E.p, t.q.B.p, t.Qs.p, Mpad, Mpad, 2.0, 1.0, 1.0, side));
    RC(adjoint_GA(m, t, 0.5, side));                                            // its diagonal -> dga
    RC(solve_with_rider(m, t, nullptr, t1, beta));                              // GB is finished above, beta alone is solved for
    RC(launch_gemv_cols(t.B.p, Npad, Mpad, Npad, beta, btb, t.scratch.p, m->st));                           // B^T beta
    RC(launch_axpby(Npad, 1.0 / (s2 * s2), m->d_y.p, -1.0 / (s2 * s2 * s2), btb, r, m->st));
    const MomentSpec uf{t.GB.p, Npad, beta, r, 1.0, true}, uu{t.GA.p, Mpad, beta, beta, -0.5 / (s2 * s2), true};
    RC(sparse_moments(m, t, sz, &uf, uu, sharded, side));

    std::vector<double> hgz((size_t)D * Mpad), hb(Mpad), hd(Mpad);
    HIP_TRY(hipMemcpyAsync(mom_uu, t.mom_uu.p, (size_t)P * T * W * sizeof(double), hipMemcpyDeviceToHost, m->st));
    HIP_TRY(hipMemcpyAsync(mom_uf, t.mom_uf.p, (size_t)C * C * T * W * sizeof(double), hipMemcpyDeviceToHost, m->st));
    HIP_TRY(hipMemcpyAsync(hgz.data(), t.gz.p, hgz.size() * sizeof(double), hipMemcpyDeviceToHost, m->st));
    HIP_TRY(hipMemcpyAsync(hb.data(), beta, Mpad * sizeof(double), hipMemcpyDeviceToHost, m->st));
    HIP_TRY(hipMemcpyAsync(hd.data(), dga, Mpad * sizeof(double), hipMemcpyDeviceToHost, m->st));
    // dELBO/dy = -(Qff + s2 I)^-1 y = -s2^-1 (y - s2^-1 v^T t1) = -s2 r  (Woodbury; r = s2^-2 y - s2^-3 B^T beta above, B^T beta = v^T t1)
    RC(mean_grad_enqueue(m, r, -s2));
    HIP_TRY(hipStreamSynchronize(m->st));
    RC(sparse_timeout_check(m));
    mean_grad_collect(m);
    for (int64_t pos = 0; pos < M; ++pos)
        for (int d = 0; d < D; ++d) gZ[sz.perm[pos] * D + d] = hgz[(size_t)d * Mpad + pos];
    double tr = 0.0;
    for (int64_t i = 0; i < M; ++i) tr += hd[i] - 0.5 * hb[i] * hb[i] / (s2 * s2);
    *trGA = tr;
    return MOGP_OK;
}

static int titsias_predict_impl(mogp_model* m, int64_t M, const double* Z, double sigma, double jitter, const double* kss_diag,
                                int64_t S, const double* Xs, double* mu, double* var, int64_t* info, bool sharded) {
    if (m) m->mean_w = nullptr;                 // dp/dr of an earlier gradient evaluation: this call may overwrite or regrow its buffer (mogp_model_fetch 3)
    if (!m || !Z || !kss_diag || !Xs || !mu || !var || M <= 0 || S <= 0) return fail(MOGP_EINVAL, "mogp_titsias_predict: bad argument");
    RC(use_device(m->ctx));
    if (info) *info = 0;
    SortedX sz, ss;
    TitsiasScalars sc;
    RC(titsias_front(m, M, Z, sigma, jitter, sz, sc, info, sharded));
    TitsiasWork& t = *m->tw;
    const int64_t Mpad = t.Mpad;
    RC(sparse_predict_panels(m, t, sz, S, Xs, ss));                                                          // a = L^-1 Kus
    const int mt = (int)(Mpad / MOGP_TILE), st = (int)(ss.Mpad / MOGP_TILE);
    const int64_t Spad = ss.Mpad;
    GemmArgs g = make_gemm(t.Wq, Mpad, 0, t.Aus.p, Spad, 1, t.Bus.p, Spad, 1.0, GM_KHI_I, mt, st, Mpad);                    // b = Wq a
    RC(gemm_call(m, g, gemm_flops(g, nullptr)));
    double* vy = t.vec.p;
    double* cvec = t.vec.p + 4 * Mpad;
    RC(launch_trmv_lower(t.Wq, Mpad, Mpad, vy, cvec, t.vec.p + 6 * Mpad, m->st));                             // c s2 = Wq vy
    // mu s2 = b^T (Wq vy);  var = K_ss,diag - colsum a^2 + colsum b^2
    return sparse_predict_finish(m, t, ss, t.Bus.p, cvec, sigma * sigma, kss_diag, mu, var);
}

extern "C" {

int mogp_titsias_eval(mogp_model* m, int64_t M, const double* Z, double sigma, double jitter, const double* kff_diag, int flags,
                      double* elbo, double* mom_uu, double* mom_uf, double* gZ, double* trGA, double* dsigma,
                      double* jitter_abs, int64_t* info) {
    return titsias_eval_impl(m, M, Z, sigma, jitter, kff_diag, flags, elbo, mom_uu, mom_uf, gZ, trGA, dsigma, jitter_abs, info, false);
}

int mogp_titsias_fetch(mogp_model* m, int which, int64_t M, double* out) {
    if (!m || !out || which < 0 || which > 8 || M <= 0) return fail(MOGP_EINVAL, "mogp_titsias_fetch: bad argument");
    if (!m->tw || m->tw->Mpad <= 0 || m->tw->GA.n == 0) return fail(MOGP_EINVAL, "mogp_titsias_fetch: no gradient evaluation of the Titsias bound on this handle yet");
    RC(use_device(m->ctx));
    TitsiasWork& t = *m->tw;
    const int64_t Mpad = t.Mpad, Npad = m->Npad, N = m->N;
    if (M > Mpad) return fail(MOGP_EINVAL, "mogp_titsias_fetch: M is larger than the last evaluation's");
    HIP_TRY(hipStreamSynchronize(m->st));
    const double* src = nullptr; int64_t rows = 0, cols = 0, ld = 0;
    switch (which) {
        case 0: src = t.GA.p; rows = M; cols = M; ld = Mpad; break;
        case 1: src = t.GB.p; rows = M; cols = N; ld = Npad; break;
        case 2: src = t.vec.p + 4 * Mpad; rows = 1; cols = M; ld = Mpad; break;
        case 3: src = t.vec.p + 8 * Mpad + Npad; rows = 1; cols = N; ld = Npad; break;
        case 4: src = t.v.p; rows = M; cols = N; ld = Npad; break;
        case 5: src = t.a.A.p; rows = M; cols = M; ld = Mpad; break;
        case 6: src = t.Qs.p; rows = M; cols = M; ld = Mpad; break;
        case 7: src = t.q.B.p; rows = M; cols = M; ld = Mpad; break;
        default: src = t.vec.p + Mpad; rows = 1; cols = M; ld = Mpad; break;
    }
    HIP_TRY(hipMemcpy2D(out, (size_t)cols * sizeof(double), src, (size_t)ld * sizeof(double), (size_t)cols * sizeof(double), (size_t)rows, hipMemcpyDeviceToHost));
    return MOGP_OK;
}

int mogp_titsias_eval_sharded(mogp_model* m, int64_t M, const double* Z, double sigma, double jitter, const double* kff_diag, int flags,
                              double* elbo, double* mom_uu, double* mom_uf, double* gZ, double* trGA, double* dsigma,
                              double* jitter_abs, int64_t* info) {
    return titsias_eval_impl(m, M, Z, sigma, jitter, kff_diag, flags, elbo, mom_uu, mom_uf, gZ, trGA, dsigma, jitter_abs, info, true);
}

int mogp_titsias_predict(mogp_model* m, int64_t M, const double* Z, double sigma, double jitter, const double* kss_diag,
                         int64_t S, const double* Xs, double* mu, double* var, int64_t* info) {
    return titsias_predict_impl(m, M, Z, sigma, jitter, kss_diag, S, Xs, mu, var, info, false);
}

int mogp_titsias_predict_sharded(mogp_model* m, int64_t M, const double* Z, double sigma, double jitter, const double* kss_diag,
                                 int64_t S, const double* Xs, double* mu, double* var, int64_t* info) {
    return titsias_predict_impl(m, M, Z, sigma, jitter, kss_diag, S, Xs, mu, var, info, true);
}

// Full predictive covariance of the LAST sparse prediction on this handle (mogp_titsias_predict, mogp_svgp_forward at test inputs; their
// sharded forms): K_ss - a^T a + b^T b with a = L^-1 K_us and b as that call left them (reference gpr/model.py:758-760, 870-872), S x S in
// the caller's order of the test points.  One Gram over the test inputs and two S x S x M products.
int mogp_sparse_predict_cov(mogp_model* m, int64_t S, double* cov) {
    if (!m || !cov || S <= 0) return fail(MOGP_EINVAL, "mogp_sparse_predict_cov: bad argument");
    RC(use_device(m->ctx));
    if (!m->tw || !m->tw->pred_valid || m->tw->pred_ss.M != S)
        return fail(MOGP_EINVAL, "mogp_sparse_predict_cov: no sparse prediction at S test points precedes it on this handle");
    TitsiasWork& t = *m->tw;
    const SortedX& ss = t.pred_ss;
    const int C = m->C, D = m->D;
    const int64_t Mpad = t.Mpad, Spad = ss.Mpad;
    std::vector<GTile> st_tiles;
    std::vector<int> ps;
    build_sym_tiles(ss.off, C, st_tiles, ps);
    RC(m->d_Kss.ensure((size_t)Spad * Spad)); RC(m->d_ptiles.ensure(st_tiles.size()));
    HIP_TRY(hipMemsetAsync(m->d_Kss.p, 0, (size_t)Spad * Spad * sizeof(double), m->st));
    HIP_TRY(hipMemcpyAsync(m->d_ptiles.p, st_tiles.data(), st_tiles.size() * sizeof(GTile), hipMemcpyHostToDevice, m->st));
    GramArgs ga{};
    ga.tiles = m->d_ptiles.p; ga.xr = m->d_xs.p; ga.ldxr = Spad; ga.xc = m->d_xs.p; ga.ldxc = Spad; ga.nrows = S; ga.ncols = S;
    RC(m->ph_ss.prepare(ss.off, ss.off, C, m->T, Spad, Spad, m->st, ga.ph));
    ga.table = m->d_table.p; ga.T = m->T; ga.D = D; ga.C = C; ga.W = m->Wt; ga.out = m->d_Kss.p; ga.ldo = Spad; ga.mirror = 1;
    RC(launch_gram(plan_cus(m->ctx), ga, (int)st_tiles.size(), m->st));
    const int st = (int)(Spad / MOGP_TILE);
    GemmArgs g = make_gemm(t.Aus.p, Spad, 1, t.Aus.p, Spad, 1, m->d_Kss.p, Spad, -1.0, GM_RECT, st, st, Mpad);
    g.beta = 1.0;
    RC(gemm_call(m, g, gemm_flops(g, nullptr)));
    g = make_gemm(t.Bus.p, Spad, 1, t.Bus.p, Spad, 1, m->d_Kss.p, Spad, 1.0, GM_RECT, st, st, Mpad);
    g.beta = 1.0;
    RC(gemm_call(m, g, gemm_flops(g, nullptr)));
    std::vector<double> hc((size_t)Spad * Spad);
    HIP_TRY(hipMemcpyAsync(hc.data(), m->d_Kss.p, hc.size() * sizeof(double), hipMemcpyDeviceToHost, m->st));
    HIP_TRY(hipStreamSynchronize(m->st));
    for (int64_t a = 0; a < S; ++a)
        for (int64_t b = 0; b < S; ++b) cov[ss.perm[a] * S + ss.perm[b]] = hc[(size_t)a * Spad + b];
    return MOGP_OK;
}

}  // extern "C"
