// snelson.hip -- the pseudo-input (FITC) sparse GP of Snelson & Ghahramani and its gradient on the device.
// Reference: gpr/model.py:516-541 (log_marginal_likelihood), :543-576 (predict_f); the gradient replaces autograd through that code.
//
//   A = Kuu + jitter mean(diag Kuu) I = L L^T,  B = Kuf,  v = L^-1 B,  q_n = sum_m v_mn^2 (= Qff_nn),
//   g_n = Kff_nn - q_n + sigma_c(n)^2,  G = diag 1/g,  Bq = I + v G v^T = Lq Lq^T,  Pq = Bq^-1,  r = Pq (v G y)
//   p = -N/2 log 2pi - sum log Lq_kk - 1/2 sum log g_n - 1/2 sum y_n^2 / g_n + 1/2 r.(v G y)        (= log N(y | 0, Qff + diag g))
// Adjoints (S = Qff + diag g;  alpha = S^-1 y = G (y - v^T r);  [S^-1]_nn = G_n - G_n^2 sum_m v_mn (Pq v)_mn;  h_n = 1/2 (alpha_n^2 - [S^-1]_nn)):
//   dp/dB = L^-T (r alpha^T - Pq v G - 2 v diag h)                       (the diagonal of Qff enters g with a minus sign: the -2 v diag h)
//   dp/dA = 1/2 L^-T (I - Pq + 2 v diag(h) v^T) L^-1 - 1/2 beta beta^T,  beta = L^-T r
//   dp/dKff_nn = dp/dsigma_n^2 = h_n
// Same building blocks as the Titsias bound (titsias.hip): solves with L by blocked substitution (trsm.hip), the inner M x M system inverted
// explicitly, the two adjoints contracted with the kernel derivatives by the dense-mode moment kernel (which also yields d/dZ).
// Checked against the reference's autograd through the numpy twin (oracle/table_model.py:snelson_eval) and on the device (snelson.npz).
#include "mogp_model.h"

#include <cmath>
#include <cstring>
#include <limits>

using namespace mogp;

#define RC(x) do { int r__ = (x); if (r__) return r__; } while (0)

namespace {

// per point (channel-sorted order): g = Kff_diag[c] - q + s2[c], G = 1/g, Gy = G y, sg = sqrt(G); zero on the padding.  kd_point (terms with
// an envelope, MOHSM): the kernel diagonal follows the points -- Kff_diag per point instead of per channel
__global__ void k_sn_point(const double* __restrict__ q, const double* __restrict__ y, const int* __restrict__ off, int C,
                           const double* __restrict__ kd, const double* __restrict__ kd_point, const double* __restrict__ s2, int64_t N, int64_t Npad,
                           double* __restrict__ g, double* __restrict__ G, double* __restrict__ Gy, double* __restrict__ sg) {
    const int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= Npad) return;
    if (n >= N) { g[n] = 1.0; G[n] = 0.0; Gy[n] = 0.0; sg[n] = 0.0; return; }
    int c = 0;
    while (c + 1 < C && n >= off[c + 1]) ++c;
    const double gv = (kd_point ? kd_point[n] : kd[c]) - q[n] + s2[c];
    g[n] = gv;
    const double Gv = 1.0 / gv;
    G[n] = Gv; Gy[n] = Gv * y[n]; sg[n] = sqrt(fabs(Gv));
}
// w[n] = sum_m a[m][n] b[m][n] over `rows` rows (row chunks of 256 into part, then summed in order)
__global__ __launch_bounds__(256) void k_coldot_part(const double* __restrict__ a, const double* __restrict__ b, int64_t ld, int64_t rows, int64_t n,
                                                      double* __restrict__ part) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    const int64_t r0 = (int64_t)blockIdx.y * 256, r1 = min(rows, r0 + 256);
    double s = 0.0;
    for (int64_t i = r0; i < r1; ++i) s = fma(a[i * ld + j], b[i * ld + j], s);
    part[(int64_t)blockIdx.y * n + j] = s;
}
__global__ void k_sum_parts_n(const double* __restrict__ part, int64_t n, int nparts, double* __restrict__ out) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    double s = 0.0;
    for (int k = 0; k < nparts; ++k) s += part[(int64_t)k * n + j];
    out[j] = s;
}
// alpha = G (y - v^T r);  h = 1/2 (alpha^2 - G + G^2 w)   (zero on the padding: G = 0 there)
__global__ void k_sn_alpha(const double* __restrict__ G, const double* __restrict__ y, const double* __restrict__ vtr, int64_t N, int64_t Npad,
                           double* __restrict__ alpha) {
    const int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= Npad) return;
    alpha[n] = n < N ? G[n] * (y[n] - vtr[n]) : 0.0;
}
__global__ void k_sn_h(const double* __restrict__ G, const double* __restrict__ alpha, const double* __restrict__ w, int64_t N, int64_t Npad,
                       double* __restrict__ h) {
    const int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= Npad) return;
    h[n] = n < N ? 0.5 * (alpha[n] * alpha[n] - G[n] + G[n] * G[n] * w[n]) : 0.0;
}
// T[m][n] = r[m] alpha[n] - R1[m][n] G[n] - 2 v[m][n] h[n]   (in place over R1)
__global__ void k_sn_adjoint(double* __restrict__ T, const double* __restrict__ v, int64_t ld, int64_t n, const double* __restrict__ r,
                             const double* __restrict__ alpha, const double* __restrict__ G, const double* __restrict__ h) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const int64_t i = blockIdx.y;
    T[i * ld + j] = r[i] * alpha[j] - T[i * ld + j] * G[j] - 2.0 * v[i * ld + j] * h[j];
}

struct SnScalars { double logdet_q, sumlogg, yGy, rvGy, jit, ntot; };

// Front end shared by the evaluation and the prediction: everything up to r = Pq (v G y) and the scalars of p.
// On return: t.a = L (Kuu), t.v = v, t.Wq = Lq^-1, t.q.B = Pq (full), t.Qs = Bq (full), t.nvec = [g | G | Gy | sqrt G | ...],
// t.vec[0:Mpad] = v G y, t.vec[Mpad:2Mpad] = r.
// sharded: this handle holds ONE SHARD of the training points (cf. mogp_titsias_eval_sharded): v G v^T, v G y, sum log g, y^T G y and N are
// all-reduced (and the per-point positivity check with them, so that every rank takes the same exit).
int snelson_front(mogp_model* m, int64_t M, const double* Z, const double* noise_var, double jitter, const double* kff_diag, SortedX& sz,
                  SnScalars& sc, int64_t* info, bool sharded) {
    const int C = m->C;
    const bool env = m->Wt > 2 + 3 * m->D;                     // terms with an envelope on the input midpoint (MOHSM)
    const int64_t N = m->N, Npad = m->Npad;
    if (env && sharded) return fail(MOGP_EINVAL, "the data-parallel Snelson path does not take terms with an envelope (MOHSM)");
    for (int c = 0; c < C; ++c) if (!(noise_var[c] > 0.0)) return fail(MOGP_EINVAL, "noise variances must be positive");
    RC(sparse_kuu(m, M, Z, jitter, true, sz, &sc.jit));
    TitsiasWork& t = *m->tw;
    const int64_t Mpad = t.Mpad;
    const int mt = (int)(Mpad / MOGP_TILE);
    RC(t.nvec.ensure((size_t)8 * Npad + 2 * C));
    // Kuf's padding (rows >= M, columns >= N) must be zero and this path overwrites t.B with scaled copies of v: cleared per call
    HIP_TRY(hipMemsetAsync(t.B.p, 0, (size_t)Mpad * Npad * sizeof(double), m->st));
    RC(sparse_kuf(m, t, sz, m->st, false, nullptr));
    RC(spd_potrf(m, t.a));
    RC(spd_check_info(m, "Kuu", info));
    HIP_TRY(hipMemcpyAsync(t.v.p, t.B.p, (size_t)Mpad * Npad * sizeof(double), hipMemcpyDeviceToDevice, m->st));
    RC(trsm_lower(m, t.a.A.p, Mpad, mt, t.v.p, Npad, Npad, false));              // v = L^-1 B   (reference gpr/model.py:525)

    // per point: g, G, G y, sqrt G
    double* g = t.nvec.p;
    double* G = g + Npad;
    double* Gy = G + Npad;
    double* sg = Gy + Npad;
    double* q = sg + Npad;                                                       // Qff_nn, then reused
    double* kd = t.nvec.p + 8 * Npad;
    double* s2 = kd + C;
    double* kd_point = nullptr;                                                  // envelope: Kff_diag per training point (caller order in, sorted order here)
    std::vector<double> hkd;
    if (env) {
        RC(t.kd_point.ensure((size_t)Npad));
        hkd.assign((size_t)Npad, 0.0);
        for (int64_t pos = 0; pos < N; ++pos) hkd[pos] = kff_diag[m->sx.perm[pos]];
        HIP_TRY(hipMemcpyAsync(t.kd_point.p, hkd.data(), Npad * sizeof(double), hipMemcpyHostToDevice, m->st));
        kd_point = t.kd_point.p;
    } else {
        HIP_TRY(hipMemcpyAsync(kd, kff_diag, C * sizeof(double), hipMemcpyHostToDevice, m->st));
    }
    HIP_TRY(hipMemcpyAsync(s2, noise_var, C * sizeof(double), hipMemcpyHostToDevice, m->st));
    RC(launch_gemv_cols(t.v.p, Npad, Mpad, Npad, nullptr, q, t.scratch.p, m->st));
    hipLaunchKernelGGL(k_sn_point, dim3((unsigned)((Npad + 255) / 256)), dim3(256), 0, m->st, q, m->d_y.p, m->d_chan_off.p, C, kd, kd_point, s2, N, Npad, g, G, Gy, sg);
    HIP_TRY(hipGetLastError());
    std::vector<double> hg(Npad);
    HIP_TRY(hipMemcpyAsync(hg.data(), g, Npad * sizeof(double), hipMemcpyDeviceToHost, m->st));
    // Bq = I + (v sqrt G)(v sqrt G)^T
    RC(launch_scale_cols(t.v.p, t.B.p, Npad, Mpad, Npad, sg, m->st));
    RC(mm_lower_splitk(m, t, t.B.p, t.B.p, t.q.A.p, mt, Mpad, Npad, Npad));
    double* vGy = t.vec.p;
    RC(launch_gemv_rows(t.v.p, Npad, Mpad, Npad, Gy, vGy, m->st));
    HIP_TRY(hipStreamSynchronize(m->st));
    int64_t bad = -1;
    sc.sumlogg = sc.yGy = 0.0;
    for (int64_t n = 0; n < N; ++n) {
        if (!(hg[n] > 0.0)) { if (bad < 0) bad = n; continue; }
        sc.sumlogg += std::log(hg[n]); sc.yGy += m->hy[n] * m->hy[n] / hg[n];
    }
    sc.ntot = (double)N;
    double nbad = bad >= 0 ? 1.0 : 0.0;
    if (sharded) {
        double hs[4] = {sc.sumlogg, sc.yGy, sc.ntot, nbad};
        RC(allreduce_vec_scalars(m, t, vGy, Mpad, hs, 4));
        sc.sumlogg = hs[0]; sc.yGy = hs[1]; sc.ntot = hs[2]; nbad = hs[3];
    }
    if (nbad > 0.0)
        return fail(MOGP_ENOTPD, bad >= 0 ? "Snelson: Kff - Qff + sigma^2 has a non-positive entry (point " + std::to_string(bad) + " in channel-sorted order)"
                                          : std::string("Snelson: Kff - Qff + sigma^2 has a non-positive entry (on another rank's shard)"));
    if (sharded) RC(comm_allreduce(m->ctx, t.q.A.p, Mpad * Mpad, m->st));
    RC(launch_add_diag(t.q.A.p, Mpad, Mpad, 1.0, m->st));
    HIP_TRY(hipMemcpyAsync(t.Qs.p, t.q.A.p, (size_t)Mpad * Mpad * sizeof(double), hipMemcpyDeviceToDevice, m->st));
    RC(launch_info_rearm(m->d_info.p, m->st));              // (not a plain overwrite: a time-out of the wide solve above must reach the host)
    RC(spd_invert(m, t.q, "v G v^T + I", info, &t.Wq));                         // t.Wq = Lq^-1, t.q.B = Pq (lower)
    RC(launch_symmetrize(t.q.B.p, Mpad, Mpad, m->st));
    RC(launch_symmetrize(t.Qs.p, Mpad, Mpad, m->st));
    double* r = t.vec.p + Mpad;
    RC(refined_apply(m, t, t.q.B.p, t.Qs.p, vGy, r));             // r = Pq (v G y): the explicit inverse plus one step of iterative refinement against Bq
    const int nbq = t.q.nb;
    std::vector<double> hv((size_t)2 * Mpad), hl(nbq);
    HIP_TRY(hipMemcpyAsync(hv.data(), t.vec.p, (size_t)2 * Mpad * sizeof(double), hipMemcpyDeviceToHost, m->st));
    HIP_TRY(hipMemcpyAsync(hl.data(), t.q.logdet.p, nbq * sizeof(double), hipMemcpyDeviceToHost, m->st));
    HIP_TRY(hipStreamSynchronize(m->st));
    sc.logdet_q = 0.0; for (double x : hl) sc.logdet_q += x;
    sc.rvGy = 0.0;
    for (int64_t i = 0; i < M; ++i) sc.rvGy += hv[Mpad + i] * hv[i];
    return 0;
}

int snelson_eval_impl(mogp_model* m, int64_t M, const double* Z, const double* noise_var, double jitter, const double* kff_diag, int flags,
                      double* lml, double* mom_uu, double* mom_uf, double* gZ, double* trGA, double* hsum, double* jitter_abs, int64_t* info,
                      bool sharded) {
    if (m) m->mean_w = nullptr;                 // dp/dr of an earlier gradient evaluation: this call may overwrite or regrow its buffer (mogp_model_fetch 3)
    if (!m || !Z || !noise_var || !kff_diag || !lml || M <= 0) return fail(MOGP_EINVAL, "mogp_snelson_eval: bad argument");
    RC(use_device(m->ctx));
    if (info) *info = 0;
    const int C = m->C, D = m->D, W = m->Wt, T = m->T, P = C * (C + 1) / 2;
    const bool env = W > 2 + 3 * D;
    const int64_t N = m->N, Npad = m->Npad;
    const bool grad = (flags & MOGP_EVAL_GRAD) != 0;
    SortedX sz;
    SnScalars sc;
    RC(snelson_front(m, M, Z, noise_var, jitter, kff_diag, sz, sc, info, sharded));
    TitsiasWork& t = *m->tw;
    const int64_t Mpad = t.Mpad;
    const int mt = (int)(Mpad / MOGP_TILE), nt = (int)(Npad / MOGP_TILE);
    *lml = -0.5 * sc.ntot * std::log(2.0 * M_PI) - sc.logdet_q - 0.5 * sc.sumlogg - 0.5 * sc.yGy + 0.5 * sc.rvGy;
    if (jitter_abs) *jitter_abs = sc.jit;
    if (!grad) return sparse_timeout_check(m);
    if (!mom_uu || !mom_uf || !gZ || !trGA || !hsum) return fail(MOGP_EINVAL, "mogp_snelson_eval: gradient outputs are null");

    RC(t.GB.ensure((size_t)Mpad * Npad)); RC(t.E.ensure((size_t)Mpad * Mpad)); RC(t.R.ensure((size_t)Mpad * Mpad));
    RC(t.GA.ensure((size_t)Mpad * Mpad));
    double* r = t.vec.p + Mpad;
    double* beta = t.vec.p + 4 * Mpad;
    double* dga = t.vec.p + 2 * Mpad;
    double* G = t.nvec.p + Npad;
    double* vtr = t.nvec.p + 4 * Npad;            // v^T r, then w = coldot(v, Pq v)
    double* alpha = t.nvec.p + 5 * Npad;
    double* h = t.nvec.p + 6 * Npad;
    const dim3 gn((unsigned)((Npad + 255) / 256)), gmn((unsigned)((Npad + 255) / 256), (unsigned)Mpad);
    RC(launch_gemv_cols(t.v.p, Npad, Mpad, Npad, r, vtr, t.scratch.p, m->st));
    hipLaunchKernelGGL(k_sn_alpha, gn, dim3(256), 0, m->st, G, m->d_y.p, vtr, N, Npad, alpha);
    // R1 = Pq v
    GemmArgs g = make_gemm(t.q.B.p, Mpad, 0, t.v.p, Npad, 1, t.GB.p, Npad, 1.0, GM_RECT, mt, nt, Mpad);
    RC(gemm_call(m, g, gemm_flops(g, nullptr)));
    {
        const int nparts = (int)((Mpad + 255) / 256);
        hipLaunchKernelGGL(k_coldot_part, dim3((unsigned)((Npad + 255) / 256), (unsigned)nparts), dim3(256), 0, m->st, t.v.p, t.GB.p, Npad, Mpad, Npad, t.scratch.p);
        hipLaunchKernelGGL(k_sum_parts_n, gn, dim3(256), 0, m->st, t.scratch.p, Npad, nparts, vtr);
    }
    hipLaunchKernelGGL(k_sn_h, gn, dim3(256), 0, m->st, G, alpha, vtr, N, Npad, h);
    hipLaunchKernelGGL(k_sn_adjoint, gmn, dim3(256), 0, m->st, t.GB.p, t.v.p, Npad, Npad, r, alpha, G, h);
    HIP_TRY(hipGetLastError());
    // E = I - Pq + 2 (v diag h) v^T;  GA = 1/2 L^-T E L^-1 (the - 1/2 beta beta^T goes through the moment kernel's rank-one term).  The M x M x N
    // product first (it needs the whole chip); the two M x M solves behind it go to the side stream, underneath the M x N solve below
    RC(launch_scale_cols(t.v.p, t.B.p, Npad, Mpad, Npad, h, m->st));
    RC(mm_lower_splitk(m, t, t.B.p, t.v.p, t.R.p, mt, Mpad, Npad, Npad));
    if (sharded) RC(comm_allreduce(m->ctx, t.R.p, Mpad * Mpad, m->st));
    RC(launch_symmetrize(t.R.p, Mpad, Mpad, m->st));
    hipStream_t side;
    RC(side_fork(m, t, &side));
    RC(launch_combine(t.E.p, t.q.B.p, t.R.p, Mpad, Mpad, 1.0, 1.0, -2.0, side));
    RC(adjoint_GA(m, t, 0.5, side));                                            // its diagonal -> dga
    // GB = L^-T T, with beta = L^-T r riding along (padding column, or a panel of its own)
    RC(solve_with_rider(m, t, t.GB.p, r, beta));
    const MomentSpec uf{t.GB.p, Npad, beta, alpha, 0.0, true}, uu{t.GA.p, Mpad, beta, beta, -0.5, true};
    RC(sparse_moments(m, t, sz, &uf, uu, sharded, side));

    std::vector<double> hgz((size_t)D * Mpad), hb(Mpad), hd(Mpad), hh(Npad);
    HIP_TRY(hipMemcpyAsync(mom_uu, t.mom_uu.p, (size_t)P * T * W * sizeof(double), hipMemcpyDeviceToHost, m->st));
    HIP_TRY(hipMemcpyAsync(mom_uf, t.mom_uf.p, (size_t)C * C * T * W * sizeof(double), hipMemcpyDeviceToHost, m->st));
    HIP_TRY(hipMemcpyAsync(hgz.data(), t.gz.p, hgz.size() * sizeof(double), hipMemcpyDeviceToHost, m->st));
    HIP_TRY(hipMemcpyAsync(hb.data(), beta, Mpad * sizeof(double), hipMemcpyDeviceToHost, m->st));
    HIP_TRY(hipMemcpyAsync(hd.data(), dga, Mpad * sizeof(double), hipMemcpyDeviceToHost, m->st));
    HIP_TRY(hipMemcpyAsync(hh.data(), h, Npad * sizeof(double), hipMemcpyDeviceToHost, m->st));
    RC(mean_grad_enqueue(m, alpha, -1.0));                  // dp/dy = -(Qff + Lambda)^-1 y = -alpha (Woodbury, k_sn_alpha)
    HIP_TRY(hipStreamSynchronize(m->st));
    RC(sparse_timeout_check(m));
    mean_grad_collect(m);
    for (int64_t pos = 0; pos < M; ++pos)
        for (int d = 0; d < D; ++d) gZ[sz.perm[pos] * D + d] = hgz[(size_t)d * Mpad + pos];
    double tr = 0.0;
    for (int64_t i = 0; i < M; ++i) tr += hd[i] - 0.5 * hb[i] * hb[i];
    *trGA = tr;
    if (env) {                                   // the diagonal follows the points: dp/dKff_nn per training point, caller order (N values)
        for (int64_t pos = 0; pos < N; ++pos) hsum[m->sx.perm[pos]] = hh[pos];
        return MOGP_OK;
    }
    for (int c = 0; c < C; ++c) {
        double s = 0.0;
        for (int pos = m->sx.off[c]; pos < m->sx.off[c + 1]; ++pos) s += hh[pos];
        hsum[c] = s;
    }
    if (sharded) RC(allreduce_vec_scalars(m, t, nullptr, 0, hsum, C));      // sum of h over the points of a channel: one more small all-reduce
    return MOGP_OK;
}

int snelson_predict_impl(mogp_model* m, int64_t M, const double* Z, const double* noise_var, double jitter, const double* kff_diag,
                         const double* kss_diag, int64_t S, const double* Xs, double* mu, double* var, int64_t* info, bool sharded) {
    if (m) m->mean_w = nullptr;                 // dp/dr of an earlier gradient evaluation: this call may overwrite or regrow its buffer (mogp_model_fetch 3)
    if (!m || !Z || !noise_var || !kff_diag || !kss_diag || !Xs || !mu || !var || M <= 0 || S <= 0)
        return fail(MOGP_EINVAL, "mogp_snelson_predict: bad argument");
    RC(use_device(m->ctx));
    if (info) *info = 0;
    SortedX sz, ss;
    SnScalars sc;
    RC(snelson_front(m, M, Z, noise_var, jitter, kff_diag, sz, sc, info, sharded));
    TitsiasWork& t = *m->tw;
    const int64_t Mpad = t.Mpad;
    RC(sparse_predict_panels(m, t, sz, S, Xs, ss));                                                        // a = L^-1 Kus
    const int64_t Spad = ss.Mpad;
    const int mt = (int)(Mpad / MOGP_TILE), st = (int)(Spad / MOGP_TILE);
    GemmArgs g = make_gemm(t.Wq, Mpad, 0, t.Aus.p, Spad, 1, t.Bus.p, Spad, 1.0, GM_KHI_I, mt, st, Mpad);          // b = Lq^-1 a
    RC(gemm_call(m, g, gemm_flops(g, nullptr)));
    double* vGy = t.vec.p;
    double* cvec = t.vec.p + 4 * Mpad;
    RC(launch_trmv_lower(t.Wq, Mpad, Mpad, vGy, cvec, t.vec.p + 6 * Mpad, m->st));                         // c = Lq^-1 v G y
    return sparse_predict_finish(m, t, ss, t.Bus.p, cvec, 1.0, kss_diag, mu, var);                         // mu = b^T c
}

}  // namespace

extern "C" {

int mogp_snelson_eval(mogp_model* m, int64_t M, const double* Z, const double* noise_var, double jitter, const double* kff_diag, int flags,
                      double* lml, double* mom_uu, double* mom_uf, double* gZ, double* trGA, double* hsum, double* jitter_abs, int64_t* info) {
    return snelson_eval_impl(m, M, Z, noise_var, jitter, kff_diag, flags, lml, mom_uu, mom_uf, gZ, trGA, hsum, jitter_abs, info, false);
}

int mogp_snelson_eval_sharded(mogp_model* m, int64_t M, const double* Z, const double* noise_var, double jitter, const double* kff_diag, int flags,
                              double* lml, double* mom_uu, double* mom_uf, double* gZ, double* trGA, double* hsum, double* jitter_abs,
                              int64_t* info) {
    return snelson_eval_impl(m, M, Z, noise_var, jitter, kff_diag, flags, lml, mom_uu, mom_uf, gZ, trGA, hsum, jitter_abs, info, true);
}

int mogp_snelson_predict(mogp_model* m, int64_t M, const double* Z, const double* noise_var, double jitter, const double* kff_diag,
                         const double* kss_diag, int64_t S, const double* Xs, double* mu, double* var, int64_t* info) {
    return snelson_predict_impl(m, M, Z, noise_var, jitter, kff_diag, kss_diag, S, Xs, mu, var, info, false);
}

int mogp_snelson_predict_sharded(mogp_model* m, int64_t M, const double* Z, const double* noise_var, double jitter, const double* kff_diag,
                                 const double* kss_diag, int64_t S, const double* Xs, double* mu, double* var, int64_t* info) {
    return snelson_predict_impl(m, M, Z, noise_var, jitter, kff_diag, kss_diag, S, Xs, mu, var, info, true);
}

}  // extern "C"
