// svgp.hip -- the variational GP of Hensman et al. (whitened), the O(N M^2) algebra around ANY likelihood, on the device.
// Reference: gpr/model.py:767-886 (SparseHensman / Hensman): q(u) = N(L q_mu, L S S^T L^T), L L^T = Kuu + jitter, S = tril(q_sqrt).
//
// Two calls per evaluation, the likelihood in between (host, O(N): its expectation E(mu, var) and e = dE/dmu, f = dE/dvar per point):
//   forward   a = L^-1 K(Z, X),  b = S^T a,  mu = a^T q_mu,  var = K_diag - colsum(a^2) + colsum(b^2)          (reference :851-868)
//             dense (the non-sparse model at its own inputs, :834-840): Z = X, a = L^T exactly, var = colsum(b^2)
//   backward  Gv = q_mu e^T + 2 (S S^T - I) v diag f                   (dense: without the - I)
//             dE/dKuf = L^-T Gv,   dE/dKuu = -1/2 L^-T Psi(Gv v^T) L^-1     (Psi(Y) = tril(Y) mirrored; dense: +1/2 L^-T Psi(v Gv^T) L^-1, no Kuf)
//             dE/dq_mu = v e,   dE/dS = 2 (v diag(f) v^T) S
// contracted with the kernel derivatives by the dense-mode moment kernel (which also yields d/dZ), like titsias.hip / snelson.hip.
// Z, q_mu and the rows of q_sqrt come in the caller's order; the device works with Z sorted by channel (rows of S permuted, columns kept).
// Checked against the reference's autograd through the numpy twin (oracle/table_model.py:svgp_forward / svgp_backward) and on the device.
#include "mogp_model.h"

#include <cmath>
#include <cstring>
#include <limits>

using namespace mogp;

#define RC(x) do { int r__ = (x); if (r__) return r__; } while (0)

namespace {

// a[i][j] = 0 for i > j   (a = L^T is upper triangular; the tiles above the diagonal of L are never written by the factorisation)
__global__ void k_sv_mask_upper(double* __restrict__ a, int64_t ld, int64_t n) {
    const int64_t i = blockIdx.x;
    for (int64_t j = threadIdx.x; j < i && j < n; j += blockDim.x) a[i * ld + j] = 0.0;
}
// Gv[m][n] = q[m] e[n] + 2 (Sb[m][n] - keep * v[m][n]) f[n]      (in place over Sb)
__global__ void k_sv_adjoint(double* __restrict__ Gv, const double* __restrict__ v, int64_t ld, int64_t n, const double* __restrict__ q,
                             const double* __restrict__ e, const double* __restrict__ f, double keep) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const int64_t i = blockIdx.y;
    Gv[i * ld + j] = q[i] * e[j] + 2.0 * (Gv[i * ld + j] - keep * v[i * ld + j]) * f[j];
}

}  // namespace

// sharded: this handle holds ONE SHARD of the training points (see mogp_titsias_eval_sharded): everything that sums over data points -- the two
// M x M products over N, v e, the (Z, X) moments and their share of d/dZ -- is all-reduced; e, f are those of the local points
static int svgp_backward_impl(mogp_model* m, const double* e, const double* f, double* mom_uu, double* mom_uf, double* gZ, double* trGA,
                              double* g_qmu, double* g_qsqrt, bool sharded) {
    if (m) m->mean_w = nullptr;                 // dp/dr of an earlier gradient evaluation: this call may overwrite or regrow its buffer (mogp_model_fetch 3)
    if (!m || !e || !f || !mom_uu || !mom_uf || !gZ || !trGA || !g_qmu || !g_qsqrt) return fail(MOGP_EINVAL, "mogp_svgp_backward: bad argument");
    RC(use_device(m->ctx));
    if (!m->tw || !m->tw->sv_valid) return fail(MOGP_EINVAL, "mogp_svgp_backward: no forward pass at the training inputs precedes it");
    TitsiasWork& t = *m->tw;
    t.sv_valid = false;                                         // the buffers of the forward pass are consumed
    const int C = m->C, D = m->D, W = m->Wt, T = m->T, P = C * (C + 1) / 2;
    const int64_t N = m->N, Npad = m->Npad, Mpad = t.Mpad, M = t.sv_sz.M;
    if (sharded && W > 2 + 3 * D) return fail(MOGP_EINVAL, "the data-parallel Hensman path does not take terms with an envelope (MOHSM)");
    const int mt = (int)(Mpad / MOGP_TILE), nt = (int)(Npad / MOGP_TILE);
    const bool dense = t.sv_dense;
    const SortedX& sz = t.sv_sz;
    // e, f in the device's (channel-sorted) order of the points
    std::vector<double> he(Npad, 0.0), hf(Npad, 0.0);
    for (int64_t pos = 0; pos < N; ++pos) { he[pos] = e[m->sx.perm[pos]]; hf[pos] = f[m->sx.perm[pos]]; }
    double* de = t.nvec.p;
    double* df = t.nvec.p + Npad;
    HIP_TRY(hipMemcpyAsync(de, he.data(), Npad * sizeof(double), hipMemcpyHostToDevice, m->st));
    HIP_TRY(hipMemcpyAsync(df, hf.data(), Npad * sizeof(double), hipMemcpyHostToDevice, m->st));
    double* q = t.vec.p;
    double* gq = t.vec.p + Mpad;
    double* dga = t.vec.p + 2 * Mpad;
    const dim3 gmn((unsigned)((Npad + 255) / 256), (unsigned)Mpad);
    // dE/dq_mu = v e
    RC(launch_gemv_rows(t.v.p, Npad, Mpad, Npad, de, gq, m->st));
    if (sharded) {
        if (dense) return fail(MOGP_EINVAL, "the dense Hensman model lives on ALL data points: it cannot be sharded over them");
        RC(comm_allreduce(m->ctx, gq, Mpad, m->st));
    }
    // Gv = q e^T + 2 (S b - v) diag f   (t.B; b = S^T v is in t.GB from the forward pass)
    GemmArgs g = make_gemm(t.R.p, Mpad, 0, t.GB.p, Npad, 1, t.B.p, Npad, 1.0, GM_RECT, mt, nt, Mpad);
    RC(gemm_call(m, g, gemm_flops(g, nullptr)));
    hipLaunchKernelGGL(k_sv_adjoint, gmn, dim3(256), 0, m->st, t.B.p, t.v.p, Npad, Npad, q, de, df, dense ? 0.0 : 1.0);
    HIP_TRY(hipGetLastError());
    // Psi: tril(Gv v^T) (dense: tril(v Gv^T)) mirrored;  GA = -/+ 1/2 L^-T Psi L^-1
    RC(mm_lower_splitk(m, t, dense ? t.v.p : t.B.p, dense ? t.B.p : t.v.p, t.E.p, mt, Mpad, Npad, Npad));
    if (sharded) RC(comm_allreduce(m->ctx, t.E.p, Mpad * Mpad, m->st));
    RC(launch_symmetrize(t.E.p, Mpad, Mpad, m->st));
    hipStream_t side;                              // the two M x M solves: on the side stream, underneath the M x N work below
    RC(side_fork(m, t, &side));
    RC(adjoint_GA(m, t, dense ? 0.5 : -0.5, side));                               // its diagonal -> dga
    // dE/dS = 2 (v diag(f) v^T) S: (v f) into t.GB (b is no longer needed), the M x M product into t.Qs, times S into t.q.A
    RC(launch_scale_cols(t.v.p, t.GB.p, Npad, Mpad, Npad, df, m->st));
    RC(mm_lower_splitk(m, t, t.GB.p, t.v.p, t.Qs.p, mt, Mpad, Npad, Npad));
    if (sharded) RC(comm_allreduce(m->ctx, t.Qs.p, Mpad * Mpad, m->st));
    RC(launch_symmetrize(t.Qs.p, Mpad, Mpad, m->st));
    g = make_gemm(t.Qs.p, Mpad, 0, t.R.p, Mpad, 1, t.q.A.p, Mpad, 2.0, GM_RECT, mt, mt, Mpad);
    RC(gemm_call(m, g, gemm_flops(g, nullptr)));
    if (!dense) RC(trsm_lower(m, t.a.A.p, Mpad, mt, t.B.p, Npad, Npad, true));      // dE/dKuf = L^-T Gv, in place
    const MomentSpec uf{t.B.p, Npad, q, de, 0.0, true}, uu{t.GA.p, Mpad, q, q, 0.0, !dense};      // dense: the inputs are the data, not parameters
    RC(sparse_moments(m, t, sz, dense ? nullptr : &uf, uu, sharded, side));

    std::vector<double> hgz((size_t)D * Mpad), hq(Mpad), hd(Mpad), hS((size_t)Mpad * Mpad);
    HIP_TRY(hipMemcpyAsync(mom_uu, t.mom_uu.p, (size_t)P * T * W * sizeof(double), hipMemcpyDeviceToHost, m->st));
    HIP_TRY(hipMemcpyAsync(mom_uf, t.mom_uf.p, (size_t)C * C * T * W * sizeof(double), hipMemcpyDeviceToHost, m->st));
    HIP_TRY(hipMemcpyAsync(hgz.data(), t.gz.p, hgz.size() * sizeof(double), hipMemcpyDeviceToHost, m->st));
    HIP_TRY(hipMemcpyAsync(hq.data(), gq, Mpad * sizeof(double), hipMemcpyDeviceToHost, m->st));
    HIP_TRY(hipMemcpyAsync(hd.data(), dga, Mpad * sizeof(double), hipMemcpyDeviceToHost, m->st));
    HIP_TRY(hipMemcpyAsync(hS.data(), t.q.A.p, hS.size() * sizeof(double), hipMemcpyDeviceToHost, m->st));
    HIP_TRY(hipStreamSynchronize(m->st));
    RC(sparse_timeout_check(m));
    double tr = 0.0;
    for (int64_t pos = 0; pos < M; ++pos) {
        const int64_t dst = sz.perm[pos];
        for (int d = 0; d < D; ++d) gZ[dst * D + d] = hgz[(size_t)d * Mpad + pos];
        g_qmu[dst] = hq[pos];
        for (int64_t c = 0; c < M; ++c) g_qsqrt[(size_t)dst * M + c] = hS[(size_t)pos * Mpad + c];
        tr += hd[pos];
    }
    *trGA = tr;
    return MOGP_OK;
}

extern "C" {

int mogp_svgp_forward(mogp_model* m, int64_t M, const double* Z, const double* q_mu, const double* q_sqrt, double jitter,
                      const double* kff_diag, int dense, int64_t S, const double* Xs, const double* kss_diag,
                      double* mu, double* var, double* jitter_abs, int64_t* info) {
    if (m) m->mean_w = nullptr;                 // dp/dr of an earlier gradient evaluation: this call may overwrite or regrow its buffer (mogp_model_fetch 3)
    if (!m || !Z || !q_mu || !q_sqrt || !kff_diag || !mu || !var || M <= 0) return fail(MOGP_EINVAL, "mogp_svgp_forward: bad argument");
    if (S > 0 && (!Xs || !kss_diag)) return fail(MOGP_EINVAL, "mogp_svgp_forward: test inputs without Xs / kss_diag");
    RC(use_device(m->ctx));
    if (info) *info = 0;
    const int C = m->C;
    const int64_t N = m->N, Npad = m->Npad;
    const bool train = S <= 0;
    if (dense && M != N) return fail(MOGP_EINVAL, "mogp_svgp_forward: the dense model has its inducing inputs at the data points (M = N)");
    if (dense && !m->sx.identity) return fail(MOGP_EINVAL, "the dense Hensman model takes data points grouped by channel, in ascending channel order");
    SortedX sz, ss;
    double jit = 0.0;
    if (m->tw) m->tw->sv_valid = false;
    // Kuu -> L (t.a), q_mu and S = tril(q_sqrt) onto the device in the sorted order of Z (t.vec[0:Mpad], t.R with rows permuted).
    // The whitened parametrisation q(u) = N(L q_mu, ..) depends on the ORDER of the inducing inputs through the Cholesky factor; the device
    // factorises Kuu with the inputs grouped by channel, so that is the order they have to come in (what init_inducing_points and the
    // reference's own data formatting produce).
    RC(sparse_kuu(m, M, Z, jitter, train && !dense, sz, &jit,
                  "the Hensman models take inducing inputs grouped by channel, in ascending channel order "
                  "(the whitened variational parameters depend on their order)"));
    TitsiasWork& t = *m->tw;
    const int64_t Mpad = t.Mpad;
    const int mt = (int)(Mpad / MOGP_TILE);
    RC(t.R.ensure((size_t)Mpad * Mpad)); RC(t.E.ensure((size_t)Mpad * Mpad)); RC(t.GA.ensure((size_t)Mpad * Mpad));
    RC(t.GB.ensure((size_t)Mpad * Npad));
    RC(t.nvec.ensure((size_t)8 * Npad + 2 * C));
    RC(spd_potrf(m, t.a));
    RC(spd_check_info(m, "Kuu", info));
    // q_mu and S in the device's order of the inducing points: row pos of the device = row sz.perm[pos] of the caller
    std::vector<double> hq(Mpad, 0.0), hS((size_t)Mpad * Mpad, 0.0);
    for (int64_t pos = 0; pos < M; ++pos) {
        const int64_t src = sz.perm[pos];
        hq[pos] = q_mu[src];
        for (int64_t c = 0; c <= src; ++c) hS[(size_t)pos * Mpad + c] = q_sqrt[(size_t)src * M + c];     // tril: columns <= the CALLER's row index
    }
    HIP_TRY(dev_upload(t.vec.p, hq.data(), Mpad * sizeof(double)));
    HIP_TRY(dev_upload(t.R.p, hS.data(), (size_t)Mpad * Mpad * sizeof(double)));
    if (jitter_abs) *jitter_abs = jit;
    double* q = t.vec.p;

    // the points mu / var are asked at: the training inputs (state kept for the backward call) or test inputs
    int64_t Qpad = Npad;
    double* a = t.v.p;
    double* b = t.GB.p;
    if (!train) {
        RC(sparse_predict_panels(m, t, sz, S, Xs, ss));                           // a = L^-1 K(Z, Xs)
        Qpad = ss.Mpad; a = t.Aus.p; b = t.Bus.p;
    } else if (dense) {
        RC(launch_transpose(a, t.a.A.p, Mpad, Mpad, m->st));                      // a = L^T  (Mpad = Npad)
        hipLaunchKernelGGL(k_sv_mask_upper, dim3((unsigned)Mpad), dim3(256), 0, m->st, a, Mpad, Mpad);
        HIP_TRY(hipGetLastError());
    } else {
        HIP_TRY(hipMemsetAsync(t.B.p, 0, (size_t)Mpad * Npad * sizeof(double), m->st));
        RC(sparse_kuf(m, t, sz, m->st, false, nullptr));
        HIP_TRY(hipMemcpyAsync(a, t.B.p, (size_t)Mpad * Npad * sizeof(double), hipMemcpyDeviceToDevice, m->st));
        RC(trsm_lower(m, t.a.A.p, Mpad, mt, a, Npad, Npad, false));               // a = L^-1 K(Z, X)
    }
    // b = S^T a;  mu = a^T q_mu;  column sums of squares
    GemmArgs g = make_gemm(t.R.p, Mpad, 1, a, Qpad, 1, b, Qpad, 1.0, GM_RECT, mt, (int)(Qpad / MOGP_TILE), Mpad);
    RC(gemm_call(m, g, gemm_flops(g, nullptr)));
    // dense at its own inputs: var = colsum(b^2) alone
    if (!train) return sparse_predict_finish(m, t, ss, a, q, 1.0, kss_diag, mu, var);
    RC(sparse_point_stats(m, t, m->sx, a, b, a, q, 1.0, dense ? nullptr : kff_diag, mu, var));
    t.sv_sz = sz; t.sv_dense = dense != 0; t.sv_valid = true;
    return MOGP_OK;
}

int mogp_svgp_backward(mogp_model* m, const double* e, const double* f, double* mom_uu, double* mom_uf, double* gZ, double* trGA,
                       double* g_qmu, double* g_qsqrt) {
    return svgp_backward_impl(m, e, f, mom_uu, mom_uf, gZ, trGA, g_qmu, g_qsqrt, false);
}

int mogp_svgp_backward_sharded(mogp_model* m, const double* e, const double* f, double* mom_uu, double* mom_uf, double* gZ, double* trGA,
                               double* g_qmu, double* g_qsqrt) {
    return svgp_backward_impl(m, e, f, mom_uu, mom_uf, gZ, trGA, g_qmu, g_qsqrt, true);
}

}  // extern "C"
