// loo.hip -- the leave-one-out predictive log-likelihood of the exact GP and its adjoint (Rasmussen & Williams 5.4.2; Sundararajan & Keerthi 2001).
// With Kj = K + noise (+ data_var) + jitter, r = y - m(X), alpha = Kj^-1 r and kappa_i = (Kj^-1)_ii -- all of which a gradient evaluation
// of the exact path (exact.hip) leaves on the device -- the predictive of y_i given every other point is
//   mu_i = y_i - alpha_i / kappa_i,   var_i = 1 / kappa_i   (noise included),
//   L    = sum_i [ 1/2 log kappa_i - alpha_i^2 / (2 kappa_i) - 1/2 log 2 pi ]
// and with a_i = 1/2 / kappa_i + alpha_i^2 / (2 kappa_i^2) (> 0), b_i = alpha_i / kappa_i, rho = Kj^-1 b
//   dL/dKj = G_loo = - Kj^-1 diag(a) Kj^-1 + 1/2 (alpha rho^T + rho alpha^T)   (symmetric),     dL/dr = -rho.
// G_loo stands where G = 1/2 (alpha alpha^T - Kj^-1) stands in mogp_exact_eval: its moments (the dense symmetric form of gram.hip:k_moments, for
// every row kind), per-channel diagonal sums and trace go back in the same layout, and the host's chain rule is the marginal likelihood's.
//   k_loo_points    one thread per point: mu, var, a, b, sqrt a and the point's term of L (zeros on the padding)
//   k_loo_sum       ONE workgroup adds the N terms: strided partial sums and a fixed LDS tree -- no atomics, the same bits every time
//   rho             a row-wise product with the mirrored inverse (launch_gemv_rows)
//   G_loo           S = Kj^-1 diag(sqrt a) (launch_scale_cols), -S S^T over the lower tiles on the fp64 MFMA GEMM, then k_loo_rank2 adds the
//                   symmetrised rank-two term entry by entry (the moment kernel's rider ru rw^T is ONE outer product: under the symmetric
//                   double count it would give alpha rho^T alone, not its symmetric part)
//   k_loo_diag      per-channel sums of the diagonal of G_loo
// Leave-fold-out cross-validation (lfo.hip) is the same schedule with its own points kernel and its own S: held_out_points and held_out_adjoint carry both.
#include "mogp_model.h"

using namespace mogp;

#define RC(x) do { int r__ = (x); if (r__) return r__; } while (0)

namespace {

__global__ __launch_bounds__(256) void k_loo_points(const double* __restrict__ kinv, int64_t ld, const double* __restrict__ alpha,
                                                    const double* __restrict__ y, int64_t N, int64_t Npad, double* __restrict__ vec) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= Npad) return;
    double mu = 0.0, var = 0.0, a = 0.0, b = 0.0, sa = 0.0, term = 0.0;
    if (i < N) {
        const double kap = kinv[i * ld + i], al = alpha[i];
        var = 1.0 / kap;
        b = al * var;
        mu = y[i] - b;
        a = 0.5 * var + 0.5 * b * b;
        sa = sqrt(a);
        term = 0.5 * log(kap) - 0.5 * al * b - 0.91893853320467274178;       // 1/2 log 2 pi
    }
    vec[LOO_MU * Npad + i] = mu; vec[LOO_VAR * Npad + i] = var; vec[LOO_A * Npad + i] = a; vec[LOO_B * Npad + i] = b;
    vec[LOO_SA * Npad + i] = sa; vec[LOO_TERM * Npad + i] = term;
}

__global__ __launch_bounds__(256) void k_loo_sum(const double* __restrict__ term, int64_t n, double* __restrict__ out) {
    __shared__ double red[256];
    double s = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += 256) s += term[i];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = red[0];
}

// G[i][j] += 1/2 (alpha_i rho_j + rho_i alpha_j) for j <= i < n
__global__ __launch_bounds__(256) void k_loo_rank2(double* __restrict__ G, int64_t ld, int64_t n, const double* __restrict__ alpha,
                                                   const double* __restrict__ rho) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x, i = blockIdx.y;
    if (j > i || i >= n) return;
    G[i * ld + j] += 0.5 * (alpha[i] * rho[j] + rho[i] * alpha[j]);
}

// out[c] = sum_{k in channel c} G_kk; one workgroup per channel, fixed order
__global__ __launch_bounds__(256) void k_loo_diag(const double* __restrict__ G, int64_t ld, const int* __restrict__ chan_off, double* __restrict__ out) {
    const int c = blockIdx.x;
    __shared__ double red[256];
    double s = 0.0;
    for (int64_t k = chan_off[c] + threadIdx.x; k < chan_off[c + 1]; k += 256) s += G[k * ld + k];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[c] = red[0];
}

}  // namespace

namespace mogp {

int loo_workspace(mogp_model* m, bool grad) {
    const int64_t Npad = m->Npad;
    RC(m->loo.vec.ensure((size_t)LOO_COUNT * Npad));
    if (grad) RC(m->loo.G.ensure((size_t)Npad * Npad));
    return 0;
}

// The points pass of both held-out scores: the inverse mirrored, the score's own kernel over the targets as the caller gave them -- per point here, per
// fold in lfo.hip (cv_folds) -- and the fixed-order sum of its terms, one per point or one per fold
int held_out_points(mogp_model* m, double* kinv, bool folds, bool grad) {
    const int64_t N = m->N, Npad = m->Npad;
    double* v = m->loo.vec.p;
    RC(launch_symmetrize(kinv, Npad, Npad, m->st));             // every tile of the inverse is read from here on, row by row
    const double* y = m->mean_on ? m->d_y0.p : m->d_y.p;        // the targets as the caller gave them (d_y: the residual under a mean table)
    if (folds) RC(cv_folds(m, kinv, y, grad));
    else hipLaunchKernelGGL(k_loo_points, dim3((unsigned)((Npad + 255) / 256)), dim3(256), 0, m->st, kinv, Npad, m->d_alpha.p, y, N, Npad, v);
    hipLaunchKernelGGL(k_loo_sum, dim3(1), dim3(256), 0, m->st, v + LOO_TERM * Npad, folds ? m->cv.nfolds : N, v + LOO_SUM * Npad);
    HIP_TRY(hipGetLastError());
    return 0;
}

// The adjoint of both held-out scores: rho = Kj^-1 b, S into scratch, -S S^T over the lower tiles into G, the symmetrised rank-two term.  Only S differs:
// Kj^-1 diag(sqrt a) for leave-one-out, the folds' columns Kj^-1[:, B] F_B (lfo.hip: cv_fill_S) for leave-fold-out
int held_out_adjoint(mogp_model* m, const double* kinv, double* scratch, bool folds) {
    const int64_t N = m->N, Npad = m->Npad;
    double* v = m->loo.vec.p;
    double* rho = v + LOO_RHO * Npad;
    RC(launch_gemv_rows(kinv, Npad, Npad, Npad, v + LOO_B * Npad, rho, m->st));
    if (folds) RC(cv_fill_S(m, kinv, scratch));
    else RC(launch_scale_cols(kinv, scratch, Npad, Npad, Npad, v + LOO_SA * Npad, m->st));
    GemmArgs g = make_gemm(scratch, Npad, 0, scratch, Npad, 0, m->loo.G.p, Npad, -1.0, GM_LOWER, m->nb, m->nb, Npad);
    RC(gemm_call(m, g, gemm_flops(g, nullptr)));
    hipLaunchKernelGGL(k_loo_rank2, dim3((unsigned)((N + 255) / 256), (unsigned)N), dim3(256), 0, m->st, m->loo.G.p, Npad, N, m->d_alpha.p, rho);
    HIP_TRY(hipGetLastError());
    return 0;
}

int loo_moment_pass(mogp_model* m) {
    const int C = m->C, D = m->D, W = m->Wt, T = m->T, P = C * (C + 1) / 2;
    const int64_t Npad = m->Npad;
    MomentArgs ma{};
    ma.tiles = m->d_tiles.p; ma.ntiles = (int)m->tiles.size();
    ma.x = m->d_x.p; ma.ldx = Npad; ma.nrows = ma.ncols = m->N;
    RC(m->ph_xx.prepare(m->sx.off, m->sx.off, C, T, Npad, Npad, m->st, ma.ph));
    ma.table = m->d_table.p; ma.T = T; ma.D = D; ma.C = C; ma.W = W;
    ma.G = m->loo.G.p; ma.ldg = Npad; ma.sym = 1; ma.ldgz = Npad;
    if (m->radial) { ma.kind = m->d_kind.p; ma.shape = m->d_shape.p; }
    ma.partial = m->d_partial.p;
    ma.phases_ready = 1;                       // ph_xx was filled by this evaluation's Gram launch: same inputs, same table
    RC(launch_moments(plan_cus(m->ctx), ma, m->st, m->radial ? m->gate_kinds : 0));
    RC(launch_moment_reduce(m->d_partial.p, m->d_pair_start.p, P, T, W, D, m->d_moments.p, m->st, 1));
    hipLaunchKernelGGL(k_loo_diag, dim3(C), dim3(256), 0, m->st, m->loo.G.p, Npad, m->d_chan_off.p, m->d_diagG.p);
    HIP_TRY(hipGetLastError());
    RC(mean_grad_enqueue(m, m->loo.vec.p + LOO_RHO * Npad, -1.0));      // dL/dr = -rho (nothing is launched without a mean table)
    return mark(m, 6);
}

}  // namespace mogp
