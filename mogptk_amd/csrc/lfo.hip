// lfo.hip -- leave-fold-out cross-validation of the exact GP and its adjoint: the predictive log-likelihood of whole index sets ("folds") given every
// other point, from what a gradient evaluation of the exact path leaves on the device.  With P = Kj^-1 (mirrored), alpha = P r and a fold B of m <= 128 points
//   Sigma_B = (P_BB)^-1,   mu_B = y_B - Sigma_B alpha_B,   log p(y_B | y_-B) = -1/2 alpha_B^T Sigma_B alpha_B + 1/2 log det P_BB - m/2 log 2 pi
// and L = sum over the folds.  With b_B = Sigma_B alpha_B (0 outside the folds), E_B = 1/2 Sigma_B + 1/2 b_B b_B^T, rho = P b
//   dL/dKj = G_cv = -P E P + 1/2 (alpha rho^T + rho alpha^T),   dL/dr = -rho,
// and -P E P = -S S^T with S[:, B] = P[:, B] F_B for any F_B F_B^T = E_B.  G_cv stands where G_loo stands (loo.hip): one-point folds give its a_i, b_i.
//   k_cv_folds   one workgroup per fold.  P_BB is gathered into LDS as a packed lower triangle and factored P_BB = L L^T by a plain right-looking
//                Cholesky in LDS (NOT leaf_dev.h's 128 x 128 tile code: that one is built around a full tile and leaves L^-1 in global memory; a fold
//                has any size 1 .. 128, its points are scattered, and nothing here is on a serial chain), then W = L^-1 column by column into a
//                second packed triangle.  Everything else is a product with W: u = W alpha_B (the forward substitution), b_B = W^T u (the backward
//                one), alpha^T Sigma alpha = u^T u, diag Sigma = column sums of W^2 -- and the factor of E_B needs no second factorisation:
//                  E_B = 1/2 W^T (I + u u^T) W,   I + u u^T = (I + c u u^T)^2 with c = 1 / (1 + sqrt(1 + u^T u)),
//                  F_B = (W^T + c b_B u^T) / sqrt 2      (m x m, dense; F_B F_B^T = E_B exactly, SPD for every u: no pivot can fail)
//                A non-positive pivot of P_BB goes to the evaluation's pivot word (atomicMin, as every factorisation here reports) and the fold
//                goes on with a unit pivot: no NaN travels.
//   the sum      loo.hip's one-workgroup fixed tree over the per-fold terms (held_out_points): no atomics, the same bits every time
//   k_cv_cols    S[:, B] = P[:, B] F_B: one workgroup per (fold, 32 rows), the gathered columns staged in LDS, plain FMAs (DESIGN 1d has the
//                measurement behind that choice); the other columns of S are zero-filled before it
//   the schedule around these two kernels -- the mirrored inverse, rho, -S S^T, the rank-two term, the moment pass -- is loo.hip's, written once for both
//   scores (held_out_points, held_out_adjoint): this file supplies cv_folds and cv_fill_S to it
#include "mogp_model.h"

using namespace mogp;

#define RC(x) do { int r__ = (x); if (r__) return r__; } while (0)

namespace {

#define CV_ROWS 32                               // rows of S per workgroup of k_cv_cols

__device__ __forceinline__ int pk(int r, int c) { return r * (r + 1) / 2 + c; }       // packed lower triangle, c <= r

// LDS doubles of k_cv_folds for a largest fold of mmax points: L, W (packed), 1 / L_kk, alpha_B, u, b, log L_kk
__host__ __device__ inline size_t cv_lds_doubles(int mmax) { return (size_t)mmax * (mmax + 1) + 5 * (size_t)mmax + 2; }

__global__ __launch_bounds__(256) void k_cv_folds(const double* __restrict__ kinv, int64_t ld, const double* __restrict__ alpha,
                                                  const double* __restrict__ y, const int* __restrict__ fold_off, const int* __restrict__ fold_idx,
                                                  const long long* __restrict__ fac_off, int mmax, int want_f, int64_t Npad,
                                                  double* __restrict__ vec, double* __restrict__ fac, unsigned long long* __restrict__ info) {
    extern __shared__ double cv_lds[];
    const int f = blockIdx.x, tid = threadIdx.x;
    const int o = fold_off[f], m = fold_off[f + 1] - o;
    const int* idx = fold_idx + o;
    const int tri = mmax * (mmax + 1) / 2;
    double* L = cv_lds;
    double* W = L + tri;
    double* invd = W + tri;
    double* al = invd + mmax;
    double* u = al + mmax;
    double* b = u + mmax;
    double* lg = b + mmax;
    double* sc = lg + mmax;                      // [2]: u^T u, sum log L_kk

    for (int e = tid; e < m * m; e += 256) {
        const int i = e / m, j = e - i * m;
        if (j <= i) L[pk(i, j)] = kinv[(int64_t)idx[i] * ld + idx[j]];
    }
    if (tid < m) al[tid] = alpha[idx[tid]];

    // P_BB = L L^T, right-looking; every thread reads the pivot, so `bad` is the same in all of them
    int bad = -1;
    const int ty = tid >> 4, tx = tid & 15;
    for (int k = 0; k < m; ++k) {
        __syncthreads();
        double d = L[pk(k, k)];
        if (!(d > 0.0)) { if (bad < 0) bad = k; d = 1.0; }
        const double rs = 1.0 / sqrt(d);
        __syncthreads();
        for (int r = k + tid; r < m; r += 256) L[pk(r, k)] = (r == k) ? d * rs : L[pk(r, k)] * rs;
        if (tid == 0) { invd[k] = rs; lg[k] = -log(rs); }
        __syncthreads();
        for (int r = k + 1 + ty; r < m; r += 16) {
            const double lrk = L[pk(r, k)];
            for (int c = k + 1 + tx; c <= r; c += 16) L[pk(r, c)] = fma(-lrk, L[pk(c, k)], L[pk(r, c)]);
        }
    }
    __syncthreads();
    if (bad >= 0 && tid == 0) atomicMin(info, (unsigned long long)f * 256ull + (unsigned long long)bad + 1ull);

    // W = L^-1: thread j solves L w = e_j down its column.  The loops are uniform over a wave (its first column on), so L[r][k] is one
    // broadcast read; a thread reads back only what it wrote itself
    if (tid < ((m + 63) & ~63) && tid < 128) {
        const int j = tid, j0 = tid & ~63;
        for (int r = j0; r < m; ++r) {
            double s = (r == j) ? 1.0 : 0.0;
            for (int k = j0; k < r; ++k) {
                const double lv = L[pk(r, k)];
                const double wv = (k >= j && j < m) ? W[pk(k, j)] : 0.0;
                s = fma(-lv, wv, s);
            }
            if (r >= j && j < m) W[pk(r, j)] = s * invd[r];
        }
    }
    __syncthreads();
    if (tid < m) {                               // u = W alpha_B
        double s = 0.0;
        for (int k = 0; k <= tid; ++k) s = fma(W[pk(tid, k)], al[k], s);
        u[tid] = s;
    }
    __syncthreads();
    double bj = 0.0, vj = 0.0;
    if (tid < m) {                               // b = W^T u, diag Sigma_B = column sums of W^2
        for (int k = tid; k < m; ++k) { const double w = W[pk(k, tid)]; bj = fma(w, u[k], bj); vj = fma(w, w, vj); }
        b[tid] = bj;
    }
    if (tid == 0) {                              // fixed order: the same bits every time
        double uu = 0.0, sl = 0.0;
        for (int k = 0; k < m; ++k) { uu = fma(u[k], u[k], uu); sl += lg[k]; }
        sc[0] = uu; sc[1] = sl;
    }
    __syncthreads();
    if (tid < m) {
        const int64_t p = idx[tid];
        vec[LOO_MU * Npad + p] = y[p] - bj;
        vec[LOO_VAR * Npad + p] = vj;
        vec[LOO_B * Npad + p] = bj;
    }
    if (tid == 0) vec[LOO_TERM * Npad + f] = -0.5 * sc[0] + sc[1] - (double)m * 0.91893853320467274178;       // 1/2 log 2 pi
    if (!want_f) return;
    const double c = 1.0 / (1.0 + sqrt(1.0 + sc[0]));
    double* F = fac + fac_off[f];
    for (int e = tid; e < m * m; e += 256) {
        const int i = e / m, j = e - i * m;
        const double wt = (j >= i) ? W[pk(j, i)] : 0.0;
        F[e] = 0.70710678118654752440 * fma(c * b[i], u[j], wt);
    }
}

// out[r][idx_j] = sum_i in[r][idx_i] F[i][j] over the fold's points, for CV_ROWS rows
__global__ __launch_bounds__(256) void k_cv_cols(const double* __restrict__ kinv, double* __restrict__ out, int64_t ld,
                                                 const int* __restrict__ fold_off, const int* __restrict__ fold_idx,
                                                 const long long* __restrict__ fac_off, const double* __restrict__ fac) {
    __shared__ double Ps[CV_ROWS * MOGP_TILE];
    const int f = blockIdx.x, tid = threadIdx.x;
    const int64_t r0 = (int64_t)blockIdx.y * CV_ROWS;
    const int o = fold_off[f], m = fold_off[f + 1] - o;
    const int* idx = fold_idx + o;
    const double* F = fac + fac_off[f];
    for (int e = tid; e < CV_ROWS * m; e += 256) {
        const int rr = e / m, i = e - rr * m;
        Ps[rr * MOGP_TILE + i] = kinv[(r0 + rr) * ld + idx[i]];
    }
    __syncthreads();
    const int j = tid & (MOGP_TILE - 1), rh = (tid >> 7) * (CV_ROWS / 2);          // a wave has ONE row half: its reads of Ps are broadcasts
    if (j >= m) return;
    double acc[CV_ROWS / 2];
#pragma unroll
    for (int q = 0; q < CV_ROWS / 2; ++q) acc[q] = 0.0;
    for (int i = 0; i < m; ++i) {
        const double fv = F[i * m + j];
#pragma unroll
        for (int q = 0; q < CV_ROWS / 2; ++q) acc[q] = fma(Ps[(rh + q) * MOGP_TILE + i], fv, acc[q]);
    }
    const int64_t col = idx[j];
#pragma unroll
    for (int q = 0; q < CV_ROWS / 2; ++q) out[(r0 + rh + q) * ld + col] = acc[q];
}

std::atomic<unsigned long long> folds_attr_done{0};

}  // namespace

namespace mogp {

int cv_workspace(mogp_model* m, const int32_t* fold, int64_t nfolds, bool grad) {
    static_assert(MOGP_TILE == 128 && CV_ROWS * 8 == 256, "k_cv_cols: 128 columns by two row halves per workgroup");
    CvWork& w = m->cv;
    const int64_t N = m->N;
    if (nfolds < 1 || nfolds > N) return fail(MOGP_EINVAL, "mogp_exact_cv: nfolds must be 1 .. N (folds are disjoint and none is empty)");
    std::vector<int> label((size_t)N);
    std::vector<int> count((size_t)nfolds, 0);
    for (int64_t pos = 0; pos < N; ++pos) {                    // through the channel sort: label[pos] is the fold of sorted position pos
        const int32_t l = fold[m->sx.perm[pos]];
        if (l < -1 || l >= nfolds) return fail(MOGP_EINVAL, "mogp_exact_cv: fold label " + std::to_string(l) + " of row " + std::to_string(m->sx.perm[pos]) +
                                                            " is neither -1 nor in 0 .. nfolds - 1");
        label[pos] = l;
        if (l >= 0) ++count[l];
    }
    if (!(w.nfolds == nfolds && w.label == label)) {           // (a training loop asks for the same folds every time: nothing to upload)
        std::vector<int> off((size_t)nfolds + 1, 0);
        std::vector<long long> foff((size_t)nfolds + 1, 0);
        int mmax = 0;
        for (int64_t f = 0; f < nfolds; ++f) {
            if (count[f] < 1 || count[f] > MOGP_TILE)
                return fail(MOGP_EINVAL, "mogp_exact_cv: fold " + std::to_string(f) + " holds " + std::to_string(count[f]) + " points; a fold holds 1 .. " +
                                         std::to_string(MOGP_TILE));
            off[f + 1] = off[f] + count[f];
            foff[f + 1] = foff[f] + (long long)count[f] * count[f];
            mmax = std::max(mmax, count[f]);
        }
        std::vector<int> idx((size_t)std::max(off[nfolds], 1)), at(off.begin(), off.end() - 1);
        for (int64_t pos = 0; pos < N; ++pos)
            if (label[pos] >= 0) idx[at[label[pos]]++] = (int)pos;                 // within a fold: ascending sorted position
        RC(w.off.ensure(off.size())); RC(w.foff.ensure(foff.size())); RC(w.idx.ensure(idx.size()));
        w.nfolds = 0;                                          // (nothing valid until all three lists are up)
        HIP_TRY(dev_upload(w.off.p, off.data(), off.size() * sizeof(int)));
        HIP_TRY(dev_upload(w.foff.p, foff.data(), foff.size() * sizeof(long long)));
        HIP_TRY(dev_upload(w.idx.p, idx.data(), idx.size() * sizeof(int)));
        w.label.swap(label); w.nfolds = nfolds; w.mmax = mmax; w.fac_doubles = (size_t)foff[nfolds];
    }
    RC(loo_workspace(m, grad));                                // the per-point vectors and, with gradients, the N x N adjoint: LOO's own
    if (grad) RC(w.fac.ensure(w.fac_doubles));
    return 0;
}

size_t cv_bytes(const mogp_model* m) {
    const CvWork& w = m->cv;
    return (w.off.n + w.idx.n) * sizeof(int) + w.foff.n * sizeof(long long) + w.fac.n * sizeof(double);
}

int cv_folds(mogp_model* m, const double* kinv, const double* y, bool grad) {
    CvWork& w = m->cv;
    w.timed = m->profiling && grad;
    if (w.timed) for (auto& e : w.ev) if (!e) HIP_TRY(hipEventCreate(&e));
    const int64_t Npad = m->Npad;
    double* v = m->loo.vec.p;
    // mu, var and b of points in no fold: zero on the device (b = 0 is the formula; the entry point makes mu and var NaN on the host)
    HIP_TRY(hipMemsetAsync(v, 0, (size_t)LOO_COUNT * Npad * sizeof(double), m->st));
    const size_t lds = cv_lds_doubles(w.mmax) * sizeof(double);
    RC(set_max_dynamic_lds(reinterpret_cast<const void*>(k_cv_folds), (int)(cv_lds_doubles(MOGP_TILE) * sizeof(double)), folds_attr_done));
    if (w.timed) HIP_TRY(hipEventRecord(w.ev[0], m->st));
    hipLaunchKernelGGL(k_cv_folds, dim3((unsigned)w.nfolds), dim3(256), lds, m->st, kinv, Npad, m->d_alpha.p, y, w.off.p, w.idx.p, w.foff.p, w.mmax,
                       grad ? 1 : 0, Npad, v, w.fac.p, m->d_info.p);
    HIP_TRY(hipGetLastError());
    if (w.timed) HIP_TRY(hipEventRecord(w.ev[1], m->st));
    return 0;
}

int cv_fill_S(mogp_model* m, const double* kinv, double* scratch) {
    const CvWork& w = m->cv;
    const int64_t Npad = m->Npad;
    if (w.timed) HIP_TRY(hipEventRecord(w.ev[2], m->st));
    HIP_TRY(hipMemsetAsync(scratch, 0, (size_t)Npad * Npad * sizeof(double), m->st));      // the columns of points in no fold, and the padding
    hipLaunchKernelGGL(k_cv_cols, dim3((unsigned)w.nfolds, (unsigned)(Npad / CV_ROWS)), dim3(256), 0, m->st, kinv, scratch, Npad, w.off.p, w.idx.p, w.foff.p, w.fac.p);
    HIP_TRY(hipGetLastError());
    if (w.timed) HIP_TRY(hipEventRecord(w.ev[3], m->st));
    return 0;
}

}  // namespace mogp
