// forecast.hip -- the rolling-origin forecast of the exact GP from ONE factorisation.  With the training points ordered by time across all
// channels and Kj = L L^T factored in that order, every leading block of L is the factor of the leading block of Kj, so with z = L^-1 r the prediction of the point
// at time position p from the points 0 .. c - 1 (any cut c <= p) is
//   E  [y_p | y_0 .. y_{c-1}] = m_p + sum_{k < c}       L[p, k] z[k],
//   Var[y_p | y_0 .. y_{c-1}] =       sum_{c <= k <= p} L[p, k]^2        (noise and jitter included),
// a prefix and a suffix sum over row p of L.  The model's storage is sorted by channel, so time order is a symmetric permutation of the Gram matrix:
//   k_sym_gather     Out[p, q] = Kj[s(p), s(q)] over the lower block triangle of the tile grid (diagonal tiles whole), the identity on the padding; without a map
//                    the plain copy of the same tiles (the way back into the factorisation's own matrix)
//   k_gather_vec     r in time order, zeros on the padding
//   k_forecast_rows  one workgroup per row of L, the longest rows first: both sums for up to MOGP_FORECAST_MAXH cuts in one pass over the row
// exact.hip (factorize with FactorPlan::gather, mogp_exact_forecast) is the schedule around them.
#include "mogp_model.h"

using namespace mogp;

namespace {

// One workgroup per 128 x 128 tile (j <= i) of the lower block triangle.  map[p] (p < N): the position in channel-sorted storage of the point at time position p.
// The element is read at (max, min) of the two storage positions: the Gram build wrote the lower triangle of `src`, nothing above it is looked at.
__global__ __launch_bounds__(256) void k_sym_gather(const double* __restrict__ src, double* __restrict__ dst, int64_t ld, int64_t N, const int* __restrict__ map) {
    const int tj = blockIdx.x, ti = blockIdx.y;
    if (tj > ti) return;
    __shared__ int sr[MOGP_TILE], sc[MOGP_TILE];
    const int64_t r0 = (int64_t)ti * MOGP_TILE, c0 = (int64_t)tj * MOGP_TILE;
    const int t = threadIdx.x;
    if (map) {
        if (t < MOGP_TILE) sr[t] = r0 + t < N ? map[r0 + t] : -1;
        else sc[t - MOGP_TILE] = c0 + (t - MOGP_TILE) < N ? map[c0 + (t - MOGP_TILE)] : -1;
        __syncthreads();
    }
    const int c = t & (MOGP_TILE - 1);
    const int64_t q = c0 + c;
    for (int r = t >> 7; r < MOGP_TILE; r += 2) {
        const int64_t p = r0 + r;
        double v;
        if (!map) v = src[p * ld + q];
        else {
            const int a = sr[r], b = sc[c];
            if (a < 0 || b < 0) v = p == q ? 1.0 : 0.0;
            else v = src[(int64_t)max(a, b) * ld + min(a, b)];
        }
        dst[p * ld + q] = v;
    }
}

__global__ __launch_bounds__(256) void k_gather_vec(const double* __restrict__ src, double* __restrict__ dst, int64_t N, int64_t Npad, const int* __restrict__ map) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p < Npad) dst[p] = p < N ? src[map[p]] : 0.0;
}

// Row p = N - 1 - blockIdx.x of L (row-major, leading dimension ld; k <= p only: the upper triangle of a diagonal tile is not L).  Thread t takes the pairs
// (k, k + 1), k = 2 t, 2 t + 512, ... in 16-byte loads, every cut's two sums in registers; then a wave64 shuffle tree and the four waves' parts added in wave
// order by one thread per sum: a fixed order, so the bits depend on (p, cut) alone -- not on H, not on the call.  cut[h * N + p] = -1: NaN.
template <int HT>
__global__ __launch_bounds__(256) void k_forecast_rows(const double* __restrict__ L, int64_t ld, int64_t N, const double* __restrict__ z,
                                                       const int* __restrict__ cut, int H, double* __restrict__ s1, double* __restrict__ s2) {
#pragma clang fp contract(off)          // a product fused into one cut's sum and not into another's would make the bits depend on H
    const int64_t p = N - 1 - (int64_t)blockIdx.x;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    __shared__ double red[4][2 * HT];
    int c[HT];
    double a1[HT], a2[HT];
#pragma unroll
    for (int h = 0; h < HT; ++h) { c[h] = h < H ? cut[(int64_t)h * N + p] : -1; a1[h] = 0.0; a2[h] = 0.0; }
    const double* row = L + p * ld;
    for (int64_t k = 2 * (int64_t)t; k <= p; k += 512) {
        double l0, l1 = 0.0, z0, z1 = 0.0;
        if (k + 1 <= p) {
            const double2 lv = *reinterpret_cast<const double2*>(row + k), zv = *reinterpret_cast<const double2*>(z + k);
            l0 = lv.x; l1 = lv.y; z0 = zv.x; z1 = zv.y;
        } else { l0 = row[k]; z0 = z[k]; }
        const double m0 = l0 * z0, m1 = l1 * z1, q0 = l0 * l0, q1 = l1 * l1;
#pragma unroll
        for (int h = 0; h < HT; ++h) {
            a1[h] += k < c[h] ? m0 : 0.0;     a2[h] += k < c[h] ? 0.0 : q0;
            a1[h] += k + 1 < c[h] ? m1 : 0.0; a2[h] += k + 1 < c[h] ? 0.0 : q1;      // (k + 1 > p: l1 = 0)
        }
    }
#pragma unroll
    for (int h = 0; h < HT; ++h) {
        for (int off = 32; off > 0; off >>= 1) { a1[h] += __shfl_down(a1[h], off, 64); a2[h] += __shfl_down(a2[h], off, 64); }
        if (lane == 0) { red[wave][2 * h] = a1[h]; red[wave][2 * h + 1] = a2[h]; }
    }
    __syncthreads();
    if (t < 2 * HT && (t >> 1) < H) {
        const int h = t >> 1;
        double s = ((red[0][t] + red[1][t]) + red[2][t]) + red[3][t];
        if (cut[(int64_t)h * N + p] < 0) s = __builtin_nan("");
        ((t & 1) ? s2 : s1)[(int64_t)h * N + p] = s;
    }
}

}  // namespace

namespace mogp {

int launch_sym_gather(const double* src, double* dst, int64_t ld, int nb, int64_t N, const int* map, hipStream_t s) {
    hipLaunchKernelGGL(k_sym_gather, dim3((unsigned)nb, (unsigned)nb), dim3(256), 0, s, src, dst, ld, N, map);
    HIP_TRY(hipGetLastError());
    return 0;
}

int launch_gather_vec(const double* src, double* dst, int64_t N, int64_t Npad, const int* map, hipStream_t s) {
    hipLaunchKernelGGL(k_gather_vec, dim3((unsigned)((Npad + 255) / 256)), dim3(256), 0, s, src, dst, N, Npad, map);
    HIP_TRY(hipGetLastError());
    return 0;
}

int launch_forecast_rows(const double* L, int64_t ld, int64_t N, const double* z, const int* cut, int H, double* s1, double* s2, hipStream_t s) {
    if (H < 1 || H > MOGP_FORECAST_MAXH) return fail(MOGP_EINVAL, "launch_forecast_rows: H outside 1 .. " + std::to_string(MOGP_FORECAST_MAXH));
    const dim3 grid((unsigned)N), block(256);
    if (H == 1) hipLaunchKernelGGL(k_forecast_rows<1>, grid, block, 0, s, L, ld, N, z, cut, H, s1, s2);
    else if (H == 2) hipLaunchKernelGGL(k_forecast_rows<2>, grid, block, 0, s, L, ld, N, z, cut, H, s1, s2);
    else if (H <= 4) hipLaunchKernelGGL(k_forecast_rows<4>, grid, block, 0, s, L, ld, N, z, cut, H, s1, s2);
    else hipLaunchKernelGGL(k_forecast_rows<8>, grid, block, 0, s, L, ld, N, z, cut, H, s1, s2);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // namespace mogp
