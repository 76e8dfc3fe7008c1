// mean.hip -- trainable mean functions on the device (reference gpr/mean.py: ConstantMean, LinearMean, MultiOutputMean).
// Every built-in mean is one affine table: row c is coef[c] = [b_c, s_c,1 .. s_c,D] and m(x) = b_c + sum_d s_c,d x_d for a point of
// channel c (the host builds the rows from the parameters and maps the table gradient back, gpr/mean.py).  The mean enters the Gaussian
// models only through the residual r = y - m(X) (reference gpr/model.py:445-448, :518-519, :701-702), and its gradient is a per-channel
// reduction of dp/dr, which every gradient evaluation already holds on the device:
//   k_mean_residual  r[pos] = y0[pos] - coef[c][0] - sum_d coef[c][1+d] x_d[pos] over the channel-sorted rows, into the buffer the
//                    evaluations read as y (d_y); padding rows stay 0.  Run by mogp_model_set_mean / mogp_model_set_y on the critical stream.
//   k_mean_grad      g[c][j] = sum_{k in c} w_k [1, x_k][j], w = dp/dr, as per-workgroup partials over fixed chunks of each channel's
//                    segment and ONE fixed-order second stage (k_mean_grad_finish): no atomics, bit-identical from one evaluation to the next.
#include "mogp_model.h"

namespace mogp {

#define MEAN_WG 256
#define MEAN_CHUNK 2048            // points of one channel segment per workgroup of the first stage

__device__ __forceinline__ int mean_channel(const int* __restrict__ off, int C, int64_t pos) {
    int c = 0;
    while (c < C && pos >= off[c + 1]) ++c;
    return c;                                    // C: a padding row
}

__global__ __launch_bounds__(MEAN_WG) void k_mean_residual(const double* __restrict__ y0, const double* __restrict__ xs, int64_t ldx,
                                                           const int* __restrict__ off, int C, int D, const double* __restrict__ coef,
                                                           int64_t Npad, double* __restrict__ y) {
    const int64_t pos = (int64_t)blockIdx.x * MEAN_WG + threadIdx.x;
    if (pos >= Npad) return;
    const int c = mean_channel(off, C, pos);
    if (c >= C) { y[pos] = 0.0; return; }
    const double* cf = coef + (size_t)c * (1 + D);
    double r = y0[pos] - cf[0];
    for (int d = 0; d < D; ++d) r = fma(-cf[1 + d], xs[(size_t)d * ldx + pos], r);       // the host's mean_residual_host, operation for operation
    y[pos] = r;
}

// grid (nbx, C): workgroup (b, c) reduces points off[c] + [b * MEAN_CHUNK, (b + 1) * MEAN_CHUNK) of channel c into part[(c nbx + b)(1 + D) + j]
__global__ __launch_bounds__(MEAN_WG) void k_mean_grad(const double* __restrict__ w, const double* __restrict__ xs, int64_t ldx,
                                                       const int* __restrict__ off, int D, int nbx, double* __restrict__ part) {
    __shared__ double red[MOGP_MAXD + 1][MEAN_WG];
    const int c = blockIdx.y, b = blockIdx.x, tid = threadIdx.x;
    const int64_t lo = off[c] + (int64_t)b * MEAN_CHUNK;
    const int64_t hi = min((int64_t)off[c + 1], lo + MEAN_CHUNK);
    double acc[MOGP_MAXD + 1];
#pragma unroll
    for (int j = 0; j <= MOGP_MAXD; ++j) acc[j] = 0.0;
    for (int64_t pos = lo + tid; pos < hi; pos += MEAN_WG) {
        const double wk = w[pos];
        acc[0] += wk;
#pragma unroll
        for (int d = 0; d < MOGP_MAXD; ++d)
            if (d < D) acc[1 + d] = fma(wk, xs[(size_t)d * ldx + pos], acc[1 + d]);
    }
#pragma unroll
    for (int j = 0; j <= MOGP_MAXD; ++j) red[j][tid] = acc[j];
    __syncthreads();
    for (int s = MEAN_WG / 2; s > 0; s >>= 1) {
        if (tid < s)
            for (int j = 0; j <= D; ++j) red[j][tid] += red[j][tid + s];
        __syncthreads();
    }
    if (tid <= D) part[((size_t)c * nbx + b) * (1 + D) + tid] = red[tid][0];
}

__global__ void k_mean_grad_finish(const double* __restrict__ part, int D, int nbx, double scale, double* __restrict__ g) {
    const int c = blockIdx.x, j = threadIdx.x;
    if (j > D) return;
    double s = 0.0;
    for (int b = 0; b < nbx; ++b) s += part[((size_t)c * nbx + b) * (1 + D) + j];
    g[(size_t)c * (1 + D) + j] = scale * s;
}

void mean_residual_host(const mogp_model* m, const double* coef, std::vector<double>& hy) {
    const int D = m->D;
    for (int c = 0; c < m->C; ++c) {
        const double* cf = coef + (size_t)c * (1 + D);
        for (int64_t pos = m->sx.off[c]; pos < m->sx.off[c + 1]; ++pos) {
            double r = m->hy0[pos] - cf[0];
            for (int d = 0; d < D; ++d) r = std::fma(-cf[1 + d], m->sx.xs[(size_t)d * m->Npad + pos], r);
            hy[pos] = r;
        }
    }
}

int mean_apply(mogp_model* m) {
    if (!m->mean_on) return 0;
    const int C = m->C, D = m->D;
    HIP_TRY(hipMemcpyAsync(m->d_mean_coef.p, m->mean_coef.data(), (size_t)C * (1 + D) * sizeof(double), hipMemcpyHostToDevice, m->st));
    hipLaunchKernelGGL(k_mean_residual, dim3((unsigned)((m->Npad + MEAN_WG - 1) / MEAN_WG)), dim3(MEAN_WG), 0, m->st,
                       m->d_y0.p, m->d_x.p, m->Npad, m->d_chan_off.p, C, D, m->d_mean_coef.p, m->Npad, m->d_y.p);
    HIP_TRY(hipGetLastError());
    mean_residual_host(m, m->mean_coef.data(), m->hy);
    // d_y is read on other streams too (the Titsias side stream, the prediction's substitution stream): they wait for the residual
    HIP_TRY(hipEventRecord(m->mean_ev, m->st));
    for (hipStream_t q : {m->st2, m->st2u, m->st3, m->st4, m->ctx->st5, m->st_priv})
        if (q && q != m->st) HIP_TRY(hipStreamWaitEvent(q, m->mean_ev, 0));
    return 0;
}

int mean_grad_enqueue(mogp_model* m, const double* w, double scale) {
    m->mean_w = w;
    m->mean_w_scale = scale;
    m->mean_g_valid = false;
    if (!m->mean_on) return 0;
    const int C = m->C, D = m->D;
    int nbx = 1;
    for (int c = 0; c < C; ++c) nbx = std::max(nbx, (m->sx.off[c + 1] - m->sx.off[c] + MEAN_CHUNK - 1) / MEAN_CHUNK);
    int rc;
    if ((rc = m->d_mean_part.ensure((size_t)C * nbx * (1 + D)))) return rc;
    hipLaunchKernelGGL(k_mean_grad, dim3((unsigned)nbx, (unsigned)C), dim3(MEAN_WG), 0, m->st, w, m->d_x.p, m->Npad, m->d_chan_off.p, D, nbx,
                       m->d_mean_part.p);
    hipLaunchKernelGGL(k_mean_grad_finish, dim3((unsigned)C), dim3(64), 0, m->st, m->d_mean_part.p, D, nbx, scale, m->d_mean_g.p);
    HIP_TRY(hipGetLastError());
    // on the evaluation's stream, next to its own device-to-host copies: the evaluation's one wait covers it
    HIP_TRY(hipMemcpyAsync(m->h_mean_pin, m->d_mean_g.p, (size_t)C * (1 + D) * sizeof(double), hipMemcpyDeviceToHost, m->st));
    m->mean_g_pending = true;
    return 0;
}

void mean_grad_collect(mogp_model* m) {
    if (!m->mean_g_pending) return;
    m->mean_g_pending = false;
    m->mean_g.assign(m->h_mean_pin, m->h_mean_pin + (size_t)m->C * (1 + m->D));
    m->mean_g_valid = true;
}

void mean_release(mogp_model* m) {
    m->d_y0.release(); m->d_mean_coef.release(); m->d_mean_part.release(); m->d_mean_g.release();
    if (m->h_mean_pin) { hipError_t e = hipHostFree(m->h_mean_pin); (void)e; m->h_mean_pin = nullptr; }
    if (m->mean_ev) { hipError_t e = hipEventDestroy(m->mean_ev); (void)e; m->mean_ev = nullptr; }
}

}  // namespace mogp

using namespace mogp;

extern "C" {

int mogp_model_set_mean(mogp_model* m, const double* coef) {
    if (!m) return fail(MOGP_EINVAL, "mogp_model_set_mean: model is null");
    int rc;
    if ((rc = use_device(m->ctx))) return rc;
    const int C = m->C, D = m->D;
    const size_t n = (size_t)C * (1 + D);
    if (!coef) {
        if (!m->mean_on) return MOGP_OK;
        m->mean_on = false;
        m->mean_g_valid = m->mean_g_pending = false;
        HIP_TRY(hipMemcpyAsync(m->d_y.p, m->d_y0.p, m->Npad * sizeof(double), hipMemcpyDeviceToDevice, m->st));
        HIP_TRY(hipStreamSynchronize(m->st));
        m->hy = m->hy0;
        mean_release(m);
        return MOGP_OK;
    }
    for (size_t i = 0; i < n; ++i)
        if (!std::isfinite(coef[i])) return fail(MOGP_ENONFINITE, "mean table has non-finite entries (mean parameters diverged)");
    if (m->mean_on && std::memcmp(m->mean_coef.data(), coef, n * sizeof(double)) == 0) return MOGP_OK;      // unchanged: d_y is current
    if (!m->mean_on) {
        if ((rc = m->d_y0.ensure(m->Npad))) return rc;
        if ((rc = m->d_mean_coef.ensure(n))) return rc;
        if ((rc = m->d_mean_g.ensure(n))) return rc;
        if (!m->h_mean_pin) HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&m->h_mean_pin), n * sizeof(double), hipHostMallocDefault));
        if (!m->mean_ev) HIP_TRY(hipEventCreateWithFlags(&m->mean_ev, hipEventDisableTiming));
        HIP_TRY(hipMemcpyAsync(m->d_y0.p, m->d_y.p, m->Npad * sizeof(double), hipMemcpyDeviceToDevice, m->st));      // d_y holds the raw targets now
        m->hy0 = m->hy;
        m->mean_on = true;
    }
    m->mean_coef.assign(coef, coef + n);
    m->mean_g_valid = m->mean_g_pending = false;
    return mean_apply(m);
}

int mogp_model_mean_grad(mogp_model* m, double* g) {
    if (!m || !g) return fail(MOGP_EINVAL, "mogp_model_mean_grad: bad argument");
    if (!m->mean_on) return fail(MOGP_EINVAL, "mogp_model_mean_grad: no mean table is set (mogp_model_set_mean)");
    if (!m->mean_g_valid) return fail(MOGP_EINVAL, "mogp_model_mean_grad: no gradient evaluation since the mean table was set");
    std::memcpy(g, m->mean_g.data(), m->mean_g.size() * sizeof(double));
    return MOGP_OK;
}

}  // extern "C"
