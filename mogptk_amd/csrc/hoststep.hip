// hoststep.hip -- the host side of one exact-GP training step of the plain MOSM kernel in native code (no device work): raw parameters ->
// constrained values, their derivatives, the term table and the noise variances; moments -> raw gradient; and the Adam update of the flat raw
// vector.  Reference: gpr/parameter.py:30-96 (Softplus / Sigmoid), gpr/multioutput.py:178-204 (the table), gpr/model.py:279-292 (loss and the
// backward autograd takes through it), torch.optim.Adam as mogptk/model.py:557-566 drives it.  The Python mirror does the same in ~60 numpy
// and ctypes operations per step, which the device waits for; every expression below keeps that mirror's operation order, so the results
// agree with it bit for bit when the caller supplies the transcendental values (lp, en) from the same exp / log1p the mirror uses.  The
// package always does (_lib.StepPlan.transcendentals: numpy's); the libm branch behind lp == en == NULL is for a C caller without numpy and
// for the stand-alone check (tools/host_step_check.cpp), and differs from numpy's values by up to 2 - 4 ulp.  These entry points have no
// model or context and return their code without a message: the binding words it.
#include "../../include/mogp_hip.h"

#include <cmath>
#include <vector>

#pragma clang fp contract(off)          // a * b + c stays two roundings, as numpy evaluates it

namespace {

// numpy's sum of a contiguous float64 vector (np.add.reduce, numpy 2.x): in order below eight elements, else eight partial sums per block
// of up to 128 and the blocks pairwise -- the shared noise scale's gradient is 2 sigma np.sum(gvar), and another association differs in the
// last bit (tests/test_host_fast_cpu.py walks every branch against the installed numpy)
double numpy_sum(const double* a, int64_t n) {
    if (n < 8) {
        double r = -0.0;
        for (int64_t i = 0; i < n; ++i) r += a[i];
        return r;
    }
    if (n <= 128) {
        double r[8];
        for (int k = 0; k < 8; ++k) r[k] = a[k];
        int64_t i = 8;
        for (; i < n - (n % 8); i += 8)
            for (int k = 0; k < 8; ++k) r[k] += a[i + k];
        double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
        for (; i < n; ++i) res += a[i];
        return res;
    }
    int64_t n2 = n / 2;
    n2 -= n2 % 8;
    return numpy_sum(a, n2) + numpy_sum(a + n2, n - n2);
}

struct Blocks {                          // offsets of [weight | mean | variance | delay | phase | scale] in the flat vector
    int64_t off[7];
    Blocks(int C, int Q, int D, int nscale) {
        const int64_t cq = (int64_t)C * Q, cqd = cq * D;
        off[0] = 0; off[1] = cq; off[2] = off[1] + cqd; off[3] = off[2] + cqd; off[4] = off[3] + cqd; off[5] = off[4] + cq; off[6] = off[5] + nscale;
    }
};

bool bad_shape(int C, int Q, int D, int nscale) { return C <= 0 || Q <= 0 || D <= 0 || (nscale != 1 && nscale != C); }

}  // namespace

extern "C" {

int mogp_mosm_step_forward(int C, int Q, int D, int nscale, const double* raw, const int* tkind, const double* lower, const double* upper,
                           const double* beta, const double* threshold, const double* lp, const double* en, double twopi, double phase_scale,
                           double* cons, double* dcons, double* table, double* noise_var) {
    if ((lp == nullptr) != (en == nullptr)) return MOGP_EINVAL;
    if (bad_shape(C, Q, D, nscale) || !raw || !tkind || !lower || !upper || !beta || !threshold || !cons || !dcons || !table || !noise_var)
        return MOGP_EINVAL;
    const Blocks b(C, Q, D, nscale);
    const int64_t n = b.off[6];
    for (int64_t k = 0; k < n; ++k) {
        const double x = raw[k];
        switch (tkind[k]) {
        case MOGP_TRANSFORM_IDENTITY:
            cons[k] = x; dcons[k] = 1.0;
            break;
        case MOGP_TRANSFORM_SOFTPLUS: {                                // parameter.py Softplus.forward / dforward
            const double z = beta[k] * x;
            if (z > threshold[k]) { cons[k] = lower[k] + x; dcons[k] = 1.0; }
            else { cons[k] = lower[k] + (lp ? lp[k] : std::log1p(std::exp(z))) / beta[k]; dcons[k] = 1.0 / (1.0 + (en ? en[k] : std::exp(-z))); }
            break;
        }
        case MOGP_TRANSFORM_SIGMOID: {                                 // parameter.py Sigmoid.forward / dforward
            const double s = 1.0 / (1.0 + (en ? en[k] : std::exp(-x))), span = upper[k] - lower[k];
            cons[k] = lower[k] + span * s; dcons[k] = span * s * (1.0 - s);
            break;
        }
        default:
            return MOGP_EINVAL;
        }
    }
    const int rc = mogp_mosm_terms(C, Q, D, cons + b.off[0], cons + b.off[1], cons + b.off[2], cons + b.off[3], cons + b.off[4], twopi, phase_scale, table);
    if (rc != MOGP_OK) return rc;
    for (int c = 0; c < C; ++c) {                                      // Model._noise_var: np.square of the scale, a shared one repeated
        const double s = cons[b.off[5] + (nscale == C ? c : 0)];
        noise_var[c] = s * s;
    }
    return MOGP_OK;
}

int mogp_mosm_step_backward(int C, int Q, int D, int nscale, const double* cons, const double* dcons, const double* table, const double* moments,
                            const double* diagG, double trG, double jitter, const double* counts, int64_t N, double twopi, double phase_scale,
                            const int* trained, double* graw) {
    if (bad_shape(C, Q, D, nscale) || N <= 0 || !cons || !dcons || !table || !moments || !diagG || !counts || !trained || !graw) return MOGP_EINVAL;
    const Blocks b(C, Q, D, nscale);
    const int W = 2 + 3 * D;
    const double jit_rel = jitter * trG / (double)N;                   // d LML / d (mean diag) through the relative jitter
    const double m2pi = -2.0 * M_PI, p2pi = 2.0 * M_PI;

    // _gtable_from_moments on Gaussian rows, the jitter's diagonal term, the sign of loss = -LML
    std::vector<double> gt((size_t)C * C * Q * W, 0.0);
    for (int i = 0; i < C; ++i)
        for (int j = 0; j <= i; ++j)
            for (int q = 0; q < Q; ++q) {
                const int64_t at = (((int64_t)i * C + j) * Q + q) * W;
                const double* tb = table + at;
                const double* mo = moments + (((int64_t)i * (i + 1) / 2 + j) * Q + q) * W;
                double* g = gt.data() + at;
                const double A = tb[0], m0 = mo[0], m4 = mo[1];
                g[0] = m0;
                g[1] = m2pi * A * m4;
                for (int d = 0; d < D; ++d) {
                    const double V = tb[2 + d], M = tb[2 + D + d], m1 = mo[2 + d], m2 = mo[2 + D + d], m3 = mo[2 + 2 * D + d];
                    g[2 + d] = -0.5 * A * m1;
                    g[2 + D + d] = m2pi * A * m3;
                    g[2 + 2 * D + d] = -V * A * m2 - p2pi * M * (A * m4);
                }
                if (i == j) g[0] += jit_rel * counts[i];
            }
    for (double& x : gt) x = -x;

    const int64_t cq = (int64_t)C * Q, cqd = cq * D;
    std::vector<double> gc(2 * cq + 3 * cqd);
    double* gw = gc.data(), *gmu = gw + cq, *gv = gmu + cqd, *gth = gv + cqd, *gph = gth + cqd;
    const int rc = mogp_mosm_terms_backward(C, Q, D, cons + b.off[0], cons + b.off[1], cons + b.off[2], cons + b.off[3], cons + b.off[4], twopi,
                                            phase_scale, gt.data(), gw, gmu, gv, gth, gph);
    if (rc != MOGP_OK) return rc;
    for (int blk = 0; blk < 5; ++blk) {                                // Parameter.accumulate_grad: times d constrained / d raw
        if (!trained[blk]) continue;
        for (int64_t k = b.off[blk]; k < b.off[blk + 1]; ++k) graw[k] = gc[k] * dcons[k];
    }
    if (trained[5]) {                                                  // Model._noise_backward
        std::vector<double> gvar(C);
        for (int c = 0; c < C; ++c) gvar[c] = diagG[c] + jit_rel * counts[c];
        const int64_t o = b.off[5];
        if (nscale == C && C > 1)
            for (int c = 0; c < C; ++c) graw[o + c] = -(2.0 * cons[o + c] * gvar[c]) * dcons[o + c];
        else
            graw[o] = -(2.0 * cons[o] * numpy_sum(gvar.data(), C)) * dcons[o];
    }
    return MOGP_OK;
}

// torch.optim.Adam over one flat vector, element for element as mogptk_amd.model._Adam.step.  The vector is `nseg` tensors end to end
// (ends[s]: one past the last element of tensor s); bc1[s] = 1 - beta1^t and bc2[s] = 1 - beta2^t of tensor s come from the caller, so no
// pow differs, and sqrt is correctly rounded on both sides
int mogp_adam_step(int nseg, const int64_t* ends, double* x, const double* g, double* m, double* v, double* vmax, double lr, double beta1,
                   double beta2, double eps, double weight_decay, int amsgrad, const double* bc1, const double* bc2) {
    if (nseg < 0 || !ends || !x || !g || !m || !v || !bc1 || !bc2 || (amsgrad && !vmax)) return MOGP_EINVAL;
    const double c1 = 1.0 - beta1, c2 = 1.0 - beta2;
    int64_t k = 0;
    for (int s = 0; s < nseg; ++s) {
        if (ends[s] < k) return MOGP_EINVAL;
        const double step = lr / bc1[s], root2 = std::sqrt(bc2[s]);
        for (; k < ends[s]; ++k) {
            double gk = g[k];
            if (weight_decay != 0.0) gk = gk + weight_decay * x[k];
            m[k] = beta1 * m[k] + c1 * gk;
            v[k] = beta2 * v[k] + c2 * gk * gk;
            double vk = v[k];
            if (amsgrad) {
                if (!(vmax[k] >= vk)) vmax[k] = (vmax[k] != vmax[k]) ? vmax[k] : vk;      // np.maximum: a NaN on either side stays
                vk = vmax[k];
            }
            x[k] = x[k] - step * m[k] / (std::sqrt(vk) / root2 + eps);
        }
    }
    return MOGP_OK;
}

}  // extern "C"
