// Stand-alone check of the native host step (csrc/hoststep.hip, csrc/hostalg.hip) for the host sanitizers: calls mogp_mosm_step_forward,
// mogp_mosm_step_backward and mogp_adam_step on the shapes of tests/test_host_fast_cpu.py with every buffer sized exactly, so that a read or
// write past an end is an error under AddressSanitizer.  Host code only, no device, never loaded into an interpreter.  Build and run:
//   hipcc --offload-arch=gfx950 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         -x hip mogptk_amd/csrc/hostalg.hip mogptk_amd/csrc/hoststep.hip tools/host_step_check.cpp -o host_step_check && ./host_step_check
#include "../include/mogp_hip.h"

#include <cmath>
#include <cstdio>
#include <vector>

static double rnd(unsigned& s) { s = s * 1664525u + 1013904223u; return (double)(s >> 8) / (double)(1u << 24); }

static int run(int C, int Q, int D, int nscale) {
    const int W = 2 + 3 * D, cq = C * Q, cqd = cq * D, n = 2 * cq + 3 * cqd + nscale, P = C * (C + 1) / 2;
    unsigned s = 12345u + 7u * C + 3u * Q + D;
    std::vector<double> raw(n), lower(n), upper(n), beta(n), thr(n), cons(n), dcons(n), graw(n, -7.0), table((size_t)C * C * Q * W), noise(C);
    std::vector<int> kind(n);
    for (int k = 0; k < n; ++k) {
        raw[k] = 60.0 * rnd(s) - 30.0 + (k % 5 == 0 ? 250.0 : 0.0);                // every fifth beyond the softplus threshold
        kind[k] = k < cq ? MOGP_TRANSFORM_SOFTPLUS : k < cq + cqd ? MOGP_TRANSFORM_SIGMOID : k < cq + 2 * cqd ? MOGP_TRANSFORM_SOFTPLUS
                : k < 2 * cq + 3 * cqd ? MOGP_TRANSFORM_IDENTITY : MOGP_TRANSFORM_SOFTPLUS;
        lower[k] = kind[k] == MOGP_TRANSFORM_SIGMOID ? 0.01 : 1e-8; upper[k] = 0.5; beta[k] = 0.1; thr[k] = 20.0;
    }
    if (mogp_mosm_step_forward(C, Q, D, nscale, raw.data(), kind.data(), lower.data(), upper.data(), beta.data(), thr.data(), nullptr, nullptr, 2.5, 1.0, cons.data(),
                               dcons.data(), table.data(), noise.data()) != MOGP_OK) return 1;
    for (double v : cons) if (!std::isfinite(v)) return 2;
    for (double v : table) if (!std::isfinite(v)) return 3;
    std::vector<double> mom((size_t)P * Q * W), diagG(C), counts(C);
    for (double& v : mom) v = rnd(s) - 0.5;
    for (int c = 0; c < C; ++c) { diagG[c] = rnd(s) - 0.5; counts[c] = 10.0 + c; }
    const int trained[6] = {1, 1, 1, C > 1, C > 1, 1};
    if (mogp_mosm_step_backward(C, Q, D, nscale, cons.data(), dcons.data(), table.data(), mom.data(), diagG.data(), 0.3, 1e-8, counts.data(), 40, 2.5, 1.0,
                                trained, graw.data()) != MOGP_OK) return 4;
    for (int k = 0; k < n; ++k) {
        const bool set = k < cq + 2 * cqd || k >= 2 * cq + 3 * cqd || C > 1;
        if (set ? !std::isfinite(graw[k]) : graw[k] != -7.0) return 5;             // a block that is not trained stays as it was
    }
    std::vector<double> m(n, 0.0), v(n, 0.0), vmax(n, 0.0), x(raw);
    const int64_t ends[3] = {cq, cq + cqd, n};
    const double bc1[3] = {0.1, 0.19, 0.1}, bc2[3] = {0.001, 0.002, 0.001};
    for (int ams = 0; ams < 2; ++ams)
        if (mogp_adam_step(3, ends, x.data(), graw.data(), m.data(), v.data(), vmax.data(), 1e-3, 0.9, 0.999, 1e-8, ams ? 0.01 : 0.0, ams, bc1, bc2) != MOGP_OK) return 6;
    if (mogp_adam_step(3, ends, x.data(), graw.data(), m.data(), v.data(), nullptr, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, bc1, bc2) != MOGP_EINVAL) return 7;
    if (mogp_mosm_step_forward(C, Q, D, C + 1, raw.data(), kind.data(), lower.data(), upper.data(), beta.data(), thr.data(), nullptr, nullptr, 2.5, 1.0, cons.data(),
                               dcons.data(), table.data(), noise.data()) != MOGP_EINVAL) return 8;
    return 0;
}

int main() {
    const int shapes[4][3] = {{1, 1, 1}, {2, 2, 1}, {4, 3, 1}, {3, 2, 2}};
    for (const auto& sh : shapes)
        for (int shared = 0; shared < 2; ++shared) {
            const int rc = run(sh[0], sh[1], sh[2], shared ? 1 : sh[0]);
            if (rc) { std::printf("FAILED: C %d Q %d D %d nscale %d -> %d\n", sh[0], sh[1], sh[2], shared ? 1 : sh[0], rc); return 1; }
        }
    std::printf("host step check ok\n");
    return 0;
}
