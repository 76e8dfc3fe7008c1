// gram.hip -- spectral Gram builder and gradient-moment pass (gfx950).
//
// Every MOSM / SM / CSM channel-pair block is   K_ab = sum_t A_t exp(-1/2 sum_d V_td u_d^2) cos(2 pi (sum_d M_td u_d + Psi_t)),
// u_d = x_a,d - x_b,d + Delta_td   (reference: gpr/multioutput.py:182-204, :432-449; gpr/singleoutput.py:594-600).
//
// Cosine: splits per point,  cos(2 pi (p_a - q_b)) = cos(2 pi p_a) cos(2 pi q_b) + sin(2 pi p_a) sin(2 pi q_b)  with
// p_a = sum_d M_d (x_a,d + Delta_d) + Psi,  q_b = sum_d M_d x_b,d.  The per-point factors are computed ONCE per launch into a phase
// table (k_phase_table: C T N sincospi instead of one per point and tile) and read back by the tiles.
//
// Gaussian: one 64x64 tile of sorted time series spans a small input range, so with the tile centres c_r, c_c
// (p = x_a - c_r, q = x_b - c_c, s = c_r - c_c + Delta, u = p - q + s)
//     exp(-1/2 V u^2) = exp(-1/2 V s^2) * exp(-1/2 V (p^2 + 2 p s)) * exp(-1/2 V (q^2 - 2 q s)) * exp(V p q)
//                       per tile            per row                     per column                   per entry, |V p q| small.
// The per-row / per-column factors are folded into the staged cosine factors (128 exp per tile and term instead of 4096) and the
// cross term is a Taylor polynomial whose degree (4 .. 14) is chosen per tile and term from max |V p q| (truncation < 2e-17): an entry
// costs one multiply, N FMAs and three more FMAs instead of a library exp.  Tiles whose inputs are spread too far for that (unsorted
// rows, huge gaps) take the general path (exp per entry); a term whose Gaussian is below e^-50 everywhere in the tile is skipped
// (absolute error < 2e-22 A).  One workgroup = one 64x64 tile of one channel-pair block, 256 threads, 4x4 entries per thread; full
// interior tiles store 32-byte runs.
#include "mogp_internal.h"

#include <algorithm>
#include <vector>
#include <cstdlib>

// measurement switches of the tile kernels (no stores / no terms / constant staging: tools/r4_gram_lds.sh) exist only in a build with
// -DMOGP_GRAM_DEBUG; in the product kernels the conditions are the constant 0 and the branches are gone
#ifdef MOGP_GRAM_DEBUG
#define GRAM_DBG(a, bit) ((a).dbg & (bit))
#else
#define GRAM_DBG(a, bit) 0
#endif

namespace mogp {

typedef double d2_t __attribute__((ext_vector_type(2)));

__device__ __forceinline__ double frac_turn(double p) { return p - rint(p); }

#define GT_SKIP (-1)     // term negligible in this tile
#define GT_GENERAL 0     // exp per entry
#define GT_SKIP_EXPONENT 50.0
// Taylor degree of the cross term exp(V p q) from max |V p q| over the tile: the smallest N with zmax^(N+1) / (N+1)! <= 2e-17 (round 6: every degree from 4 to 12 instead
// of 4 / 6 / 8 / 11 / 14 -- at configs[1] (zmax 0.012 .. 0.12) an entry's polynomial is 1 - 2 terms shorter)
#define GT_DEGREE(zmax) ((zmax) <= 1.19e-3 ? 4 : (zmax) <= 4.93e-3 ? 5 : (zmax) <= 0.0139 ? 6 : (zmax) <= 0.0308 ? 7 : (zmax) <= 0.0578 ? 8 : (zmax) <= 0.0968 ? 9 : \
                         (zmax) <= 0.149 ? 10 : (zmax) <= 0.2147 ? 11 : (zmax) <= 0.294 ? 12 : 14)
#define GT_DEGREE_CASES(X) X(4) X(5) X(6) X(7) X(8) X(9) X(10) X(11) X(12) X(14)

// e^x for |x| < 700: Cody-Waite reduction, degree-13 Taylor on |r| <= ln2 / 2 (truncation 4e-18), ldexp
__device__ __forceinline__ double fast_exp(double x) {
    const double n = rint(x * 1.44269504088896338700e+00);
    double r = fma(-n, 6.93147180369123816490e-01, x);
    r = fma(-n, 1.90821492927058770002e-10, r);
    double p = 1.6059043836821613e-10;                  // 1/13!
    p = fma(p, r, 2.08767569878681e-09);                // 1/12!
    p = fma(p, r, 2.505210838544172e-08);               // 1/11!
    p = fma(p, r, 2.755731922398589e-07);               // 1/10!
    p = fma(p, r, 2.7557319223985893e-06);              // 1/9!
    p = fma(p, r, 2.48015873015873e-05);                // 1/8!
    p = fma(p, r, 1.984126984126984e-04);               // 1/7!
    p = fma(p, r, 1.388888888888889e-03);               // 1/6!
    p = fma(p, r, 8.333333333333333e-03);               // 1/5!
    p = fma(p, r, 4.1666666666666664e-02);              // 1/4!
    p = fma(p, r, 1.6666666666666666e-01);              // 1/3!
    p = fma(p, r, 0.5);
    p = fma(p, r, 1.0);
    p = fma(p, r, 1.0);
    return ldexp(p, (int)n);
}

// sum_{k <= N} z^k / k!   (Horner)
template <int N>
__device__ __forceinline__ double exp_taylor(double z) {
    constexpr double c[15] = {1.0, 1.0, 0.5, 1.6666666666666666e-01, 4.1666666666666664e-02, 8.333333333333333e-03,
                              1.388888888888889e-03, 1.984126984126984e-04, 2.48015873015873e-05, 2.7557319223985893e-06,
                              2.755731922398589e-07, 2.505210838544172e-08, 2.08767569878681e-09, 1.6059043836821613e-10,
                              1.1470745597729725e-11};
    double p = c[N];
#pragma unroll
    for (int k = N - 1; k >= 0; --k) p = fma(p, z, c[k]);
    return p;
}

// ---- phase table: cos / sin of the per-point phases, once per launch --------------------------------------------------------
// role 0 (rows):    cs[(o T + t) ld + a] = cos 2 pi (sum_d M_d (x_a,d + Delta_d) + Psi)   of pair (chan(a), o), term t
// role 1 (columns): cs[(o T + t) ld + b] = cos 2 pi (sum_d M_d x_b,d)                     of pair (o, chan(b)), term t
struct PhaseArgs {
    const double* x; int64_t ld; const int* off; const double* table; int T, D, C, W, role; double* cs; double* sn;
};
__global__ __launch_bounds__(256) void k_phase_table(PhaseArgs a) {
    const int64_t pt = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (pt >= a.off[a.C]) return;
    const int o = blockIdx.y, t = blockIdx.z, D = a.D, W = a.W;
    int c = 0;
    while (pt >= a.off[c + 1]) ++c;
    const int pair = a.role == 0 ? c * a.C + o : o * a.C + c;
    const double* row = a.table + ((size_t)pair * a.T + t) * W;
    double ph = a.role == 0 ? row[1] : 0.0;
    for (int d = 0; d < D; ++d) {
        const double m = row[2 + D + d], xv = a.x[(size_t)d * a.ld + pt];
        ph = a.role == 0 ? fma(m, xv + row[2 + 2 * D + d], ph) : fma(m, xv, ph);
    }
    double sn, cs;
    sincospi(2.0 * frac_turn(ph), &sn, &cs);
    const size_t idx = ((size_t)o * a.T + t) * a.ld + pt;
    a.cs[idx] = cs;
    a.sn[idx] = sn;
}

// centre and half span of every 64-point block of every channel (the row / column ranges of the tiles), stored at the index of the
// block's first point:  cen[d * ld + start], half[d * ld + start].  One wave per block.
struct CentreArgs { const double* x; int64_t ld; const int* off; int C, D; double* cen; double* half; };
__global__ __launch_bounds__(64) void k_block_centres(CentreArgs a) {
    int b = blockIdx.x, c = 0;
    for (; c < a.C; ++c) {
        const int nb = (a.off[c + 1] - a.off[c] + MOGP_GT - 1) / MOGP_GT;
        if (b < nb) break;
        b -= nb;
    }
    if (c >= a.C) return;
    const int start = a.off[c] + b * MOGP_GT, n = min(MOGP_GT, a.off[c + 1] - start), lane = threadIdx.x;
    for (int d = 0; d < a.D; ++d) {
        const double v = a.x[(size_t)d * a.ld + start + (lane < n ? lane : 0)];
        double lo = v, hi = v;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) { lo = fmin(lo, __shfl_xor(lo, off, 64)); hi = fmax(hi, __shfl_xor(hi, off, 64)); }
        if (lane == 0) { a.cen[(size_t)d * a.ld + start] = 0.5 * (lo + hi); a.half[(size_t)d * a.ld + start] = 0.5 * (hi - lo); }
    }
}

// workspace layout: [row cos | row sin] (C T ldr each) [col cos | col sin] (C T ldc each) [row centres | row half spans] (D ldr each)
// [col centres | col half spans] (D ldc each)
size_t phase_ws_doubles(int C, int T, int64_t ldr, int64_t ldc) { return (size_t)2 * (C * T + MOGP_MAXD) * (size_t)(ldr + ldc); }   // sized for any D

struct PhaseView {                       // device pointers into the workspace of one launch
    const double *rcs, *rsn, *ccs, *csn, *rcen, *rhalf, *ccen, *chalf;
};
__host__ __device__ static inline PhaseView phase_view(double* ws, int C, int T, int D, int64_t ldr, int64_t ldc) {
    PhaseView v;
    double* p = ws;
    v.rcs = p; p += (size_t)C * T * ldr; v.rsn = p; p += (size_t)C * T * ldr;
    v.ccs = p; p += (size_t)C * T * ldc; v.csn = p; p += (size_t)C * T * ldc;
    v.rcen = p; p += (size_t)D * ldr; v.rhalf = p; p += (size_t)D * ldr;
    v.ccen = p; p += (size_t)D * ldc; v.chalf = p;
    return v;
}

static int launch_phase_tables(const PhaseRef& ph, const double* xr, int64_t ldxr, int64_t nr, const double* xc, int64_t ldxc, int64_t nc,
                               const double* table, int T, int D, int C, int W, hipStream_t s) {
    if (!ph.ws || !ph.offr || !ph.offc) { set_error("Gram / moment launch without a phase workspace"); return -1; }
    const PhaseView v = phase_view(ph.ws, C, T, D, ldxr, ldxc);
    PhaseArgs a;
    a.table = table; a.T = T; a.D = D; a.C = C; a.W = W;
    a.x = xr; a.ld = ldxr; a.off = ph.offr; a.role = 0; a.cs = const_cast<double*>(v.rcs); a.sn = const_cast<double*>(v.rsn);
    if (nr > 0) hipLaunchKernelGGL(k_phase_table, dim3((unsigned)((nr + 255) / 256), C, T), dim3(256), 0, s, a);
    a.x = xc; a.ld = ldxc; a.off = ph.offc; a.role = 1; a.cs = const_cast<double*>(v.ccs); a.sn = const_cast<double*>(v.csn);
    if (nc > 0) hipLaunchKernelGGL(k_phase_table, dim3((unsigned)((nc + 255) / 256), C, T), dim3(256), 0, s, a);
    CentreArgs c;
    c.C = C; c.D = D;
    c.x = xr; c.ld = ldxr; c.off = ph.offr; c.cen = const_cast<double*>(v.rcen); c.half = const_cast<double*>(v.rhalf);
    if (nr > 0) hipLaunchKernelGGL(k_block_centres, dim3((unsigned)((nr + MOGP_GT - 1) / MOGP_GT + C)), dim3(64), 0, s, c);
    c.x = xc; c.ld = ldxc; c.off = ph.offc; c.cen = const_cast<double*>(v.ccen); c.half = const_cast<double*>(v.chalf);
    if (nc > 0) hipLaunchKernelGGL(k_block_centres, dim3((unsigned)((nc + MOGP_GT - 1) / MOGP_GT + C)), dim3(64), 0, s, c);
    HIP_TRY(hipGetLastError());
    return 0;
}

// ---- per-tile staging shared by the Gram and the moment kernel -----------------------------------------------------------------
// Everything a tile needs from global memory depends on its descriptor only and is requested in ONE batch (the thread's own centred
// inputs, and for each of its staging items the term-table row, the point's input and its phase factors); every thread derives the
// term's mode and tile scalars itself (a handful of flops, identical in all threads), so a chunk of terms costs one barrier.
template <int DM>
struct TileLds {
    double cu[MOGP_TC][MOGP_GT], su[MOGP_TC][MOGP_GT], cw[MOGP_TC][MOGP_GT], sw[MOGP_TC][MOGP_GT];
    double V[MOGP_TC][DM], s[MOGP_TC][DM], M[MOGP_TC][DM], A[MOGP_TC];
    double Kp[MOGP_TC][DM];                                // coefficient of the cross term p q: V - L / 4 (= V without an envelope)
    double L[MOGP_TC][DM], e[MOGP_TC][DM];                 // envelope precision and offset: (x_a + x_b)/2 - c = (p + q)/2 + e
    int deg[MOGP_TC];
};
template <int DM>
struct TileCtx { double cr[DM], cc[DM], hr[DM], hc[DM]; };      // tile centres and half spans (rows, columns)

template <int DM>
__device__ __forceinline__ void tile_centres(TileCtx<DM>& X, const GTile& tl, int D, const PhaseView& v, int64_t ldxr, int64_t ldxc) {
    for (int d = 0; d < D; ++d) {
        X.cr[d] = v.rcen[(size_t)d * ldxr + tl.r0]; X.hr[d] = v.rhalf[(size_t)d * ldxr + tl.r0];
        X.cc[d] = v.ccen[(size_t)d * ldxc + tl.c0]; X.hc[d] = v.chalf[(size_t)d * ldxc + tl.c0];
    }
}

template <int DM>
__device__ __forceinline__ void tile_context(TileCtx<DM>& X, double (&p)[4][DM], double (&q)[4][DM], const GTile& tl, int D,
                                             const PhaseView& v, const double* __restrict__ xr, int64_t ldxr,
                                             const double* __restrict__ xc, int64_t ldxc, int rg, int cg) {
    tile_centres<DM>(X, tl, D, v, ldxr, ldxc);
#pragma unroll
    for (int m = 0; m < 4; ++m)
        for (int d = 0; d < D; ++d) {
            p[m][d] = xr[(size_t)d * ldxr + tl.r0 + min(rg * 4 + m, tl.nr - 1)] - X.cr[d];
            q[m][d] = xc[(size_t)d * ldxc + tl.c0 + min(cg * 4 + m, tl.nc - 1)] - X.cc[d];
        }
}

constexpr int STAGE_ITEMS = MOGP_TC * MOGP_GT * 2 / 256;      // staging items per thread and chunk (4)
template <int DM>
struct StageItem { double x[DM], cs, sn; };                   // what is prefetched per item: the point's input and its phase factors

template <int DM>
__device__ __forceinline__ void stage_item_load(StageItem<DM>& I, int which, int t, int pnt, const GTile& tl, int D, int C, int T, int t0,
                                                const PhaseView& v, const double* __restrict__ xr, int64_t ldxr,
                                                const double* __restrict__ xc, int64_t ldxc) {
    const int i = tl.pair / C, j = tl.pair - i * C;
    if (which == 0) {
        const int64_t g = tl.r0 + min(pnt, tl.nr - 1);
        const size_t k = ((size_t)j * T + t0 + t) * ldxr + g;             // rows: table (j, t, point)
        I.cs = v.rcs[k]; I.sn = v.rsn[k];
        for (int d = 0; d < D; ++d) I.x[d] = xr[(size_t)d * ldxr + g];
    } else {
        const int64_t g = tl.c0 + min(pnt, tl.nc - 1);
        const size_t k = ((size_t)i * T + t0 + t) * ldxc + g;             // columns: table (i, t, point)
        I.cs = v.ccs[k]; I.sn = v.csn[k];
        for (int d = 0; d < D; ++d) I.x[d] = xc[(size_t)d * ldxc + g];
    }
}

// AMP: fold the amplitude A_t into the row factors (Gram); otherwise unit amplitude (moments).  `tab`: the pair's term rows (LDS copy or
// global memory -- a generic pointer), W doubles each.
// RAD: a launch with radial profiles (below): no Gaussian factor is split off, every term runs entry by entry (GT_GENERAL) and the staged
// factors are the plain phase factors (times the amplitude; not for the periodic profile, whose phase is the profile's argument).
// `kinds`: the pair's kind row (RAD only).  GATE: 1 = the instantiation that carries the gate row, 2 = the one that carries the gate,
// weighted-dot and white rows (all below); an instantiation holds none of the code of the rows it does not carry
// SPLIT = false (k_gram_dx): no tile-centred split -- a Gaussian term is GT_SKIP or GT_GENERAL and the staged factors are the plain phase factors
template <int DM, bool AMP, bool RAD = false, int GATE = 0, bool SPLIT = true>
__device__ __forceinline__ void stage_item_compute(TileLds<DM>& L, const StageItem<DM>& I, const TileCtx<DM>& X, const double* tab, int W,
                                                   int which, int t, int pnt, int D, int t0, const int* kinds = nullptr) {
    const double* row = tab + (size_t)(t0 + t) * W;
    const double A = row[0];
    if constexpr (RAD) {
        const int kd = kinds[t0 + t] & MOGP_KIND_MASK;
        const bool per = kd == MOGP_KIND_PERIODIC, dot = kd == MOGP_KIND_DOT;
        const int deg = (AMP && A == 0.0 && !dot) ? GT_SKIP : GT_GENERAL;      // (a dot-product row of zero amplitude is c^n, not zero)
        if (pnt == 0 && which == 0) {
            L.deg[t] = deg; L.A[t] = A;
            for (int d = 0; d < D; ++d) {
                L.V[t][d] = row[2 + d]; L.M[t][d] = row[2 + D + d];
                L.s[t][d] = (X.cr[d] - X.cc[d]) + row[2 + 2 * D + d];
                L.Kp[t][d] = X.cr[d]; L.L[t][d] = X.cc[d];      // the tile centres: a dot-product row needs the inputs themselves (dot_row_base)
            }
            L.e[t][0] = row[1];                                 // its bias rides in the Psi slot
        }
        if (deg == GT_SKIP) return;
        if (dot) return;                                        // no phase factors: the staged slots of the row are not read
        if (GATE > 1 && (kd == MOGP_KIND_WDOT || kd == MOGP_KIND_WHITE)) return;      // nothing per point: the centres above, the tile's diagonal flag
        if (GATE && kd == MOGP_KIND_GATE) {
            // the sigmoid weight of the point, h = sigmoid(z), z = beta (x - l) (beta in the V slot, l in the M slot; D = 1), once per row / column
            // point of the tile: cu / cw carry h (the rows' times the amplitude when AMP), su / sw its complement sigmoid(-z) -- never 1 - h.
            // e = exp(-|z|) <= 1 for every finite z: nothing overflows, and a saturated gate gives 0 or 1
            const double z = row[2] * (I.x[0] - row[2 + D]);
            const double e = exp(-fabs(z)), r = 1.0 / (1.0 + e);
            const double h = z >= 0.0 ? r : e * r, hc = z >= 0.0 ? e * r : r;
            if (which == 0) { L.cu[t][pnt] = (AMP ? A : 1.0) * h; L.su[t][pnt] = hc; }
            else { L.cw[t][pnt] = h; L.sw[t][pnt] = hc; }
            return;
        }
        const double f = (AMP && !per) ? A : 1.0;
        if (which == 0) { L.cu[t][pnt] = f * I.cs; L.su[t][pnt] = f * I.sn; }
        else { L.cw[t][pnt] = I.cs; L.sw[t][pnt] = I.sn; }
        return;
    }
    const bool env = W > 2 + 3 * D;
    double zmax = 0.0, es = 0.0, emin = 0.0, efac = 0.0, s[DM], V[DM], Lv[DM], er[DM], ec[DM];
    for (int d = 0; d < D; ++d) {
        V[d] = row[2 + d];
        Lv[d] = env ? row[2 + 3 * D + d] : 0.0;
        const double cn = env ? row[2 + 4 * D + d] : 0.0;
        er[d] = X.cr[d] - cn; ec[d] = X.cc[d] - cn;
        const double hr = X.hr[d], hc = X.hc[d];
        s[d] = (X.cr[d] - X.cc[d]) + row[2 + 2 * D + d];
        zmax += fabs(V[d] - 0.25 * Lv[d]) * hr * hc;
        es += V[d] * s[d] * s[d];
        const double mu = fmax(0.0, fabs(s[d]) - hr - hc);                      // smallest |u_d| in the tile
        emin += V[d] * mu * mu;
        const double amax = 0.5 * (fabs(er[d]) + hr + fabs(ec[d]) + hc);          // largest |midpoint - c| in the tile
        efac += fabs(V[d]) * (hr * hr + hc * hc + 2.0 * (hr + hc) * fabs(s[d])) + Lv[d] * amax * amax;    // bound on the row / column exponents
    }
    int deg;
    if ((AMP && A == 0.0) || 0.5 * emin > GT_SKIP_EXPONENT) deg = GT_SKIP;
    else if (!SPLIT || !(zmax <= 0.45) || !(0.5 * es < 600.0) || !(0.5 * efac < 600.0)) deg = GT_GENERAL;
    else deg = GT_DEGREE(zmax);
    if (pnt == 0 && which == 0) {
        L.deg[t] = deg; L.A[t] = A;
        for (int d = 0; d < D; ++d) {
            L.V[t][d] = V[d]; L.s[t][d] = s[d]; L.M[t][d] = row[2 + D + d];
            L.Kp[t][d] = V[d] - 0.25 * Lv[d]; L.L[t][d] = Lv[d]; L.e[t][d] = 0.5 * (er[d] + ec[d]);
        }
    }
    if (deg == GT_SKIP) return;
    double f = 1.0;
    if (deg != GT_GENERAL) {
        // exponent = -1/2 V (p - q + s)^2 - L/8 ((p + er) + (q + ec))^2, split into a row part, a column part and the cross term (V - L/4) p q
        double e = 0.0;
        if (which == 0) {                                  // rows: the tile scalars exp(-1/2 V s^2 - L/4 er ec) included
            for (int d = 0; d < D; ++d) {
                const double pp = I.x[d] - X.cr[d];
                e = fma(V[d], fma(pp, pp, s[d] * s[d]) + 2.0 * pp * s[d], e);
                const double pe = pp + er[d];
                e = fma(0.25 * Lv[d], pe * pe + 2.0 * ec[d] * pe, e);
            }
        } else {                                           // columns
            for (int d = 0; d < D; ++d) {
                const double qq = I.x[d] - X.cc[d];
                e = fma(V[d], qq * qq - 2.0 * qq * s[d], e);
                const double qe = qq + ec[d];
                e = fma(0.25 * Lv[d], qe * qe + 2.0 * qq * er[d], e);
            }
        }
        f = fast_exp(-0.5 * e);
    }
    if (which == 0) {
        if (AMP) f *= A;
        L.cu[t][pnt] = f * I.cs; L.su[t][pnt] = f * I.sn;
    } else {
        L.cw[t][pnt] = f * I.cs; L.sw[t][pnt] = f * I.sn;
    }
}

// Staging items of a chunk: (rows | columns) x term x point.  Wave w of the workgroup handles rows (w even) or columns (w odd) of the terms
// w / 2, w / 2 + 2, w / 2 + 4, w / 2 + 6, lane = point: no index arithmetic, and which / t are wave-uniform.
#define STAGE_MAP(tid) const int st_wave = __builtin_amdgcn_readfirstlane((tid) >> 6), st_which = st_wave & 1, st_tb = st_wave >> 1, st_pnt = (tid) & 63

// one chunk of terms into LDS; BATCH: all items' loads first (one memory round trip), else item by item (large D: registers)
template <int DM, bool AMP, bool BATCH, bool RAD = false, int GATE = 0, bool SPLIT = true>
__device__ __forceinline__ void stage_chunk(TileLds<DM>& L, const TileCtx<DM>& X, const GTile& tl, const double* tab, int W, int D,
                                            int C, int T, int t0, int nt, const PhaseView& v, const double* __restrict__ xr, int64_t ldxr,
                                            const double* __restrict__ xc, int64_t ldxc, int tid, const int* kinds = nullptr) {
    STAGE_MAP(tid);
    if (BATCH) {
        StageItem<DM> I[STAGE_ITEMS];
#pragma unroll
        for (int k = 0; k < STAGE_ITEMS; ++k)
            if (st_tb + 2 * k < nt) stage_item_load<DM>(I[k], st_which, st_tb + 2 * k, st_pnt, tl, D, C, T, t0, v, xr, ldxr, xc, ldxc);
#pragma unroll
        for (int k = 0; k < STAGE_ITEMS; ++k)
            if (st_tb + 2 * k < nt) stage_item_compute<DM, AMP, RAD, GATE, SPLIT>(L, I[k], X, tab, W, st_which, st_tb + 2 * k, st_pnt, D, t0, kinds);
    } else {
        for (int t = st_tb; t < nt; t += 2) {
            StageItem<DM> I;
            stage_item_load<DM>(I, st_which, t, st_pnt, tl, D, C, T, t0, v, xr, ldxr, xc, ldxc);
            stage_item_compute<DM, AMP, RAD, GATE, SPLIT>(L, I, X, tab, W, st_which, t, st_pnt, D, t0, kinds);
        }
    }
}

// Gaussian factor of one entry on the general path
template <int DM>
__device__ __forceinline__ double gauss_general(const double (&p)[DM], const double (&q)[DM], const double* V, const double* s,
                                                const double* Lv, const double* ev, int D) {
    double arg = 0.0;
    for (int d = 0; d < D; ++d) {
        const double u = (p[d] - q[d]) + s[d];
        arg = fma(V[d] * u, u, arg);
        const double a = 0.5 * (p[d] + q[d]) + ev[d];          // envelope on the midpoint (L = 0 without one)
        arg = fma(Lv[d] * a, a, arg);
    }
    return exp(-0.5 * arg);
}

template <int DM, int N>
__device__ __forceinline__ void gram_term(double (&acc)[4][4], const double (&p)[4][DM], const double (&q)[4][DM], const TileLds<DM>& L, int t,
                                          int D, const double (&cu)[4], const double (&su)[4], const double (&cw)[4], const double (&sw)[4]) {
    double vp[4][DM];
    if (N > 0) {
#pragma unroll
        for (int m = 0; m < 4; ++m)
            for (int d = 0; d < D; ++d) vp[m][d] = L.Kp[t][d] * p[m][d];
    }
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        if (m == 2) __builtin_amdgcn_sched_barrier(0);      // two groups of eight independent Horner chains: enough to cover the FMA
                                                            // latency, half the live registers of sixteen
#pragma unroll
        for (int n = 0; n < 4; ++n) {
            double e;
            if (N > 0) {
                double z = vp[m][0] * q[n][0];
                for (int d = 1; d < D; ++d) z = fma(vp[m][d], q[n][d], z);
                e = exp_taylor<N>(z);
            } else {
                e = gauss_general<DM>(p[m], q[n], L.V[t], L.s[t], L.L[t], L.e[t], D);
            }
            acc[m][n] = fma(e, fma(cu[m], cw[n], su[m] * sw[n]), acc[m][n]);
        }
    }
}

// ---- radial profiles --------------------------------------------------------------------------------------------------
// A term's Gaussian exp(-s/2), s = sum_d V_d u_d^2, generalised to a profile phi_kind(s) per (channel pair, term): rational quadratic and
// Matern 1/2, 3/2, 5/2 (reference gpr/singleoutput.py: RationalQuadraticKernel, MaternKernel, ExponentialKernel).  None of them factorises
// over rows and columns, so there is no tile-centred split: one library exp (and a square root) per entry and term.  The kind is uniform
// over a tile's term -- a tile never straddles a channel pair -- so the switch below does not diverge.
// PSI: also psi = -2 dphi/ds, the weight of the moments m1_d, m2_d (d/dV_d).  The only singular one is Matern 1/2 at s = 0 (exp(-r) / r):
// there psi is RETURNED as 0, which makes the products u_d^2 psi and u_d psi the limit they have (0) without ever forming 0 * inf.
template <bool PSI>
__device__ __forceinline__ void radial_profile(int kind, double shape, double s, double& phi, double& psi) {
    s = fmax(s, 0.0);
    switch (kind) {
        case MOGP_KIND_RQ: {
            const double b = fma(s, 0.5 / shape, 1.0);
            phi = exp(-shape * log(b));
            if (PSI) psi = phi / b;
        } break;
        case MOGP_KIND_MATERN12: {
            const double r = sqrt(s);
            phi = exp(-r);
            if (PSI) psi = s > 0.0 ? phi / r : 0.0;
        } break;
        case MOGP_KIND_MATERN32: {
            const double r = sqrt(3.0 * s), e = exp(-r);
            phi = fma(r, e, e);
            if (PSI) psi = 3.0 * e;
        } break;
        case MOGP_KIND_MATERN52: {
            const double r = sqrt(5.0 * s), e = exp(-r);
            phi = fma(r, r, 3.0 * (1.0 + r)) * (e * (1.0 / 3.0));
            if (PSI) psi = (5.0 / 3.0) * fma(r, e, e);
        } break;
        case MOGP_KIND_SINC: {
            // phi = sin(pi r) / (pi r), psi = (phi - cos(pi r)) / r^2; both are even power series in x = pi^2 s with removable singularities at 0:
            //   phi = sum_k (-x)^k / (2k + 1)!,   psi = pi^2 sum_k (-x)^k (2k + 2) / (2k + 3)!   (phi(0) = 1, psi(0) = pi^2 / 3).
            // Below x = 1 (r < 0.32) the series: the first neglected terms are x^9 / 19! < 9e-18 (beside 1) and 18 x^8 / 19! < 1.5e-16 (beside 1/3); above it the
            // closed forms, where the difference phi - cos has lost at most log2(3 / x) < 2 bits.  No 0 / 0 is ever formed.
            const double x = 9.869604401089358 * s;
            if (x <= 1.0) {
                double a = 2.8114572543455206e-15;                       // 1 / 17!
                a = fma(-x, a, 7.6471637318198164e-13);                 // 1 / 15!
                a = fma(-x, a, 1.6059043836821613e-10);                 // 1 / 13!
                a = fma(-x, a, 2.505210838544172e-08);                  // 1 / 11!
                a = fma(-x, a, 2.7557319223985893e-06);                 // 1 / 9!
                a = fma(-x, a, 1.984126984126984e-04);                  // 1 / 7!
                a = fma(-x, a, 8.333333333333333e-03);                  // 1 / 5!
                a = fma(-x, a, 1.6666666666666666e-01);                 // 1 / 3!
                phi = fma(-x, a, 1.0);
                if (PSI) {
                    double b = 4.4983316069528329e-14;                   // 16 / 17!
                    b = fma(-x, b, 1.0706029224547743e-11);             // 14 / 15!
                    b = fma(-x, b, 1.9270852604185937e-09);             // 12 / 13!
                    b = fma(-x, b, 2.505210838544172e-07);              // 10 / 11!
                    b = fma(-x, b, 2.2045855379188714e-05);             // 8 / 9!
                    b = fma(-x, b, 1.1904761904761906e-03);             // 6 / 7!
                    b = fma(-x, b, 3.3333333333333333e-02);             // 4 / 5!
                    b = fma(-x, b, 3.3333333333333331e-01);             // 2 / 3!
                    psi = 9.869604401089358 * b;
                }
            } else {
                const double r = sqrt(s);
                double sn, cs;
                sincospi(r, &sn, &cs);
                phi = sn / (3.14159265358979323846 * r);
                if (PSI) psi = (phi - cs) / s;
            }
        } break;
        default:
            phi = exp(-0.5 * s);
            if (PSI) psi = phi;
            break;
    }
}

template <int DM>
__device__ __forceinline__ double radial_s(const double (&p)[DM], const double (&q)[DM], const double* V, const double* s, int D) {
    double arg = 0.0;
    for (int d = 0; d < D; ++d) {
        const double u = (p[d] - q[d]) + s[d];
        arg = fma(V[d] * u, u, arg);
    }
    return arg;
}

// The periodic profile (MOGP_KIND_PERIODIC, D = 1): exp(V (cos theta - 1)) with theta the term's phase -- the Gaussian profile of
// s = 2 V (1 - cos theta), and no cosine factor beside it.  `cc` = cos theta from the staged UNIT phase factors; the amplitude is L.A[t].
__device__ __forceinline__ double periodic_s(double V, double cc) { return 2.0 * V * (1.0 - cc); }

// The dot-product row (MOGP_KIND_DOT): k = b^n, b = A <x_a, x_b> + c -- LinearKernel (n = 1) and PolynomialKernel of the reference.  Not a
// profile of s and not stationary: it needs the inputs themselves, which a thread holds relative to the tile centres (p = x_a - c_r,
// q = x_b - c_c); the staging keeps the centres in L.Kp / L.L and the bias c (the row's Psi slot) in L.e[t][0], none of which a radial
// launch uses otherwise.  x = p + c_r is the input to half an ulp.
template <int DM>
__device__ __forceinline__ double dot_row_inner(const double (&p)[DM], const double (&q)[DM], const TileLds<DM>& L, int t, int D) {
    double ip = (p[0] + L.Kp[t][0]) * (q[0] + L.L[t][0]);
    for (int d = 1; d < D; ++d) ip = fma(p[d] + L.Kp[t][d], q[d] + L.L[t][d], ip);
    return ip;
}
// b^n by repeated multiplication (n = 1 .. MOGP_DOT_DEGREE_MAX, uniform over the tile)
__device__ __forceinline__ double dot_row_power(double b, int n) {
    double k = b;
    for (int i = 1; i < n; ++i) k *= b;
    return k;
}
__device__ __forceinline__ int dot_row_degree(double shape) { return __builtin_amdgcn_readfirstlane((int)shape); }

// The gate row (MOGP_KIND_GATE, D = 1): k = A h(x_a) h(x_b), h(x) = sigmoid(beta (x - l)) -- the separable weight of the reference's
// ChangePointsKernel.  h is a property of the point: the staging evaluates it (and its complement) once per row and column point into the
// slots the phase factors take for other rows, and an entry only multiplies: cu = (A) h_a, cw = h_b, su = 1 - h_a, sw = 1 - h_b.

// The weighted-dot row (MOGP_KIND_WDOT, D >= 2: check_kinds): k = A sum_d V_d x_a,d x_b,d -- the reference's FunctionKernel, whose feature values the host
// appends to the inputs as columns of their own.  Inputs as for the dot-product row (dot_row_inner: centred inputs plus the tile centres in
// L.Kp / L.L); the weights are the row's V.  Without the amplitude: it is A times something, and the callers place A.
template <int DM>
__device__ __forceinline__ double wdot_row_inner(const double (&p)[DM], const double (&q)[DM], const TileLds<DM>& L, int t, int D) {
    double ip = L.V[t][0] * ((p[0] + L.Kp[t][0]) * (q[0] + L.L[t][0]));
    for (int d = 1; d < D; ++d) ip = fma(L.V[t][d], (p[d] + L.Kp[t][d]) * (q[d] + L.L[t][d]), ip);
    return ip;
}
// The white row (MOGP_KIND_WHITE): k = A where row and column are the SAME point of the same set, 0 elsewhere -- also between two different
// points with equal inputs.  Only the tile lists of a symmetric launch carry GT_DIAG, on the tiles of the matrix diagonal; there a thread's
// entry (m, n) has equal global indices when rg == cg and m == n.  `ondiag` = GT_DIAG && rg == cg.

// Chunks of a radial launch end at a group end (a group never straddles two chunks): at most MOGP_TC rows from t0 on, shortened while the
// last one still multiplies with its successor.  `kinds`: one pair's kind row -- the flags are the same in every pair.
__device__ __forceinline__ int radial_chunk(const int* kinds, int T, int t0) {
    int nt = min(MOGP_TC, T - t0);
    while (nt > 1 && t0 + nt < T && (kinds[t0 + nt - 1] & MOGP_KIND_TIMES)) --nt;
    return nt;
}

template <int DM, int GATE = 0>
__device__ __forceinline__ void gram_term_radial(double (&acc)[4][4], const double (&p)[4][DM], const double (&q)[4][DM], const TileLds<DM>& L, int t,
                                                 int D, int kind, double shape, const double (&cu)[4], const double (&su)[4],
                                                 const double (&cw)[4], const double (&sw)[4], bool ondiag = false) {
    const bool per = kind == MOGP_KIND_PERIODIC;
    if (kind == MOGP_KIND_DOT) {                            // the row's value is the whole entry: no amplitude in front, no cosine beside it
        const int n = dot_row_degree(shape);
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
            for (int nn = 0; nn < 4; ++nn) acc[m][nn] += dot_row_power(fma(L.A[t], dot_row_inner<DM>(p[m], q[nn], L, t, D), L.e[t][0]), n);
        return;
    }
    if (GATE && kind == MOGP_KIND_GATE) {                   // A h_a h_b from the staged factors (the amplitude rides in cu)
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
            for (int nn = 0; nn < 4; ++nn) acc[m][nn] = fma(cu[m], cw[nn], acc[m][nn]);
        return;
    }
    if (GATE > 1 && kind == MOGP_KIND_WDOT) {
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
            for (int nn = 0; nn < 4; ++nn) acc[m][nn] = fma(L.A[t], wdot_row_inner<DM>(p[m], q[nn], L, t, D), acc[m][nn]);
        return;
    }
    if (GATE > 1 && kind == MOGP_KIND_WHITE) {
        if (ondiag) {
#pragma unroll
            for (int m = 0; m < 4; ++m) acc[m][m] += L.A[t];
        }
        return;
    }
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        __builtin_amdgcn_sched_barrier(0);                  // one row of four library exps at a time: interleaving all sixteen is what spills
#pragma unroll
        for (int n = 0; n < 4; ++n) {
            double phi, psi;
            const double cc = fma(cu[m], cw[n], su[m] * sw[n]);
            radial_profile<false>(kind, shape, per ? periodic_s(L.V[t][0], cc) : radial_s<DM>(p[m], q[n], L.V[t], L.s[t], D), phi, psi);
            acc[m][n] = per ? fma(L.A[t], phi, acc[m][n]) : fma(phi, cc, acc[m][n]);
        }
    }
}

// One row of a product group: prod *= k_t per entry, k_t = A phi cos theta (the amplitude rides in the staged row factors when AMPF, else
// it is L.A[t]: the moment pass stages unit amplitudes) -- for a row whose value is A times something, the moment pass leaves the row's OWN
// amplitude to the host and this function supplies the other rows'.  A dot-product row is not of that form and always brings its full value.
template <int DM, bool AMPF, int GATE = 0>
__device__ __forceinline__ void group_factor_radial(double (&prod)[4][4], const double (&p)[4][DM], const double (&q)[4][DM],
                                                    const TileLds<DM>& L, int t, int D, int kind, double shape, int rg, int cg, bool ondiag = false) {
    const bool per = kind == MOGP_KIND_PERIODIC;
    const double A = L.A[t];
    if (kind == MOGP_KIND_DOT) {                            // the full value b^n with or without AMPF: the row's amplitude is inside the power, and
        const int n = dot_row_degree(shape);                // the host's chain rule never multiplies a dot-product row's moments by it
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
            for (int nn = 0; nn < 4; ++nn) prod[m][nn] *= dot_row_power(fma(A, dot_row_inner<DM>(p[m], q[nn], L, t, D), L.e[t][0]), n);
        return;
    }
    if (GATE && kind == MOGP_KIND_GATE) {                   // a row of the form A times something: the staged factors, and A where they do not carry it
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const double hu = AMPF ? L.cu[t][rg * 4 + m] : A * L.cu[t][rg * 4 + m];
#pragma unroll
            for (int nn = 0; nn < 4; ++nn) prod[m][nn] *= hu * L.cw[t][cg * 4 + nn];
        }
        return;
    }
    if (GATE > 1 && kind == MOGP_KIND_WDOT) {                   // A times something, nothing staged: A from L.A with or without AMPF
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
            for (int nn = 0; nn < 4; ++nn) prod[m][nn] *= A * wdot_row_inner<DM>(p[m], q[nn], L, t, D);
        return;
    }
    if (GATE > 1 && kind == MOGP_KIND_WHITE) {                  // White x k = diag(A k(x, x))
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
            for (int nn = 0; nn < 4; ++nn) prod[m][nn] *= (ondiag && m == nn) ? A : 0.0;
        return;
    }
    double cw[4], sw[4];
#pragma unroll
    for (int n = 0; n < 4; ++n) { cw[n] = L.cw[t][cg * 4 + n]; sw[n] = L.sw[t][cg * 4 + n]; }
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        __builtin_amdgcn_sched_barrier(0);
        const double cu = L.cu[t][rg * 4 + m], su = L.su[t][rg * 4 + m];
#pragma unroll
        for (int n = 0; n < 4; ++n) {
            double phi, psi;
            const double cc = fma(cu, cw[n], su * sw[n]);
            radial_profile<false>(kind, shape, per ? periodic_s(L.V[t][0], cc) : radial_s<DM>(p[m], q[n], L.V[t], L.s[t], D), phi, psi);
            double k = per ? phi : phi * cc;
            if (per || !AMPF) k *= A;
            prod[m][n] *= k;
        }
    }
}

// tile epilogue: full interior tiles store 32-byte runs; diagonal / ragged tiles take the per-element path (augmentation, lower part only)
__device__ __forceinline__ void gram_store(const GramArgs& a, const GTile& tl, const double (&acc)[4][4], int rg, int cg) {
    const bool full = tl.nr == MOGP_GT && tl.nc == MOGP_GT && !(tl.flags & GT_DIAG) && ((tl.c0 & 1) == 0) && ((a.ldo & 1) == 0);
    if (full) {
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const int64_t at = (int64_t)(tl.r0 + rg * 4 + m) * a.ldo + tl.c0 + cg * 4;
            double* o = a.out + at;
            *reinterpret_cast<d2_t*>(o) = (d2_t){acc[m][0], acc[m][1]};
            *reinterpret_cast<d2_t*>(o + 2) = (d2_t){acc[m][2], acc[m][3]};
            if (a.out2) {
                *reinterpret_cast<d2_t*>(a.out2 + at) = (d2_t){acc[m][0], acc[m][1]};
                *reinterpret_cast<d2_t*>(a.out2 + at + 2) = (d2_t){acc[m][2], acc[m][3]};
            }
        }
        if (a.mirror && (tl.flags & GT_MIRROR)) {
#pragma unroll
            for (int n = 0; n < 4; ++n)
#pragma unroll
                for (int m = 0; m < 4; ++m) a.out[(int64_t)(tl.c0 + cg * 4 + n) * a.ldo + tl.r0 + rg * 4 + m] = acc[m][n];
        }
        return;
    }
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        const int lr = rg * 4 + m;
        if (lr >= tl.nr) continue;
        const int64_t r = tl.r0 + lr;
#pragma unroll
        for (int n = 0; n < 4; ++n) {
            const int lc = cg * 4 + n;
            if (lc >= tl.nc) continue;
            const int64_t c = tl.c0 + lc;
            if ((tl.flags & GT_DIAG) && lc > lr) continue;       // diagonal tiles: lower part computed, upper part mirrored
            double v = acc[m][n];
            if (a.noise != nullptr && r == c) {
                v += a.noise[tl.pair / a.C] + a.jitter_abs;
                if (a.dvar != nullptr) v += a.dvar[r];
            }
            a.out[r * a.ldo + c] = v;
            if (a.out2) a.out2[r * a.ldo + c] = v;
            if (a.mirror && ((tl.flags & GT_MIRROR) || ((tl.flags & GT_DIAG) && lr > lc))) a.out[c * a.ldo + r] = v;
        }
    }
}

// Persistent workgroups (two per CU), software pipelined over tiles blockIdx.x, + gridDim.x, ...: a tile's global reads (its centred
// inputs and staging items, all functions of the descriptor alone) are issued one tile ahead, before the previous tile's main loop, and
// the descriptor itself two tiles ahead -- a tile-per-workgroup launch spends more time in these two dependent memory round trips than
// in its arithmetic (measured: 66 of 126 us).  The staged factors are double buffered in LDS: one barrier per tile.
// RAD: the radial instantiation (a.kind / a.shape are set): same pipeline, entry-by-entry profiles.  The Gaussian instantiations (RAD = false)
// contain nothing of it.
template <int DT, bool RAD = false, int GATE = 0>
__global__ __launch_bounds__(256, 2) void k_gram(GramArgs a, int ntiles) {
    constexpr int DM = DT > 0 ? DT : MOGP_MAXD;
    constexpr bool BATCH = DT == 1;
    const int D = DT > 0 ? DT : a.D;
    const int W = a.W;
    const int tid = threadIdx.x;
    const int cg = tid & 15, rg = tid >> 4;
    __shared__ TileLds<DM> Lb[2];
    extern __shared__ __attribute__((aligned(16))) double s_tab[];     // the whole term table when it fits (a.tab_lds)
    const PhaseView v = phase_view(a.ph.ws, a.C, a.T, D, a.ldxr, a.ldxc);
    const int stride = gridDim.x;
    int nt0 = min(MOGP_TC, a.T);
    if constexpr (RAD) nt0 = radial_chunk(a.kind, a.T, 0);     // (the same in every pair)
    STAGE_MAP(tid);

    int tile = blockIdx.x;
    if (tile >= ntiles) return;
    if (a.tab_lds) {
        for (int e = tid; e < a.C * a.C * a.T * W; e += 256) s_tab[e] = a.table[e];
        __syncthreads();
    }
    const double* tabbase = a.tab_lds ? s_tab : a.table;
    GTile tl = a.tiles[tile];
    GTile tl1 = a.tiles[min(tile + stride, ntiles - 1)];
    TileCtx<DM> X;
    double p[4][DM], q[4][DM];
    StageItem<DM> I[BATCH ? STAGE_ITEMS : 1];
    tile_context<DM>(X, p, q, tl, D, v, a.xr, a.ldxr, a.xc, a.ldxc, rg, cg);
    if (BATCH) {
#pragma unroll
        for (int k = 0; k < STAGE_ITEMS; ++k)
            if (st_tb + 2 * k < nt0) stage_item_load<DM>(I[k], st_which, st_tb + 2 * k, st_pnt, tl, D, a.C, a.T, 0, v, a.xr, a.ldxr, a.xc, a.ldxc);
    }
    int buf = 0;
    while (true) {
        TileLds<DM>& L = Lb[buf];
        const GTile cur = tl;
        const double* tab = tabbase + (size_t)cur.pair * a.T * W;
        // stage this tile's first chunk of terms (from the prefetched registers when batched)
        if (BATCH) {
#pragma unroll
            for (int k = 0; k < STAGE_ITEMS; ++k)
                if (st_tb + 2 * k < nt0) stage_item_compute<DM, true, RAD, GATE>(L, I[k], X, tab, W, st_which, st_tb + 2 * k, st_pnt, D, 0, RAD ? a.kind + (size_t)cur.pair * a.T : nullptr);
        } else {
            stage_chunk<DM, true, false, RAD, GATE>(L, X, cur, tab, W, D, a.C, a.T, 0, nt0, v, a.xr, a.ldxr, a.xc, a.ldxc, tid, RAD ? a.kind + (size_t)cur.pair * a.T : nullptr);
        }
        double pc[4][DM], qc[4][DM];
#pragma unroll
        for (int m = 0; m < 4; ++m)
            for (int d = 0; d < D; ++d) { pc[m][d] = p[m][d]; qc[m][d] = q[m][d]; }
        // prefetch the next tile (its descriptor arrived during the previous iteration), and the descriptor after it
        const int nxt = tile + stride;
        const bool more = nxt < ntiles;
        if (more) {
            tl = tl1;
            tl1 = a.tiles[min(nxt + stride, ntiles - 1)];
            tile_context<DM>(X, p, q, tl, D, v, a.xr, a.ldxr, a.xc, a.ldxc, rg, cg);
            if (BATCH) {
#pragma unroll
                for (int k = 0; k < STAGE_ITEMS; ++k)
                    if (st_tb + 2 * k < nt0) stage_item_load<DM>(I[k], st_which, st_tb + 2 * k, st_pnt, tl, D, a.C, a.T, 0, v, a.xr, a.ldxr, a.xc, a.ldxc);
            }
        }
        __syncthreads();

        double acc[4][4];
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
            for (int n = 0; n < 4; ++n) acc[m][n] = 0.0;
        for (int t0 = 0, nt; t0 < a.T; t0 += RAD ? nt : MOGP_TC) {
            if constexpr (RAD) nt = radial_chunk(a.kind, a.T, t0); else nt = min(MOGP_TC, a.T - t0);
            if (t0 > 0) {                                   // more than MOGP_TC terms: the later chunks are staged in place
                __syncthreads();
                TileCtx<DM> Xc;
                tile_centres<DM>(Xc, cur, D, v, a.ldxr, a.ldxc);
                stage_chunk<DM, true, false, RAD, GATE>(L, Xc, cur, tab, W, D, a.C, a.T, t0, nt, v, a.xr, a.ldxr, a.xc, a.ldxc, tid, RAD ? a.kind + (size_t)cur.pair * a.T : nullptr);
                __syncthreads();
            }
            if constexpr (RAD) {
                // group by group: [t, te] is a maximal run of rows flagged MOGP_KIND_TIMES plus the row that ends it (a chunk holds whole groups);
                // a row of zero amplitude makes its whole group zero
                const int* kd = a.kind + (size_t)cur.pair * a.T + t0;
                const double* sh = a.shape + (size_t)cur.pair * a.T + t0;
                const bool ondiag = GATE > 1 && (cur.flags & GT_DIAG) && rg == cg;      // (white rows: the thread's entries (m, m) are matrix-diagonal entries)
                for (int t = 0, te; t < nt; t = te + 1) {
                    bool skip = GRAM_DBG(a, 2);
                    for (te = t;; ++te) {
                        skip |= L.deg[te] == GT_SKIP;
                        if (te == nt - 1 || !(__builtin_amdgcn_readfirstlane(kd[te]) & MOGP_KIND_TIMES)) break;
                    }
                    if (skip) continue;
                    if (te == t) {                          // a group of one: the plain radial term
                        double cu[4], su[4], cw[4], sw[4];
#pragma unroll
                        for (int m = 0; m < 4; ++m) {
                            cu[m] = L.cu[t][rg * 4 + m]; su[m] = L.su[t][rg * 4 + m];
                            cw[m] = L.cw[t][cg * 4 + m]; sw[m] = L.sw[t][cg * 4 + m];
                        }
                        gram_term_radial<DM, GATE>(acc, pc, qc, L, t, D, __builtin_amdgcn_readfirstlane(kd[t]) & MOGP_KIND_MASK, sh[t], cu, su, cw, sw, ondiag);
                        continue;
                    }
                    double prod[4][4];
#pragma unroll
                    for (int m = 0; m < 4; ++m)
#pragma unroll
                        for (int n = 0; n < 4; ++n) prod[m][n] = 1.0;
                    for (int f = t; f <= te; ++f)
                        group_factor_radial<DM, true, GATE>(prod, pc, qc, L, f, D, __builtin_amdgcn_readfirstlane(kd[f]) & MOGP_KIND_MASK, sh[f], rg, cg, ondiag);
#pragma unroll
                    for (int m = 0; m < 4; ++m)
#pragma unroll
                        for (int n = 0; n < 4; ++n) acc[m][n] += prod[m][n];
                }
            } else
            for (int t = 0; t < nt; ++t) {
                const int deg = L.deg[t];
                if (deg == GT_SKIP || GRAM_DBG(a, 2)) continue;
                double cu[4], su[4], cw[4], sw[4];
#pragma unroll
                for (int m = 0; m < 4; ++m) {
                    cu[m] = L.cu[t][rg * 4 + m]; su[m] = L.su[t][rg * 4 + m];
                    cw[m] = L.cw[t][cg * 4 + m]; sw[m] = L.sw[t][cg * 4 + m];
                }
                switch (deg) {
                    #define GT_CASE(N) case N: gram_term<DM, N>(acc, pc, qc, L, t, D, cu, su, cw, sw); break;
                    GT_DEGREE_CASES(GT_CASE)
#undef GT_CASE
                    default: gram_term<DM, 0>(acc, pc, qc, L, t, D, cu, su, cw, sw); break;
                }
            }
        }
        if (a.T > MOGP_TC) __syncthreads();                // the in-place chunks above must be consumed before this buffer is restaged
        if (!(GRAM_DBG(a, 1) && acc[0][0] != 12345.678)) gram_store(a, cur, acc, rg, cg);
        if (!more) break;
        tile = nxt;
        buf ^= 1;
    }
}

// ---- strip kernel: D = 1, no envelope, runs of full interior tiles ---------------------------------------------------------------
// The general kernel above pays two dependent global round trips per tile (descriptor -> inputs and phase factors) or, software
// pipelined, the registers to hide them (it spills).  Training data are channel-sorted series: almost every tile is a full 64 x 64
// interior tile, and consecutive tiles of the list share their 64 rows.  One workgroup takes a RUN of such tiles: the rows' inputs and
// phase factors are read once, the next tile's 64 columns (input + 2 T phase factors: at most five doubles per thread) are fetched under
// the current tile's arithmetic, and the tile-centred factors are staged from LDS.  Same arithmetic as the general kernel, term by term.
// TC = terms a launch may carry (LDS is sized by it); raw rows of a block of 64 points: x | cos_t | sin_t.  Two workgroups per CU: the
// arithmetic needs ~200 VGPRs, and three or four waves per SIMD bought with spills ran 1.3x / 2x slower.
#define GS_TC_MAX 8
// one term into a thread's 4 x NC entries (NC = 4 is the only width left: the 4 x 2 form on 512 threads went with the two-barrier kernel)
template <int N, int NC>
__device__ __forceinline__ void strip_term(double (&acc)[4][NC], const double (&p)[4], const double (&q)[NC], double V, double s,
                                           const double (&cu)[4], const double (&su)[4], const double (&cw)[NC], const double (&sw)[NC]) {
    double vp[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) vp[m] = V * p[m];
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        if (m == 2 && NC == 4) __builtin_amdgcn_sched_barrier(0);      // two groups of eight independent Horner chains (see gram_term)
#pragma unroll
        for (int n = 0; n < NC; ++n) {
            double e;
            if (N > 0) {
                e = exp_taylor<N>(vp[m] * q[n]);
            } else {
                const double u = (p[m] - q[n]) + s;
                e = fast_exp(fmax(-0.5 * (V * u) * u, -745.0));
            }
            acc[m][n] = fma(e, fma(cu[m], cw[n], su[m] * sw[n]), acc[m][n]);
        }
    }
}

// ---- the strip kernel (round 6): ONE barrier per tile -------------------------------------------------------------------------------
// Its first form (k_gram_strip, round 5; removed) synchronised twice per tile (staged factors written -> read; read -> the buffers are restaged) and
// its waves were parked at s_waitcnt / s_barrier 36 % of their cycles.  Here the tile-centred factors are double buffered and staged one tile AHEAD: iteration u stages tile
// u + 1 into F[b ^ 1], computes tile u from F[b], commits the columns of tile u + 2 (prefetched an iteration earlier) and the scalars of tile u + 2
// (degree, centre distance: computed ONCE per tile and term by wave 0, not by every staging item), stores tile u; one barrier; the columns of tile
// u + 3 are requested behind it.  The 2 T 64 staging items of a tile do not divide over 256 threads for T = 3 (384): the half wave-pair that takes a
// second item alternates with the tile's parity.  The addresses of the column prefetch and the LDS slots of its commit are per-thread constants,
// worked out once per run.  Same arithmetic, entry by entry, as the first form (the same row / column factors, the same polynomial): same bits.
template <int TC>
struct Strip2Lds {
    static constexpr int RAW = 1 + 2 * TC, PF = (RAW * MOGP_GT + 255) / 256;      // PF: prefetch registers per thread
    // column-side arrays in two planes: a thread's four columns 4 cg .. 4 cg + 3 are two 16-byte reads, and with the points in order lane cg's reads sat
    // 32 bytes apart -- every fourth lane on the same banks (SQ_LDS_BANK_CONFLICT: 54 % of the first form's LDS cycles).  Columns 4 cg, 4 cg + 1 at
    // [2 cg], columns 4 cg + 2, 4 cg + 3 at [CP + 2 cg]: each read is 16 contiguous lanes x 16 bytes.
    static constexpr int CP = 36, CL = 72;
    __device__ static __forceinline__ int cs(int pnt) { return ((pnt & 2) ? CP : 0) + ((pnt >> 2) << 1) + (pnt & 1); }
    double rowraw[RAW][MOGP_GT];
    double colraw[2][RAW][CL];
    double cu[2][TC][MOGP_GT], su[2][TC][MOGP_GT], cw[2][TC][CL], sw[2][TC][CL];
    double qv[2][CL];                             // q = x_b - (column tile centre) of the staged tile, in the column planes' order
    double tab[TC][3];                            // A, V, Delta of the pair's terms
    double s[3][TC];                              // centre distance + delay of tile u mod 3 (written two tiles ahead of its last reader)
    int deg[3][TC];
};

template <int TC>
__global__ __launch_bounds__(256, 2) void k_gram_strip2(GramArgs a, const GSeg* __restrict__ segs) {
    using SL = Strip2Lds<TC>;
    constexpr int PF = SL::PF, NT = 256;
    __shared__ SL L;
    const int tid = threadIdx.x, cg = tid & 15, rg = tid >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const GSeg sg = segs[blockIdx.x];
    const int T = a.T, W = a.W;
    const int ci = sg.pair / a.C, cj = sg.pair - ci * a.C;
    const PhaseView v = phase_view(a.ph.ws, a.C, T, 1, a.ldxr, a.ldxc);
    const double* __restrict__ tab = a.table + (size_t)sg.pair * T * W;
    const int nraw = (1 + 2 * T) * MOGP_GT;
    auto slot = [&](int k) { return k <= T ? k : k - T + TC; };

    for (int e = tid; e < nraw; e += NT) {               // the row block, once per run (rows take the table of the COLUMN channel)
        const int k = e >> 6, pnt = e & 63;
        const int64_t gp = sg.r0 + pnt;
        double val;
        if (k == 0) val = a.xr[gp];
        else if (k <= T) val = v.rcs[((size_t)cj * T + (k - 1)) * a.ldxr + gp];
        else val = v.rsn[((size_t)cj * T + (k - 1 - T)) * a.ldxr + gp];
        L.rowraw[slot(k)][pnt] = val;
    }
    if (tid < 3 * T) { const int t = tid / 3, k = tid - 3 * t; L.tab[t][k] = tab[(size_t)t * W + (k == 0 ? 0 : 2 * k)]; }      // columns 0, 2, 4
    const double cr = v.rcen[sg.r0], hr = v.rhalf[sg.r0];
    // column prefetch: per-thread constants (source array + point, LDS slot), columns take the table of the ROW channel
    const double* psrc[PF];
    int pdst[PF];
#pragma unroll
    for (int k5 = 0; k5 < PF; ++k5) {
        const int e = tid + NT * k5, k = e >> 6, pnt = e & 63;
        psrc[k5] = nullptr; pdst[k5] = 0;
        if (e < nraw) {
            if (k == 0) psrc[k5] = a.xc + pnt;
            else if (k <= T) psrc[k5] = v.ccs + ((size_t)ci * T + (k - 1)) * a.ldxc + pnt;
            else psrc[k5] = v.csn + ((size_t)ci * T + (k - 1 - T)) * a.ldxc + pnt;
            pdst[k5] = slot(k) * SL::CL + SL::cs(pnt);
        }
    }
    double pf[PF], cc_n = 0.0, hc_n = 0.0;
    auto col_fetch = [&](int c0) {
#pragma unroll
        for (int k5 = 0; k5 < PF; ++k5) if (psrc[k5]) pf[k5] = psrc[k5][c0];
        cc_n = v.ccen[c0]; hc_n = v.chalf[c0];
    };
    auto col_commit = [&](int b) {
        double* plane = &L.colraw[b][0][0];
#pragma unroll
        for (int k5 = 0; k5 < PF; ++k5) if (psrc[k5]) plane[pdst[k5]] = pf[k5];
    };
    // degree / centre distance of tile `u` (column centre cc, half span hc): ONE wave, one lane per term
    auto scalars = [&](int u, double cc, double hc) {
        if (wave == 0 && tid < T) {
            const double A = L.tab[tid][0], V = L.tab[tid][1], s = (cr - cc) + L.tab[tid][2];
            const double zmax = fabs(V) * hr * hc, es = V * s * s;
            const double mu = fmax(0.0, fabs(s) - hr - hc), emin = V * mu * mu;
            const double efac = fabs(V) * (hr * hr + hc * hc + 2.0 * (hr + hc) * fabs(s));
            int deg;
            if (A == 0.0 || 0.5 * emin > GT_SKIP_EXPONENT) deg = GT_SKIP;
            else if (!(zmax <= 0.45) || !(0.5 * es < 600.0) || !(0.5 * efac < 600.0)) deg = GT_GENERAL;
            else deg = GT_DEGREE(zmax);
            L.deg[u % 3][tid] = deg; L.s[u % 3][tid] = s;
        }
    };
    // the tile-centred factors of tile u (columns in colraw[u & 1], centre cc) into F[u & 1]
    auto stage = [&](int u, double cc) {
        const int b = u & 1, u3 = u % 3;
        auto item = [&](int e) {
            const int which = e >= T * MOGP_GT, rem = e - which * T * MOGP_GT, t = rem >> 6, pnt = rem & 63;
            const int deg = L.deg[u3][t];
            if (deg == GT_SKIP) return;
            if (GRAM_DBG(a, 4)) { L.cu[b][t][pnt] = 1.0; L.su[b][t][pnt] = 0.5; L.cw[b][t][SL::cs(pnt)] = 0.25; L.sw[b][t][SL::cs(pnt)] = 2.0; return; }
            const double V = L.tab[t][1], s = L.s[u3][t];
            double f = 1.0;
            if (which == 0) {
                if (deg != GT_GENERAL) {
                    const double pp = L.rowraw[0][pnt] - cr;
                    f = fast_exp(-0.5 * (V * (fma(pp, pp, s * s) + 2.0 * pp * s)));
                }
                f *= L.tab[t][0];
                L.cu[b][t][pnt] = f * L.rowraw[1 + t][pnt]; L.su[b][t][pnt] = f * L.rowraw[1 + TC + t][pnt];
            } else {
                const int cp = SL::cs(pnt);
                const double qq = L.colraw[b][0][cp] - cc;
                if (deg != GT_GENERAL) f = fast_exp(-0.5 * (V * (qq * qq - 2.0 * qq * s)));
                L.cw[b][t][cp] = f * L.colraw[b][1 + t][cp]; L.sw[b][t][cp] = f * L.colraw[b][1 + TC + t][cp];
            }
        };
        const int items = 2 * T * MOGP_GT, full = items / NT;                // (items come in multiples of 128: which / t are wave-uniform)
        for (int r = 0; r < full; ++r) item(tid + NT * r);
        if ((items & (NT - 1)) && (wave & 2) == ((u & 1) << 1)) item(NT * full + (tid & 127));      // T odd: 128 items left, the wave pairs take turns
        if (tid < MOGP_GT) { const int cp = SL::cs(tid); L.qv[b][cp] = L.colraw[b][0][cp] - cc; }
    };

    // ---- prologue: tile 0 staged, tile 1's columns and scalars in LDS, tile 2's columns requested.  The columns of tiles 0 and 1 are requested TOGETHER
    // (one memory round trip behind the run descriptor's, not two) ----
    double pf1[PF], cc0, hc0, cc1 = 0.0, hc1 = 0.0;
    col_fetch(sg.c0);
    if (sg.n > 1) {
#pragma unroll
        for (int k5 = 0; k5 < PF; ++k5) if (psrc[k5]) pf1[k5] = psrc[k5][sg.c0 + MOGP_GT];
        cc1 = v.ccen[sg.c0 + MOGP_GT]; hc1 = v.chalf[sg.c0 + MOGP_GT];
    }
    col_commit(0);
    cc0 = cc_n; hc0 = hc_n;
    if (sg.n > 1) {
        double* plane = &L.colraw[1][0][0];
#pragma unroll
        for (int k5 = 0; k5 < PF; ++k5) if (psrc[k5]) plane[pdst[k5]] = pf1[k5];
    }
    __syncthreads();                                    // rowraw, tab, colraw[0], colraw[1]
    scalars(0, cc0, hc0);
    if (sg.n > 1) scalars(1, cc1, hc1);
    if (sg.n > 2) col_fetch(sg.c0 + 2 * MOGP_GT);
    __syncthreads();                                    // the scalars of tiles 0 and 1
    stage(0, cc0);
    __syncthreads();                                    // F[0]
    double p[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) p[m] = L.rowraw[0][rg * 4 + m] - cr;

    for (int u = 0; u < sg.n; ++u) {
        const int b = u & 1, u3 = u % 3, c0 = sg.c0 + u * MOGP_GT;
        if (u + 1 < sg.n) stage(u + 1, cc1);
        double q[4], acc[4][4];
#pragma unroll
        for (int n = 0; n < 4; ++n) q[n] = L.qv[b][SL::cs(cg * 4 + n)];
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
            for (int n = 0; n < 4; ++n) acc[m][n] = 0.0;
        for (int t = 0; t < T; ++t) {
            const int deg = __builtin_amdgcn_readfirstlane(L.deg[u3][t]);
            if (deg == GT_SKIP || GRAM_DBG(a, 2)) continue;
            const double V = L.tab[t][1], s = L.s[u3][t];
            double cu[4], su[4], cw[4], sw[4];
#pragma unroll
            for (int m = 0; m < 4; ++m) { cu[m] = L.cu[b][t][rg * 4 + m]; su[m] = L.su[b][t][rg * 4 + m]; }
#pragma unroll
            for (int n = 0; n < 4; ++n) { cw[n] = L.cw[b][t][SL::cs(cg * 4 + n)]; sw[n] = L.sw[b][t][SL::cs(cg * 4 + n)]; }
            switch (deg) {
                #define GT_CASE(N) case N: strip_term<N, 4>(acc, p, q, V, s, cu, su, cw, sw); break;
                GT_DEGREE_CASES(GT_CASE)
#undef GT_CASE
                default: strip_term<0, 4>(acc, p, q, V, s, cu, su, cw, sw); break;
            }
        }
        if (u + 2 < sg.n) {                                // the columns of tile u + 2 (requested an iteration ago) and its scalars
            col_commit(b);
            scalars(u + 2, cc_n, hc_n);
        }
        cc0 = cc1; cc1 = cc_n;
        if (sg.diag && u + 1 == sg.n) {
            // the run's last tile sits on the matrix diagonal: lower part only, noise + jitter (+ per-point variance) on the diagonal entries
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                const int lr = rg * 4 + m;
                const int64_t r = sg.r0 + lr;
#pragma unroll
                for (int n = 0; n < 4; ++n) {
                    const int lc = cg * 4 + n;
                    if (lc > lr) continue;
                    double val = acc[m][n];
                    if (a.noise != nullptr && lc == lr) {
                        val += a.noise[ci] + a.jitter_abs;
                        if (a.dvar != nullptr) val += a.dvar[r];
                    }
                    a.out[r * a.ldo + c0 + lc] = val;
                    if (a.out2) a.out2[r * a.ldo + c0 + lc] = val;
                }
            }
        } else if (!(GRAM_DBG(a, 1) && acc[0][0] != 12345.678)) {
            double* o = a.out + (int64_t)(sg.r0 + rg * 4) * a.ldo + c0 + cg * 4;
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                *reinterpret_cast<d2_t*>(o + m * a.ldo) = (d2_t){acc[m][0], acc[m][1]};
                *reinterpret_cast<d2_t*>(o + m * a.ldo + 2) = (d2_t){acc[m][2], acc[m][3]};
            }
            if (a.out2) {                                  // the sparse models' working copy of K_uf (same leading dimension)
                double* o2 = a.out2 + (int64_t)(sg.r0 + rg * 4) * a.ldo + c0 + cg * 4;
#pragma unroll
                for (int m = 0; m < 4; ++m) {
                    *reinterpret_cast<d2_t*>(o2 + m * a.ldo) = (d2_t){acc[m][0], acc[m][1]};
                    *reinterpret_cast<d2_t*>(o2 + m * a.ldo + 2) = (d2_t){acc[m][2], acc[m][3]};
                }
            }
        }
        // F[b ^ 1], colraw[b], the scalars of tile u + 2: written; F[b], qv[b]: read.  An LDS-only barrier: __syncthreads() would also wait for the
        // tile's stores to land, which nobody here reads
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
        if (u + 3 < sg.n) col_fetch(c0 + 3 * MOGP_GT);
    }
}

void split_strip_tiles(const std::vector<GTile>& tiles, int maxrun, std::vector<GSeg>& segs, std::vector<GTile>& rest) {
    segs.clear(); rest.clear();
    for (const GTile& t : tiles) {
        // round 5: a full-size tile ON the diagonal rides at the end of its row block's run (the strip kernel's store handles it: lower part only,
        // noise + jitter on the diagonal) instead of going to the general kernel in a launch of its own -- 128 tiles, 17 us at the head of every
        // configs[1] evaluation.  (The strip kernel never mirrors: launch_gram takes it only when a.mirror is 0.)
        const bool fast = t.nr == MOGP_GT && t.nc == MOGP_GT && (t.c0 & 1) == 0;
        if (!fast) { rest.push_back(t); continue; }
        const int dg = (t.flags & GT_DIAG) ? 1 : 0;
        if (!segs.empty()) {
            GSeg& g = segs.back();
            if (!g.diag && g.pair == t.pair && g.r0 == t.r0 && g.c0 + g.n * MOGP_GT == t.c0 && g.n < maxrun) { ++g.n; g.diag = dg; continue; }
        }
        segs.push_back(GSeg{t.r0, t.c0, 1, t.pair, dg, {0, 0, 0}});
    }
}

int launch_gram(int ncu, const GramArgs& a0, int ntiles, hipStream_t s, int rows) {
    if (ntiles <= 0) return 0;
    GramArgs a = a0;
    if (a.W <= 0) a.W = 2 + 3 * a.D;
#ifdef MOGP_GRAM_DEBUG
    static const int dbg = []() { const char* e = std::getenv("MOGP_GRAM_DBG"); return e ? std::atoi(e) : 0; }();
    a.dbg = dbg;
#else
    a.dbg = 0;
#endif
    int rc = a.phases_ready ? 0 : launch_phase_tables(a.ph, a.xr, a.ldxr, a.nrows, a.xc, a.ldxc, a.ncols, a.table, a.T, a.D, a.C, a.W, s);
    if (rc) return rc;
    const int grid = std::min(ntiles, 2 * ncu);              // persistent: two workgroups per CU (__launch_bounds__(256, 2))
    const size_t tab_bytes = (size_t)a.C * a.C * a.T * a.W * sizeof(double);
    a.tab_lds = tab_bytes <= 24 * 1024;                      // the term table rides in LDS when small (it is read by every staging item)
    const size_t dyn = a.tab_lds ? tab_bytes : 0;
    if (a.ev0) HIP_TRY(hipEventRecord(a.ev0, s));
    if (a.kind) {                                            // radial profiles: every tile of the list through the radial general kernel
        if (!a.shape) { set_error("launch_gram: kinds without shapes"); return -1; }
        if (a.W != 2 + 3 * a.D) { set_error("launch_gram: radial profiles do not combine with enveloped term rows"); return -1; }
        if (rows == 1 && a.D != 1) { set_error("launch_gram: gate rows take one input dimension"); return -1; }
        if (rows == 1) {                                     // gate rows only (the instantiations below hold no gate code)
            hipLaunchKernelGGL((k_gram<1, true, 1>), dim3(grid), dim3(256), dyn, s, a, ntiles);
        } else if (rows > 1) {                               // weighted-dot or white rows, with or without gate rows
        switch (a.D) {
            case 1: hipLaunchKernelGGL((k_gram<1, true, 2>), dim3(grid), dim3(256), dyn, s, a, ntiles); break;
            case 2: hipLaunchKernelGGL((k_gram<2, true, 2>), dim3(grid), dim3(256), dyn, s, a, ntiles); break;
            case 3: hipLaunchKernelGGL((k_gram<3, true, 2>), dim3(grid), dim3(256), dyn, s, a, ntiles); break;
            default: hipLaunchKernelGGL((k_gram<0, true, 2>), dim3(grid), dim3(256), dyn, s, a, ntiles); break;
        }
        } else {
        switch (a.D) {
            case 1: hipLaunchKernelGGL((k_gram<1, true>), dim3(grid), dim3(256), dyn, s, a, ntiles); break;
            case 2: hipLaunchKernelGGL((k_gram<2, true>), dim3(grid), dim3(256), dyn, s, a, ntiles); break;
            case 3: hipLaunchKernelGGL((k_gram<3, true>), dim3(grid), dim3(256), dyn, s, a, ntiles); break;
            default: hipLaunchKernelGGL((k_gram<0, true>), dim3(grid), dim3(256), dyn, s, a, ntiles); break;
        }
        }
        if (a.ev1) HIP_TRY(hipEventRecord(a.ev1, s));
        HIP_TRY(hipGetLastError());
        return 0;
    }
    if (a.segs && a.nsegs > 0 && a.D == 1 && a.W == 5 && a.T <= GS_TC_MAX && !a.mirror && (a.ldo & 1) == 0) {
        if (a.T <= 4) hipLaunchKernelGGL((k_gram_strip2<4>), dim3(a.nsegs), dim3(256), 0, s, a, a.segs);
        else hipLaunchKernelGGL((k_gram_strip2<8>), dim3(a.nsegs), dim3(256), 0, s, a, a.segs);
        if (a.nrest > 0) {
            a.tiles = a.rest;
            hipLaunchKernelGGL(k_gram<1>, dim3(std::min(a.nrest, 2 * ncu)), dim3(256), dyn, s, a, a.nrest);
        }
        if (a.ev1) HIP_TRY(hipEventRecord(a.ev1, s));
        HIP_TRY(hipGetLastError());
        return 0;
    }
    switch (a.D) {
        case 1: hipLaunchKernelGGL(k_gram<1>, dim3(grid), dim3(256), dyn, s, a, ntiles); break;
        case 2: hipLaunchKernelGGL(k_gram<2>, dim3(grid), dim3(256), dyn, s, a, ntiles); break;
        case 3: hipLaunchKernelGGL(k_gram<3>, dim3(grid), dim3(256), dyn, s, a, ntiles); break;
        default: hipLaunchKernelGGL(k_gram<0>, dim3(grid), dim3(256), dyn, s, a, ntiles); break;
    }
    if (a.ev1) HIP_TRY(hipEventRecord(a.ev1, s));
    HIP_TRY(hipGetLastError());
    return 0;
}

// ---- the Jacobian of a rectangular Gram with respect to its ROW inputs ----------------------------------------------------
// J_d[a][b] = dK(x_a, x_b)/dx_a,d for every input dimension d, WRITTEN as D row blocks (block d at out + d * dstride): the right-hand sides of
// the posterior of df/dx (exact.hip: mogp_exact_predict_grad).  The entry formula is the one moment_term<.., ZG> contracts against an adjoint,
// here for every row kind the exact path differentiates:
//   Gaussian (and enveloped) rows   A E [ -V_d u_d cos - 2 pi M_d sin ]  ( - 1/2 L_d a_d k,  a = midpoint - centre )
//   profile rows (1, 3, 4, 6)       A [ -psi(s) V_d u_d cos - 2 pi M_d phi(s) sin ],  psi = -2 dphi/ds (radial_profile<true>: u psi = 0 at r = 0)
//   periodic rows                   -A 2 pi M_d V_0 sin exp(V_0 (cos - 1))
//   dot-product rows                n b^(n-1) A x_b,d,  b = A <x_a, x_b> + c
//   a product group                 sum_h dk_h prod_{g != h} k_g   (the other rows recomputed, never divided out: group_factor_radial)
// One 64 x 64 tile per workgroup, 4 x 4 entries per thread (the rg / cg mapping of k_moments), staged by tile_context / stage_chunk without the
// tile-centred split (SPLIT = false): every term entry by entry.  A plain launch: nothing accumulates across tiles, no flags, no atomics.  A thread
// keeps 16 DB running sums: DB = D for D <= 3, and the generic instantiation walks the dimensions two at a time (the terms are staged and evaluated
// again for every pair of dimensions) instead of holding 128 sums.  Kinds 2, 8, 9 and 10 never get here: the entry point refuses them by name.
template <int DM, int DB, bool ENV>
__device__ __forceinline__ void dx_term(double (&acc)[DB][4][4], const double (&p)[4][DM], const double (&q)[4][DM],
                                        const TileLds<DM>& L, int t, int D, int d0,
                                        const double (&cu)[4], const double (&su)[4], const double (&cw)[4], const double (&sw)[4]) {
    const double* V = L.V[t];
    const double* s = L.s[t];
    const double* Mv = L.M[t];
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        __builtin_amdgcn_sched_barrier(0);                  // one row of four library exps at a time (see gram_term_radial)
#pragma unroll
        for (int n = 0; n < 4; ++n) {
            const double e = gauss_general<DM>(p[m], q[n], V, s, L.L[t], L.e[t], D);
            const double kc = e * fma(cu[m], cw[n], su[m] * sw[n]);
            const double ks = e * fma(su[m], cw[n], -cu[m] * sw[n]);
            for (int d = 0; d < D; ++d) {
                if (d < d0 || d >= d0 + DB) continue;
                const double u = (p[m][d] - q[n][d]) + s[d];
                double j = -fma(V[d] * u, kc, 6.283185307179586476925286766559 * Mv[d] * ks);
                if (ENV) j = fma(-0.5 * L.L[t][d] * (0.5 * (p[m][d] + q[n][d]) + L.e[t][d]), kc, j);      // the envelope sits on the MIDPOINT
#pragma unroll
                for (int dd = 0; dd < DB; ++dd) acc[dd][m][n] += (d - d0 == dd) ? j : 0.0;
            }
        }
    }
}

// w (WT): the entry's weight, the product of the group's other rows
template <int DM, int DB, bool WT>
__device__ __forceinline__ void dx_term_radial(double (&acc)[DB][4][4], const double (&w)[4][4], const double (&p)[4][DM], const double (&q)[4][DM],
                                               const TileLds<DM>& L, int t, int D, int d0, int kind, double shape, int rg, int cg) {
    const double* V = L.V[t];
    const double* s = L.s[t];
    const double* Mv = L.M[t];
    const double A = L.A[t];
    if (kind == MOGP_KIND_DOT) {                            // x_b = q + the column centre the staging left in L.L
        const int n = dot_row_degree(shape);
        const double c = L.e[t][0];
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
            for (int nn = 0; nn < 4; ++nn) {
                const double b = fma(A, dot_row_inner<DM>(p[m], q[nn], L, t, D), c);
                double g = (double)n * A * (n > 1 ? dot_row_power(b, n - 1) : 1.0);
                if (WT) g *= w[m][nn];
                for (int d = 0; d < D; ++d) {
                    if (d < d0 || d >= d0 + DB) continue;
                    const double j = g * (q[nn][d] + L.L[t][d]);
#pragma unroll
                    for (int dd = 0; dd < DB; ++dd) acc[dd][m][nn] += (d - d0 == dd) ? j : 0.0;
                }
            }
        return;
    }
    const bool per = kind == MOGP_KIND_PERIODIC;
    double cw[4], sw[4];
#pragma unroll
    for (int n = 0; n < 4; ++n) { cw[n] = L.cw[t][cg * 4 + n]; sw[n] = L.sw[t][cg * 4 + n]; }
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        const double cu = L.cu[t][rg * 4 + m], su = L.su[t][rg * 4 + m];      // (times the amplitude, but for the periodic row: stage_item_compute)
#pragma unroll
        for (int n = 0; n < 4; ++n) {
            if ((n & 1) == 0) __builtin_amdgcn_sched_barrier(0);      // two entries' profiles at a time (see moment_term_radial)
            const double cc = fma(cu, cw[n], su * sw[n]), sn = fma(su, cw[n], -cu * sw[n]);
            double phi, psi, kc, ks;
            if (per) {                                      // k = A exp(V_0 (cos - 1)): dk/dtheta = -A V_0 sin exp(..), nothing through s
                radial_profile<false>(MOGP_KIND_GAUSS, shape, periodic_s(V[0], cc), phi, psi);
                kc = 0.0;
                ks = A * V[0] * sn * phi;
            } else {
                radial_profile<true>(kind, shape, radial_s<DM>(p[m], q[n], V, s, D), phi, psi);
                kc = psi * cc;
                ks = phi * sn;
            }
            if (WT) { kc *= w[m][n]; ks *= w[m][n]; }
            for (int d = 0; d < D; ++d) {
                if (d < d0 || d >= d0 + DB) continue;
                const double u = (p[m][d] - q[n][d]) + s[d];
                const double j = -fma(V[d] * u, kc, 6.283185307179586476925286766559 * Mv[d] * ks);
#pragma unroll
                for (int dd = 0; dd < DB; ++dd) acc[dd][m][n] += (d - d0 == dd) ? j : 0.0;
            }
        }
    }
}

template <int DT, bool ENV, bool RAD>
__global__ __launch_bounds__(256) void k_gram_dx(GramArgs a, int ntiles, int64_t dstride) {
    static_assert(!(ENV && RAD), "radial rows carry no envelope");
    constexpr int DM = DT > 0 ? DT : MOGP_MAXD;
    constexpr int DB = RAD ? 1 : (DT > 0 ? DT : 2);          // (the profiles' library calls leave a radial thread registers for one block of sums)
    const int D = DT > 0 ? DT : a.D;
    const int W = a.W;
    const int tid = threadIdx.x;
    const int cg = tid & 15, rg = tid >> 4;
    if ((int)blockIdx.x >= ntiles) return;
    const GTile tl = a.tiles[blockIdx.x];
    const double* tab = a.table + (size_t)tl.pair * a.T * W;
    const int* kinds = RAD ? a.kind + (size_t)tl.pair * a.T : nullptr;
    __shared__ TileLds<DM> L;
    const PhaseView v = phase_view(a.ph.ws, a.C, a.T, D, a.ldxr, a.ldxc);
    TileCtx<DM> X;
    double p[4][DM], q[4][DM];
    tile_context<DM>(X, p, q, tl, D, v, a.xr, a.ldxr, a.xc, a.ldxc, rg, cg);
    double one[4][4];                                        // (the weight of a group of one: never read, WT = false)
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int n = 0; n < 4; ++n) one[m][n] = 1.0;
    const bool full = tl.nr == MOGP_GT && tl.nc == MOGP_GT && ((tl.c0 & 1) == 0) && ((a.ldo & 1) == 0) && ((dstride & 1) == 0);

    for (int d0 = 0; d0 < D; d0 += DB) {
        double acc[DB][4][4];
#pragma unroll
        for (int dd = 0; dd < DB; ++dd)
#pragma unroll
            for (int m = 0; m < 4; ++m)
#pragma unroll
                for (int n = 0; n < 4; ++n) acc[dd][m][n] = 0.0;
        for (int t0 = 0, nt; t0 < a.T; t0 += nt) {
            if constexpr (RAD) nt = radial_chunk(a.kind, a.T, t0); else nt = min(MOGP_TC, a.T - t0);
            if (t0 > 0 || d0 > 0) __syncthreads();           // the chunk before this one has been consumed
            stage_chunk<DM, true, false, RAD, 0, false>(L, X, tl, tab, W, D, a.C, a.T, t0, nt, v, a.xr, a.ldxr, a.xc, a.ldxc, tid, kinds);
            __syncthreads();
            if constexpr (RAD) {
                const int* kd = kinds + t0;
                const double* sh = a.shape + (size_t)tl.pair * a.T + t0;
                for (int t = 0, te; t < nt; t = te + 1) {    // group by group, as k_gram walks them
                    bool skip = false;
                    for (te = t;; ++te) {
                        skip |= L.deg[te] == GT_SKIP;
                        if (te == nt - 1 || !(__builtin_amdgcn_readfirstlane(kd[te]) & MOGP_KIND_TIMES)) break;
                    }
                    if (skip) continue;                      // a row of zero amplitude: the group and every term of its derivative are zero
                    if (te == t) {
                        dx_term_radial<DM, DB, false>(acc, one, p, q, L, t, D, d0, __builtin_amdgcn_readfirstlane(kd[t]) & MOGP_KIND_MASK, sh[t], rg, cg);
                        continue;
                    }
                    for (int h = t; h <= te; ++h) {
                        double prod[4][4];
#pragma unroll
                        for (int m = 0; m < 4; ++m)
#pragma unroll
                            for (int n = 0; n < 4; ++n) prod[m][n] = 1.0;
                        for (int f = t; f <= te; ++f)
                            if (f != h) group_factor_radial<DM, true, 0>(prod, p, q, L, f, D, __builtin_amdgcn_readfirstlane(kd[f]) & MOGP_KIND_MASK, sh[f], rg, cg);
                        dx_term_radial<DM, DB, true>(acc, prod, p, q, L, h, D, d0, __builtin_amdgcn_readfirstlane(kd[h]) & MOGP_KIND_MASK, sh[h], rg, cg);
                    }
                }
            } else {
                for (int t = 0; t < nt; ++t) {
                    if (L.deg[t] == GT_SKIP) continue;
                    double cu[4], su[4], cw[4], sw[4];
#pragma unroll
                    for (int m = 0; m < 4; ++m) {
                        cu[m] = L.cu[t][rg * 4 + m]; su[m] = L.su[t][rg * 4 + m];
                        cw[m] = L.cw[t][cg * 4 + m]; sw[m] = L.sw[t][cg * 4 + m];
                    }
                    dx_term<DM, DB, ENV>(acc, p, q, L, t, D, d0, cu, su, cw, sw);
                }
            }
        }
        // block d0 + dd: a thread's four consecutive columns of a row are 32 bytes, sixteen neighbouring lanes cover 512 contiguous bytes of it
#pragma unroll
        for (int dd = 0; dd < DB; ++dd) {
            if (d0 + dd >= D) continue;
            double* out = a.out + (int64_t)(d0 + dd) * dstride;
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                const int lr = rg * 4 + m;
                if (lr >= tl.nr) continue;
                double* o = out + (int64_t)(tl.r0 + lr) * a.ldo + tl.c0 + cg * 4;
                if (full) {
                    *reinterpret_cast<d2_t*>(o) = (d2_t){acc[dd][m][0], acc[dd][m][1]};
                    *reinterpret_cast<d2_t*>(o + 2) = (d2_t){acc[dd][m][2], acc[dd][m][3]};
                } else {
#pragma unroll
                    for (int n = 0; n < 4; ++n)
                        if (cg * 4 + n < tl.nc) o[n] = acc[dd][m][n];
                }
            }
        }
    }
}

// every row block of the Jacobian in one launch: block d at a.out + d * dstride.  The table's kinds must hold no gate, weighted-dot, white or
// Matern 1/2 row (the caller has refused them: mogp_exact_predict_grad)
int launch_gram_dx(const GramArgs& a0, int ntiles, int64_t dstride, hipStream_t s) {
    if (ntiles <= 0) return 0;
    GramArgs a = a0;
    if (a.W <= 0) a.W = 2 + 3 * a.D;
    a.dbg = 0; a.tab_lds = 0;
    if (a.D < 1 || a.D > MOGP_MAXD) { set_error("launch_gram_dx: input dimension out of range"); return -1; }
    const bool env = a.W > 2 + 3 * a.D;
    if (a.kind && (!a.shape || env)) { set_error("launch_gram_dx: kinds without shapes, or with enveloped term rows"); return -1; }
    if (a.W != 2 + 3 * a.D && a.W != 2 + 5 * a.D) { set_error("launch_gram_dx: table rows of an unknown width"); return -1; }
    int rc = a.phases_ready ? 0 : launch_phase_tables(a.ph, a.xr, a.ldxr, a.nrows, a.xc, a.ldxc, a.ncols, a.table, a.T, a.D, a.C, a.W, s);
    if (rc) return rc;
    if (a.ev0) HIP_TRY(hipEventRecord(a.ev0, s));
#define DX_LAUNCH(DT, ENV, RAD) hipLaunchKernelGGL((k_gram_dx<DT, ENV, RAD>), dim3(ntiles), dim3(256), 0, s, a, ntiles, dstride)
    if (a.kind) {
        switch (a.D) {
            case 1: DX_LAUNCH(1, false, true); break;
            case 2: DX_LAUNCH(2, false, true); break;
            case 3: DX_LAUNCH(3, false, true); break;
            default: DX_LAUNCH(0, false, true); break;
        }
    } else if (env) {
        switch (a.D) {
            case 1: DX_LAUNCH(1, true, false); break;
            case 2: DX_LAUNCH(2, true, false); break;
            case 3: DX_LAUNCH(3, true, false); break;
            default: DX_LAUNCH(0, true, false); break;
        }
    } else {
        switch (a.D) {
            case 1: DX_LAUNCH(1, false, false); break;
            case 2: DX_LAUNCH(2, false, false); break;
            case 3: DX_LAUNCH(3, false, false); break;
            default: DX_LAUNCH(0, false, false); break;
        }
    }
#undef DX_LAUNCH
    if (a.ev1) HIP_TRY(hipEventRecord(a.ev1, s));
    HIP_TRY(hipGetLastError());
    return 0;
}

// ---- the mixed second derivative of a symmetric Gram -----------------------------------------------------------------------
// H_de[a][b] = d^2 K(x_a, x_b) / dx_a,d dx_b,e over (Xs, Xs): the prior covariance of df/dx_d(x_a) and df/dx_e(x_b), from which the joint
// posterior covariance of the derivative subtracts one product (exact.hip: mogp_exact_predict_grad_cov).  With u = x_a - x_b + Delta,
// theta = 2 pi (M u + Psi), s = sum V u^2 and the three profile functions phi, psi = -2 dphi/ds, chi = -2 dpsi/ds (radial_profile3):
//   profile rows (0, 1, 3, 4, 6)  k = A phi cos:  k_d  = dk/du_d = A [ -psi V_d u_d cos - 2 pi M_d phi sin ]
//                                 k_de = A [ (chi V_d u_d V_e u_e - delta_de V_d psi - 4 pi^2 M_d M_e phi) cos + 2 pi psi (V_d u_d M_e + V_e u_e M_d) sin ]
//                                 d/dx_a,d = k_d,  d/dx_b,e = -k_e,  H_de = -k_de      (Gaussian rows: phi = psi = chi = exp(-s/2))
//   periodic rows (D = 1)         k = A exp(V (cos - 1)):  k_u = -A V 2 pi M sin E,  H = A V (2 pi M)^2 E (cos - V sin^2)
//   dot-product rows              k = b^n:  d/dx_a,d = n b^(n-1) A x_b,d,  d/dx_b,e = n b^(n-1) A x_a,e,
//                                 H_de = n (n-1) b^(n-2) A^2 x_b,d x_a,e + n b^(n-1) A delta_de
//   enveloped rows                k = g(m) h(u), m the midpoint less the centre, g = exp(-1/2 sum L m^2): d/dx_a = d_u + 1/2 d_m, d/dx_b = -d_u + 1/2 d_m,
//                                 H_de = -g h_de + 1/2 g_e h_d - 1/2 g_d h_e + 1/4 g_de h,  g_d = -L_d m_d g,  g_de = (L_d m_d L_e m_e - delta_de L_d) g
//   a product group               the product rule carried FORWARD over the group's rows: with (P, Pa, Pb, Pab) the product so far, its two first
//                                 derivatives and its mixed one, a row (k, ka, kb, kab) makes Pab <- Pab k + Pa kb + Pb ka + P kab, Pa <- Pa k + P ka,
//                                 Pb <- Pb k + P kb, P <- P k -- sum_h H_h prod k_g + sum_{h != g} (d_a k_h)(d_b k_g) prod k_f term by term, every row
//                                 evaluated once and nothing ever divided out.  A row on its own is a group of one.
// One 64 x 64 tile of the SYMMETRIC tile list per workgroup (lower tiles only), 4 x 4 entries per thread, staged by tile_context / stage_chunk
// without the tile-centred split, ONE (d, e) pair per pass: D^2 passes over the terms.  The output is ONE (D Spad) x (D Spad) matrix, block
// (d, e) at row offset d * bstride and column offset e * bstride.  A tile of the matrix diagonal (GT_DIAG) holds both triangles of its 64 x 64
// entries and is stored once; any other tile is stored twice, as H_de[a][b] and -- by H_de[a][b] = H_ed[b][a] -- transposed into block (e, d)
// at [b][a].  Every element of the matrix is written exactly once: a plain launch, no flags, no atomics.  A group is walked row of entries
// by row of entries (m outermost), so the recurrence keeps 16 values for four entries, not 64 for sixteen.

// phi, psi = -2 dphi/ds and chi = -2 dpsi/ds of the kinds the derivative carries (Matern 1/2 never gets here).  The only singular one is
// Matern 3/2 at s = 0 (chi = 9 exp(-r) / r): there chi is RETURNED as 0, the limit of the only product it enters (chi u_d u_e = O(r)).
__device__ __forceinline__ void radial_profile3(int kind, double shape, double s, double& phi, double& psi, double& chi) {
    s = fmax(s, 0.0);
    switch (kind) {
        case MOGP_KIND_RQ: {
            const double b = fma(s, 0.5 / shape, 1.0), ib = 1.0 / b;
            phi = exp(-shape * log(b));
            psi = phi * ib;
            chi = ((shape + 1.0) / shape) * psi * ib;
        } break;
        case MOGP_KIND_MATERN32: {
            const double r = sqrt(3.0 * s), e = exp(-r);
            phi = fma(r, e, e);
            psi = 3.0 * e;
            chi = r > 0.0 ? 9.0 * e / r : 0.0;
        } break;
        case MOGP_KIND_MATERN52: {
            const double r = sqrt(5.0 * s), e = exp(-r);
            phi = fma(r, r, 3.0 * (1.0 + r)) * (e * (1.0 / 3.0));
            psi = (5.0 / 3.0) * fma(r, e, e);
            chi = (25.0 / 3.0) * e;
        } break;
        case MOGP_KIND_SINC: {
            // chi = (3 psi - pi^2 phi) / s = 2 pi^4 sum_j (-x)^j (j + 1)(2j + 4) / (2j + 5)!,  x = pi^2 s  (chi(0) = pi^4 / 15).  The series below
            // x = 1 (first neglected term 10 * 22 x^9 / 23! < 1e-20 beside 1 / 30); above it the closed forms, where 3 psi - pi^2 phi has lost at
            // most log2(15 / x) < 4 bits more than psi.  phi and psi exactly as radial_profile<true> has them.
            const double x = 9.869604401089358 * s;
            if (x <= 1.0) {
                double a = 2.8114572543455206e-15;                       // 1 / 17!
                a = fma(-x, a, 7.6471637318198164e-13);                 // 1 / 15!
                a = fma(-x, a, 1.6059043836821613e-10);                 // 1 / 13!
                a = fma(-x, a, 2.505210838544172e-08);                  // 1 / 11!
                a = fma(-x, a, 2.7557319223985893e-06);                 // 1 / 9!
                a = fma(-x, a, 1.984126984126984e-04);                  // 1 / 7!
                a = fma(-x, a, 8.333333333333333e-03);                  // 1 / 5!
                a = fma(-x, a, 1.6666666666666666e-01);                 // 1 / 3!
                phi = fma(-x, a, 1.0);
                double b = 4.4983316069528329e-14;                       // 16 / 17!
                b = fma(-x, b, 1.0706029224547743e-11);                 // 14 / 15!
                b = fma(-x, b, 1.9270852604185937e-09);                 // 12 / 13!
                b = fma(-x, b, 2.505210838544172e-07);                  // 10 / 11!
                b = fma(-x, b, 2.2045855379188714e-05);                 // 8 / 9!
                b = fma(-x, b, 1.1904761904761906e-03);                 // 6 / 7!
                b = fma(-x, b, 3.3333333333333333e-02);                 // 4 / 5!
                b = fma(-x, b, 3.3333333333333331e-01);                 // 2 / 3!
                psi = 9.869604401089358 * b;
                double c = 3.5231792294250488e-18;                       // 9 * 20 / 21!
                c = fma(-x, c, 1.1837882210868172e-15);                 // 8 * 18 / 19!
                c = fma(-x, c, 3.1487144778081596e-13);                 // 7 * 16 / 17!
                c = fma(-x, c, 6.4236175347286462e-11);                 // 6 * 14 / 15!
                c = fma(-x, c, 9.6354263020929683e-09);                 // 5 * 12 / 13!
                c = fma(-x, c, 1.0020843354176688e-06);                 // 4 * 10 / 11!
                c = fma(-x, c, 6.6137566137566142e-05);                 // 3 * 8 / 9!
                c = fma(-x, c, 2.3809523809523812e-03);                 // 2 * 6 / 7!
                c = fma(-x, c, 3.3333333333333333e-02);                 // 1 * 4 / 5!
                chi = 2.0 * 97.409091034002437 * c;                      // 2 pi^4
            } else {
                const double r = sqrt(s);
                double sn, cs;
                sincospi(r, &sn, &cs);
                phi = sn / (3.14159265358979323846 * r);
                psi = (phi - cs) / s;
                chi = fma(3.0, psi, -9.869604401089358 * phi) / s;
            }
        } break;
        default:
            phi = exp(-0.5 * s);
            psi = phi;
            chi = phi;
            break;
    }
}

// x[d] for a d the compiler does not know: a blend over the (few) registers of a specialised instantiation -- an index would send the thread's
// inputs to scratch --, a plain index in the generic one, whose inputs live there anyway
template <int DM>
__device__ __forceinline__ double pick(const double (&x)[DM], int d) {
    if constexpr (DM <= 3) {
        double r = 0.0;                                     // (a blend by 0 / 1 weights, exact: a chain of selects is turned back into an index)
#pragma unroll
        for (int j = 0; j < DM; ++j) r = fma(x[j], d == j ? 1.0 : 0.0, r);
        return r;
    } else {
        return x[d];
    }
}

// (k, d/dx_a,d, d/dx_b,e, d^2/dx_a,d dx_b,e) of the radial row t at the four entries of one thread row: p = the row point, q the four column points
template <int DM>
__device__ __forceinline__ void dxdx_row_radial(double (&k)[4], double (&ka)[4], double (&kb)[4], double (&kab)[4], const double (&p)[DM],
                                                const double (&q)[4][DM], const TileLds<DM>& L, int t, int D, int d, int e, int kind, double shape,
                                                int lr, int cg) {
    constexpr double TWO_PI = 6.283185307179586476925286766559;
    const double* V = L.V[t];
    const double* s = L.s[t];
    const double A = L.A[t];
    if (kind == MOGP_KIND_DOT) {                            // x_a = p + the row centre (L.Kp), x_b = q + the column centre (L.L): dot_row_inner
        const int n = dot_row_degree(shape);
        const double c = L.e[t][0], xae = pick<DM>(p, e) + L.Kp[t][e];
#pragma unroll
        for (int nn = 0; nn < 4; ++nn) {
            double ip = 0.0;                                // (dot_row_inner, its loop unrolled by name: an index the compiler keeps sends q to scratch)
#pragma unroll
            for (int j = 0; j < DM; ++j)
                if (j < D) ip = fma(p[j] + L.Kp[t][j], q[nn][j] + L.L[t][j], ip);
            const double b = fma(A, ip, c), xbd = pick<DM>(q[nn], d) + L.L[t][d];
            const double b1 = n > 1 ? dot_row_power(b, n - 1) : 1.0, b2 = n > 2 ? dot_row_power(b, n - 2) : 1.0;
            const double g = (double)n * A * b1;
            k[nn] = b1 * b;
            ka[nn] = g * xbd;
            kb[nn] = g * xae;
            kab[nn] = (n > 1 ? (double)(n * (n - 1)) * A * A * b2 * xbd * xae : 0.0) + (d == e ? g : 0.0);
        }
        return;
    }
    const bool per = kind == MOGP_KIND_PERIODIC;
    const double cu = L.cu[t][lr], su = L.su[t][lr];        // (times the amplitude, but for the periodic row: stage_item_compute)
    const double md = TWO_PI * L.M[t][d], me = TWO_PI * L.M[t][e], pd = pick<DM>(p, d), pe = pick<DM>(p, e);
#pragma unroll
    for (int nn = 0; nn < 4; ++nn) {
        if ((nn & 1) == 0) __builtin_amdgcn_sched_barrier(0);      // two entries' profiles at a time (see dx_term_radial)
        const double cw = L.cw[t][cg * 4 + nn], sw = L.sw[t][cg * 4 + nn];
        const double cc = fma(cu, cw, su * sw), sn = fma(su, cw, -cu * sw);
        double phi, psi, chi;
        if (per) {                                          // D = 1: k_u = -A V 2 pi M sin E and k_uu = A V (2 pi M)^2 E (V sin^2 - cos)
            radial_profile<false>(MOGP_KIND_GAUSS, shape, periodic_s(V[0], cc), phi, psi);
            const double E = A * phi, ku = -E * V[0] * md * sn;
            k[nn] = E;
            ka[nn] = ku;
            kb[nn] = -ku;
            kab[nn] = E * V[0] * md * md * (cc - V[0] * sn * sn);
            continue;
        }
        double arg = 0.0;                                   // (radial_s, unrolled by name)
#pragma unroll
        for (int j = 0; j < DM; ++j)
            if (j < D) { const double u = (p[j] - q[nn][j]) + s[j]; arg = fma(V[j] * u, u, arg); }
        radial_profile3(kind, shape, arg, phi, psi, chi);
        const double wd = V[d] * ((pd - pick<DM>(q[nn], d)) + s[d]), we = V[e] * ((pe - pick<DM>(q[nn], e)) + s[e]);
        k[nn] = phi * cc;
        ka[nn] = -fma(psi * wd, cc, md * phi * sn);
        kb[nn] = fma(psi * we, cc, me * phi * sn);
        double h = fma(chi * wd, we, -md * me * phi);
        if (d == e) h -= V[d] * psi;
        kab[nn] = -fma(h, cc, psi * fma(wd, me, we * md) * sn);
    }
}

// one Gaussian or enveloped term of a table without kinds: acc += H_de at the thread's sixteen entries
template <int DM, bool ENV>
__device__ __forceinline__ void dxdx_term(double (&acc)[4][4], const double (&p)[4][DM], const double (&q)[4][DM], const TileLds<DM>& L, int t,
                                          int D, int d, int e, const double (&cu)[4], const double (&su)[4], const double (&cw)[4], const double (&sw)[4]) {
    constexpr double TWO_PI = 6.283185307179586476925286766559;
    const double* V = L.V[t];
    const double* s = L.s[t];
    const double md = TWO_PI * L.M[t][d], me = TWO_PI * L.M[t][e];
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        __builtin_amdgcn_sched_barrier(0);                  // one row of four library exps at a time (see gram_term_radial)
#pragma unroll
        for (int n = 0; n < 4; ++n) {
            const double E = gauss_general<DM>(p[m], q[n], V, s, L.L[t], L.e[t], D);      // (the envelope's g included)
            const double cc = E * fma(cu[m], cw[n], su[m] * sw[n]), sn = E * fma(su[m], cw[n], -cu[m] * sw[n]);
            const double wd = V[d] * ((p[m][d] - q[n][d]) + s[d]), we = V[e] * ((p[m][e] - q[n][e]) + s[e]);
            double h = fma(wd, we, -md * me);
            if (d == e) h -= V[d];
            double H = -fma(h, cc, fma(wd, me, we * md) * sn);                            // -g h_de
            if (ENV) {
                const double gd = -L.L[t][d] * (0.5 * (p[m][d] + q[n][d]) + L.e[t][d]), ge = -L.L[t][e] * (0.5 * (p[m][e] + q[n][e]) + L.e[t][e]);
                const double hd = -fma(wd, cc, md * sn), he = -fma(we, cc, me * sn);      // g h_d, g h_e
                H = fma(0.5 * ge, hd, H);
                H = fma(-0.5 * gd, he, H);
                H = fma(0.25 * (gd * ge - (d == e ? L.L[t][d] : 0.0)), cc, H);
            }
            acc[m][n] += H;
        }
    }
}

template <int DT, bool ENV, bool RAD>
__global__ __launch_bounds__(256) void k_gram_dxdx(GramArgs a, int ntiles, int64_t bstride) {
    static_assert(!(ENV && RAD), "radial rows carry no envelope");
    constexpr int DM = DT > 0 ? DT : MOGP_MAXD;
    const int D = DT > 0 ? DT : a.D;
    const int W = a.W;
    const int tid = threadIdx.x;
    const int cg = tid & 15, rg = tid >> 4;
    if ((int)blockIdx.x >= ntiles) return;
    const GTile tl = a.tiles[blockIdx.x];
    const double* tab = a.table + (size_t)tl.pair * a.T * W;
    const int* kinds = RAD ? a.kind + (size_t)tl.pair * a.T : nullptr;
    __shared__ TileLds<DM> L;
    const PhaseView v = phase_view(a.ph.ws, a.C, a.T, D, a.ldxr, a.ldxc);
    TileCtx<DM> X;
    double p[4][DM], q[4][DM];
    tile_context<DM>(X, p, q, tl, D, v, a.xr, a.ldxr, a.xc, a.ldxc, rg, cg);
    const bool mirror = !(tl.flags & GT_DIAG);

    for (int de = 0; de < D * D; ++de) {
        const int d = de / D, e = de - d * D;
        double acc[4][4];
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
            for (int n = 0; n < 4; ++n) acc[m][n] = 0.0;
        for (int t0 = 0, nt; t0 < a.T; t0 += nt) {
            if constexpr (RAD) nt = radial_chunk(a.kind, a.T, t0); else nt = min(MOGP_TC, a.T - t0);
            if (t0 > 0 || de > 0) __syncthreads();           // the chunk before this one has been consumed
            stage_chunk<DM, true, false, RAD, 0, false>(L, X, tl, tab, W, D, a.C, a.T, t0, nt, v, a.xr, a.ldxr, a.xc, a.ldxc, tid, kinds);
            __syncthreads();
            if constexpr (RAD) {
                const int* kd = kinds + t0;
                const double* sh = a.shape + (size_t)tl.pair * a.T + t0;
                for (int t = 0, te; t < nt; t = te + 1) {    // group by group, as k_gram_dx walks them
                    bool skip = false;
                    for (te = t;; ++te) {
                        skip |= L.deg[te] == GT_SKIP;
                        if (te == nt - 1 || !(__builtin_amdgcn_readfirstlane(kd[te]) & MOGP_KIND_TIMES)) break;
                    }
                    if (skip) continue;                      // a row of zero amplitude: the group and every term of its derivatives are zero
#pragma unroll 1
                    for (int m = 0; m < 4; ++m) {            // a LOOP over the thread's rows: the row's inputs by an exact 0 / 1 blend, one copy of the group's code
                        double pm[DM], P[4], Pa[4], Pb[4], Pab[4];
#pragma unroll
                        for (int j = 0; j < DM; ++j) {
                            pm[j] = 0.0;
#pragma unroll
                            for (int mm = 0; mm < 4; ++mm) pm[j] = fma(p[mm][j], mm == m ? 1.0 : 0.0, pm[j]);
                        }
                        dxdx_row_radial<DM>(P, Pa, Pb, Pab, pm, q, L, t, D, d, e, __builtin_amdgcn_readfirstlane(kd[t]) & MOGP_KIND_MASK, sh[t], rg * 4 + m, cg);
                        for (int h = t + 1; h <= te; ++h) {
                            double k[4], ka[4], kb[4], kab[4];
                            dxdx_row_radial<DM>(k, ka, kb, kab, pm, q, L, h, D, d, e, __builtin_amdgcn_readfirstlane(kd[h]) & MOGP_KIND_MASK, sh[h], rg * 4 + m, cg);
#pragma unroll
                            for (int n = 0; n < 4; ++n) {
                                Pab[n] = fma(Pab[n], k[n], fma(Pa[n], kb[n], fma(Pb[n], ka[n], P[n] * kab[n])));
                                Pa[n] = fma(Pa[n], k[n], P[n] * ka[n]);
                                Pb[n] = fma(Pb[n], k[n], P[n] * kb[n]);
                                P[n] *= k[n];
                            }
                        }
#pragma unroll
                        for (int mm = 0; mm < 4; ++mm)
#pragma unroll
                            for (int n = 0; n < 4; ++n) acc[mm][n] += mm == m ? Pab[n] : 0.0;
                    }
                }
            } else {
                for (int t = 0; t < nt; ++t) {
                    if (L.deg[t] == GT_SKIP) continue;
                    double cu[4], su[4], cw[4], sw[4];
#pragma unroll
                    for (int m = 0; m < 4; ++m) {
                        cu[m] = L.cu[t][rg * 4 + m]; su[m] = L.su[t][rg * 4 + m];
                        cw[m] = L.cw[t][cg * 4 + m]; sw[m] = L.sw[t][cg * 4 + m];
                    }
                    dxdx_term<DM, ENV>(acc, p, q, L, t, D, d, e, cu, su, cw, sw);
                }
            }
        }
        // block (d, e) at [a][b], and for a tile off the matrix diagonal block (e, d) at [b][a]; rows and columns past the tile's points are not stored
        double* out = a.out + ((int64_t)d * bstride) * a.ldo + (int64_t)e * bstride;
        double* outT = a.out + ((int64_t)e * bstride) * a.ldo + (int64_t)d * bstride;
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const int lr = rg * 4 + m;
            if (lr >= tl.nr) continue;
#pragma unroll
            for (int n = 0; n < 4; ++n) {
                const int lc = cg * 4 + n;
                if (lc >= tl.nc) continue;
                out[(int64_t)(tl.r0 + lr) * a.ldo + tl.c0 + lc] = acc[m][n];
                if (mirror) outT[(int64_t)(tl.c0 + lc) * a.ldo + tl.r0 + lr] = acc[m][n];
            }
        }
    }
}

// H over the symmetric tile list of (xr, xr) (build_sym_tiles; a.xc = a.xr) into the (D bstride)^2 matrix a.out of leading dimension a.ldo.
// Tables and kinds as launch_gram_dx takes them; noise, dvar, mirror, out2 and the strip lists are not read.
int launch_gram_dxdx(const GramArgs& a0, int ntiles, int64_t bstride, hipStream_t s) {
    if (ntiles <= 0) return 0;
    GramArgs a = a0;
    if (a.W <= 0) a.W = 2 + 3 * a.D;
    a.dbg = 0; a.tab_lds = 0;
    if (a.D < 1 || a.D > MOGP_MAXD) { set_error("launch_gram_dxdx: input dimension out of range"); return -1; }
    const bool env = a.W > 2 + 3 * a.D;
    if (a.kind && (!a.shape || env)) { set_error("launch_gram_dxdx: kinds without shapes, or with enveloped term rows"); return -1; }
    if (a.W != 2 + 3 * a.D && a.W != 2 + 5 * a.D) { set_error("launch_gram_dxdx: table rows of an unknown width"); return -1; }
    if (a.xc != a.xr || a.ldxc != a.ldxr || a.ldo < a.D * bstride) { set_error("launch_gram_dxdx: not a symmetric launch, or the output is too narrow for D blocks"); return -1; }
    int rc = a.phases_ready ? 0 : launch_phase_tables(a.ph, a.xr, a.ldxr, a.nrows, a.xc, a.ldxc, a.ncols, a.table, a.T, a.D, a.C, a.W, s);
    if (rc) return rc;
    if (a.ev0) HIP_TRY(hipEventRecord(a.ev0, s));
#define DXDX_LAUNCH(DT, ENV, RAD) hipLaunchKernelGGL((k_gram_dxdx<DT, ENV, RAD>), dim3(ntiles), dim3(256), 0, s, a, ntiles, bstride)
    if (a.kind) {
        switch (a.D) {
            case 1: DXDX_LAUNCH(1, false, true); break;
            case 2: DXDX_LAUNCH(2, false, true); break;
            case 3: DXDX_LAUNCH(3, false, true); break;
            default: DXDX_LAUNCH(0, false, true); break;
        }
    } else if (env) {
        switch (a.D) {
            case 1: DXDX_LAUNCH(1, true, false); break;
            case 2: DXDX_LAUNCH(2, true, false); break;
            case 3: DXDX_LAUNCH(3, true, false); break;
            default: DXDX_LAUNCH(0, true, false); break;
        }
    } else {
        switch (a.D) {
            case 1: DXDX_LAUNCH(1, false, false); break;
            case 2: DXDX_LAUNCH(2, false, false); break;
            case 3: DXDX_LAUNCH(3, false, false); break;
            default: DXDX_LAUNCH(0, false, false); break;
        }
    }
#undef DXDX_LAUNCH
    if (a.ev1) HIP_TRY(hipEventRecord(a.ev1, s));
    HIP_TRY(hipGetLastError());
    return 0;
}

// ---- gradient moments ---------------------------------------------------------------------------------
// partial[tile][t][w], w = [ m0 = sum g E cos, m4 = sum g E sin, m1_d = sum g u_d^2 E cos, m2_d = sum g u_d E cos,
//                           m3_d = sum g u_d E sin ].
// Exact mode (DENSE = false):  g = weight * 1/2 (alpha_a alpha_b - Kinv_ab), weight = 2 (symmetric double count: strictly
// lower entries of diagonal channel blocks, every entry of off-diagonal channel blocks -- reference kernel.py:466-467
// writes k and k.T), 1 on the matrix diagonal, 0 above it.
// Dense mode (DENSE = true, Titsias):  g = weight * (G[a][b] + rcoef ru[a] rw[b]); weight as above when a.sym, else 1.
// ZG: also accumulate the gradient w.r.t. the row / column INPUTS (inducing points):
//     dK_ab/dx_a,d = sum_t A_t E [ -V_d u_d cos - 2 pi M_d sin ] = - dK_ab/dx_b,d.
// A thread accumulates the W moments of its 16 entries of one term in registers; the workgroup reduction goes through LDS (16 slice sums
// of 16 threads each, then a 4-step butterfly: fixed order, bit-reproducible) with ONE barrier per term.
template <int DM, int N, bool ZG, bool ENV>
__device__ __forceinline__ void moment_term(double* mom, const double (&g)[4][4], const double (&p)[4][DM], const double (&q)[4][DM],
                                            const TileLds<DM>& L, int t, int D,
                                            const double (&cu)[4], const double (&su)[4], const double (&cw)[4], const double (&sw)[4],
                                            double (&zr)[4][DM], double (&zc)[4][DM]) {
    const double* V = L.V[t];
    const double* s = L.s[t];
    const double* Mv = L.M[t];
    const double A = L.A[t];
    double vp[4][DM];
    if (N > 0) {
#pragma unroll
        for (int m = 0; m < 4; ++m)
            for (int d = 0; d < D; ++d) vp[m][d] = L.Kp[t][d] * p[m][d];
    }
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int n = 0; n < 4; ++n) {
            double u[DM];
            for (int d = 0; d < D; ++d) u[d] = (p[m][d] - q[n][d]) + s[d];
            double e;
            if (N > 0) {
                double z = vp[m][0] * q[n][0];
                for (int d = 1; d < D; ++d) z = fma(vp[m][d], q[n][d], z);
                e = exp_taylor<N>(z);
            } else {
                e = gauss_general<DM>(p[m], q[n], V, s, L.L[t], L.e[t], D);
            }
            const double ge = g[m][n] * e;
            const double kc = ge * fma(cu[m], cw[n], su[m] * sw[n]);
            const double ks = ge * fma(su[m], cw[n], -cu[m] * sw[n]);
            mom[0] += kc;
            mom[1] += ks;
            for (int d = 0; d < D; ++d) {
                const double uk = u[d] * kc;
                mom[2 + d] = fma(u[d], uk, mom[2 + d]);
                mom[2 + D + d] += uk;
                mom[2 + 2 * D + d] = fma(u[d], ks, mom[2 + 2 * D + d]);
                if (ENV) {                                 // envelope moments: a = midpoint - centre
                    const double a = 0.5 * (p[m][d] + q[n][d]) + L.e[t][d];
                    const double ak = a * kc;
                    mom[2 + 3 * D + d] = fma(a, ak, mom[2 + 3 * D + d]);
                    mom[2 + 4 * D + d] += ak;
                }
                if (ZG) {
                    const double j = -A * fma(V[d], uk, 6.283185307179586476925286766559 * Mv[d] * ks);
                    zr[m][d] += j;
                    zc[n][d] -= j;
                    if (ENV) {                             // the envelope sits on the MIDPOINT: d/dx_a = d/dx_b = -1/2 L_d a_d K
                        const double je = -0.5 * A * L.L[t][d] * (0.5 * (p[m][d] + q[n][d]) + L.e[t][d]) * kc;
                        zr[m][d] += je;
                        zc[n][d] += je;
                    }
                }
            }
        }
}

// the radial form of moment_term (exact mode, no envelope, no input gradients): phi weighs m0, m4, m3_d; psi = -2 dphi/ds weighs m1_d, m2_d
template <int DM, int GATE = 0>
__device__ __forceinline__ void moment_term_radial(double* mom, const double (&g)[4][4], const double (&p)[4][DM], const double (&q)[4][DM],
                                                   const TileLds<DM>& L, int t, int D, int kind, double shape,
                                                   const double (&cu)[4], const double (&su)[4], const double (&cw)[4], const double (&sw)[4],
                                                   bool ondiag = false) {
    const double* V = L.V[t];
    const double* s = L.s[t];
    const bool per = kind == MOGP_KIND_PERIODIC;             // (it reads V_0 and the row's phase: m1_0 and m3_0, slots 2 and 2 + 2 D)
    if (kind == MOGP_KIND_DOT) {
        // k = b^n, b = A <x_a, x_b> + c:  m0 = sum g n b^(n-1) <x_a, x_b> = d/dA,  m1_0 = sum g n b^(n-1) = d/dc (slots 0 and 2: both even in tau,
        // k_moment_reduce keeps them on diagonal channel blocks); the other slots stay 0
        const int n = dot_row_degree(shape);
        const double A = L.A[t], c = L.e[t][0];
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
            for (int nn = 0; nn < 4; ++nn) {
                const double ip = dot_row_inner<DM>(p[m], q[nn], L, t, D);
                const double w = g[m][nn] * ((double)n * (n > 1 ? dot_row_power(fma(A, ip, c), n - 1) : 1.0));
                mom[0] = fma(w, ip, mom[0]);
                mom[2] += w;
            }
        return;
    }
    if (GATE && kind == MOGP_KIND_GATE) {
        // k = h_a h_b (unit amplitude staged: the row's own A is the host's, as for a profile row), h = sigmoid(beta (x - l)), dh/dz = h (1 - h):
        // m0 = sum g k,  m1_0 = sum g k [(1 - h_a)(x_a - l) + (1 - h_b)(x_b - l)] = d/dbeta / A,  m3_0 = -beta sum g k [(1 - h_a) + (1 - h_b)] = d/dl / A  (slots 0, 2, 4: all
        // even under a <-> b, k_moment_reduce keeps them on diagonal channel blocks); the other slots stay 0.  x - l from the thread's centred
        // input and the tile centre the staging left in L.Kp / L.L; the complements come staged (su, sw)
        const double er = L.Kp[t][0] - L.M[t][0], ec = L.L[t][0] - L.M[t][0];
        double m3 = 0.0;
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
            for (int nn = 0; nn < 4; ++nn) {
                const double k = g[m][nn] * (cu[m] * cw[nn]);
                mom[0] += k;
                mom[2] = fma(k, fma(su[m], p[m][0] + er, sw[nn] * (q[nn][0] + ec)), mom[2]);
                m3 = fma(k, su[m] + sw[nn], m3);
            }
        mom[4] = fma(-V[0], m3, mom[4]);
        return;
    }
    if (GATE > 1 && kind == MOGP_KIND_WDOT) {
        // k = sum_d V_d x_a,d x_b,d (the row's own A is the host's): m0 = sum g k = d/dA, m1_d = sum g x_a,d x_b,d = d/dV_d / A (slots 0 and 2 + d: even
        // under a <-> b); the other slots stay 0
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
            for (int nn = 0; nn < 4; ++nn) {
                double k = 0.0;
                for (int d = 0; d < D; ++d) {
                    const double xx = (p[m][d] + L.Kp[t][d]) * (q[nn][d] + L.L[t][d]);
                    mom[2 + d] = fma(g[m][nn], xx, mom[2 + d]);
                    k = fma(V[d], xx, k);
                }
                mom[0] = fma(g[m][nn], k, mom[0]);
            }
        return;
    }
    if (GATE > 1 && kind == MOGP_KIND_WHITE) {                  // m0 = sum_k g_kk; the other slots stay 0
        if (ondiag) {
#pragma unroll
            for (int m = 0; m < 4; ++m) mom[0] += g[m][m];
        }
        return;
    }
#pragma unroll
    for (int m = 0; m < 4; ++m) {
#pragma unroll
        for (int n = 0; n < 4; ++n) {
            if ((n & 1) == 0) __builtin_amdgcn_sched_barrier(0);      // two entries' profiles at a time (see gram_term_radial; a whole row spills here)
            double u[DM], arg = 0.0;
            for (int d = 0; d < D; ++d) {
                u[d] = (p[m][d] - q[n][d]) + s[d];
                arg = fma(V[d] * u[d], u[d], arg);
            }
            double phi, psi;
            const double cc = fma(cu[m], cw[n], su[m] * sw[n]), sn = fma(su[m], cw[n], -cu[m] * sw[n]);
            if (per) {                                      // E = exp(V (cos - 1)): m0 = g E, m4 = g E V sin, m1 = g E 2 (1 - cos), m2 = 0, m3 = g E V u sin
                radial_profile<false>(MOGP_KIND_GAUSS, shape, periodic_s(V[0], cc), phi, psi);
                const double ge = g[m][n] * phi, ks = ge * V[0] * sn;
                mom[0] += ge;
                mom[1] += ks;
                mom[2] = fma(ge, 2.0 * (1.0 - cc), mom[2]);
                mom[2 + 2 * D] = fma(u[0], ks, mom[2 + 2 * D]);
                continue;
            }
            radial_profile<true>(kind, shape, arg, phi, psi);
            const double kc = g[m][n] * phi * cc;
            const double ks = g[m][n] * phi * sn;
            const double kp = g[m][n] * psi * cc;
            mom[0] += kc;
            mom[1] += ks;
            for (int d = 0; d < D; ++d) {
                const double uk = u[d] * kp;
                mom[2 + d] = fma(u[d], uk, mom[2 + d]);
                mom[2 + D + d] += uk;
                mom[2 + 2 * D + d] = fma(u[d], ks, mom[2 + 2 * D + d]);
            }
        }
    }
}

// Two workgroups per CU wherever the registers allow it with a handful of spills (D = 1: the input-gradient variant needs 268 VGPRs
// unconstrained, i.e. ONE wave per SIMD and nothing to hide its loads behind).
// (round 4: cutting the registers to three or four waves per SIMD -- __launch_bounds__(256, 3 / 4) -- costs 81 / 92 spilled VGPRs; the pressure is
// the tile's adjoint block (g: 32 VGPRs), the staged factors and the staging prefetch, not the Horner chains)
// RAD: the radial instantiation (a.kind / a.shape are set; ZG and ENV are false); the others contain nothing of it.  RAD with DENSE takes
// g from a dense symmetric adjoint (a.G, lower-stored, the `sym` weights) where the exact form makes it of alpha and Kj^-1 -- the walk over
// rows and groups is the same (mogp_exact_loo: the adjoint of the leave-one-out likelihood).
template <int DT, bool DENSE, bool ZG, bool ENV, bool RAD = false, int GATE = 0>
__global__ __launch_bounds__(256, (DT == 1 && !RAD ? 2 : 1)) void k_moments(MomentArgs a) {      // (RAD, D = 1: the library exps push two workgroups per CU into scratch)
    static_assert(!RAD || (!ZG && !ENV), "radial moments: no input gradients, no envelope");
    constexpr int DM = DT > 0 ? DT : MOGP_MAXD;
    constexpr int WM = 2 + (ENV ? 5 : 3) * DM;
    constexpr int RSTRIDE = 256 + 16;                        // one moment of all threads, +1 per 16 (the slice reads hit distinct banks)
    constexpr int NBUF = WM <= 11 ? 2 : 1;                   // double-buffered reduction staging: one barrier per term instead of two
    const int D = DT > 0 ? DT : a.D;
    const int W = a.W;
    const GTile tl = a.tiles[blockIdx.x];
    const double* tab = a.table + (size_t)tl.pair * a.T * W;
    const int tid = threadIdx.x;
    const int cg = tid & 15, rg = tid >> 4;
    const double* xcol = a.xc ? a.xc : a.x;
    const int64_t ldxc = a.xc ? a.ldxc : a.ldx;

    __shared__ TileLds<DM> L;
    __shared__ double s_red[NBUF][WM * RSTRIDE];
    __shared__ double s_gr[ZG ? DM : 1][MOGP_GT], s_gc[ZG ? DM : 1][MOGP_GT];

    double* outp = a.partial + (size_t)blockIdx.x * a.T * W;
    bool any = false;
    for (int t = 0; t < a.T; ++t) any |= (tab[(size_t)t * W] != 0.0);
    if constexpr (RAD)                                       // (a dot-product row of zero amplitude is c^n)
        for (int t = 0; t < a.T; ++t) any |= (a.kind[(size_t)tl.pair * a.T + t] & MOGP_KIND_MASK) == MOGP_KIND_DOT;
    if (!any) {
        for (int idx = tid; idx < a.T * W; idx += 256) outp[idx] = 0.0;
        return;
    }

    const PhaseView v = phase_view(a.ph.ws, a.C, a.T, D, a.ldx, ldxc);
    TileCtx<DM> X;
    double p[4][DM], q[4][DM];
    tile_context<DM>(X, p, q, tl, D, v, a.x, a.ldx, xcol, ldxc, rg, cg);
    if (ZG) {
        for (int idx = tid; idx < D * MOGP_GT; idx += 256) { s_gr[idx / MOGP_GT][idx % MOGP_GT] = 0.0; s_gc[idx / MOGP_GT][idx % MOGP_GT] = 0.0; }
    }

    // g for this thread's 4x4 entries
    double g[4][4];
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        const int lr = rg * 4 + m;
        const int64_t r = tl.r0 + lr;
        double ar = 0.0;
        if (lr < tl.nr) ar = DENSE ? (a.ru ? a.rcoef * a.ru[r] : 0.0) : a.alpha[r];
#pragma unroll
        for (int n = 0; n < 4; ++n) {
            const int lc = cg * 4 + n;
            const int64_t c = tl.c0 + lc;
            double w = 0.0, v = 0.0;
            if (lr < tl.nr && lc < tl.nc) {
                w = (!DENSE || a.sym) ? 2.0 : 1.0;
                if ((!DENSE || a.sym) && (tl.flags & GT_DIAG)) w = r > c ? 2.0 : (r == c ? 1.0 : 0.0);
                if (DENSE) {
                    const int64_t hi = (a.sym && c > r) ? c : r, lo = (a.sym && c > r) ? r : c;
                    v = a.G[hi * a.ldg + lo] + (a.ru ? ar * a.rw[c] : 0.0);
                } else {
                    const int64_t hi = r > c ? r : c, lo = r > c ? c : r;
                    if (a.row_mod > 1 && (int)((hi / MOGP_TILE) % a.row_mod) != a.row_rem) w = 0.0;       // row owned by another rank
                    else v = 0.5 * (ar * a.alpha[c] - a.kinv_sign * a.kinv[hi * a.ld + lo]);
                }
            }
            g[m][n] = w * v;
        }
    }

    double zr[4][DM], zc[4][DM];
    if (ZG) {
#pragma unroll
        for (int m = 0; m < 4; ++m)
            for (int d = 0; d < D; ++d) { zr[m][d] = 0.0; zc[m][d] = 0.0; }
    }

    int nred = 0;                                            // reductions done so far (selects the staging buffer)
    int tg = 0, te = -1;                                     // RAD: the product group [tg, te] (chunk-relative) that row t belongs to
    const bool ondiag = GATE > 1 && (tl.flags & GT_DIAG) && rg == cg;      // (white rows: the thread's entries (m, m) are matrix-diagonal entries)
    for (int t0 = 0, nt; t0 < a.T; t0 += RAD ? nt : MOGP_TC) {
        if constexpr (RAD) nt = radial_chunk(a.kind, a.T, t0); else nt = min(MOGP_TC, a.T - t0);
        if (t0 > 0) __syncthreads();                         // the first chunk has nothing to wait for
        stage_chunk<DM, false, (DT == 1 && !RAD), RAD, GATE>(L, X, tl, tab, W, D, a.C, a.T, t0, nt, v, a.x, a.ldx, xcol, ldxc, tid, RAD ? a.kind + (size_t)tl.pair * a.T : nullptr);
        __syncthreads();
        te = -1;
        for (int t = 0; t < nt; ++t) {
            const int deg = L.deg[t];
            if (deg == GT_SKIP) {                            // uniform across the workgroup
                if (tid < W) outp[(size_t)(t0 + t) * W + tid] = 0.0;
                continue;
            }
            double mom[WM];
#pragma unroll
            for (int w = 0; w < WM; ++w) mom[w] = 0.0;
            double cu[4], su[4], cw[4], sw[4];
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                cu[m] = L.cu[t][rg * 4 + m]; su[m] = L.su[t][rg * 4 + m];
                cw[m] = L.cw[t][cg * 4 + m]; sw[m] = L.sw[t][cg * 4 + m];
            }
            if constexpr (RAD) {
                // Row t of a product group: today's radial moments with g replaced by g prod_{h != t} k_h per entry (the other rows' values are
                // recomputed, never divided out: a cosine factor passes through zero).  A group of one keeps g itself.
                const int* kd = a.kind + (size_t)tl.pair * a.T + t0;
                const double* sh = a.shape + (size_t)tl.pair * a.T + t0;
                if (t > te) {
                    tg = t;
                    for (te = t; te < nt - 1 && (__builtin_amdgcn_readfirstlane(kd[te]) & MOGP_KIND_TIMES); ++te) {}
                }
                const int kind = __builtin_amdgcn_readfirstlane(kd[t]) & MOGP_KIND_MASK;
                if (te > tg) {
                    double wg[4][4];
#pragma unroll
                    for (int m = 0; m < 4; ++m)
#pragma unroll
                        for (int n = 0; n < 4; ++n) wg[m][n] = g[m][n];
                    for (int h = tg; h <= te; ++h)
                        if (h != t) group_factor_radial<DM, false, GATE>(wg, p, q, L, h, D, __builtin_amdgcn_readfirstlane(kd[h]) & MOGP_KIND_MASK, sh[h], rg, cg, ondiag);
                    moment_term_radial<DM, GATE>(mom, wg, p, q, L, t, D, kind, sh[t], cu, su, cw, sw, ondiag);
                } else {
                    moment_term_radial<DM, GATE>(mom, g, p, q, L, t, D, kind, sh[t], cu, su, cw, sw, ondiag);
                }
            } else
            switch (deg) {
                #define GT_CASE(N) case N: moment_term<DM, N, ZG, ENV>(mom, g, p, q, L, t, D, cu, su, cw, sw, zr, zc); break;
                GT_DEGREE_CASES(GT_CASE)
#undef GT_CASE
                default: moment_term<DM, 0, ZG, ENV>(mom, g, p, q, L, t, D, cu, su, cw, sw, zr, zc); break;
            }
            // workgroup reduction of the W moments of this term through LDS, fixed order: thread (w, i) adds the values of threads
            // 16 i .. 16 i + 15, a 4-step butterfly over i finishes.  With two staging buffers the next term's writes need no second
            // barrier (a buffer is reused two terms later, behind the barrier of the term in between).
            double* rb = s_red[nred % NBUF];
            ++nred;
            for (int w = 0; w < W; ++w) rb[w * RSTRIDE + tid + (tid >> 4)] = mom[w];
            __syncthreads();
            // 256 threads take 16 moments at a time: rows of more than 16 (2 + 3 D from D = 5 on, 2 + 5 D from D = 3 on) need a second pass --
            // without it moments 16 .. W - 1 were never written, and the pair's sum read whatever the scratch held
            constexpr int NPASS = (WM + 15) / 16;
#pragma unroll
            for (int pass = 0; pass < NPASS; ++pass) {
                const int w = pass * 16 + (tid >> 4), i = tid & 15;
                if (w < W) {
                    const double* src = rb + w * RSTRIDE + i * 17;
                    double v = 0.0;
#pragma unroll
                    for (int k = 0; k < 16; ++k) v += src[k];
#pragma unroll
                    for (int off = 8; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
                    if (i == 0) outp[(size_t)(t0 + t) * W + w] = v;
                }
            }
            if (NBUF == 1) __syncthreads();
        }
    }

    if (ZG) {
        // rows: the 16 threads of a row group (cg = 0..15) are consecutive lanes -> butterfly; columns: the 16 row groups' values of a column
        // go through LDS and are added in row-group order.  The tile's sums land in ITS slot of the scratch (no atomics anywhere: the order
        // of every sum is fixed); k_gz_reduce adds the slots of a block.
        double* stage = s_red[0];                              // [16 row groups][64 columns]
        for (int d = 0; d < D; ++d) {
            __syncthreads();
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                double v = zr[m][d];
#pragma unroll
                for (int off = 8; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
                if (cg == 0) s_gr[d][rg * 4 + m] = v;
                stage[rg * MOGP_GT + cg * 4 + m] = zc[m][d];
            }
            __syncthreads();
            if (tid < MOGP_GT) {
                double v = 0.0;
#pragma unroll
                for (int r = 0; r < 16; ++r) v += stage[r * MOGP_GT + tid];
                s_gc[d][tid] = v;
            }
        }
        __syncthreads();
        double* slot_r = a.gzp + ((size_t)tl.rb * a.ncb + tl.cb) * D * MOGP_GT;
        double* slot_c = a.gzp + (size_t)a.nrb * a.ncb * D * MOGP_GT + ((size_t)tl.cb * a.nrb + tl.rb) * D * MOGP_GT;
        for (int idx = tid; idx < D * MOGP_GT; idx += 256) {
            const int d = idx / MOGP_GT, pnt = idx - d * MOGP_GT;
            if (a.gzr) slot_r[idx] = pnt < tl.nr ? s_gr[d][pnt] : 0.0;
            if (a.gzc) slot_c[idx] = pnt < tl.nc ? s_gc[d][pnt] : 0.0;
        }
    }
}

// ---- exact mode, D = 1, no envelope: the persistent, software-pipelined form (round 4) -------------------------------------------------------
// k_moments above is one workgroup per tile: descriptor -> inputs and adjoint entries -> staging are three DEPENDENT memory round trips (12 of
// the 16 us a tile takes), two tiles in flight per CU, the VALUs busy half the time.  Here one 512-thread workgroup per CU walks over tiles
// blockIdx.x, + gridDim.x, ...: everything tile i + 1 needs from memory (its 64 x 64 block of Kj^-1: 8 entries per thread, alpha, inputs, phase
// factors; the descriptor came one tile earlier still) is REQUESTED BEFORE tile i's arithmetic and lands under it -- in registers: with one
// workgroup per CU a wave may use 256 VGPRs, which the one-tile-per-workgroup form could not afford.  A thread owns 2 x 4 entries, accumulates
// the five moments of every term over the whole tile in registers, and the workgroup reduces them ONCE per tile (wave butterflies, then eight
// partial sums through LDS in wave order: fixed order, bit-reproducible) instead of once per term.  Same arithmetic per entry as moment_term.
template <int N>
__device__ __forceinline__ void mx_term(double (&mom)[5], const double (&g)[2][4], const double (&p)[2], const double (&q)[4], double V, double s,
                                        const double (&cu)[2], const double (&su)[2], const double (&cw)[4], const double (&sw)[4]) {
#pragma unroll
    for (int m = 0; m < 2; ++m) {
        const double vp = V * p[m];
#pragma unroll
        for (int n = 0; n < 4; ++n) {
            const double u = (p[m] - q[n]) + s;
            double e;
            if (N > 0) e = exp_taylor<N>(vp * q[n]);
            else e = exp(-0.5 * (V * u) * u);
            const double ge = g[m][n] * e;
            const double kc = ge * fma(cu[m], cw[n], su[m] * sw[n]);
            const double ks = ge * fma(su[m], cw[n], -cu[m] * sw[n]);
            mom[0] += kc;
            mom[1] += ks;
            const double uk = u * kc;
            mom[2] = fma(u, uk, mom[2]);
            mom[3] += uk;
            mom[4] = fma(u, ks, mom[4]);
        }
    }
}

#define MX_T 8                                             // terms at most (registers: 5 moments per term)
struct MxFetch {                                           // what a thread requests for a tile one iteration ahead
    double kv[2][4], ar[2], ac[4], xr[2], xc[4];
    StageItem<1> it[2];
    double cr, hr, cc, hc;
};

template <int TT>
__global__ __launch_bounds__(512, 2) void k_moments_x(MomentArgs a) {
    const int T = a.T, W = a.W, tid = threadIdx.x;
    const int cg = tid & 15, rg = tid >> 4;                  // rows 2 rg, 2 rg + 1; columns 4 cg .. 4 cg + 3
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int st_which = wave & 1, st_tb = wave >> 1, st_pnt = lane;      // staging: wave -> (rows | columns) of the terms wave / 2 and wave / 2 + 4
    __shared__ TileLds<1> Lb[2];
    constexpr int MXS = 512 + 32;                          // one moment of all threads, +1 per 16 (the slice reads hit distinct banks)
    __shared__ double s_red[TT * 5 * MXS];
    const PhaseView v = phase_view(a.ph.ws, a.C, T, 1, a.ldx, a.ldx);
    // round 5: a workgroup walks a CONTIGUOUS chunk of the tile list and keeps the moments in registers from tile to tile for as long as the
    // channel pair stays the same (the tiles of a pair are contiguous in the list: a chunk crosses a pair boundary once or twice); the LDS
    // reduction and its two barriers then happen once per run instead of once per tile, and the slots of the run's other tiles receive zeros
    // (k_moment_reduce adds the slots of a pair in fixed order, as before).  The counters had the kernel's waves parked at s_waitcnt / s_barrier
    // 41 % of their cycles (SQ_WAIT_ANY; profiles/r5_pmc_tile_kernels.txt), the vector ALUs busy half the time.
    const int per = (a.ntiles + (int)gridDim.x - 1) / (int)gridDim.x;
    int tile = blockIdx.x * per;
    const int tend = min(tile + per, a.ntiles);
    if (tile >= tend) return;

    auto fetch = [&](MxFetch& F, const GTile& tl) {
        F.cr = v.rcen[tl.r0]; F.hr = v.rhalf[tl.r0]; F.cc = v.ccen[tl.c0]; F.hc = v.chalf[tl.c0];
#pragma unroll
        for (int m = 0; m < 2; ++m) {
            const int64_t r = tl.r0 + min(2 * rg + m, tl.nr - 1);
            F.ar[m] = a.alpha[r];
            F.xr[m] = a.x[r];
#pragma unroll
            for (int n = 0; n < 4; ++n) {
                const int64_t c = tl.c0 + min(4 * cg + n, tl.nc - 1);
                const int64_t hi = r > c ? r : c, lo = r > c ? c : r;      // the lower triangle holds the matrix
                F.kv[m][n] = a.kinv[hi * a.ld + lo];
            }
        }
#pragma unroll
        for (int n = 0; n < 4; ++n) {
            const int64_t c = tl.c0 + min(4 * cg + n, tl.nc - 1);
            F.ac[n] = a.alpha[c];
            F.xc[n] = a.x[c];
        }
#pragma unroll
        for (int k = 0; k < 2; ++k)
            if (st_tb + 4 * k < T) stage_item_load<1>(F.it[k], st_which, st_tb + 4 * k, st_pnt, tl, 1, a.C, T, 0, v, a.x, a.ldx, a.x, a.ldx);
    };

    GTile tl = a.tiles[tile];
    GTile tl1 = a.tiles[min(tile + 1, tend - 1)];
    MxFetch F;
    fetch(F, tl);
    int buf = 0;
    double mom[TT][5];
#pragma unroll
    for (int t = 0; t < TT; ++t)
#pragma unroll
        for (int w = 0; w < 5; ++w) mom[t][w] = 0.0;
    while (true) {
        TileLds<1>& L = Lb[buf];
        const GTile cur = tl;
        const double* tab = a.table + (size_t)cur.pair * T * W;
        double* outp = a.partial + (size_t)tile * T * W;
        // ---- this tile out of the registers its requests landed in ----
        TileCtx<1> X;
        X.cr[0] = F.cr; X.hr[0] = F.hr; X.cc[0] = F.cc; X.hc[0] = F.hc;
#pragma unroll
        for (int k = 0; k < 2; ++k)
            if (st_tb + 4 * k < T) stage_item_compute<1, false>(L, F.it[k], X, tab, W, st_which, st_tb + 4 * k, st_pnt, 1, 0);
        double g[2][4], p[2], q[4];
#pragma unroll
        for (int n = 0; n < 4; ++n) q[n] = F.xc[n] - F.cc;
#pragma unroll
        for (int m = 0; m < 2; ++m) {
            p[m] = F.xr[m] - F.cr;
            const int lr = 2 * rg + m;
#pragma unroll
            for (int n = 0; n < 4; ++n) {
                const int lc = 4 * cg + n;
                double w = 0.0;
                if (lr < cur.nr && lc < cur.nc) {
                    w = 2.0;
                    if (cur.flags & GT_DIAG) w = lr > lc ? 2.0 : (lr == lc ? 1.0 : 0.0);
                }
                g[m][n] = w * 0.5 * (F.ar[m] * F.ac[n] - a.kinv_sign * F.kv[m][n]);
            }
        }
        // ---- the next tile's requests go out now, under this tile's arithmetic ----
        const int nxt = tile + 1;
        const bool more = nxt < tend;
        if (more) {
            tl = tl1;
            tl1 = a.tiles[min(nxt + 1, tend - 1)];
            fetch(F, tl);
        }
        const bool flush = !more || tl.pair != cur.pair;      // the run of this channel pair ends with this tile
        // LDS-only barrier: __syncthreads() would also wait for the requests just issued -- the whole point is that they stay in flight
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");      // the staged factors of this tile are in L
#pragma unroll
        for (int t = 0; t < TT; ++t) {
            if (t >= T) break;
            const int deg = __builtin_amdgcn_readfirstlane(L.deg[t]);
            if (deg == GT_SKIP) continue;
            const double V = L.V[t][0], sft = L.s[t][0];
            double cu[2], su[2], cw[4], sw[4];
#pragma unroll
            for (int m = 0; m < 2; ++m) { cu[m] = L.cu[t][2 * rg + m]; su[m] = L.su[t][2 * rg + m]; }
#pragma unroll
            for (int n = 0; n < 4; ++n) { cw[n] = L.cw[t][4 * cg + n]; sw[n] = L.sw[t][4 * cg + n]; }
            switch (deg) {
                #define GT_CASE(N) case N: mx_term<N>(mom[t], g, p, q, V, sft, cu, su, cw, sw); break;
                GT_DEGREE_CASES(GT_CASE)
#undef GT_CASE
                default: mx_term<0>(mom[t], g, p, q, V, sft, cu, su, cw, sw); break;
            }
        }
        if (!flush) {
            if (tid < T * 5) outp[tid] = 0.0;                 // this tile's moments ride on in registers: its slot adds nothing
        } else {
            // ---- one reduction per RUN through LDS, fixed order: thread (w, i) adds the values of threads 16 i .. 16 i + 15 of moment w, a
            // 5-step butterfly over i finishes (32 slices)
#pragma unroll
            for (int t = 0; t < TT; ++t) {
                if (t >= T) break;
#pragma unroll
                for (int w = 0; w < 5; ++w) { s_red[(t * 5 + w) * MXS + tid + (tid >> 4)] = mom[t][w]; mom[t][w] = 0.0; }
            }
            asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
            for (int e = tid; e < T * 5 * 32; e += 512) {
                const int w = e >> 5, i = e & 31;
                const double* src = s_red + w * MXS + i * 17;
                double x = 0.0;
#pragma unroll
                for (int k = 0; k < 16; ++k) x += src[k];
#pragma unroll
                for (int off = 16; off > 0; off >>= 1) x += __shfl_xor(x, off, 64);
                if (i == 0) outp[w] = x;                     // (a skipped term left zeros)
            }
            asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");      // s_red is read: the next run may write it
        }
        if (!more) break;
        tile = nxt;
        buf ^= 1;                                            // the other staging buffer: its last readers passed the barrier above
    }
}

// out[d][first + pnt] += sum over the `nminor` slots of block b (slot layout [block][minor][d][64]), in slot order: four interleaved partial
// sums per point, combined as (s0 + s1) + (s2 + s3).  Slots no tile wrote are zero (the scratch is cleared per launch).
__global__ __launch_bounds__(256) void k_gz_reduce(const double* __restrict__ gzp, int nminor, int D, const int* __restrict__ blk,
                                                   double* __restrict__ out, int64_t ld) {
    const int b = blockIdx.x, pnt = threadIdx.x & 63, part = threadIdx.x >> 6;
    const int first = blk[2 * b], n = blk[2 * b + 1];
    __shared__ double red[4][MOGP_GT], redc[4][MOGP_GT];
    const double* base = gzp + (size_t)b * nminor * D * MOGP_GT;
    // The slots of one inducing point cancel to a small fraction of their size (at configs[4] the derivative with respect to an inducing input
    // is O(1e-2), the residue of sums many orders larger), so the long sums here are compensated (Neumaier): the result is the correctly
    // rounded sum of the slots to within a few ulp of the RESULT, whatever the number of slots.
    for (int d = 0; d < D; ++d) {
        double s = 0.0, c = 0.0;
        for (int k = part; k < nminor; k += 4) {
            const double x = base[((size_t)k * D + d) * MOGP_GT + pnt];
            const double t = s + x;
            c += fabs(s) >= fabs(x) ? (s - t) + x : (x - t) + s;
            s = t;
        }
        __syncthreads();
        red[part][pnt] = s; redc[part][pnt] = c;
        __syncthreads();
        if (part == 0 && pnt < n) {
            double hs = 0.0, hc = 0.0;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const double x = red[q][pnt];
                const double t = hs + x;
                hc += fabs(hs) >= fabs(x) ? (hs - t) + x : (x - t) + hs;
                hs = t;
                hc += redc[q][pnt];
            }
            out[(size_t)d * ld + first + pnt] += hs + hc;
        }
    }
}

template <bool DENSE, bool ZG, bool ENV>
static int launch_moments_t(const MomentArgs& a, hipStream_t s) {
    switch (a.D) {
        case 1: hipLaunchKernelGGL((k_moments<1, DENSE, ZG, ENV>), dim3(a.ntiles), dim3(256), 0, s, a); break;
        case 2: hipLaunchKernelGGL((k_moments<2, DENSE, ZG, ENV>), dim3(a.ntiles), dim3(256), 0, s, a); break;
        case 3: hipLaunchKernelGGL((k_moments<3, DENSE, ZG, ENV>), dim3(a.ntiles), dim3(256), 0, s, a); break;
        default: hipLaunchKernelGGL((k_moments<0, DENSE, ZG, ENV>), dim3(a.ntiles), dim3(256), 0, s, a); break;
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

// the radial instantiations: GATE by `rows` (mogp_internal.h: launch_gram), D = 1, 2, 3 or generic; DENSE: the adjoint comes from a.G
template <bool DENSE>
static void launch_moments_radial(const MomentArgs& a, hipStream_t s, int rows) {
    if (rows == 1) {
        hipLaunchKernelGGL((k_moments<1, DENSE, false, false, true, 1>), dim3(a.ntiles), dim3(256), 0, s, a);
    } else if (rows > 1) {
        switch (a.D) {
            case 1: hipLaunchKernelGGL((k_moments<1, DENSE, false, false, true, 2>), dim3(a.ntiles), dim3(256), 0, s, a); break;
            case 2: hipLaunchKernelGGL((k_moments<2, DENSE, false, false, true, 2>), dim3(a.ntiles), dim3(256), 0, s, a); break;
            case 3: hipLaunchKernelGGL((k_moments<3, DENSE, false, false, true, 2>), dim3(a.ntiles), dim3(256), 0, s, a); break;
            default: hipLaunchKernelGGL((k_moments<0, DENSE, false, false, true, 2>), dim3(a.ntiles), dim3(256), 0, s, a); break;
        }
    } else {
        switch (a.D) {
            case 1: hipLaunchKernelGGL((k_moments<1, DENSE, false, false, true>), dim3(a.ntiles), dim3(256), 0, s, a); break;
            case 2: hipLaunchKernelGGL((k_moments<2, DENSE, false, false, true>), dim3(a.ntiles), dim3(256), 0, s, a); break;
            case 3: hipLaunchKernelGGL((k_moments<3, DENSE, false, false, true>), dim3(a.ntiles), dim3(256), 0, s, a); break;
            default: hipLaunchKernelGGL((k_moments<0, DENSE, false, false, true>), dim3(a.ntiles), dim3(256), 0, s, a); break;
        }
    }
}

int launch_moments(int ncu, const MomentArgs& a0, hipStream_t s, int rows) {
    if (a0.ntiles <= 0) return 0;
    MomentArgs a = a0;
    if (a.W <= 0) a.W = 2 + 3 * a.D;
    const bool env = a.W > 2 + 3 * a.D;
    const double* xc = a.xc ? a.xc : a.x;
    const int64_t ldxc = a.xc ? a.ldxc : a.ldx;
    int rc = a.phases_ready ? 0 : launch_phase_tables(a.ph, a.x, a.ldx, a.nrows, xc, ldxc, a.xc ? a.ncols : a.nrows, a.table, a.T, a.D, a.C, a.W, s);
    if (rc) return rc;
    if (a.kind) {                                            // radial profiles: every tile through the radial form of the staged kernel
        if (!a.shape) { set_error("launch_moments: kinds without shapes"); return -1; }
        // (a dense adjoint: the symmetric lower-tile form alone -- no rank-one rider, no input gradients, square)
        if (env || (a.G != nullptr && (!a.sym || a.ru || a.gzr || a.gzc || a.xc))) { set_error("launch_moments: radial profiles take the exact mode or a dense symmetric adjoint, without an envelope"); return -1; }
        if (a.ev0) HIP_TRY(hipEventRecord(a.ev0, s));
        if (rows == 1 && a.D != 1) { set_error("launch_moments: gate rows take one input dimension"); return -1; }
        if (a.G != nullptr) launch_moments_radial<true>(a, s, rows); else launch_moments_radial<false>(a, s, rows);
        HIP_TRY(hipGetLastError());
        if (a.ev1) HIP_TRY(hipEventRecord(a.ev1, s));
        return 0;
    }
    if (a.G == nullptr) {
        if (a.ev0) HIP_TRY(hipEventRecord(a.ev0, s));
        // D = 1 without an envelope, every row this rank's own: the persistent pipelined kernel
        if (!env && a.D == 1 && a.W == 5 && a.T <= 4 && a.row_mod <= 1 && a.xc == nullptr) {
            // (the reduction staging of eight terms does not fit in LDS; three terms -- every BASELINE config of the exact model -- get an instantiation of their
            // own: the moments now live in registers across tiles, and five fewer accumulators keep the kernel clear of spills)
            if (a.T <= 3) hipLaunchKernelGGL(k_moments_x<3>, dim3(std::min(a.ntiles, ncu)), dim3(512), 0, s, a);
            else hipLaunchKernelGGL(k_moments_x<4>, dim3(std::min(a.ntiles, ncu)), dim3(512), 0, s, a);
            HIP_TRY(hipGetLastError());
            rc = 0;
        } else
        rc = env ? launch_moments_t<false, false, true>(a, s) : launch_moments_t<false, false, false>(a, s);
        if (!rc && a.ev1) HIP_TRY(hipEventRecord(a.ev1, s));
        return rc;
    }
    if (a.gzr || a.gzc) {
        if (!a.gzp || !a.rblk || !a.cblk || a.nrb <= 0 || a.ncb <= 0) { set_error("launch_moments: the input-gradient pass needs its scratch and block tables"); return -1; }
        const size_t half = (size_t)a.nrb * a.ncb * a.D * MOGP_GT;
        HIP_TRY(hipMemsetAsync(a.gzp, 0, 2 * half * sizeof(double), s));
        if ((rc = env ? launch_moments_t<true, true, true>(a, s) : launch_moments_t<true, true, false>(a, s))) return rc;
        if (a.gzr) hipLaunchKernelGGL(k_gz_reduce, dim3(a.nrb), dim3(256), 0, s, a.gzp, a.ncb, a.D, a.rblk, a.gzr, a.ldgz);
        if (a.gzc) hipLaunchKernelGGL(k_gz_reduce, dim3(a.ncb), dim3(256), 0, s, a.gzp + half, a.nrb, a.D, a.cblk, a.gzc, a.ldgz);
        HIP_TRY(hipGetLastError());
        return 0;
    }
    return env ? launch_moments_t<true, false, true>(a, s) : launch_moments_t<true, false, false>(a, s);
}

// one workgroup per (lower channel pair, moment entry): 256 threads stride over that pair's tiles, then a fixed-shape
// LDS tree -- the summation order depends only on the tile list, so results are bit-reproducible.
// On a diagonal channel block (i == j) the moments that are odd in tau (m4 = sum g E sin, m2_d = sum g u_d E cos)
// cancel between (a, b) and (b, a) in the full symmetric sum; the lower-triangle pass cannot see that, so they are
// set to their exact value, zero, here.
__global__ __launch_bounds__(256) void k_moment_reduce(const double* __restrict__ partial, const int* __restrict__ pair_start,
                                                       int TW, int W, int D, int lower_pairs, double* __restrict__ out) {
    const int p = blockIdx.x, tw = blockIdx.y;
    const int b = pair_start[p], e = pair_start[p + 1];
    __shared__ double red[256];
    double s = 0.0;
    for (int t = b + threadIdx.x; t < e; t += 256) s += partial[(size_t)t * TW + tw];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        int i = (int)((sqrt(8.0 * (double)p + 1.0) - 1.0) * 0.5);
        while ((i + 1) * (i + 2) / 2 <= p) ++i;
        while (i * (i + 1) / 2 > p) --i;
        const bool diag = lower_pairs && (p - i * (i + 1) / 2) == i;
        const int w = tw % W;
        double v = red[0];
        if (diag && (w == 1 || (w >= 2 + D && w < 2 + 2 * D))) v = 0.0;
        out[(size_t)p * TW + tw] = v;
    }
}

int launch_moment_reduce(const double* partial, const int* pair_start, int npairs, int T, int W, int D, double* out, hipStream_t s, int lower_pairs) {
    hipLaunchKernelGGL(k_moment_reduce, dim3(npairs, T * W), dim3(256), 0, s, partial, pair_start, T * W, W, D, lower_pairs, out);
    HIP_TRY(hipGetLastError());
    return 0;
}

// out[c] = sum_{k in channel c} 1/2 (alpha_k^2 - kinv_kk); one workgroup per channel
__global__ void k_diagG(const double* __restrict__ kinv, int64_t ld, const double* __restrict__ alpha,
                        const int* __restrict__ chan_off, double* __restrict__ out, double kinv_sign, int row_mod, int row_rem) {
    const int c = blockIdx.x;
    __shared__ double red[256];
    double s = 0.0;
    for (int64_t k = chan_off[c] + threadIdx.x; k < chan_off[c + 1]; k += 256)
        if (row_mod <= 1 || (int)((k / MOGP_TILE) % row_mod) == row_rem) s += 0.5 * (alpha[k] * alpha[k] - kinv_sign * kinv[k * ld + k]);
    red[threadIdx.x] = s;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[c] = red[0];
}

int launch_diagG(const double* kinv, int64_t ld, const double* alpha, const int* chan_off, int C, double* out, hipStream_t s,
                 double kinv_sign, int row_mod, int row_rem) {
    hipLaunchKernelGGL(k_diagG, dim3(C), dim3(256), 0, s, kinv, ld, alpha, chan_off, out, kinv_sign, row_mod, row_rem);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // namespace mogp
