// sparse.hip -- the inducing-point scaffold shared by the Titsias bound (titsias.hip), the Snelson model (snelson.hip) and the Hensman models
// (svgp.hip): workspace, tile lists, K_uu up to its factorisation, K_uf, the small linear-algebra idioms the three bounds have in common
// (refined explicit inverse, adjoint of K_uu, a vector riding through a panel solve, vector + scalars through one all-reduce), the two moment
// passes, and the prediction panels.  What differs between the models is a parameter here; which kernel runs on which stream in which order
// is the caller's.  oa.hip shares the column-scaling kernel only.
#include "mogp_model.h"

#include <cmath>
#include <cstdlib>
#include <cstring>
#include <limits>

using namespace mogp;

#define RC(x) do { int r__ = (x); if (r__) return r__; } while (0)

namespace {

// out[m][n] = in[m][n] * s[n]
__global__ void k_scale_cols(const double* __restrict__ in, double* __restrict__ out, int64_t ld, int64_t n, const double* __restrict__ s) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const int64_t r = blockIdx.y;
    out[r * ld + j] = in[r * ld + j] * s[j];
}

}  // namespace

namespace mogp {

int launch_scale_cols(const double* in, double* out, int64_t ld, int64_t rows, int64_t n, const double* s, hipStream_t st) {
    hipLaunchKernelGGL(k_scale_cols, dim3((unsigned)((n + 255) / 256), (unsigned)rows), dim3(256), 0, st, in, out, ld, n, s);
    HIP_TRY(hipGetLastError());
    return 0;
}

int side_fork(mogp_model* m, TitsiasWork& t, hipStream_t* side) {
    static const bool on = !(std::getenv("MOGP_SIDE_STREAM") && std::atoi(std::getenv("MOGP_SIDE_STREAM")) == 0);
    *side = m->st;
    if (!on || !m->st3) return 0;
    for (auto& e : t.side_ev) if (!e) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    HIP_TRY(hipEventRecord(t.side_ev[0], m->st));
    HIP_TRY(hipStreamWaitEvent(m->st3, t.side_ev[0], 0));
    *side = m->st3;
    return 0;
}

int side_join(mogp_model* m, TitsiasWork& t, hipStream_t side) {
    if (side == m->st) return 0;
    HIP_TRY(hipEventRecord(t.side_ev[1], side));
    HIP_TRY(hipStreamWaitEvent(m->st, t.side_ev[1], 0));
    return 0;
}

// defer_check: the caller reads the pivot word itself at its next synchronisation (a failed factorisation then runs on with garbage: bounded, harmless)
int spd_invert(mogp_model* m, Spd& w, const char* which, int64_t* info, const double** W, bool defer_check) {
    RC(spd_potrf(m, w));
    if (!defer_check) RC(spd_check_info(m, which, info));
    RC(spd_trtri(m, w));                                                        // w.A = L^-1
    RC(spd_lauum(m, w));                                                        // w.B = inverse (lower)
    *W = w.A.p;
    return 0;
}

int gz_prepare(mogp_model* m, TitsiasWork& t, const std::vector<int>& offz, int D) {
    std::vector<int> hz, hx;
    tile_blocks(offz, m->C, hz);
    tile_blocks(m->sx.off, m->C, hx);
    if (hz != t.hblk_z) {
        RC(t.blk_z.ensure(hz.size()));
        t.hblk_z = hz;
        HIP_TRY(hipMemcpyAsync(t.blk_z.p, t.hblk_z.data(), hz.size() * sizeof(int), hipMemcpyHostToDevice, m->st));
    }
    if (hx != t.hblk_x) {
        RC(t.blk_x.ensure(hx.size()));
        t.hblk_x = hx;
        HIP_TRY(hipMemcpyAsync(t.blk_x.p, t.hblk_x.data(), hx.size() * sizeof(int), hipMemcpyHostToDevice, m->st));
    }
    const int nbz = (int)hz.size() / 2, nbx = (int)hx.size() / 2;
    return t.gzp.ensure(gz_scratch_doubles(nbz, std::max(nbz, nbx), D));
}

void gz_attach(const TitsiasWork& t, MomentArgs& ma, bool zx) {
    ma.gzp = t.gzp.p;
    ma.nrb = (int)t.hblk_z.size() / 2; ma.rblk = t.blk_z.p;
    ma.ncb = zx ? (int)t.hblk_x.size() / 2 : ma.nrb; ma.cblk = zx ? t.blk_x.p : t.blk_z.p;
}

int spd_check_info(mogp_model* m, const char* which, int64_t* info) {
    unsigned long long hinfo = 0;
    HIP_TRY(hipMemcpyAsync(&hinfo, m->d_info.p, sizeof(hinfo), hipMemcpyDeviceToHost, m->st));
    HIP_TRY(hipStreamSynchronize(m->st));
    return spd_info_verdict(m, which, hinfo, info);
}

int spd_info_verdict(mogp_model* m, const char* which, unsigned long long hinfo, int64_t* info) {
    if (hinfo == MOGP_INFO_CHAIN_TIMEOUT) {
        m->no_chain = true;                                  // gates the chain kernel AND the stream-K launches (mogp_api.hip:stream_k_setup)
        return fail(MOGP_EHIP, "a hand-off between workgroups timed out (chain kernel, chain.hip, or a stream-K GEMM, linalg.hip:k_gemm_sk: the GPU is "
                               "shared with another process?).  The model has switched both forms off (the chain kernel as MOGP_CHAIN=0 does): repeat the call");
    }
    if (hinfo != std::numeric_limits<unsigned long long>::max()) {
        if (info) *info = (int64_t)hinfo;
        return fail(MOGP_ENOTPD, std::string("linalg.cholesky: ") + which + " is not positive-definite (the leading minor of order " +
                                 std::to_string(hinfo) + " is not positive-definite).");
    }
    return 0;
}

int sparse_timeout_check(mogp_model* m) {
    unsigned long long hinfo = 1;
    HIP_TRY(hipMemcpy(&hinfo, m->d_info.p, sizeof(hinfo), hipMemcpyDeviceToHost));     // the caller has just synchronised the stream
    if (hinfo != MOGP_INFO_CHAIN_TIMEOUT) return 0;
    m->no_chain = true;
    return fail(MOGP_EHIP, "a hand-off between workgroups timed out during this evaluation (stream-K GEMM of a triangular solve, linalg.hip:k_gemm_sk, "
                           "or the chain kernel: the GPU is shared with another process?): its result is not valid.  The model has switched both forms "
                           "off (the chain kernel as MOGP_CHAIN=0 does): repeat the call");
}

// mt (mt + 1) / 2 = 136 tiles at configs[4] would leave half the chip idle over K = N: K is cut into ks slices, each slice into a block of
// its own, and the blocks are summed.  ks minimises rounds(tiles ks / 512 slots) / ks: 136 tiles -> ks = 15, 2040 workgroups = four
// full rounds (two slices left every second CU with two workgroups and the rest with one: 12.5 ms; fifteen: see DESIGN 4b)
int mm_lower_splitk(mogp_model* m, TitsiasWork& t, const double* A, const double* B, double* out, int mt, int64_t Mpad, int64_t ldk, int64_t K,
                    double alpha) {
    GemmArgs g = make_gemm(A, ldk, 0, B, ldk, 0, out, Mpad, alpha, GM_LOWER, mt, mt, K);
    const int tiles_q = mt * (mt + 1) / 2;
    int ks = 1;
    if (tiles_q < 512 && K >= 4096) {
        double best = 1e30;
        for (int c = 1; c <= 16; ++c) {
            if (K / c < 2048) break;
            const double cost = std::ceil((double)tiles_q * c / 512.0) / c;
            if (cost < best - 1e-12) { best = cost; ks = c; }
        }
        // (round 4: eight or sixteen slices, each on ONE XCD -- k_gemm: ksplit_xcd, the workgroups that share an L2 then share a k window as well --
        // measured no faster than fifteen slice-major ones, 45.4 vs 45.3 ms at configs[4], although those fetch 12.4 GB for 1.6 GB of v: the product is
        // not bound by that traffic; no caller sets GemmArgs::ksplit_xcd any more)
    }
    if (ks > 1) {
        if (t.kslices.n < (size_t)ks * Mpad * Mpad) {         // the upper tiles are never written: keep them finite
            RC(t.kslices.ensure((size_t)ks * Mpad * Mpad));
            HIP_TRY(hipMemsetAsync(t.kslices.p, 0, (size_t)ks * Mpad * Mpad * sizeof(double), m->st));
        }
        g.C = t.kslices.p; g.ksplit = ks; g.c_split = (int64_t)Mpad * Mpad;
    }
    RC(gemm_call(m, g, gemm_flops(g, nullptr)));
    if (ks > 1) RC(launch_sum_slices(t.kslices.p, (int64_t)Mpad * Mpad, ks, out, m->st));
    return 0;
}

int sparse_workspace(mogp_model* m, TitsiasWork& t, int64_t Mpad, int64_t M) {
    const int C = m->C, D = m->D;
    const int64_t Npad = m->Npad;
    if (t.Mpad != Mpad) {
        t.Mpad = Mpad;
        RC(spd_alloc(t.a, Mpad)); RC(spd_alloc(t.q, Mpad));
        RC(t.zx.ensure((size_t)D * Mpad));
        RC(t.B.ensure((size_t)Mpad * Npad)); RC(t.v.ensure((size_t)Mpad * Npad));
        RC(t.Qs.ensure((size_t)Mpad * Mpad));
        RC(t.vec.ensure((size_t)8 * Mpad + 4 * Npad));
        RC(t.scratch.ensure((size_t)(Mpad / 256 + 2) * std::max(Npad, Mpad) + (size_t)(Mpad / 512 + 2) * Mpad));
        RC(t.zero_noise.ensure(C));
        RC(dev_fill_zero(t.zero_noise.p, C * sizeof(double)));
        RC(dev_fill_zero(t.B.p, (size_t)Mpad * Npad * sizeof(double)));      // padding of Kuf stays zero: the Gram kernel never writes it
        RC(dev_fill_zero(t.v.p, (size_t)Mpad * Npad * sizeof(double)));      // ... nor that of its working copy (the solves keep zeros zero)
        t.Mrows = 0;
    }
    // A smaller inducing set under the same Mpad (256 points, then 192): rows M .. Mrows - 1 of both panels still hold the larger set's K_uf and
    // v.  Snelson and the Hensman models clear B themselves; Titsias writes both panels with one Gram kernel and relies on the padding here --
    // without this its v v^T took 64 rows of the previous set along (tests/test_sparse_sweep_gpu.py: one handle, several inducing sets)
    if (M < t.Mrows) {
        HIP_TRY(hipMemsetAsync(t.B.p + (size_t)M * Npad, 0, (size_t)(t.Mrows - M) * Npad * sizeof(double), m->st));
        HIP_TRY(hipMemsetAsync(t.v.p + (size_t)M * Npad, 0, (size_t)(t.Mrows - M) * Npad * sizeof(double), m->st));
    }
    t.Mrows = M;
    return 0;
}

// the tile lists depend on the channel offsets of Z and X only: built and uploaded when those change, not per evaluation (50 000 tiles and 1.2 MB
// of pageable copies at configs[4], all of it in front of the evaluation's first kernel); the (Z, X) list also as strip-kernel runs.
// want_uf false (the dense Hensman model, a Hensman prediction): lists over (Z, Z) alone will do -- but lists that hold (Z, X) as well serve too
int sparse_tiles(mogp_model* m, TitsiasWork& t, const SortedX& sz, bool want_uf) {
    std::vector<int> key(sz.off);
    key.insert(key.end(), m->sx.off.begin(), m->sx.off.end());
    const int ncu = plan_cus(m->ctx);
    key.push_back(ncu);                                         // the CU count the strip runs of (Z, X) are cut for (mogp_ctx_plan_cus may change it)
    key.push_back(1);                                           // last entry: the (Z, X) lists are there
    if (key == t.tile_key) return 0;
    if (!want_uf) { key.back() = 0; if (key == t.tile_key) return 0; }
    t.tile_key.clear();
    std::vector<GTile> tuu, tuf;
    std::vector<int> psuu, psuf;
    build_sym_tiles(sz.off, m->C, tuu, psuu);
    if (want_uf) build_rect_tiles(sz.off, m->sx.off, m->C, tuf, &psuf);
    HIP_TRY(hipStreamSynchronize(m->st));                   // a previous evaluation's kernels may still read the lists (first call / a new Z layout only)
    RC(t.tiles_uu.ensure(tuu.size())); RC(t.ps_uu.ensure(psuu.size()));
    HIP_TRY(dev_upload(t.tiles_uu.p, tuu.data(), tuu.size() * sizeof(GTile)));
    HIP_TRY(dev_upload(t.ps_uu.p, psuu.data(), psuu.size() * sizeof(int)));
    if (want_uf) {
        RC(t.tiles_uf.ensure(tuf.size())); RC(t.ps_uf.ensure(psuf.size()));
        HIP_TRY(dev_upload(t.tiles_uf.p, tuf.data(), tuf.size() * sizeof(GTile)));
        HIP_TRY(dev_upload(t.ps_uf.p, psuf.data(), psuf.size() * sizeof(int)));
        RC(t.strip_uf.build(tuf, ncu));
    }
    t.n_tuu = tuu.size(); t.n_tuf = tuf.size();
    t.tile_key = key;
    return 0;
}

int sparse_kuu(mogp_model* m, int64_t M, const double* Z, double jitter, bool want_uf, SortedX& sz, double* jit, const char* need_grouped) {
    const int C = m->C, D = m->D, W = m->Wt;                   // 2 + 3 D, or 2 + 5 D: terms with an envelope on the input midpoint (MOHSM)
    if (m->T <= 0) return fail(MOGP_EINVAL, "mogp_model_set_terms must be called before an evaluation");
    RC(sort_inputs(Z, M, D, C, MOGP_TILE, sz));
    if (need_grouped && !sz.identity) return fail(MOGP_EINVAL, need_grouped);
    const int64_t Mpad = sz.Mpad;
    if (!m->tw) m->tw = new TitsiasWork();
    TitsiasWork& t = *m->tw;
    RC(sparse_workspace(m, t, Mpad, M));
    m->gemm_ev_used = 0; m->gemm_launches = 0; m->gemm_flops = 0.0;
    HIP_TRY(hipMemcpyAsync(t.zx.p, sz.xs.data(), (size_t)D * Mpad * sizeof(double), hipMemcpyHostToDevice, m->st));
    RC(sparse_tiles(m, t, sz, want_uf));
    const unsigned long long big = std::numeric_limits<unsigned long long>::max();
    HIP_TRY(hipMemcpyAsync(m->d_info.p, &big, sizeof(big), hipMemcpyHostToDevice, m->st));

    // relative jitter on Kuu (reference gpr/model.py:710 -> :244, :524, :855)
    *jit = jitter * table_diag_points(m, sz) / (double)M;      // with an envelope the diagonal of Kuu follows the inducing inputs

    GramArgs ga{};
    ga.tiles = t.tiles_uu.p; ga.xr = t.zx.p; ga.xc = t.zx.p; ga.ldxr = ga.ldxc = Mpad; ga.nrows = ga.ncols = M;
    RC(t.ph_zz.prepare(sz.off, sz.off, C, m->T, Mpad, Mpad, m->st, ga.ph));
    ga.table = m->d_table.p; ga.T = m->T; ga.D = D; ga.C = C; ga.W = W; ga.out = t.a.A.p; ga.ldo = Mpad;
    ga.noise = t.zero_noise.p; ga.dvar = nullptr; ga.jitter_abs = *jit; ga.mirror = 0;
    RC(launch_gram(plan_cus(m->ctx), ga, (int)t.n_tuu, m->st));
    RC(launch_pad_identity(t.a.A.p, Mpad, M, Mpad, m->st));
    t.a.keep_L = true;                                                          // the solves need L itself, diagonal tiles included
    t.a.refine_panels = true;                                                   // K_uu + jitter is ill-conditioned: mogp_api.hip:spd_potrf
    return 0;
}

int sparse_kuf(mogp_model* m, TitsiasWork& t, const SortedX& sz, hipStream_t stream, bool use_strips, double* out2) {
    const int64_t Mpad = t.Mpad, Npad = m->Npad;
    GramArgs ga{};
    ga.tiles = t.tiles_uf.p; ga.xr = t.zx.p; ga.ldxr = Mpad; ga.xc = m->d_x.p; ga.ldxc = Npad; ga.nrows = sz.M; ga.ncols = m->N;
    RC(t.ph_zx.prepare(sz.off, m->sx.off, m->C, m->T, Mpad, Npad, stream, ga.ph));
    ga.table = m->d_table.p; ga.T = m->T; ga.D = m->D; ga.C = m->C; ga.W = m->Wt; ga.out = t.B.p; ga.ldo = Npad; ga.mirror = 0;
    ga.out2 = out2;
    if (use_strips) t.strip_uf.attach(ga);                                      // full interior tiles in runs of four on the strip kernel
    return launch_gram(plan_cus(m->ctx), ga, (int)t.n_tuf, stream);
}

// out = P rhs with P = Q^-1 formed explicitly, plus ONE step of iterative refinement against Q (Titsias: t1 = Pq (v y) against Qs; Snelson:
// r = Pq (v G y) against Bq).  Of the three places Pq enters the gradient, this vector is the one where the explicitly formed inverse costs
// accuracy on dELBO/dZ (tools/titsias_numerics.py: 1.3e-4 -> 7e-5, the same as two triangular solves with Lq), and three M x M mat-vecs are
// far cheaper than 2 nb dependent launches of a vector solve
int refined_apply(mogp_model* m, TitsiasWork& t, const double* P, const double* Q, const double* rhs, double* out) {
    const int64_t Mpad = t.Mpad;
    double* tmp = t.vec.p + 5 * Mpad;
    double* res = t.vec.p + 6 * Mpad;
    RC(launch_gemv_rows(P, Mpad, Mpad, Mpad, rhs, out, m->st));
    RC(launch_gemv_rows(Q, Mpad, Mpad, Mpad, out, tmp, m->st));
    RC(launch_axpby(Mpad, 1.0, rhs, -1.0, tmp, res, m->st));
    RC(launch_gemv_rows(P, Mpad, Mpad, Mpad, res, tmp, m->st));
    RC(launch_axpby(Mpad, 1.0, out, 1.0, tmp, out, m->st));
    return 0;
}

int allreduce_vec_scalars(mogp_model* m, TitsiasWork& t, double* vec, int64_t n, double* hs, int k) {
    RC(t.red.ensure((size_t)n + k));
    if (n) HIP_TRY(hipMemcpyAsync(t.red.p, vec, n * sizeof(double), hipMemcpyDeviceToDevice, m->st));
    HIP_TRY(hipMemcpyAsync(t.red.p + n, hs, k * sizeof(double), hipMemcpyHostToDevice, m->st));
    HIP_TRY(hipStreamSynchronize(m->st));                                   // hs may be a stack buffer
    RC(comm_allreduce(m->ctx, t.red.p, n + k, m->st));
    if (n) HIP_TRY(hipMemcpyAsync(vec, t.red.p, n * sizeof(double), hipMemcpyDeviceToDevice, m->st));
    HIP_TRY(hipMemcpyAsync(hs, t.red.p + n, k * sizeof(double), hipMemcpyDeviceToHost, m->st));
    HIP_TRY(hipStreamSynchronize(m->st));
    return 0;
}

int adjoint_GA(mogp_model* m, TitsiasWork& t, double scale, hipStream_t stream) {
    const int64_t Mpad = t.Mpad;
    const int mt = (int)(Mpad / MOGP_TILE);
    RC(trsm_lower(m, t.a.A.p, Mpad, mt, t.E.p, Mpad, Mpad, true, stream));
    RC(launch_transpose(t.GA.p, t.E.p, Mpad, Mpad, stream));
    RC(trsm_lower(m, t.a.A.p, Mpad, mt, t.GA.p, Mpad, Mpad, true, stream));
    RC(launch_sym_lower_avg(t.GA.p, Mpad, Mpad, scale, stream));
    RC(launch_get_diag(t.GA.p, Mpad, Mpad, t.vec.p + 2 * Mpad, stream));
    return 0;
}

int solve_with_rider(mogp_model* m, TitsiasWork& t, double* panel, const double* r, double* beta) {
    const int64_t Mpad = t.Mpad, N = m->N, Npad = m->Npad;
    const int mt = (int)(Mpad / MOGP_TILE);
    const bool ride = panel && Npad > N;
    if (ride) RC(launch_copy2d(panel + N, Npad, r, 1, Mpad, 1, 1.0, m->st));
    if (panel) RC(trsm_lower(m, t.a.A.p, Mpad, mt, panel, Npad, Npad, true));
    if (ride) {
        if (t.zero_col.n < (size_t)Mpad) { RC(t.zero_col.ensure(Mpad)); HIP_TRY(hipMemsetAsync(t.zero_col.p, 0, Mpad * sizeof(double), m->st)); }
        RC(launch_copy2d(beta, 1, panel + N, Npad, Mpad, 1, 1.0, m->st));
        RC(launch_copy2d(panel + N, Npad, t.zero_col.p, 1, Mpad, 1, 1.0, m->st));          // the padding column is zero again
    } else {
        RC(t.Hm.ensure((size_t)Mpad * MOGP_TILE));
        HIP_TRY(hipMemsetAsync(t.Hm.p, 0, (size_t)Mpad * MOGP_TILE * sizeof(double), m->st));
        RC(launch_copy2d(t.Hm.p, MOGP_TILE, r, 1, Mpad, 1, 1.0, m->st));
        RC(trsm_lower(m, t.a.A.p, Mpad, mt, t.Hm.p, MOGP_TILE, MOGP_TILE, true));
        RC(launch_copy2d(beta, 1, t.Hm.p, MOGP_TILE, Mpad, 1, 1.0, m->st));
    }
    return 0;
}

int sparse_moments(mogp_model* m, TitsiasWork& t, const SortedX& sz, const MomentSpec* uf, const MomentSpec& uu, bool sharded, hipStream_t side) {
    const int C = m->C, D = m->D, W = m->Wt, T = m->T, P = C * (C + 1) / 2;
    const int64_t Mpad = t.Mpad, Npad = m->Npad;
    RC(t.partial_uu.ensure(t.n_tuu * (size_t)T * W)); RC(t.mom_uu.ensure((size_t)P * T * W));
    RC(t.mom_uf.ensure((size_t)C * C * T * W));
    RC(t.gz.ensure((size_t)D * Mpad));
    HIP_TRY(hipMemsetAsync(t.gz.p, 0, (size_t)D * Mpad * sizeof(double), m->st));
    RC(gz_prepare(m, t, sz.off, D));

    MomentArgs ma{};
    ma.x = t.zx.p; ma.ldx = Mpad; ma.nrows = sz.M;
    ma.table = m->d_table.p; ma.T = T; ma.D = D; ma.C = C; ma.W = W; ma.ldgz = Mpad;
    if (uf) {
        RC(t.partial_uf.ensure(t.n_tuf * (size_t)T * W));
        ma.tiles = t.tiles_uf.p; ma.ntiles = (int)t.n_tuf; ma.xc = m->d_x.p; ma.ldxc = Npad; ma.ncols = m->N;
        RC(t.ph_zx.prepare(sz.off, m->sx.off, C, T, Mpad, Npad, m->st, ma.ph));
        ma.G = uf->G; ma.ldg = uf->ldg; ma.ru = uf->ru; ma.rw = uf->rw; ma.rcoef = uf->rcoef; ma.sym = 0;
        ma.gzr = uf->dz ? t.gz.p : nullptr; ma.gzc = nullptr; ma.partial = t.partial_uf.p;
        gz_attach(t, ma, true);
        RC(launch_moments(plan_cus(m->ctx), ma, m->st));
        RC(launch_moment_reduce(t.partial_uf.p, t.ps_uf.p, C * C, T, W, D, t.mom_uf.p, m->st, 0));
        if (sharded) {                       // the (Z, X) moments and their share of d/dZ are sums over data points; the (Z, Z) pass below is not
            RC(comm_allreduce(m->ctx, t.mom_uf.p, (int64_t)C * C * T * W, m->st));
            RC(comm_allreduce(m->ctx, t.gz.p, (int64_t)D * Mpad, m->st));
        }
    } else {
        HIP_TRY(hipMemsetAsync(t.mom_uf.p, 0, (size_t)C * C * T * W * sizeof(double), m->st));
    }
    RC(side_join(m, t, side));
    ma.tiles = t.tiles_uu.p; ma.ntiles = (int)t.n_tuu; ma.xc = nullptr; ma.ldxc = 0; ma.ncols = sz.M;
    RC(t.ph_zz.prepare(sz.off, sz.off, C, T, Mpad, Mpad, m->st, ma.ph));
    ma.G = uu.G; ma.ldg = uu.ldg; ma.ru = uu.ru; ma.rw = uu.rw; ma.rcoef = uu.rcoef; ma.sym = 1;
    ma.gzr = ma.gzc = uu.dz ? t.gz.p : nullptr; ma.partial = t.partial_uu.p;
    gz_attach(t, ma, false);
    RC(launch_moments(plan_cus(m->ctx), ma, m->st));
    RC(launch_moment_reduce(t.partial_uu.p, t.ps_uu.p, P, T, W, D, t.mom_uu.p, m->st, 1));
    return 0;
}

int sparse_predict_panels(mogp_model* m, TitsiasWork& t, const SortedX& sz, int64_t S, const double* Xs, SortedX& ss) {
    t.pred_valid = false;                                   // t.Aus / t.Bus are about to be overwritten
    const int C = m->C, D = m->D;
    const int64_t Mpad = t.Mpad;
    RC(sort_inputs(Xs, S, D, C, MOGP_TILE, ss));
    const int64_t Spad = ss.Mpad;
    std::vector<GTile> tus;
    build_rect_tiles(sz.off, ss.off, C, tus);
    RC(t.Kus.ensure((size_t)Mpad * Spad)); RC(t.Aus.ensure((size_t)Mpad * Spad)); RC(t.Bus.ensure((size_t)Mpad * Spad));
    RC(m->d_xs.ensure((size_t)D * Spad)); RC(m->d_ptiles.ensure(tus.size()));
    HIP_TRY(hipMemcpyAsync(m->d_xs.p, ss.xs.data(), (size_t)D * Spad * sizeof(double), hipMemcpyHostToDevice, m->st));
    HIP_TRY(hipMemcpyAsync(m->d_ptiles.p, tus.data(), tus.size() * sizeof(GTile), hipMemcpyHostToDevice, m->st));
    HIP_TRY(hipMemsetAsync(t.Kus.p, 0, (size_t)Mpad * Spad * sizeof(double), m->st));
    GramArgs ga{};
    ga.tiles = m->d_ptiles.p; ga.xr = t.zx.p; ga.ldxr = Mpad; ga.xc = m->d_xs.p; ga.ldxc = Spad; ga.nrows = sz.M; ga.ncols = S;
    RC(t.ph_zs.prepare(sz.off, ss.off, C, m->T, Mpad, Spad, m->st, ga.ph));
    ga.table = m->d_table.p; ga.T = m->T; ga.D = D; ga.C = C; ga.W = m->Wt; ga.out = t.Kus.p; ga.ldo = Spad; ga.mirror = 0;
    RC(launch_gram(plan_cus(m->ctx), ga, (int)tus.size(), m->st));
    HIP_TRY(hipMemcpyAsync(t.Aus.p, t.Kus.p, (size_t)Mpad * Spad * sizeof(double), hipMemcpyDeviceToDevice, m->st));
    return trsm_lower(m, t.a.A.p, Mpad, (int)(Mpad / MOGP_TILE), t.Aus.p, Spad, Spad, false);             // a = L^-1 Kus
}

int sparse_point_stats(mogp_model* m, TitsiasWork& t, const SortedX& pts, const double* a, const double* b, const double* mu_panel,
                       const double* mu_vec, double mu_div, const double* kdiag, double* mu, double* var) {
    const int C = m->C;
    const int64_t Mpad = t.Mpad, Q = pts.Mpad;
    const bool env = m->Wt > 2 + 3 * m->D;                       // enveloped terms: K_diag per point (caller's order) instead of per channel
    RC(m->d_mu.ensure(Q)); RC(m->d_var.ensure(2 * Q));
    RC(launch_gemv_cols(mu_panel, Q, Mpad, Q, mu_vec, m->d_mu.p, t.scratch.p, m->st));
    RC(launch_gemv_cols(a, Q, Mpad, Q, nullptr, m->d_var.p, t.scratch.p, m->st));               // colsum a^2
    RC(launch_gemv_cols(b, Q, Mpad, Q, nullptr, m->d_var.p + Q, t.scratch.p, m->st));           // colsum b^2
    std::vector<double> hmu(Q), hv(2 * Q);
    HIP_TRY(hipMemcpyAsync(hmu.data(), m->d_mu.p, Q * sizeof(double), hipMemcpyDeviceToHost, m->st));
    HIP_TRY(hipMemcpyAsync(hv.data(), m->d_var.p, 2 * Q * sizeof(double), hipMemcpyDeviceToHost, m->st));
    HIP_TRY(hipStreamSynchronize(m->st));
    RC(sparse_timeout_check(m));
    for (int c = 0; c < C; ++c)
        for (int pos = pts.off[c]; pos < pts.off[c + 1]; ++pos) {
            mu[pts.perm[pos]] = hmu[pos] / mu_div;
            var[pts.perm[pos]] = kdiag ? (env ? kdiag[pts.perm[pos]] : kdiag[c]) - hv[pos] + hv[Q + pos] : hv[Q + pos];
        }
    return 0;
}

int sparse_predict_finish(mogp_model* m, TitsiasWork& t, const SortedX& ss, const double* mu_panel, const double* mu_vec, double mu_div,
                          const double* kss_diag, double* mu, double* var) {
    RC(sparse_point_stats(m, t, ss, t.Aus.p, t.Bus.p, mu_panel, mu_vec, mu_div, kss_diag, mu, var));
    t.pred_ss = ss; t.pred_valid = true;                    // a, b stay in t.Aus / t.Bus for mogp_sparse_predict_cov
    return 0;
}

}  // namespace mogp
