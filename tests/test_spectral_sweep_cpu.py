"""
The conditions the cases of the spectral sweep (tests/spectral_sweep.py) must meet for tests/test_spectral_sweep_gpu.py to mean what it says,
checked without a GPU: which Taylor degrees, skips and general tiles the cases reach (a numpy restatement of the strip kernel's `scalars`,
for accounting only), that Kj is well conditioned from the reference's own matrix, that the float64 twin of the oracle agrees with the
longdouble reference, and what the strip plan (mogp_strip_plan: the run cutting of csrc/mogp_api.hip as numbers) does with the sizes.
"""
import numpy as np
import pytest

from mogptk_amd import _lib
from oracle.table_model import gram_from_table
import kernel_family as kf
import spectral_ref as ref
import spectral_sweep as sw

NCUS = (1, 2, 3, 256)


def test_every_band_skip_and_general_is_reached():
    """every degree 4 .. 12 / 14, GT_GENERAL, a tile with some terms skipped and a tile with all of them skipped occur in a full tile at an even
    offset of some bands case; the table of what each case reaches is printed"""
    print("np.finfo(np.longdouble).eps =", ref.EPS)
    seen, partial, whole = {}, [], []
    for name in sw.BANDS:
        c = sw.bands_case(name)
        modes = sw.tile_modes(c)
        here = sorted({m for _, _, _, ms in modes for m in ms})
        for m in here:
            seen.setdefault(m, []).append(name)
        skips = [sum(m == sw.SKIP for m in ms) for _, _, _, ms in modes]
        if name != "zero_amp":
            partial += [name] * any(0 < k < c.T for k in skips)
            whole += [name] * any(k == c.T for k in skips)
        print("spectral sweep | bands | %-9s | %3d full even tiles | modes %s | tiles with some terms skipped %d, with all %d"
              % (name, len(modes), here, sum(0 < k < c.T for k in skips), sum(k == c.T for k in skips)))
    for m in sw.DEGREES + (sw.GENERAL, sw.SKIP):
        print("spectral sweep | mode %2d | reached by %s" % (m, seen.get(m, [])))
        assert m in seen, m
    assert partial and whole, (partial, whole)
    zero = sw.tile_modes(sw.bands_case("zero_amp"))
    assert all(ms[1] == sw.SKIP for _, _, _, ms in zero)                      # the term with A = 0, in every tile
    # wide tiles everywhere: a half span of 300 and more puts zmax above 0.45 for all but the flattest term, and that one four bands up
    assert all(ms[1:] == [sw.GENERAL] * 3 and ms[0] in (12, 14) for _, _, _, ms in sw.tile_modes(sw.bands_case("shuffled")))
    equal = [ms for r0, c0, _, ms in sw.tile_modes(sw.bands_case("equal")) if r0 == c0 == 128]
    assert equal == [[4] * 4]                                                 # hr = hc = 0: zmax = 0


@pytest.mark.parametrize("name,make", sw.all_cases(), ids=[n for n, _ in sw.all_cases()])
def test_case_is_well_conditioned_and_the_twin_agrees(name, make):
    """lambda_min(Kj) >= 0.1 from the reference's matrix; oracle.table_model.gram_from_table within 1e-13 of the longdouble reference"""
    c = make()
    K = ref.gram(c.table, c.X)
    twin = gram_from_table(c.table, c.X)
    e = kf.err(twin, K.astype(np.float64))
    e_ld = float(np.max(np.abs(twin - K)) / max(1.0, float(np.max(np.abs(K)))))
    Kj, jit = ref.kj(c.table, c.X, c.noise, c.jitter)
    ev = np.linalg.eigvalsh(Kj.astype(np.float64))
    print("spectral sweep | %s | N %d T %d | twin - reference %.3g (%.3g before rounding the reference) | lambda_min %.4g cond %.4g"
          % (name, c.N, c.T, e, e_ld, ev[0], ev[-1] / ev[0]))
    assert ev[0] >= sw.LAMBDA_MIN
    assert e <= 1e-13 and e_ld <= 1e-13


def test_sparse_case_is_well_conditioned():
    """the Titsias case of the GPU module: cond(K_uu + jitter) within the sparse sweep's own bound, and T and the row width what the strip
    kernel takes (T <= 8, rows of 5)"""
    import sparse_sweep as ss
    import test_sparse_sweep_cpu as sparse_cpu
    c = sw.sparse_case()
    cond = ss.cond_kuu(c.table, c.Z, c.jitter)
    bound = max(sparse_cpu.raw_case_conditions())
    print("spectral sweep | sparse | cond(K_uu + jitter) %.4g | bound %.4g" % (cond, bound))
    assert cond <= bound
    assert c.table.shape[2:] == (3, 5) and c.train == (640, 0, 0) and c.induce == (192, 0, 0)


def expand(plan):
    """the tiles (r0, c0, pair) a plan covers: the runs' and the rest's"""
    tiles = []
    for is_run, r0, c0, n, pair, diag, nr, nc in plan:
        tiles += [(r0, c0 + u * sw.GT, pair) for u in range(n)]
    return tiles


def sym_tiles(sizes):
    """the lower tile list of the symmetric Gram, restated: pairs i >= j, 64-point blocks per channel, lower blocks on the diagonal pairs"""
    off = np.concatenate([[0], np.cumsum(sizes)])
    C, out = len(sizes), {}
    for i in range(C):
        for j in range(i + 1):
            for bi in range(0, sizes[i], sw.GT):
                for bj in range(0, sizes[j], sw.GT):
                    if i == j and bj > bi:
                        continue
                    out[(off[i] + bi, off[j] + bj, i * C + j)] = (min(sw.GT, sizes[i] - bi), min(sw.GT, sizes[j] - bj))
    return out


@pytest.mark.parametrize("ncu", NCUS)
@pytest.mark.parametrize("sizes", sw.PLAN_SIZES, ids=sw.case_id)
def test_strip_plan_partitions_the_tile_list(sizes, ncu):
    plan = _lib.strip_plan(sizes, ncu)
    want = sym_tiles(sizes)
    got = expand(plan)
    assert len(got) == len(set(got)) == len(want) and set(got) == set(want)       # every tile exactly once
    runs = plan[plan[:, 0] == 1]
    assert np.all(plan[:len(runs), 0] == 1)                                       # the runs first
    for _, r0, c0, n, pair, diag, nr, nc in plan:
        assert (nr, nc) == want[(r0, c0, pair)] if n == 1 else (nr, nc) == (sw.GT, sw.GT)
    for _, r0, c0, n, pair, diag, nr, nc in runs:
        assert 1 <= n <= 8 and c0 % 2 == 0 and (nr, nc) == (sw.GT, sw.GT)
        for u in range(n):                                                        # one pair, one row block, consecutive columns, full tiles
            assert want[(r0, c0 + u * sw.GT, pair)] == (sw.GT, sw.GT)
        on_diagonal = [c0 + u * sw.GT == r0 for u in range(n)]
        assert diag == int(on_diagonal[-1]) and not any(on_diagonal[:-1])
    for _, r0, c0, n, pair, diag, nr, nc in plan[len(runs):]:                     # the rest: what the strip kernel cannot take
        assert n == 1 and ((nr, nc) != (sw.GT, sw.GT) or c0 % 2 == 1) and diag == int(r0 == c0)
    if ncu == 256:
        assert np.all(runs[:, 3] == 1)                                            # fewer runs than 2 * slots: single tiles (what the suite ran so far)


def test_one_cu_gives_the_long_runs():
    runs = [tuple(int(v) for v in r[1:6]) for r in _lib.strip_plan((640,), 1) if r[0] == 1]
    assert (448, 0, 8, 0, 1) in runs                                              # a run of 8 that ends on the diagonal
    k = runs.index((512, 0, 8, 0, 0))
    assert runs[k + 1] == (512, 512, 1, 0, 1)                                     # a run of 8, then the diagonal tile on its own
    assert sorted({r[2] for r in runs}) == [1, 2, 3, 4, 5, 6, 7, 8]
    lengths = lambda sizes: sorted({int(r[3]) for r in _lib.strip_plan(sizes, 1) if r[0] == 1})
    assert lengths((128, 256, 192)) == [1, 2, 3, 4]
    cross = [int(r[3]) for r in _lib.strip_plan((128, 256, 192), 1) if r[0] == 1 and r[4] in (3, 6, 7)]
    assert set(cross) == {2, 4}                                                   # rectangular cross-pair runs
    # a channel at an odd offset: none of its own full tiles is in a run, its cross-pair tiles against channel 0 are
    plan = _lib.strip_plan((65, 640), 1)
    assert not [r for r in plan if r[0] == 1 and r[4] == 3]
    assert len([r for r in plan if r[0] == 0 and r[4] == 3 and (r[6], r[7]) == (64, 64)]) == 55
    assert len([r for r in plan if r[0] == 1 and r[4] == 2]) == 10
    assert lengths((66, 576)) == [1, 2, 3, 4, 5, 6, 7, 8]                         # an even offset that is no multiple of 64


def test_strip_plan_refuses_bad_arguments():
    import ctypes
    cnt = ctypes.c_int64(0)
    sizes = np.array([64], dtype=np.int64)
    for C, ncu in ((0, 1), (1, 0), (1, -1)):
        assert _lib.lib().mogp_strip_plan(C, sizes.ctypes.data_as(_lib.c_i64p), ncu, None, 0, ctypes.byref(cnt)) != 0
    out = np.zeros(4, dtype=np.int64)
    assert _lib.lib().mogp_strip_plan(1, sizes.ctypes.data_as(_lib.c_i64p), 1, out.ctypes.data_as(_lib.c_i64p), out.size, ctypes.byref(cnt)) != 0
    assert cnt.value == 1
