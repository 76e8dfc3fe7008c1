"""
The sparse sweep without a device (tests/sparse_sweep.py): the conditions every generated case has to meet before the device is compared
with the numpy twin on it, and the twin's own pin at D = 2, 3, 5, 8 and under the envelope, where no golden reaches -- the gradient
outputs of `titsias_eval` and `snelson_eval` (which share `moments_dense`, `_jr_block` and `_jc_block` with the Hensman and
Opper-Archambeau entries) against central differences of the twin's own bound, through the host's `_gtable_from_moments` as
`Model._inducing_backward` puts it together.

The conditioning bound: cond(K_uu + jitter_abs I) at jitter 1e-6 of the Snelson raw cases of tests/test_gpu_parity.py, from the twin, is
6.3e6 at (699, 150), 8.3e6 at (1024, 300) and 1.39e7 at (2048, 520) (`raw_case_conditions`, printed by the first test).  The worst of
them, 1.39e7, is what every new case is held to; the figure is computed again on every run, not copied from here.
"""
import functools
import numpy as np
import pytest

from mogptk_amd import gpr, synth
from mogptk_amd.gpr.model import _gtable_from_moments
import sparse_sweep as ss

SLOT_RATIO = 1e-3
# d/dZ is a sum over b of G_ab dK_ab / dz_a through K_uf and K_uu, and where a channel's inducing points lie dense the two halves cancel.  The
# device's Gram entries are held to 1e-12 of the largest (tests/test_kinds_sweep_gpu.py: TOL_GRAM), so an entry of gZ can be off by
# [sum of |terms|] 1e-12: for gZ to be measurable at its bound (1e-7 Titsias, 1e-6 Snelson and the Hensman models, of its largest entry) that
# sum has to stay below 1e5 resp. 1e6 times the largest entry.  Found by the first device run of this sweep: with 129 inducing points in one
# channel on [0, 10] and V from 6 to 24 that ratio was 3.4e5 and the device's gZ 4.4e-7 from the twin's, its moments 2e-14; the twin's own
# fp64 sums were 3.5e-11 from np.longdouble ones, so the distance is the entries' accuracy times the cancellation and no fault of the sums.
GZ_CANCELLATION = {"titsias": 1e5, "snelson": 1e6, "svgp": 1e6}
RAW_CASES = [(699, 150), (1024, 300), (2048, 520)]


@functools.lru_cache(maxsize=None)
def raw_case_conditions():
    """cond(K_uu + jitter_abs I) of test_snelson_device_raw_outputs_against_numpy_model's cases: its table and its inducing inputs, drawn as
    it draws them (the generator's state before Z: the two permutations of X and the targets)"""
    out = []
    for N, M in RAW_CASES:
        rng = np.random.default_rng(N)
        Cr, Q = 3, 2
        X, _ = synth.make_data(N - N % Cr + (3 if N % Cr else 0), Cr)
        rng.permutation(X.shape[0])
        rng.random(N)
        rng.standard_normal(N)
        Z = np.concatenate([np.stack([np.full(M // Cr, float(c)), np.sort(rng.uniform(0, 100, M // Cr))], axis=1) for c in range(Cr)])
        h = synth.mosm_hypers(Cr, Q)
        k = gpr.MultiOutputSpectralMixtureKernel(Q=Q, output_dims=Cr)
        for name in ("weight", "mean", "variance", "delay", "phase"):
            getattr(k, name).assign(h[name])
        out.append(ss.cond_kuu(k._spectral_terms(1), Z, 1e-6))
    return tuple(out)


def test_the_bound_on_conditioning_is_the_raw_cases_own():
    conds = raw_case_conditions()
    print("cond(K_uu + jitter_abs I) of the raw cases", dict(zip(RAW_CASES, conds)))
    assert all(np.isfinite(conds)) and max(conds) > 1.0


def test_the_sweep_holds_what_it_is_meant_to():
    """the sizes the case list exists for"""
    cases = [ss.case(*s) for s in ss.SWEEP]
    assert {c.program for c in cases} == set(ss.PROGRAMS)
    assert any(c.N % 128 == 0 for c in cases) and any(c.N % 128 for c in cases)
    assert any(c.M > c.N for c in cases)
    assert any(any(t > 0 and m == 0 for t, m in zip(c.train, c.induce)) for c in cases)      # a training channel without inducing points
    assert any(any(t == 0 and m > 0 for t, m in zip(c.train, c.induce)) for c in cases)      # an inducing channel without data
    assert all(c.N <= 400 and c.M <= 260 for c in cases)
    for p in ss.PROGRAMS:                                    # every program with two inducing shapes that span several 64-point blocks
        assert sum(1 for c in cases if c.program == p and max(c.induce) > 64) >= 2, p
    for m in ss.INDUCE:
        assert {c.program for c in cases if c.induce == ss.pad(m)} >= set(ss.EVERY_SHAPE), m
    widths = {p: ss.case(p, *ss.TINY).W for p in ss.PROGRAMS}
    assert widths["d5"] == 17 and widths["d8"] == 26 and widths["d3_env"] == 17 and widths["d4_env"] == 22
    assert ss.case("d1_t9", *ss.TINY).T == 9


@pytest.mark.parametrize("program,train,induce", ss.SWEEP, ids=ss.case_id)
def test_every_case_is_well_conditioned_and_no_slot_hides(program, train, induce):
    """conditions on the inputs, not measurements: K_uu + jitter_abs I no worse conditioned than the worst raw case, and every column of gZ and
    every moment slot that bears a parameter at least 1e-3 of its tensor's largest entry, in each of the three sparse models; gZ not the
    residue of a cancellation that the entries' accuracy cannot carry (GZ_CANCELLATION)"""
    c = ss.case(program, train, induce)
    cond = ss.cond_kuu(c.table, c.Z, c.jitter)
    twins = {"titsias": ss.twin_titsias(program, train, induce), "snelson": ss.twin_snelson(program, train, induce),
             "svgp": ss.twin_svgp(program, train, induce)[1]}
    ratios = {model: ss.slot_ratios(c, res) for model, res in twins.items()}
    cancel = {model: res["gz_cancellation"] for model, res in twins.items()}
    smallest = min(v for r in ratios.values() for v in r.values())
    print("sparse sweep |", program, ss.case_id(train), ss.case_id(induce), "| cond(K_uu)", cond, "| smallest slot ratio", smallest, "|", ratios,
          "| cancellation in gZ", cancel)
    assert cond <= max(raw_case_conditions())
    assert smallest >= SLOT_RATIO, ratios
    assert all(cancel[model] <= GZ_CANCELLATION[model] for model in cancel), cancel
    Zd = c.Z[np.argsort(c.Z[:, 0], kind="stable")]
    lo, hi = np.min(c.X[:, 1:], axis=0), np.max(c.X[:, 1:], axis=0)
    assert np.all(Zd[:, 1:] >= lo) and np.all(Zd[:, 1:] <= hi)      # inside the data's range


@pytest.mark.parametrize("program", ss.DENSE_PROGRAMS)
def test_the_dense_cases_are_well_conditioned_too(program):
    """the dense Hensman model's K_uu is K_ff at jitter 1e-4, the raw tests' value for it: the same bound on its conditioning, and its
    mom_uf and gZ are exactly zero in the twin"""
    c = ss.dense_case(program)
    cond = ss.cond_kuu(c.table, c.Z, c.jitter)
    _, bwd, _ = ss.twin_svgp_dense(program)
    ratios = ss.slot_ratios(c, bwd, names=("mom_uu",))
    print("sparse sweep |", program, "dense | cond(K_uu)", cond, "| smallest slot ratio", ratios)
    assert cond <= max(raw_case_conditions())
    assert ratios["mom_uu"] >= SLOT_RATIO
    assert not np.any(bwd["mom_uf"]) and not np.any(bwd["gZ"])


@pytest.mark.parametrize("train", ss.TRAIN, ids=ss.case_id)
@pytest.mark.parametrize("program", ss.OA_PROGRAMS)
def test_no_slot_hides_in_the_opper_archambeau_cases(program, train):
    c = ss.oa_case(program, train)
    ratios = ss.slot_ratios(c, ss.twin_oa(program, train)[1], names=("mom",))
    print("sparse sweep |", program, ss.case_id(train), "oa | smallest slot ratio", ratios)
    assert ratios["mom"] >= SLOT_RATIO


def parameter_columns(c, cross):
    D = c.D
    cols = [0] + list(range(2, 2 + 2 * D)) + ([1] + list(range(2 + 2 * D, 2 + 3 * D)) if cross else [])
    return cols + (list(range(2 + 3 * D, 2 + 5 * D)) if c.envelope else [])


def table_gradient(c, res, jitter, kernel):
    """d bound / d table as Model._inducing_backward builds it: the moments over the lower pairs (K_uu) and over all pairs (K_uf), and what
    K_uu's relative jitter adds -- with an envelope through the per-point diagonal, and then d/dZ gets a share too"""
    gt = _gtable_from_moments(c.table, res["mom_uu"], c.D, lower=True) + _gtable_from_moments(c.table, res["mom_uf"], c.D, lower=False)
    gz = res["gZ"].copy()
    if c.envelope:
        gt += (jitter * res["trGA"] / c.M) * kernel._point_diag_table_grad(c.table, c.Z, c.D)
        gz += (jitter * res["trGA"] / c.M) * kernel._point_diag_input_grad(c.table, c.Z, c.D)
    else:
        for i in range(c.C):
            gt[i, i, :, 0] += jitter * res["trGA"] * c.induce[i] / c.M
    return gt, gz


def central(fn, x, idx):
    step = 1e-6 * max(1.0, abs(x[idx]))
    up, dn = x.copy(), x.copy()
    up[idx] += step
    dn[idx] -= step
    return (fn(up) - fn(dn)) / (2.0 * step)


@pytest.mark.parametrize("model", ["titsias", "snelson"])
@pytest.mark.parametrize("program", list(ss.PROGRAMS))
def test_twin_gradients_are_the_derivatives_of_the_twins_own_bound(program, model):
    """central differences of the twin's bound (step 1e-6 max(1, |theta|)) in every inducing coordinate, in every parameter column of every
    ordered channel pair, and in the noise, at the project's finite-difference bound 1e-5 max(1, |g|).  The kernel diagonal K_ff is an
    argument of the entry points and stays what it was: its share of the gradient is the host's, not the twin's"""
    c = ss.case(program, *ss.TINY)
    h = ss.twin(c)
    value = "elbo" if model == "titsias" else "lml"

    def bound(table=None, Z=None, noise=None, kff=None):
        h.set_terms(c.table if table is None else table)
        Z = c.Z if Z is None else Z
        kff = c.kff if kff is None else kff
        if model == "titsias":
            return h.titsias_eval(Z, c.sigma if noise is None else noise, c.jitter, kff, grad=False)[value]
        return h.snelson_eval(Z, c.noise if noise is None else noise, c.jitter, kff, grad=False)[value]

    res = h.titsias_eval(c.Z, c.sigma, c.jitter, c.kff) if model == "titsias" else h.snelson_eval(c.Z, c.noise, c.jitter, c.kff)
    gt, gz = table_gradient(c, res, c.jitter, c.kernel)
    worst = {}

    def check(name, got, fd, where):
        e = abs(got - fd) / max(1.0, abs(fd))
        worst[name] = max(worst.get(name, 0.0), e)
        assert e <= 1e-5, (program, model, name, where, got, fd)

    for a in range(c.M):
        for d in range(c.D):
            check("gZ", gz[a, d], central(lambda Z: bound(Z=Z), c.Z, (a, 1 + d)), (a, d))
    for i in range(c.C):
        for j in range(c.C):
            if c.induce[i] == 0 or (c.train[j] == 0 and c.induce[j] == 0):
                continue
            for t in range(c.T):
                for col in parameter_columns(c, i != j):
                    check("table", gt[i, j, t, col], central(lambda tb: bound(table=tb), c.table, (i, j, t, col)), (i, j, t, col))
    if model == "titsias":
        check("dsigma", res["dsigma"], central(lambda s: bound(noise=float(s[0])), np.array([c.sigma]), (0,)), None)
    else:
        hs = np.bincount(c.X[:, 0].astype(np.int64), weights=res["hsum"], minlength=c.C) if c.envelope else res["hsum"]
        for ch in range(c.C):                                # dp / dsigma_c^2, summed per channel
            check("hsum", hs[ch], central(lambda nv: bound(noise=nv), c.noise, (ch,)), ch)
        if c.envelope:                                       # per point: dp / dK_ff,nn
            for n in range(c.N):
                check("hsum per point", res["hsum"][n], central(lambda kf: bound(kff=kf), c.kff, (n,)), n)
    print("sparse sweep |", program, model, "| largest finite-difference error", max(worst.values()), "|", worst)
