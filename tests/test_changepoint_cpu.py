"""
Host side of ChangePointsKernel (the gate row, kind 8), without a device: the class surface; the rows, kinds and flags it emits
alone and under AddKernel, MulKernel, IndependentMultiOutputKernel and LMC; the table form through the numpy twin of the device handle
(oracle/table_model.py with the gate row of tests/changepoint_twin.py) against the reference's K / K_diag (tests/golden/changepoint.npz,
written by tests/golden/gen_family.py from the models of tests/changepoint_cases.py); the twin's gate moments against central differences of
its own Gram; the chain rule and the per-point diagonal's backward against the reference's autograd; the refusals; checkpoints.  The bodies
shared with the other kernel families, and their tolerances, are in tests/kernel_family.py.
"""
import os
import numpy as np
import pytest

from mogptk_amd import gpr, _lib
from mogptk_amd.gpr.kernel import KIND_TIMES, KIND_DOT, KIND_GATE
import changepoint_cases as cc
import changepoint_twin as twin
import kernel_family as kf
from family_cases import exact, full_cases
import oracle.table_model as tm

FAMILY = "changepoint"
X_ = KIND_TIMES
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def kinds_of(case):
    return cc.kernel(gpr, case)._spectral_kinds(1)[0]


def test_class_surface_matches_the_reference():
    k = gpr.ChangePointsKernel([3.0, 7.0], [2.0, 5.0], gpr.MaternKernel(nu=1.5), gpr.SquaredExponentialKernel(), gpr.RationalQuadraticKernel())
    assert [p._name.split(".")[-1] for p in k.parameters()][:2] == ["locations", "steepness"]      # its own first, then the sub-kernels'
    assert k.locations().shape == (2,) and k.steepness().shape == (2,) and k.locations.lower is None
    assert float(np.asarray(k.steepness.lower).reshape(-1)[0]) == gpr.config.positive_minimum
    assert np.array_equal(k.locations(), [3.0, 7.0]) and np.allclose(k.steepness(), [2.0, 5.0], rtol=2e-5)      # (the softplus link, as for every positive parameter)
    assert k.input_dims == 1 and k.output_dims is None and len(k.kernels) == 3 and k[1] is k.kernels[1]
    k = gpr.ChangePointsKernel(4.0, 2.0, gpr.MaternKernel(nu=1.5), gpr.SquaredExponentialKernel())      # a bare location, the default shape of the steepness
    assert k.locations().shape == (1,) and k.steepness().shape == ()
    assert gpr.ChangePointsKernel([4.0], [2.0], gpr.MaternKernel(), gpr.MaternKernel()).steepness().shape == (1,)
    with pytest.raises(ValueError, match="Must pass one more kernel than the number of locations points. Got 1 kernels and 1 locations points."):
        gpr.ChangePointsKernel([4.0], 1.0, gpr.MaternKernel())
    with pytest.raises(ValueError, match=r"Must pass as many locations as steepness point\(s\). Got 1 locations and 2 steepness points."):
        gpr.ChangePointsKernel([4.0], [1.0, 2.0], gpr.MaternKernel(), gpr.MaternKernel())
    with pytest.raises(ValueError, match="'locations' must be sorted ascendingly"):
        gpr.ChangePointsKernel([7.0, 3.0], 1.0, gpr.MaternKernel(), gpr.MaternKernel(), gpr.MaternKernel())
    with pytest.raises(ValueError, match="Must pass kernels defined over a 1D input domain."):
        gpr.ChangePointsKernel([4.0], 1.0, gpr.SquaredExponentialKernel(input_dims=2), gpr.SquaredExponentialKernel(input_dims=2))
    assert isinstance(k + gpr.SquaredExponentialKernel(), gpr.AddKernel) and isinstance(gpr.CosineKernel() * k, gpr.MulKernel)
    # K_diag = sum_i a_i(x)^2 k_i(x, x) follows the point
    x = np.array([[0.5], [4.0], [9.0]])
    h = twin.sigmoid(float(k.steepness()) * (x[:, 0] - 4.0))
    assert np.allclose(k.K_diag(x), (1.0 - h) ** 2 * float(k.kernels[0].magnitude()) + h ** 2 * float(k.kernels[1].magnitude()), rtol=1e-13)
    assert k._radial(1) and k._pointwise(1)


def test_rows_kinds_and_flags():
    assert KIND_GATE == 8 and KIND_DOT == 7
    # two: [m32, falling gate at 4] [se, rising gate at 4]
    k = cc.kernel(gpr, "two")
    assert kinds_of("two").tolist() == [[[3 | X_, 8, 0 | X_, 8]]]
    t = k._spectral_terms(1)[0, 0]
    s = float(k.steepness())
    assert np.array_equal(t[1], [1.0, 0.0, -s, 4.0, 0.0]) and np.array_equal(t[3], [1.0, 0.0, s, 4.0, 0.0])      # [A, Psi, beta, l, Delta]
    assert np.array_equal(t[0], k.kernels[0]._spectral_terms(1)[0, 0, 0]) and np.array_equal(t[2], k.kernels[1]._spectral_terms(1)[0, 0, 0])
    # three: the middle kernel m52 * cos with its rising gate at 3 and its falling gate at 7 is a full group of four; one steepness per location
    k = cc.kernel(gpr, "three")
    kd, sh = k._spectral_kinds(1)
    assert kd.tolist() == [[[3 | X_, 8, 4 | X_, 0 | X_, 8 | X_, 8, 1 | X_, 8]]] and sh[0, 0, 6] == 0.7 and not np.any(np.delete(sh[0, 0], 6))
    t = k._spectral_terms(1)[0, 0]
    s = k.steepness()
    assert np.array_equal(t[[1, 4, 5, 7], 2], [-s[0], s[0], -s[1], s[1]]) and np.array_equal(t[[1, 4, 5, 7], 3], [3.0, 3.0, 7.0, 7.0])
    assert np.all(t[[1, 4, 5, 7], 0] == 1.0) and not np.any(t[[1, 4, 5, 7]][:, [1, 4]])
    # shared: four gate rows carry the one steepness; the linear kernel's dot-product row leads the last group
    k = cc.kernel(gpr, "shared")
    assert kinds_of("shared").tolist() == [[[0 | X_, 8, 5 | X_, 8 | X_, 8, 7 | X_, 8]]]
    t = k._spectral_terms(1)[0, 0]
    s = float(k.steepness())
    assert np.array_equal(t[[1, 3, 4, 6], 2], [-s, s, -s, s]) and np.array_equal(t[[1, 3, 4, 6], 3], [3.0, 3.0, 7.0, 7.0])
    # sums distribute: (m32 + cos) and the two rows of the spectral mixture get a gate each
    assert kinds_of("sums").tolist() == [[[3 | X_, 8, 0 | X_, 8, 0 | X_, 8, 0 | X_, 8]]]
    assert kinds_of("plus").tolist() == [[[3 | X_, 8, 0 | X_, 8, 0]]]
    assert kinds_of("times").tolist() == [[[0 | X_, 3 | X_, 8, 0 | X_, 0 | X_, 8]]]      # the cosine row in front of either group
    assert kinds_of("straddle").tolist() == [[[0, 3, 0, 1, 4, 5, 2, 3 | X_, 8, 0 | X_, 8]]]
    # LMC scales the first row of a group: a kernel row, never a gate
    k = cc.kernel(gpr, "lmc")
    kd, t, B = k._spectral_kinds(1)[0], k._spectral_terms(1), k._coreg()
    assert np.all(kd == np.array([3 | X_, 8, 0 | X_, 8, 3]))
    cp = k.kernels[0]
    assert np.allclose(t[..., 0, 0], B[..., 0] * cp.kernels[0].magnitude(), rtol=1e-15) and np.allclose(t[..., 2, 0], B[..., 0] * cp.kernels[1].magnitude(), rtol=1e-15)
    assert np.all(t[..., [1, 3], 0] == 1.0)
    # IndependentMultiOutputKernel of two change-point kernels whose groups line up: shared rows, each channel its own gates
    kd = kinds_of("imo")
    assert kd[0, 0].tolist() == [3 | X_, 8, 0 | X_, 8] and kd[1, 1].tolist() == [5 | X_, 8, 4 | X_, 8] and kd[0, 1].tolist() == [X_, 0, X_, 0]
    # nested in itself (through an AddKernel: the base class takes a directly nested one apart): inner gates, then the outer one
    inner = gpr.AddKernel(gpr.ChangePointsKernel([3.0], 1.0, gpr.MaternKernel(nu=1.5), gpr.SquaredExponentialKernel()))
    k = gpr.ChangePointsKernel([6.0], 2.0, inner, gpr.MaternKernel(nu=2.5))
    assert k._spectral_kinds(1)[0].tolist() == [[[3 | X_, 8 | X_, 8, 0 | X_, 8 | X_, 8, 4 | X_, 8]]]


@pytest.mark.parametrize("case", full_cases(FAMILY))
def test_table_and_kinds_reproduce_the_reference_gram(case, monkeypatch):
    twin.install(monkeypatch)
    kf.check_table_and_kinds(FAMILY, case)


@pytest.mark.parametrize("case", full_cases(FAMILY))
def test_chain_rule_reproduces_reference_gradients(case, monkeypatch):
    twin.install(monkeypatch)
    m = kf.check_chain_rule(FAMILY, case, monkeypatch)
    assert isinstance(m._handle, twin.GateTableDevice) and np.any((m._handle.kind & 0xff) == KIND_GATE)


@pytest.mark.parametrize("case", ["two", "shared", "lmc"])
def test_predictions_over_the_twin_match_the_reference(case, monkeypatch):
    """the per-point test diagonal h(x)^2-weighted, as Exact.predict_f hands it over"""
    twin.install(monkeypatch)
    monkeypatch.setattr(_lib, "ExactHandle", twin.GateTableDevice)
    kf.check_predictions(FAMILY, case)


def test_gate_moments_are_derivatives_of_the_twins_own_gram(monkeypatch):
    """m1_0 = d/dbeta and m3_0 = d/dl of sum_ab g_ab K_ab for a gate row alone, in a group with a Matern row, and with beta < 0, against
    central differences of kinds_block's own value; the other slots are zero"""
    twin.install(monkeypatch)
    rng = np.random.default_rng(5)
    x1, x2 = rng.uniform(0, 10, (9, 1)), rng.uniform(0, 10, (7, 1))
    g = rng.standard_normal((9, 7))
    for tab, kind in (([[1.3, 0.0, 1.7, 4.2, 0.0]], [8]), ([[0.9, 0.0, 2.0, 0.0, 0.0], [1.0, 0.0, -2.5, 6.1, 0.0]], [3 | X_, 8]),
                      ([[0.9, 0.0, 2.0, 0.0, 0.0], [1.0, 0.0, 0.8, 3.0, 0.0], [1.0, 0.0, -40.0, 5.0, 0.0]], [4 | X_, 8 | X_, 8])):
        tab, kind = np.array(tab), np.array(kind)
        shape = np.zeros(len(kind))
        K, mom = tm.kinds_block(tab, kind, shape, x1, x2, g)
        for t in np.nonzero((kind & 0xff) == 8)[0]:
            assert mom[t, 1] == 0.0 and mom[t, 3] == 0.0
            for col, slot in ((2, 2), (3, 4), (0, 0)):
                up, dn = tab.copy(), tab.copy()
                h = 1e-6
                up[t, col] += h; dn[t, col] -= h
                fd = (np.sum(g * tm.kinds_block(up, kind, shape, x1, x2)[0]) - np.sum(g * tm.kinds_block(dn, kind, shape, x1, x2)[0])) / (2 * h)
                want = mom[t, slot] * (1.0 if col == 0 else tab[t, 0])      # a row's moments leave its own amplitude out (1 for a pure weight)
                assert abs(want - fd) <= 1e-8 * max(1.0, abs(fd)), (kind.tolist(), t, col, want, fd)
    # a saturated gate: exp(-|z|) underflows, nothing overflows, the complement is exact
    z = np.array([-800.0, -40.0, 0.0, 40.0, 800.0])
    assert np.all(np.isfinite(twin.sigmoid(z))) and twin.sigmoid(z)[0] == 0.0 and twin.sigmoid(z)[-1] == 1.0
    assert np.array_equal(twin.sigmoid(-z), twin.sigmoid(z)[::-1]) and twin.sigmoid(-z)[3] == np.exp(-40.0) / (1.0 + np.exp(-40.0))


def test_refusals_come_before_any_device_call(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "lib", no_device)
    monkeypatch.setattr(_lib, "ExactHandle", no_device)
    m32, cos, per, se = (lambda: gpr.MaternKernel(nu=1.5)), gpr.CosineKernel, gpr.PeriodicKernel, gpr.SquaredExponentialKernel
    # the row limit: three rows for an end kernel, two for a middle kernel; the message names the sub-kernel and the count
    end = gpr.ChangePointsKernel([4.0], 1.0, gpr.MulKernel(m32(), cos(), per(), se()), se())
    with pytest.raises(NotImplementedError, match=r"sub-kernel 0, \[MaternKernel,CosineKernel,PeriodicKernel,SquaredExponentialKernel\]: 5 rows.*at most 4 rows"):
        end._spectral_terms(1)
    middle = gpr.ChangePointsKernel([3.0, 7.0], 1.0, se(), gpr.MulKernel(m32(), cos(), per()), se())
    with pytest.raises(NotImplementedError, match=r"sub-kernel 1, \[MaternKernel,CosineKernel,PeriodicKernel\]: 5 rows with its 2 gate rows"):
        middle._spectral_kinds(1)
    gpr.ChangePointsKernel([4.0], 1.0, gpr.MulKernel(m32(), cos(), per()), se())._spectral_terms(1)      # three rows and one gate fit
    with pytest.raises(NotImplementedError, match="more than 4"):      # as a factor: cos * (m32 * per with its gate) * se is five rows
        gpr.MulKernel(cos(), gpr.ChangePointsKernel([4.0], 1.0, gpr.MulKernel(m32(), per(), se()), se()))._spectral_terms(1)
    lmc = gpr.LinearModelOfCoregionalizationKernel(gpr.ChangePointsKernel([3.0, 7.0], 1.0, se(), gpr.MulKernel(gpr.LinearKernel(), per()), se()), output_dims=2)
    with pytest.raises(NotImplementedError, match="at most 4 rows"):      # dot-product row first: the leading coregionalization row is the fifth
        lmc._spectral_terms(1)
    # input dimensions, multi-output and enveloped sub-kernels, a directly nested change-point kernel
    with pytest.raises(ValueError, match="1D input domain"):
        gpr.ChangePointsKernel([4.0], 1.0, se(input_dims=2), se(input_dims=2))
    with pytest.raises(ValueError, match="1D input domain"):
        cc.kernel(gpr, "two")._spectral_terms(2)
    mo = lambda: gpr.IndependentMultiOutputKernel(se(), se(), output_dims=2)
    with pytest.raises(NotImplementedError, match="multi-output"):
        gpr.ChangePointsKernel([4.0], 1.0, mo(), mo())
    with pytest.raises(NotImplementedError, match="single- and multi-output"):
        gpr.ChangePointsKernel([4.0], 1.0, se(), mo())
    with pytest.raises(NotImplementedError, match="wrap the inner one in an AddKernel"):
        gpr.ChangePointsKernel([6.0], 1.0, gpr.ChangePointsKernel([3.0], 1.0, se(), se()), se())
    with pytest.raises(NotImplementedError, match="active_dims"):
        gpr.ChangePointsKernel([4.0], 1.0, gpr.MaternKernel(active_dims=[0]), se())
    env = gpr.AddKernel(gpr.MultiOutputHarmonizableSpectralKernel(output_dims=1, input_dims=1), gpr.IndependentMultiOutputKernel(cc.kernel(gpr, "two"), output_dims=1))
    with pytest.raises(NotImplementedError, match="enveloped"):
        env(np.zeros((4, 2)))
    # the sparse and variational models and the sharded evaluation refuse it as they refuse every non-zero kind, with today's message --
    # also when every sub-kernel is Gaussian: the change-point kernel is radial as a whole
    X, y, _ = cc.data("two")
    Xc, yc, _ = cc.data("imo")
    gauss = lambda: gpr.ChangePointsKernel([4.0], 2.0, se(), se())
    sparse = dict(Titsias=dict(Z=4), Snelson=dict(Z=4), OpperArchambeau={}, SparseHensman=dict(Z=4), Hensman={})
    for name, kw in sparse.items():
        for build in (lambda: (cc.kernel(gpr, "two"), X, y), lambda: (gauss(), X, y), lambda: (cc.kernel(gpr, "plus"), X, y), lambda: (cc.kernel(gpr, "times"), X, y),
                      lambda: (cc.kernel(gpr, "imo"), Xc, yc), lambda: (cc.kernel(gpr, "lmc"), Xc, yc)):
            with pytest.raises(NotImplementedError, match="%s with a non-Gaussian" % name):
                getattr(gpr, name)(*build(), **kw)

    class Comm:                                                 # what use_distributed() leaves in config.comm
        native, world, rank, force = True, 2, 0, False
    saved = getattr(gpr.config, "comm", None)
    gpr.config.comm = Comm()
    try:
        for case in ("two", "shared", "lmc"):
            m = exact(FAMILY, gpr, case)
            with pytest.raises(NotImplementedError, match="use_distributed"):
                m.loss()
            assert m._handle is None
    finally:
        gpr.config.comm = saved


def test_header_and_host_agree_on_the_kind():
    src = open(os.path.join(ROOT, "include", "mogp_hip.h")).read()
    assert "#define MOGP_KIND_GATE %d\n" % KIND_GATE in src


CHECKPOINTS = ("cp", "lmc")


def _walk(k):
    yield k
    for s in getattr(k, "kernels", None) or []:
        yield from _walk(s)


@pytest.mark.parametrize("tag", CHECKPOINTS)
def test_reference_checkpoint_round_trip(tag, tmp_path):
    pytest.importorskip("torch")
    k = kf.check_checkpoint_loads(FAMILY, tag, tmp_path)
    want = dict(cp={"ChangePointsKernel", "MaternKernel", "MulKernel", "CosineKernel", "RationalQuadraticKernel"},
                lmc={"LinearModelOfCoregionalizationKernel", "ChangePointsKernel", "PeriodicKernel"})[tag]
    assert want <= set(kf.kernel_names(k))
    cp = [s for s in _walk(k) if type(s).__name__ == "ChangePointsKernel"]
    assert len(cp) == 1 and cp[0].steepness().shape == dict(cp=(2,), lmc=())[tag] and cp[0].locations().shape == dict(cp=(2,), lmc=(1,))[tag]
    kf.check_checkpoint_is_written_as_the_reference_writes_it(FAMILY, tag)


@pytest.mark.parametrize("tag", CHECKPOINTS)
def test_loaded_checkpoint_evaluates_as_the_reference(tag, tmp_path, monkeypatch):
    """loss and every gradient of the loaded model over the twin against what the reference computed on the file it wrote (the locations of
    `cp` were drawn unsorted: the loader does not ask)"""
    pytest.importorskip("torch")
    import mogptk_amd
    from helpers import load
    twin.install(monkeypatch)
    monkeypatch.setattr(_lib, "ExactHandle", twin.GateTableDevice)
    fx = load(FAMILY + "_checkpoints.npz")
    (tmp_path / "ref.npy").write_bytes(fx[tag + "_file"].tobytes())
    m = mogptk_amd.LoadModel(str(tmp_path / "ref"))
    loss = float(m.gpr.loss())
    assert abs(loss - float(fx[tag + "_loss"])) <= 1e-9 * max(1.0, abs(float(fx[tag + "_loss"])))
    for i, p in enumerate(m.gpr.parameters()):
        g = fx["%s_g%d" % (tag, i)]
        if g.size:
            assert np.max(np.abs(p.grad - g)) <= 1e-9 * max(1.0, np.max(np.abs(g))), p._name
