"""
Host side of FunctionKernel and WhiteKernel (the weighted-dot row, kind 9, whose basis functions travel as input columns, and
the white row, kind 10), without a device: the class surface; the rows, kinds and feature columns alone and under AddKernel, MulKernel,
IndependentMultiOutputKernel and LMC; the table re-laid to the device's columns through the numpy twin of the device handle
(oracle/table_model.py with the rows of tests/function_twin.py) against the reference's K / K(X, Xs) / K_diag (tests/golden/function.npz,
written by tests/golden/gen_function.py from the models of tests/function_cases.py); the twin's moments against central differences of its
own Gram; the chain rule against the reference's autograd; predictions; the refusals; neutrality; checkpoints.  The bodies shared with the
other kernel families, and their tolerances, are in tests/kernel_family.py.
"""
import os
import numpy as np
import pytest

import mogptk_amd
from mogptk_amd import gpr, _lib
from mogptk_amd.gpr.kernel import KIND_TIMES, KIND_WDOT, KIND_WHITE
import function_cases as fc
import function_twin as twin
import kernel_family as kf
from family_cases import exact, full_cases
import oracle.table_model as tm

FAMILY = "function"
X_ = KIND_TIMES
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f2 = lambda: gpr.FunctionKernel(fc.feature_map(gpr, "f2"))
se = gpr.SquaredExponentialKernel


def test_class_surface_matches_the_reference():
    k = gpr.FunctionKernel(fc.feature_map(gpr, "f4"))
    assert [p._name.split(".")[-1] for p in k.parameters()] == ["magnitude"]
    assert k.magnitude().shape == (4,) and np.allclose(k.magnitude(), 1.0, rtol=2e-5) and k.input_dims == 1 and k.output_dims is None
    assert float(np.asarray(k.magnitude.lower).reshape(-1)[0]) == gpr.config.positive_minimum
    seen = []
    gpr.FunctionKernel(lambda x: (seen.append(x), np.stack([x[:, 0], x[:, 1]], 1))[1], input_dims=2)
    assert seen[0].shape == (42, 2) and seen[0].dtype == np.float64 and np.all(seen[0] == 1.0)      # the reference's probe
    with pytest.raises(ValueError, match="phi must return an array of the same dtype as the input"):
        gpr.FunctionKernel(lambda x: x.astype(np.float32))
    with pytest.raises(ValueError, match="phi must return an array of the same dtype as the input"):
        gpr.FunctionKernel(lambda x: x.tolist())
    for bad in (lambda x: x[:, 0], lambda x: x[:7]):
        with pytest.raises(ValueError, match=r"phi must take \(data_points,input_dims\) as input, and return \(data_points,feature_dims\) as output"):
            gpr.FunctionKernel(bad)
    w = gpr.WhiteKernel()
    assert [p._name.split(".")[-1] for p in w.parameters()] == ["magnitude"] and w.magnitude().shape == () and w.input_dims == 1
    assert isinstance(k + w, gpr.AddKernel) and isinstance(w * k, gpr.MulKernel)
    # K_diag: phi diag(mag) phi^T on the diagonal follows the point; the white kernel's is its magnitude
    x = np.array([[0.5], [4.0], [9.0]])
    k = f2()
    k.magnitude.assign([0.7, 0.4])
    assert np.allclose(k.K_diag(x), 0.7 + 0.4 * (x[:, 0] / 10.0) ** 2, rtol=1e-5) and k._radial(1) and k._pointwise(1)
    w.magnitude.assign(0.3)
    assert np.allclose(w.K_diag(x), 0.3, rtol=1e-5) and w._radial(1) and not w._pointwise(1)
    with pytest.raises(NotImplementedError, match="active_dims"):
        gpr.FunctionKernel(fc.feature_map(gpr, "f2"), active_dims=[0])
    with pytest.raises(NotImplementedError, match="active_dims"):
        gpr.WhiteKernel(active_dims=[0])


def test_rows_kinds_and_feature_columns():
    assert KIND_WDOT == 9 and KIND_WHITE == 10
    # in the composition's own table a FunctionKernel is [1, 0, ...] of kind 9; the device's table carries its magnitude on its feature columns
    k = fc.kernel(gpr, "trend")
    fk = k.kernels[0]
    assert k._spectral_kinds(1)[0].tolist() == [[[9, 0]]] and np.array_equal(k._spectral_terms(1)[0, 0, 0], [1.0, 0.0, 0.0, 0.0, 0.0])
    X = np.linspace(0.0, 10.0, 7)[:, None]
    Xk = k._kernel_format(X)
    assert Xk.shape == (7, 4) and np.all(Xk[:, 0] == 0.0) and np.array_equal(Xk[:, 1], X[:, 0])
    assert np.array_equal(Xk[:, 2], np.ones(7)) and np.array_equal(Xk[:, 3], X[:, 0] / 10.0)
    table, kind, shape, D = k._device_terms(3)
    assert D == 1 and table.shape == (1, 1, 2, 11) and kind.tolist() == [[[9, 0]]]
    assert np.array_equal(table[0, 0, 0], np.concatenate([[1.0, 0.0, 0.0], fk.magnitude(), np.zeros(6)]))
    own = k.kernels[1]._spectral_terms(1)[0, 0, 0]
    assert np.array_equal(table[0, 0, 1], [own[0], 0.0, own[2], 0.0, 0.0, own[3], 0.0, 0.0, own[4], 0.0, 0.0])      # V, M, Delta widened with zeros
    # two leaves: columns in leaf order, each row finds its own; one leaf used twice travels once
    a, b = f2(), gpr.FunctionKernel(fc.feature_map(gpr, "fs"))
    b.magnitude.assign([0.2, 0.9])
    k = gpr.AddKernel(gpr.MulKernel(a, se()), b, gpr.MulKernel(a, gpr.CosineKernel()))
    assert [id(x) for x in k._feature_leaves()] == [id(a), id(b)] and (a._feature_offset, b._feature_offset) == (0, 2)
    assert k._kernel_format(X).shape == (7, 6)
    table, kind, shape, D = k._device_terms(5)
    assert kind.tolist() == [[[9 | X_, 0, 9, 9 | X_, 0]]] and shape[0, 0].tolist() == [0.0, 0.0, 2.0, 0.0, 0.0]
    V = table[0, 0, :, 2:7]
    assert np.array_equal(V[0], np.concatenate([[0.0], a.magnitude(), [0.0, 0.0]])) and np.array_equal(V[3], V[0])
    assert np.array_equal(V[2], np.concatenate([[0.0, 0.0, 0.0], b.magnitude()]))
    # white: one row of kind 10
    k = fc.kernel(gpr, "white_f")
    assert k._spectral_kinds(1)[0].tolist() == [[[10 | X_, 9, 0]]]
    assert k._spectral_terms(1)[0, 0, 0, 0] == float(k.kernels[0].kernels[0].magnitude())
    # LMC scales the amplitude of kinds 9 and 10 like any first row
    k = fc.kernel(gpr, "lmc")
    kd, t, B = k._spectral_kinds(1)[0], k._spectral_terms(1), k._coreg()
    assert np.all(kd == np.array([9, 10, 0]))
    assert np.allclose(t[..., 0, 0], B[..., 0], rtol=1e-15) and np.allclose(t[..., 1, 0], B[..., 1] * k.kernels[1].magnitude(), rtol=1e-15)
    wide = k._device_terms(3)[0]
    assert np.all(wide[..., 0, 3:5] == k.kernels[0].magnitude()) and not np.any(wide[..., 1:, 3:5])
    # IndependentMultiOutputKernel: different rows per channel, the features of channel 0's leaf are columns of every point
    k = fc.kernel(gpr, "imo")
    kd = k._spectral_kinds(1)[0]
    assert kd[0, 0].tolist() == [9, 0] and kd[1, 1].tolist() == [10, 3] and kd[0, 1].tolist() == [0, 0]
    Xc = fc.data("imo")[0]
    assert k._kernel_format(Xc).shape == (115, 4) and np.array_equal(k._kernel_format(Xc)[:, :2], Xc)
    wide = k._device_terms(3)[0]
    assert np.all(wide[0, 0, 0, 3:5] == k.kernels[0].kernels[0].magnitude()) and not np.any(wide[1, 1, :, 3:5]) and not np.any(wide[0, 1])


def table_check(case):
    """the scaffold's check_table_and_kinds on the device's columns: the table of `_device_terms`, the kinds and the feature columns through
    the twin's Gram against the reference's K, K(X, Xs) and K_diag"""
    m, _, fx = kf.reference_model(FAMILY, case)
    k = m.kernel
    X, Xs = k._kernel_format(fx[case + "__X"]), k._kernel_format(fx[case + "__Xs"])
    Dd = X.shape[1] - 1
    table, kind, shape, D = k._device_terms(Dd)
    assert table.shape[3] == 2 + 3 * Dd and kind.shape == table.shape[:3] == shape.shape and shape.dtype == np.float64
    assert D == 1 and Dd == 1 + sum(f._features() for f in k._feature_leaves())
    want = kf.golden_K(FAMILY, case)
    tol = 1e-12 * max(1.0, np.max(np.abs(want)))
    K = tm.gram_from_table(table, X, kind=kind, shape=shape)
    assert np.max(np.abs(K - want)) <= tol
    assert np.max(np.abs(tm.gram_from_table(table, X, Xs, kind, shape) - fx[case + "__K12"])) <= tol
    kd = k.K_diag(fx[case + "__X"])
    assert np.max(np.abs(kd - fx[case + "__Kdiag"])) <= tol
    assert np.max(np.abs(np.diag(K) - kd)) <= tol           # what the relative jitter takes
    return K, fx


@pytest.mark.parametrize("case", full_cases(FAMILY))
def test_table_kinds_and_feature_columns_reproduce_the_reference_gram(case, monkeypatch):
    twin.install(monkeypatch)
    K, fx = table_check(case)
    if "white" in fc.CASES[case]["kern"] and "n" not in fc.CASES[case]:
        # rows 13 and 97 are the same input: a white kernel that went by distance would put its magnitude at (13, 97) as well
        assert np.array_equal(fx[case + "__X"][13], fx[case + "__X"][97]) and K[13, 13] - K[13, 97] >= 0.04


@pytest.mark.parametrize("case", full_cases(FAMILY))
def test_chain_rule_reproduces_reference_gradients(case, monkeypatch):
    twin.install(monkeypatch)
    m = kf.check_chain_rule(FAMILY, case, monkeypatch)
    assert isinstance(m._handle, twin.FunctionTableDevice) and np.any(np.isin(m._handle.kind & 0xff, (KIND_WDOT, KIND_WHITE)))
    assert m._handle.D == m.X.shape[1] - (0 if m.kernel.output_dims is None else 1) + sum(f._features() for f in m.kernel._feature_leaves())


@pytest.mark.parametrize("case", ["alone", "modulated", "seasonal", "white_f", "imo", "lmc"])
def test_predictions_over_the_twin_match_the_reference(case, monkeypatch):
    twin.install(monkeypatch)
    monkeypatch.setattr(_lib, "ExactHandle", twin.FunctionTableDevice)
    kf.check_predictions(FAMILY, case)


def test_twin_moments_are_derivatives_of_the_twins_own_gram(monkeypatch):
    """kind 9: m0 = d/dA and m1_d = d/dV_d over A; kind 10: m0 = d/dA on a block that pairs a point set with itself, nothing elsewhere; kind 5
    at D = 3: m1_0 and m3_0 -- against central differences of kinds_block's own value, alone and inside groups"""
    twin.install(monkeypatch)
    rng = np.random.default_rng(5)
    x1 = rng.uniform(0, 2, (9, 3))
    g = rng.standard_normal((9, 9))
    wd, wh, m32 = [1.3, 0.0, 0.0, 0.6, 0.9, 0, 0, 0, 0, 0, 0], [0.4, 0.0] + [0.0] * 9, [0.9, 0.0, 2.0, 0.0, 0.0, 0, 0, 0, 0, 0, 0]
    per = [0.8, 0.0, 1.4, 0.0, 0.0, 0.3, 0.0, 0.0, 0, 0, 0]
    for same in (True, False):
        for tab, kind in (([wd], [9]), ([wh], [10]), ([m32, wd], [3 | X_, 9]), ([wh, wd, m32], [10 | X_, 9 | X_, 3]), ([per, wd], [5 | X_, 9])):
            tab, kind = np.array(tab, dtype=np.float64), np.array(kind)
            shape = np.zeros(len(kind))
            x2 = x1 if same else rng.uniform(0, 2, (9, 3))
            twin._STATE["same"] = same
            try:
                K, mom = tm.kinds_block(tab, kind, shape, x1, x2, g)
                value = lambda t: np.sum(g * tm.kinds_block(t, kind, shape, x1, x2)[0])
                if 10 in kind and not same:
                    assert not np.any(K)
                for t, kd in enumerate(kind & 0xff):
                    cols = {9: [(0, 0, 1.0), (3, 3, tab[t, 0]), (4, 4, tab[t, 0])], 10: [(0, 0, 1.0)], 3: [(0, 0, 1.0)],
                            5: [(0, 0, 1.0), (2, 2, -0.5 * tab[t, 0]), (5, 8, -2.0 * np.pi * tab[t, 0])]}[int(kd)]
                    for col, slot, factor in cols:
                        up, dn = tab.copy(), tab.copy()
                        h = 1e-6
                        up[t, col] += h; dn[t, col] -= h
                        fd = (value(up) - value(dn)) / (2 * h)
                        assert abs(factor * mom[t, slot] - fd) <= 1e-7 * max(1.0, abs(fd)), (kind.tolist(), t, col, factor * mom[t, slot], fd)
                    if kd in (9, 10):
                        assert not np.any(mom[t, [1] + list(range(5, 11))]) and (kd == 9 or not np.any(mom[t, 1:]))
            finally:
                twin._STATE["same"] = False


def test_refusals_come_before_any_device_call(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "lib", no_device)
    monkeypatch.setattr(_lib, "ExactHandle", no_device)
    X, y, _ = fc.data("trend")
    Xc, yc, _ = fc.data("imo")

    def refused(kernel, match, X=X, y=y):
        m = gpr.Exact(kernel, X, y, variance=0.1)
        for call in (m.loss, m.log_marginal_likelihood, lambda: m.predict_f(X[:5]), lambda: kernel(X), lambda: kernel.K_diag(X)):
            with pytest.raises(NotImplementedError, match=match):
                call()
        assert m._handle is None
    # more columns than the device takes: one input and eight features
    wide = gpr.AddKernel(gpr.FunctionKernel(fc.feature_map(gpr, "f4")), gpr.FunctionKernel(lambda x: np.concatenate([x, x ** 2, x ** 3, x ** 4], axis=1)))
    refused(wide, r"1 input dimension and 8 features make 9 columns, the device takes 8; use fewer basis functions")
    gpr.AddKernel(gpr.FunctionKernel(fc.feature_map(gpr, "f4")), gpr.FunctionKernel(lambda x: np.concatenate([x, x ** 2, x ** 3], axis=1)))._device_terms(8)
    # the dot-product row sums over every device column, a gate row takes one
    refused(gpr.AddKernel(f2(), gpr.LinearKernel()), "put x among the features")
    refused(gpr.AddKernel(gpr.MulKernel(f2(), se()), gpr.PolynomialKernel(2)), "put x among the features")
    refused(gpr.AddKernel(f2(), gpr.ChangePointsKernel([4.0], 1.0, se(), se())), "gate rows take one input column.*inside phi")
    refused(gpr.IndependentMultiOutputKernel(f2(), gpr.LinearKernel(), output_dims=2), "put x among the features", Xc, yc)
    # enveloped rows
    env = gpr.AddKernel(gpr.MultiOutputHarmonizableSpectralKernel(output_dims=1, input_dims=1), gpr.IndependentMultiOutputKernel(f2(), output_dims=1))
    with pytest.raises(NotImplementedError, match="enveloped"):
        env(np.zeros((4, 2)))
    env = gpr.AddKernel(gpr.MultiOutputHarmonizableSpectralKernel(output_dims=1, input_dims=1), gpr.IndependentMultiOutputKernel(gpr.WhiteKernel(), output_dims=1))
    with pytest.raises(NotImplementedError, match="enveloped"):
        env(np.zeros((4, 2)))
    # the sparse and variational models and the sharded evaluation refuse both as they refuse every non-zero kind, with today's message
    sparse = dict(Titsias=dict(Z=4), Snelson=dict(Z=4), OpperArchambeau={}, SparseHensman=dict(Z=4), Hensman={})
    for name, kw in sparse.items():
        for build in (lambda: (f2(), X, y), lambda: (gpr.WhiteKernel(), X, y), lambda: (fc.kernel(gpr, "trend"), X, y), lambda: (fc.kernel(gpr, "white_se"), X, y),
                      lambda: (fc.kernel(gpr, "imo"), Xc, yc), lambda: (fc.kernel(gpr, "lmc"), Xc, yc)):
            with pytest.raises(NotImplementedError, match="%s with a non-Gaussian" % name):
                getattr(gpr, name)(*build(), **kw)

    class Comm:                                                 # what use_distributed() leaves in config.comm
        native, world, rank, force = True, 2, 0, False
    saved = getattr(gpr.config, "comm", None)
    gpr.config.comm = Comm()
    try:
        for case in ("trend", "white", "lmc"):
            m = exact(FAMILY, gpr, case)
            with pytest.raises(NotImplementedError, match="use_distributed"):
                m.loss()
            assert m._handle is None
    finally:
        gpr.config.comm = saved
    # checkpoints hold data: a FunctionKernel is refused by name, when written and when read
    pytest.importorskip("torch")
    from mogptk_amd import compat
    mm = mogptk_amd.Model(mogptk_amd.DataSet(mogptk_amd.Data(X[:, 0], y, name="a")), gpr.IndependentMultiOutputKernel(fc.kernel(gpr, "trend"), output_dims=1),
                          inference=mogptk_amd.Exact(variance=0.1))
    with pytest.raises(NotImplementedError, match="FunctionKernel.*holds code"):
        compat.dump_reference_model(mm)


class Recorder:
    """a device handle that only records what it is handed"""
    calls = []

    def __init__(self, device, X, y, C):
        Recorder.calls.append(("create", np.array(X)))

    def set_terms(self, table):
        Recorder.calls.append(("set_terms", table))

    def set_kinds(self, kind, shape):
        Recorder.calls.append(("set_kinds", kind, shape))

    def set_point_diag(self, kdiag):
        Recorder.calls.append(("set_point_diag", kdiag))

    def eval(self, *a, **k):
        raise StopIteration


def test_a_model_without_the_new_kernels_hands_over_what_it_did_before(monkeypatch):
    """the product family's `dist`, `se_cos_d2` and `imo` models: the inputs, the table and the kinds that reach the handle are the kernel's own arrays, in
    the kernels' own width -- `_kernel_format`, `_device_terms` and `_table_backward` are the identity without a FunctionKernel"""
    monkeypatch.setattr(_lib, "ExactHandle", Recorder)
    for case in ("dist", "se_cos_d2", "imo"):
        Recorder.calls = []
        m = exact("product", gpr, case)
        D = m.X.shape[1] - (0 if m.kernel.output_dims is None else 1)
        with pytest.raises(StopIteration):
            m.loss()
        got = {c[0]: c[1:] for c in Recorder.calls}
        want_X = m.X if m.kernel.output_dims is not None else np.concatenate([np.zeros((len(m.X), 1)), m.X], axis=1)
        assert np.array_equal(got["create"][0], want_X)
        table, (kind, shape) = m.kernel._spectral_terms(D), m.kernel._spectral_kinds(D)
        assert got["set_terms"][0].shape == table.shape == table.shape[:3] + (2 + 3 * D,) and np.array_equal(got["set_terms"][0], table)
        assert np.array_equal(got["set_kinds"][0], kind) and got["set_kinds"][0].dtype == kind.dtype and np.array_equal(got["set_kinds"][1], shape)
        assert "set_point_diag" not in got and m.kernel._feature_leaves() == []
        g = np.arange(table.size, dtype=np.float64).reshape(table.shape)
        seen = []
        monkeypatch.setattr(m.kernel, "_spectral_backward", lambda gt: seen.append(gt), raising=False)
        m.kernel._table_backward(g)
        assert len(seen) == 1 and seen[0] is g


def test_header_and_host_agree_on_the_kinds():
    src = open(os.path.join(ROOT, "include", "mogp_hip.h")).read()
    assert "#define MOGP_KIND_WDOT %d\n" % KIND_WDOT in src and "#define MOGP_KIND_WHITE %d\n" % KIND_WHITE in src


CHECKPOINTS = ("wm", "lmc")


@pytest.mark.parametrize("tag", CHECKPOINTS)
def test_reference_checkpoint_round_trip(tag, tmp_path):
    pytest.importorskip("torch")
    k = kf.check_checkpoint_loads(FAMILY, tag, tmp_path)
    assert "WhiteKernel" in kf.kernel_names(k)
    kf.check_checkpoint_is_written_as_the_reference_writes_it(FAMILY, tag)


@pytest.mark.parametrize("tag", CHECKPOINTS)
def test_loaded_checkpoint_evaluates_as_the_reference(tag, tmp_path, monkeypatch):
    pytest.importorskip("torch")
    from helpers import load
    twin.install(monkeypatch)
    monkeypatch.setattr(_lib, "ExactHandle", twin.FunctionTableDevice)
    fx = load(FAMILY + "_checkpoints.npz")
    (tmp_path / "ref.npy").write_bytes(fx[tag + "_file"].tobytes())
    m = mogptk_amd.LoadModel(str(tmp_path / "ref"))
    loss = float(m.gpr.loss())
    assert abs(loss - float(fx[tag + "_loss"])) <= 1e-9 * max(1.0, abs(float(fx[tag + "_loss"])))
    for i, p in enumerate(m.gpr.parameters()):
        g = fx["%s_g%d" % (tag, i)]
        if g.size:
            assert np.max(np.abs(p.grad - g)) <= 1e-9 * max(1.0, np.max(np.abs(g))), p._name
