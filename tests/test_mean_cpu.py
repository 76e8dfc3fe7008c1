"""Trainable mean functions on the host (no device): the classes against the reference's surface (tests/golden/mean.npz for the
parameter lists), the affine table and its chain rule against central differences, checkpoints, and the combinations that are refused
before any device call."""
import pickle
import numpy as np
import pytest

import mogptk_amd
from mogptk_amd import gpr
import mean_cases
from helpers import load


def test_class_surface_and_argument_checks():
    c, l = gpr.ConstantMean(), gpr.LinearMean(3)
    assert [p._name for p in c.parameters()] == ["ConstantMean.bias"] and c.bias().shape == ()
    assert [p._name for p in l.parameters()] == ["LinearMean.bias", "LinearMean.slope"] and l.slope().shape == (3,)
    assert gpr.LinearMean().slope().shape == (1,)
    assert c.name() == "ConstantMean" and isinstance(c, gpr.Mean)
    with pytest.raises(ValueError, match="must pass at least one mean"):
        gpr.MultiOutputMean()
    with pytest.raises(ValueError, match="must pass means"):
        gpr.MultiOutputMean(gpr.ConstantMean(), 3)
    with pytest.raises(ValueError, match="can not nest MultiOutputMeans"):
        gpr.MultiOutputMean(gpr.MultiOutputMean(gpr.ConstantMean()))
    with pytest.raises(ValueError, match="two dimensions"):
        c(np.zeros(3))
    with pytest.raises(ValueError, match="must not be empty"):
        c(np.zeros((0, 1)))
    with pytest.raises(AttributeError):
        c.bias = gpr.Parameter(1.0)
    assert gpr.MultiOutputMean([gpr.ConstantMean(), gpr.LinearMean()]).name() == "[ConstantMean,LinearMean]"
    l.train = False
    assert not any(p.train for p in l.parameters())


def test_mean_values():
    rng = np.random.default_rng(0)
    X = np.concatenate([rng.integers(0, 3, (20, 1)).astype(float), rng.uniform(0, 5, (20, 2))], axis=1)
    c = gpr.ConstantMean(); c.bias.assign(0.7)
    assert np.array_equal(c(X), np.full((20, 1), 0.7))
    l = gpr.LinearMean(3); l.bias.assign(0.2); l.slope.assign([0.5, -1.0, 2.0])
    assert np.allclose(l(X), 0.2 + X @ np.array([[0.5], [-1.0], [2.0]]), rtol=1e-15)
    a, b = gpr.ConstantMean(), gpr.LinearMean(2)
    a.bias.assign(1.0); b.bias.assign(-1.0); b.slope.assign([0.1, 0.2])
    mom = gpr.MultiOutputMean(a, b, gpr.ConstantMean())
    want = np.where(X[:, :1] == 0, 1.0, np.where(X[:, :1] == 1, -1.0 + X[:, 1:] @ np.array([[0.1], [0.2]]), 0.0))
    assert np.allclose(mom(X), want, rtol=1e-15)                          # shuffled channels: each sub-mean on its own rows, X[:, 1:]


@pytest.mark.parametrize("case", list(mean_cases.CASES) + list(mean_cases.SPARSE_CASES))
def test_parameter_order_matches_the_reference(case):
    """registration order kernel, mean, likelihood (then the model's own, e.g. Z); Q8: no sub-mean of a MultiOutputMean is listed"""
    fx = load("mean.npz")
    m = mean_cases.exact(gpr, case) if case in mean_cases.CASES else mean_cases.sparse(gpr, case)
    names = [p._name for p in m.parameters()]
    assert names == [str(n) for n in fx[case + "__names"]]
    for s in mean_cases.sub_means(m):
        assert not any(p is q for p in s.parameters() for q in m.parameters())
    if isinstance(m.mean, gpr.MultiOutputMean):
        assert list(m.mean.parameters()) == []


def _mo(case):
    return mean_cases.CASES[case]["kern"] != "sm"


@pytest.mark.parametrize("case", ["const_sm", "const_mosm3", "lin_mosm2_d1", "lin_mosm2_d2", "mom_shuf"])
def test_affine_table_and_chain_rule(case):
    """the table reproduces m(X) point by point, and its backward is the gradient of sum_k g[c(k)] . [1, x_k] -- central differences"""
    X, _, _ = mean_cases.data(case)
    mean = mean_cases.mean(gpr, case)
    mo = _mo(case)
    C = mean_cases.CASES[case]["C"]
    D = X.shape[1] - (1 if mo else 0)
    ch = X[:, 0].astype(int) if mo else np.zeros(X.shape[0], int)
    xs = X[:, 1:] if mo else X
    t = mean._affine(C, D, mo)
    assert t.shape == (C, 1 + D)
    assert np.allclose(t[ch, 0] + np.sum(t[ch, 1:] * xs, axis=1), np.reshape(mean(X), -1), rtol=1e-14, atol=1e-14)
    rng = np.random.default_rng(3)
    g = rng.standard_normal((C, 1 + D))
    f = lambda: float(np.sum(g * mean._affine(C, D, mo)))
    holders = mean_cases.sub_means(type("M", (), {"mean": mean})) or [mean]
    params = [p for h in holders for p in h.parameters()]
    for p in params:
        p.grad = None
    mean._affine_backward(g, mo)
    for p in params:
        num = np.zeros(p.data.size)
        for i in range(p.data.size):
            old = p.data.copy()
            e = np.zeros(p.data.size); e[i] = 1e-6
            p.data = old + e.reshape(old.shape); fp = f()
            p.data = old - e.reshape(old.shape); fm = f()
            p.data = old
            num[i] = (fp - fm) / 2e-6
        assert np.allclose(np.reshape(p.grad, -1), num, rtol=1e-7, atol=1e-8), (p._name, p.grad, num)


def test_user_mean_without_backward_is_refused():
    class NoBackward(gpr.Mean):
        def __init__(self):
            super().__init__()
            self.a = gpr.Parameter(1.0)

        def mean(self, X):
            return self.a() * X[:, -1:]

    X, y, _ = mean_cases.data("lin_mosm2_d1")
    with pytest.raises(NotImplementedError, match="backward"):
        gpr.Exact(mean_cases.kernel(gpr, "lin_mosm2_d1"), X, y, mean=NoBackward())
    assert mean_cases.poly_mean(gpr)._has_backward()


def test_trainable_mean_refusals_come_before_any_device_call():
    X, y, _ = mean_cases.data("lin_mosm2_d1")
    k = lambda: mean_cases.kernel(gpr, "lin_mosm2_d1")
    for cls in (gpr.Hensman, gpr.OpperArchambeau):
        with pytest.raises(NotImplementedError, match=cls.__name__):
            cls(k(), X, y, mean=gpr.ConstantMean())
    with pytest.raises(NotImplementedError, match="SparseHensman"):
        gpr.SparseHensman(k(), X, y, Z=4, mean=gpr.ConstantMean())
    fixed = lambda Z: 0.1 * np.ones(len(Z))                    # fixed means keep today's behaviour
    gpr.Hensman(k(), X, y, mean=fixed)
    gpr.OpperArchambeau(k(), X, y, mean=fixed)

    class Comm:                                                 # what use_distributed() leaves in config.comm (no device touched)
        native, world, rank, force = True, 2, 0, False
    saved = getattr(gpr.config, "comm", None)
    gpr.config.comm = Comm()
    try:
        for build in (lambda: gpr.Exact(k(), X, y, mean=gpr.ConstantMean()),
                      lambda: gpr.Titsias(k(), X, y, Z=4, mean=gpr.LinearMean(2)),
                      lambda: gpr.Snelson(k(), X, y, Z=4, mean=gpr.ConstantMean())):
            m = build()
            with pytest.raises(NotImplementedError, match="use_distributed"):
                m.loss()
            assert m._handle is None
    finally:
        gpr.config.comm = saved


@pytest.mark.parametrize("case", ["const_mosm3", "lin_mosm2_d2", "mom_shuf", "const_sm"])
def test_checkpoint_round_trip(case, tmp_path):
    """the package's own checkpoint: the restricted loader admits the built-in means, values and the Q8 structure survive"""
    from mogptk_amd import compat          # (imported here, as the other checkpoint tests do: compat's writer copies the pickler's dispatch table on import)
    m = mean_cases.exact(gpr, case)
    m2 = compat.load_native_model(pickle.dumps(m))
    assert type(m2.mean) is type(m.mean)
    for a, b in zip(m.parameters(), m2.parameters()):
        assert a._name == b._name and np.array_equal(a.data, b.data)
    for a, b in zip(mean_cases.sub_means(m), mean_cases.sub_means(m2)):
        assert type(a) is type(b) and all(np.array_equal(p.data, q.data) for p, q in zip(a.parameters(), b.parameters()))
    assert np.array_equal(m.mean(m.X), m2.mean(m2.X))
    if isinstance(m2.mean, gpr.MultiOutputMean):
        assert list(m2.mean.parameters()) == []


def test_wrapper_takes_a_mean_and_prints_it(capsys):
    rng = np.random.default_rng(2)
    x = np.sort(rng.uniform(0, 10, 30))
    mean = gpr.ConstantMean()
    m = mogptk_amd.SM(mogptk_amd.Data(x, np.sin(x) + 1.0), Q=1, mean=mean)
    assert m.gpr.mean is mean
    assert "‣ Mean: ConstantMean" in str(m)
    assert "ConstantMean.bias" in [p._name for p in m.gpr.parameters()]


MEAN_CHECKPOINTS = ("const", "linear", "mom", "mom_titsias")


@pytest.mark.parametrize("tag", MEAN_CHECKPOINTS)
def test_reference_checkpoint_with_a_mean_loads(tag, tmp_path):
    """bytes the reference's Model.save() wrote with each built-in mean load without the reference: values, bounds, train flags, the
    sub-means of a MultiOutputMean outside the parameter list (Q8) with their values"""
    pytest.importorskip("torch")
    fx = load("mean_checkpoints.npz")
    (tmp_path / "ref.npy").write_bytes(fx[tag + "_file"].tobytes())
    m = mogptk_amd.LoadModel(str(tmp_path / "ref"))
    ps = list(m.gpr.parameters())
    assert [p._name for p in ps] == [str(n) for n in fx[tag + "_names"]]
    for i, p in enumerate(ps):
        ref = fx["%s_p%d" % (tag, i)]
        assert np.max(np.abs(np.asarray(p()) - ref)) <= 1e-12 * max(1.0, np.max(np.abs(ref))), p._name
        assert bool(p.train) == bool(fx["%s_train%d" % (tag, i)]), p._name
    assert isinstance(m.gpr.mean, gpr.Mean)
    if tag == "linear":
        assert m.gpr.mean.bias.lower == -1.0 and m.gpr.mean.bias.upper == 1.0 and not m.gpr.mean.slope.train
    for j, s in enumerate(mean_cases.sub_means(m.gpr)):
        assert not any(p is q for p in s.parameters() for q in ps)
        for i, p in enumerate(s.parameters()):
            assert np.array_equal(np.asarray(p()), fx["%s_sub%d_p%d" % (tag, j, i)])


@pytest.mark.parametrize("tag", MEAN_CHECKPOINTS)
def test_reference_checkpoint_with_a_mean_is_written_as_the_reference_writes_it(tag, tmp_path):
    """read back and written in the reference's layout (compat.dump_reference_model): the same object tree as the reference's own file"""
    pytest.importorskip("torch")
    import io
    from mogptk_amd import compat
    from test_host_logic import _checkpoint_tree, _tree_differences
    fx = load("mean_checkpoints.npz")
    raw = fx[tag + "_file"].tobytes()
    written = compat.dump_reference_model(compat.load_reference_model(raw))
    assert compat.is_reference_checkpoint(written)
    theirs = _checkpoint_tree(compat._Unpickler(io.BytesIO(raw)).load(), {})
    ours = _checkpoint_tree(compat._Unpickler(io.BytesIO(written)).load(), {})
    out = []
    _tree_differences(theirs, ours, tag, out)
    assert not out, out[:5]
    m = compat.load_reference_model(written)                 # and it reads back with the same values
    for i, p in enumerate(m.gpr.parameters()):
        assert np.max(np.abs(np.asarray(p()) - fx["%s_p%d" % (tag, i)])) <= 1e-12 * max(1.0, np.max(np.abs(fx["%s_p%d" % (tag, i)])))


def test_user_mean_is_not_written_in_the_reference_layout(tmp_path):
    from mogptk_amd import compat
    rng = np.random.default_rng(2)
    x = np.sort(rng.uniform(0, 10, 30))
    m = mogptk_amd.SM(mogptk_amd.Data(x, np.sin(x)), Q=1, mean=mean_cases.poly_mean(gpr))
    with pytest.raises(NotImplementedError, match="PolynomialMean"):
        compat.dump_reference_model(m)
