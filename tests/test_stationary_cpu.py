"""
Host side of the stationary kernels (SquaredExponential, RationalQuadratic, Matern, Exponential), without a device: the class
surface against the reference's, the term table and kinds through the numpy twin of the device handle (oracle/table_model.py) against the
reference's K / K_diag (tests/golden/stationary.npz, written by tests/golden/gen_family.py from the models of tests/stationary_cases.py),
the chain rule against the reference's autograd with the moments taken from that twin, the combinations that are refused, and checkpoints.
The bodies shared with the other kernel families are in tests/kernel_family.py.
"""
import numpy as np
import pytest

from mogptk_amd import gpr, _lib
import stationary_cases as sc
import kernel_family as kf
from family_cases import exact, full_cases
from helpers import load

FAMILY = "stationary"


def test_class_surface_matches_the_reference():
    k = gpr.SquaredExponentialKernel()
    assert (k.order, k.input_dims) == (0, 1) and k.magnitude().shape == () and k.lengthscale().shape == (1,)
    assert gpr.SquaredExponentialKernel(order=-1, input_dims=3).lengthscale().shape == ()
    assert gpr.SquaredExponentialKernel(input_dims=3).lengthscale().shape == (3,)
    k = gpr.RationalQuadraticKernel(0.7, 0, 2)                 # alpha, order, input_dims: the reference's order of arguments
    assert (k.alpha, k.order, k.input_dims) == (0.7, 0, 2) and k.lengthscale().shape == (2,)
    assert isinstance(k.alpha, float) and not isinstance(k.alpha, gpr.Parameter)
    assert gpr.RationalQuadraticKernel().alpha == 1.0
    k = gpr.MaternKernel(1.5, 1)
    assert k.nu == 1.5 and gpr.MaternKernel().nu == 0.5
    with pytest.raises(ValueError, match="nu parameter must be 0.5, 1.5, or 2.5"):
        gpr.MaternKernel(nu=2.0)
    assert gpr.ExponentialKernel(1).lengthscale().shape == (1,)
    for k in (gpr.SquaredExponentialKernel(), gpr.RationalQuadraticKernel(), gpr.ExponentialKernel()):
        assert float(k.magnitude.lower) == float(k.lengthscale.lower) == gpr.config.positive_minimum
    k = gpr.MaternKernel()
    assert float(k.magnitude.lower) == float(k.lengthscale.lower) == 1e-6
    for k in (gpr.SquaredExponentialKernel(), gpr.RationalQuadraticKernel(), gpr.MaternKernel(), gpr.ExponentialKernel()):
        assert abs(float(k.magnitude()) - 1.0) < 2e-5 and np.all(np.abs(k.lengthscale() - 1.0) < 2e-5)      # (through the softplus link, as in the reference)
        assert [p._name.split(".")[-1] for p in k.parameters()] == ["magnitude", "lengthscale"]


@pytest.mark.parametrize("case", list(sc.CASES))
def test_parameter_order_and_printing_match_the_reference(case, capsys):
    fx = load("stationary.npz")
    m = exact(FAMILY, gpr, case)
    ps = kf.with_reference_raw(m, fx, case + "__")
    for i, p in enumerate(ps):
        ref = fx["%s__p%d_cons" % (case, i)]
        assert np.max(np.abs(np.asarray(p()) - ref)) <= 1e-14 * max(1.0, np.max(np.abs(ref))), p._name
    m.print_parameters()
    lines = capsys.readouterr().out.splitlines()[1:]
    assert [ln.split()[0] for ln in lines] == [str(n) for n in fx[case + "__names"]]


@pytest.mark.parametrize("case", full_cases(FAMILY))
def test_table_and_kinds_reproduce_the_reference_gram(case):
    _, table, kind, _, _, _, _, _ = kf.check_table_and_kinds(FAMILY, case)
    assert kind.dtype == np.int32
    assert np.all(kind[table[..., 0] == 0.0] == 0)             # padding rows are Gaussian


def test_kinds_of_the_cases():
    kinds = lambda case: sc.kernel(gpr, case)._spectral_kinds(sc.CASES[case].get("D", 1))
    assert not gpr.SquaredExponentialKernel()._radial(1) and not sc.kernel(gpr, "se_d2")._radial(2)
    assert kinds("rq")[0].tolist() == [[[1]]] and kinds("rq")[1].tolist() == [[[0.7]]]
    assert [kinds(c)[0][0, 0, 0] for c in ("m12", "m32", "m52", "exp")] == [2, 3, 4, 2]
    assert kinds("sum")[0][0, 0].tolist() == [0, 3, 0]
    kd, sh = kinds("imo")                                        # different kinds at the same t, nothing off the block diagonal
    assert kd[:, :, 0].tolist() == [[1, 0], [0, 4]] and sh[0, 0, 0] == 0.7
    kd, _ = kinds("lmc")
    assert kd.shape == (2, 2, 2) and np.all(kd[..., 0] == 0) and np.all(kd[..., 1] == 3)
    mix = gpr.MixtureKernel(gpr.MaternKernel(nu=2.5), 3)
    assert mix._spectral_kinds(1)[0][0, 0].tolist() == [4, 4, 4]


@pytest.mark.parametrize("case", full_cases(FAMILY))
def test_chain_rule_reproduces_reference_gradients(case, monkeypatch):
    kf.check_chain_rule(FAMILY, case, monkeypatch)


def test_refusals_come_before_any_device_call(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "lib", no_device)
    monkeypatch.setattr(_lib, "ExactHandle", no_device)
    for cls in (gpr.SquaredExponentialKernel, gpr.RationalQuadraticKernel):
        with pytest.raises(NotImplementedError, match="order > 0"):
            cls(order=1, input_dims=2)
    with pytest.raises(NotImplementedError, match="input_dims > 1"):
        gpr.MaternKernel(nu=1.5, input_dims=2)
    with pytest.raises(NotImplementedError, match="input_dims > 1"):
        gpr.ExponentialKernel(input_dims=2)
    for cls in (gpr.SquaredExponentialKernel, gpr.RationalQuadraticKernel, gpr.MaternKernel, gpr.ExponentialKernel):
        with pytest.raises(NotImplementedError, match="active_dims"):
            cls(active_dims=[0])
    X, y, _ = sc.data("m32")
    Xc, yc, _ = sc.data("imo")
    sparse = dict(Titsias=dict(Z=4), Snelson=dict(Z=4), OpperArchambeau={}, SparseHensman=dict(Z=4), Hensman={})
    for name, kw in sparse.items():
        for build in (lambda: (gpr.MaternKernel(nu=1.5), X, y), lambda: (gpr.RationalQuadraticKernel(), X, y), lambda: (gpr.ExponentialKernel(), X, y),
                      lambda: (gpr.SquaredExponentialKernel() + gpr.MaternKernel(nu=0.5), X, y), lambda: (sc.kernel(gpr, "imo"), Xc, yc),
                      lambda: (sc.kernel(gpr, "lmc"), Xc, yc)):
            with pytest.raises(NotImplementedError, match=name):
                getattr(gpr, name)(*build(), **kw)
        getattr(gpr, name)(gpr.SquaredExponentialKernel(), X, y, **kw)          # kind 0 is an ordinary table: accepted

    class Comm:                                                 # what use_distributed() leaves in config.comm
        native, world, rank, force = True, 2, 0, False
    saved = getattr(gpr.config, "comm", None)
    gpr.config.comm = Comm()
    try:
        m = exact(FAMILY, gpr, "m32")
        with pytest.raises(NotImplementedError, match="use_distributed"):
            m.loss()
        with pytest.raises(NotImplementedError, match="use_distributed"):
            m.predict_f(X[:5])
        assert m._handle is None
    finally:
        gpr.config.comm = saved


CHECKPOINTS = ("add", "imo", "lmc")


@pytest.mark.parametrize("tag", CHECKPOINTS)
def test_reference_checkpoint_loads(tag, tmp_path):
    pytest.importorskip("torch")
    k = kf.check_checkpoint_loads(FAMILY, tag, tmp_path)
    want = dict(add={"SquaredExponentialKernel", "MaternKernel", "RationalQuadraticKernel", "ExponentialKernel"},
                imo={"RationalQuadraticKernel", "MaternKernel"}, lmc={"SquaredExponentialKernel", "ExponentialKernel", "MaternKernel"})[tag]
    assert want <= set(kf.kernel_names(k))
    if tag == "add":
        add = k.kernels[0]
        assert add.kernels[0].order == -1 and add.kernels[1].nu == 1.5 and add.kernels[2].alpha == 0.7
    if tag == "imo":
        assert k.kernels[0].alpha == 1.3 and k.kernels[1].nu == 2.5


@pytest.mark.parametrize("tag", CHECKPOINTS)
def test_reference_checkpoint_is_written_as_the_reference_writes_it(tag):
    pytest.importorskip("torch")
    from mogptk_amd import compat
    written, fx = kf.check_checkpoint_is_written_as_the_reference_writes_it(FAMILY, tag)
    m = compat.load_reference_model(written)
    for i, p in enumerate(m.gpr.parameters()):
        assert np.max(np.abs(np.asarray(p()) - fx["%s_p%d" % (tag, i)])) <= 1e-12 * max(1.0, np.max(np.abs(fx["%s_p%d" % (tag, i)])))
