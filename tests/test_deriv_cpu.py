"""
The posterior of df/dx without a device: gpr.Exact.predict_df -- the host's prior variance kappa, chunking, the mean's slope, the
refusals -- over the numpy twin (tests/deriv_twin.py) against the reference-side goldens (tests/golden/deriv.npz, gen_deriv.py: torch autograd
of the reference's own kernel objects), and the public surface.  Tolerances, relative to max(1, max |want|): 1e-9 for dmu and dvar
(what test_parts_cpu.py holds predict_parts to), 1e-10 for kappa, 1e-12 for the Jacobian's entries.
"""
import numpy as np
import pytest

import mogptk_amd
from mogptk_amd import gpr, _lib
from mogptk_amd.gpr.config import config

import deriv_cases
import deriv_twin
from helpers import load
from kernel_family import err, with_reference_raw

FX = load("deriv.npz")
TOL = 1e-9


def model(case):
    m = deriv_cases.exact(gpr, case)
    with_reference_raw(m, FX, case + "__")
    return m, deriv_cases.data(case)[2]


def check_case(case):
    """predict_df against the golden; every stored point is compared"""
    pre = case + "__"
    m, Xs = model(case)
    dmu, dvar = m.predict_df(Xs)
    S, D = FX[pre + "dmu"].shape
    assert dmu.shape == dvar.shape == (S, D) == (len(Xs), deriv_cases.CASES[case]["D"]) and dmu.dtype == dvar.dtype == config.dtype
    for name, got in (("dmu", dmu), ("dvar", dvar)):
        e = err(got, FX[pre + name])
        print(pre, name, e)
        assert e <= TOL, name
    return m, Xs, dmu, dvar


@pytest.mark.parametrize("case", list(deriv_cases.CASES))
def test_twin_matches_the_reference(case, monkeypatch):
    deriv_twin.install(monkeypatch)
    m, Xs, dmu, dvar = check_case(case)
    h = m._handle
    assert isinstance(h, deriv_twin.DerivTableDevice)
    J = deriv_twin.jacobian_from_table(h.table, m.kernel._kernel_format(Xs)[:deriv_cases.KROWS], h.X, h.kind, h.shape)
    e = err(J, FX[case + "__J"])
    print(case, "J", e)
    assert e <= 1e-12
    if deriv_cases.CASES[case].get("coincide"):              # test point 3 is training point 13: r = 0, J = 0
        assert np.all(J[3, 13] == 0.0) and np.any(J[3] != 0.0)


@pytest.mark.parametrize("case", list(deriv_cases.CASES))
def test_host_kappa_matches_the_reference(case, monkeypatch):
    seen = []
    deriv_twin.install(monkeypatch)
    real = deriv_twin.DerivTableDevice.predict_grad
    monkeypatch.setattr(deriv_twin.DerivTableDevice, "predict_grad", lambda self, nv, j, kap, X, **kw: (seen.append(np.array(kap)), real(self, nv, j, kap, X, **kw))[1])
    m, Xs = model(case)
    m.predict_df(Xs)
    assert len(seen) == 1 and seen[0].shape == FX[case + "__kappa"].T.shape
    e = err(seen[0].T, FX[case + "__kappa"])
    print(case, "kappa", e)
    assert e <= 1e-10


def test_test_points_are_taken_in_chunks(monkeypatch):
    deriv_twin.install(monkeypatch)
    m, Xs = model("sm3")                                      # D = 3, S = 24: 72 stacked rows
    dmu, dvar = m.predict_df(Xs)
    calls = []
    real = deriv_twin.DerivTableDevice.predict_grad
    monkeypatch.setattr(deriv_twin.DerivTableDevice, "predict_grad", lambda self, nv, j, kap, X, **kw: (calls.append((kap.shape, X.shape[0])), real(self, nv, j, kap, X, **kw))[1])
    m.PART_ROWS = 30                                          # lowered on the instance: 10 points per call
    dmu2, dvar2 = m.predict_df(Xs)
    assert calls == [((3, 10), 10), ((3, 10), 10), ((3, 4), 4)] and all(k[0] * S <= 30 for k, S in calls)
    assert dmu2.shape == dmu.shape and np.array_equal(dmu2, dmu) and np.array_equal(dvar2, dvar)
    assert gpr.Exact.PART_ROWS == 65536


def test_the_slope_of_the_mean_is_added(monkeypatch):
    """`linmean` is `m32cos`'s kernel, unchanged, under a LinearMean: the device sees the residual, the host adds the slope"""
    deriv_twin.install(monkeypatch)
    m, Xs = model("linmean")
    dmu, dvar = m.predict_df(Xs)
    h = m._handle
    raw, _ = h.predict_grad(m._noise_var(), m.jitter, FX["linmean__kappa"].T.copy(), m.kernel._kernel_format(Xs))
    assert np.array_equal(dmu, raw.T + deriv_cases.SLOPE) and err(dmu, FX["linmean__dmu"]) <= TOL
    c = gpr.ConstantMean()
    c.bias.assign(0.7)
    X, y, _ = deriv_cases.data("m32cos")
    m2 = gpr.Exact(deriv_cases.kernel(gpr, "m32cos"), X, y, variance=deriv_cases.NOISE, mean=c)
    m3 = gpr.Exact(deriv_cases.kernel(gpr, "m32cos"), X, y - 0.7, variance=deriv_cases.NOISE)
    assert err(m2.predict_df(Xs)[0], m3.predict_df(Xs)[0]) <= 1e-12      # a constant has no slope


def test_loss_and_gradients_are_unchanged_by_a_derivative_call(monkeypatch):
    deriv_twin.install(monkeypatch)
    m, Xs = model("linmean")
    ps = list(m.parameters())

    def lml_loss():
        loss = float(m.loss())
        return [np.float64(loss).tobytes()] + [p.grad.tobytes() for p in ps if p.grad is not None]

    before = lml_loss()
    m.predict_df(Xs)
    assert lml_loss() == before and len(before) > 1


# ---- refusals and the public surface -----------------------------------------------------------------------------------------------------
class NoDevice:
    def __init__(self, *a, **k):
        raise AssertionError("a device handle was created")


def _exact(kernel, **kw):
    rng = np.random.default_rng(3)
    X = rng.uniform(0, 10, (30, 1))
    return gpr.Exact(kernel, X, np.sin(X[:, 0]), variance=0.1, **kw), X[:5]


@pytest.mark.parametrize("name, make, match", [
    ("matern12", lambda: gpr.MaternKernel(nu=0.5, input_dims=1), "Matern 1/2.*not differentiable"),
    ("exponential", lambda: gpr.AddKernel(gpr.SquaredExponentialKernel(input_dims=1), gpr.ExponentialKernel(input_dims=1)), "Matern 1/2.*not differentiable"),
    ("white", lambda: gpr.AddKernel(gpr.SquaredExponentialKernel(input_dims=1), gpr.WhiteKernel(input_dims=1)), "white.*not differentiable"),
    ("gate", lambda: gpr.ChangePointsKernel([5.0], 1.0, gpr.SquaredExponentialKernel(input_dims=1), gpr.MaternKernel(nu=1.5, input_dims=1)), "gate.*yet"),
    ("function", lambda: gpr.AddKernel(gpr.FunctionKernel(lambda x: np.concatenate([x, x * x], axis=1), input_dims=1), gpr.SquaredExponentialKernel(input_dims=1)),
     "FunctionKernel.*yet"),
])
def test_rows_without_a_derivative_are_refused_by_name(name, make, match, monkeypatch):
    monkeypatch.setattr(_lib, "ExactHandle", NoDevice)        # before any device call
    m, Xs = _exact(make())
    with pytest.raises(NotImplementedError, match=match):
        m.predict_df(Xs)


def test_the_twin_refuses_what_the_library_refuses(monkeypatch):
    """past the host's refusal, as a caller of the handle would come: kinds 2 and 10 are MOGP_EINVAL"""
    deriv_twin.install(monkeypatch, "function")
    for kern in (gpr.MaternKernel(nu=0.5, input_dims=1), gpr.AddKernel(gpr.SquaredExponentialKernel(input_dims=1), gpr.WhiteKernel(input_dims=1))):
        m, Xs = _exact(kern)
        m.predict_f(Xs)
        with pytest.raises(_lib.MogpError) as e:
            m._handle.predict_grad(m._noise_var(), m.jitter, np.ones((1, 5)), m.kernel._kernel_format(Xs))
        assert e.value.code == _lib.MOGP_EINVAL


def test_a_mean_that_is_not_affine_is_refused_by_name(monkeypatch):
    monkeypatch.setattr(_lib, "ExactHandle", NoDevice)

    class Wave(gpr.Mean):
        def mean(self, X):
            return np.sin(X[:, :1])

    m, Xs = _exact(gpr.SquaredExponentialKernel(input_dims=1), mean=Wave())
    with pytest.raises(NotImplementedError, match="Wave is not affine"):
        m.predict_df(Xs)

    def bump(X):
        return np.cos(X[:, :1])

    m, Xs = _exact(gpr.SquaredExponentialKernel(input_dims=1), mean=bump)
    with pytest.raises(NotImplementedError, match="bump is not affine"):
        m.predict_df(Xs)


def test_sharded_evaluation_is_refused_before_any_device_call(monkeypatch):
    monkeypatch.setattr(_lib, "ExactHandle", NoDevice)
    monkeypatch.setattr(config, "comm", type("Comm", (), dict(world=2, rank=0, force=False, native=True))(), raising=False)
    m = deriv_cases.exact(gpr, "ard")
    with pytest.raises(NotImplementedError, match="use_distributed"):
        m.predict_df(deriv_cases.data("ard")[2])


def test_other_models_have_no_derivative():
    import stationary_cases as sc
    X, y, _ = sc.data("se0")
    k = lambda: sc.kernel(gpr, "se0")
    for m in (gpr.Titsias(k(), X, y, Z=5), gpr.Snelson(k(), X, y, Z=5), gpr.OpperArchambeau(k(), X, y), gpr.Hensman(k(), X, y),
              gpr.SparseHensman(k(), X, y, Z=5)):
        assert not hasattr(m, "predict_df"), m.name()
    mm = mogptk_amd.Model(mogptk_amd.DataSet(mogptk_amd.Data(X[:, 0], y, name="a")), gpr.IndependentMultiOutputKernel(k(), output_dims=1),
                          inference=mogptk_amd.Titsias(inducing_points=5))
    with pytest.raises(ValueError, match="exact inference"):
        mm.predict_derivative()
    import inspect
    assert "full" not in inspect.signature(gpr.Exact.predict_df).parameters      # no covariance between derivatives


def test_model_predict_derivative_on_two_channels(monkeypatch):
    deriv_twin.install(monkeypatch)
    rng = np.random.default_rng(5)
    xa, xb = np.sort(rng.uniform(0, 10, 40)), np.sort(rng.uniform(0, 10, 30))
    ds = mogptk_amd.DataSet(mogptk_amd.Data(xa, np.sin(xa) + 0.1 * rng.standard_normal(40), name="a"),
                            mogptk_amd.Data(xb, np.cos(xb) + 0.1 * rng.standard_normal(30), name="b"))
    mm = mogptk_amd.Model(ds, gpr.MultiOutputSpectralMixtureKernel(Q=2, output_dims=2, input_dims=1), inference=mogptk_amd.Exact(variance=0.1))
    Xp = [np.linspace(0, 10, 12)[:, None], np.linspace(1, 9, 7)[:, None]]
    X, dmu, lower, upper = mm.predict_derivative(Xp, sigma=3)
    assert len(X) == len(dmu) == len(lower) == len(upper) == 2
    assert [v.shape for v in dmu] == [(12, 1), (7, 1)] == [v.shape for v in lower] == [v.shape for v in upper]
    g_mu, g_var = mm.gpr.predict_df(mm._to_kernel_format(X))
    assert np.array_equal(np.concatenate(dmu), g_mu)
    assert np.array_equal(np.concatenate(lower), g_mu - 3 * np.sqrt(g_var)) and np.array_equal(np.concatenate(upper), g_mu + 3 * np.sqrt(g_var))
    # the slope of the latent mean in transformed space: the central difference of predict_f, to the difference's own error (h^2 f''' / 6)
    Xk, h = mm._to_kernel_format(X), 1e-4
    P, M = Xk.copy(), Xk.copy()
    P[:, 1] += h
    M[:, 1] -= h
    fd = (mm.gpr.predict_f(P)[0] - mm.gpr.predict_f(M)[0]) / (2 * h)
    assert np.max(np.abs(fd - g_mu)) <= 1e-6 * max(1.0, np.max(np.abs(g_mu)))
    X2, dmu2, _, _ = mm.predict_derivative()                  # the data set's own prediction inputs
    assert [len(v) for v in dmu2] == [len(x) for x in X2]
