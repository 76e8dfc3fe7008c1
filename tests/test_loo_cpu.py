"""
The leave-one-out predictive likelihood without a device: gpr.Exact's LOO path -- push, kinds, per-point diagonal, moments -> table
gradient, the jitter term, noise and mean -- over the numpy twin (tests/loo_twin.py) against the reference-side goldens
(tests/golden/loo.npz, gen_loo.py), and the public surface.  Tolerances: DESIGN 8, relative to max(1, max |want|).
"""
import numpy as np
import pytest

import mogptk_amd
from mogptk_amd import gpr
from mogptk_amd.gpr.config import config

import loo_cases
import loo_twin
from family_cases import cases
from helpers import load
from kernel_family import err, with_reference_raw, check_adam_trace

FX = load("loo.npz")


def model_at_reference_raw(case):
    m, (fx, pre) = loo_cases.exact(gpr, case)
    return m, with_reference_raw(m, fx, pre)


def check_case(case, tol_value, tol_grad):
    """value, per-point predictions and every gradient of `case` on whatever device handle the model gets; -> the model"""
    pre = case + "__"
    m, ps = model_at_reference_raw(case)
    L = float(m.loo_log_likelihood())
    e = err(L, float(FX[pre + "loo"]))
    print(pre, "loo", e)
    assert e <= tol_value, (L, float(FX[pre + "loo"]))
    if not loo_cases.CASES[case].get("light"):
        mu, var = m.loo()
        assert mu.shape == var.shape == (m.X.shape[0], 1) and mu.dtype == var.dtype == config.dtype
        for name, got in (("mu", mu), ("var", var)):
            e = err(got.reshape(-1), FX[pre + name])
            print(pre, name, e)
            assert e <= tol_value, name
    loss = float(m.loo_loss())
    e = err(loss, float(FX[pre + "loss"]))
    print(pre, "loss", e)
    assert e <= tol_value
    for i, p in enumerate(ps):
        g = FX["%sp%d_grad" % (pre, i)]
        e = err(p.grad, g)
        print(pre, p._name, "grad", e)
        assert e <= tol_grad, (p._name, p.grad, g)
    return m


@pytest.mark.parametrize("case", list(loo_cases.CASES))
def test_twin_matches_the_reference(case, monkeypatch):
    loo_twin.install(monkeypatch, loo_cases.twin_kind(case))
    m = check_case(case, 1e-9, 1e-9)
    h = m._handle
    assert isinstance(h, loo_twin.LooTableDevice)
    assert (h.kind is not None) == any(k._radial(h.D) for k in [m.kernel])      # the kinds travelled where the kernel has some


def test_loss_is_unchanged_and_loo_leaves_nothing_behind(monkeypatch):
    """the marginal likelihood's loss and gradients against the family's own golden, before and after LOO evaluations on the same model"""
    loo_twin.install(monkeypatch)
    m, ps = model_at_reference_raw("sum")
    fx = load("stationary.npz")

    def lml_loss():
        loss = float(m.loss())
        assert err(loss, float(fx["sum__loss"])) <= 1e-9
        for i, p in enumerate(ps):
            assert err(p.grad, fx["sum__p%d_grad" % i]) <= 1e-9
        return [np.float64(loss).tobytes()] + [p.grad.tobytes() for p in ps]

    before = lml_loss()
    m.loo_loss(); m.loo(); m.loo_log_likelihood()
    assert lml_loss() == before


def test_loo_loss_zeroes_the_gradients_first(monkeypatch):
    loo_twin.install(monkeypatch)
    m, ps = model_at_reference_raw("m32")
    m.loo_loss()
    first = [p.grad.copy() for p in ps]
    m.loo_loss()
    assert all(np.array_equal(a, p.grad) for a, p in zip(first, ps))


def test_sharded_evaluation_is_refused_before_any_device_call(monkeypatch):
    class NoDevice:
        def __init__(self, *a, **k):
            raise AssertionError("a device handle was created")

    from mogptk_amd import _lib
    monkeypatch.setattr(_lib, "ExactHandle", NoDevice)
    monkeypatch.setattr(config, "comm", type("Comm", (), dict(world=2, rank=0, force=False, native=True))(), raising=False)
    m, _ = loo_cases.exact(gpr, "m32")
    for call in (m.loo, m.loo_log_likelihood, m.loo_loss):
        with pytest.raises(NotImplementedError, match="sharded"):
            call()


def test_other_models_have_no_loo():
    sc = cases("stationary")
    X, y, _ = sc.data("se0")
    for m in (gpr.Titsias(sc.kernel(gpr, "se0"), X, y, Z=5), gpr.Snelson(sc.kernel(gpr, "se0"), X, y, Z=5),
              gpr.OpperArchambeau(sc.kernel(gpr, "se0"), X, y), gpr.Hensman(sc.kernel(gpr, "se0"), X, y)):
        for name in ("loo", "loo_log_likelihood", "loo_loss"):
            assert not hasattr(m, name), (m.name(), name)
    mm = mogptk_amd.Model(mogptk_amd.DataSet(mogptk_amd.Data(X[:, 0], y, name="a")), gpr.IndependentMultiOutputKernel(sc.kernel(gpr, "se0"), output_dims=1),
                          inference=mogptk_amd.Titsias(inducing_points=5))
    with pytest.raises(ValueError, match="exact inference"):
        mm.train(method="Adam", iters=1, objective="loo")
    with pytest.raises(ValueError, match="exact inference"):
        mm.loo_log_likelihood()
    with pytest.raises(ValueError, match="objective"):
        mm.train(method="Adam", iters=1, objective="elbo")


def adam_model():
    c = loo_cases.CASES[loo_cases.ADAM_CASE]
    sc = cases(c["family"])
    X, y, _ = sc.data(c["case"])
    return mogptk_amd.Model(mogptk_amd.DataSet(mogptk_amd.Data(X[:, 0], y, name="a")),
                            gpr.IndependentMultiOutputKernel(sc.kernel(gpr, c["case"]), output_dims=1), inference=mogptk_amd.Exact(variance=sc.NOISE))


def check_loo_adam_trace():
    mm = adam_model()
    assert err(mm.loo_log_likelihood(), float(FX[loo_cases.ADAM_CASE + "__loo"])) <= 1e-9
    losses, _ = mm.train(method="Adam", iters=loo_cases.ADAM_ITERS, lr=loo_cases.ADAM_LR, verbose=False, objective="loo")
    want = FX["adam__losses"]
    e = err(np.asarray(losses, dtype=np.float64), want)
    print("loo adam trace", e)
    assert e <= 1e-7
    assert losses[-1] < losses[0]
    final = np.concatenate([np.asarray(p.data, dtype=np.float64).reshape(-1) for p in mm.gpr.parameters()])
    assert err(final, FX["adam__final"]) <= 1e-7


def test_train_with_the_loo_objective_follows_the_reference_side_trace(monkeypatch):
    loo_twin.install(monkeypatch)
    check_loo_adam_trace()


@pytest.mark.parametrize("method", ["LBFGS", "SGD", "AdaGrad"])
def test_every_optimiser_takes_the_loo_closure(method, monkeypatch):
    loo_twin.install(monkeypatch)
    mm = adam_model()
    calls = []
    real = gpr.Exact.loo_loss
    monkeypatch.setattr(gpr.Exact, "loo_loss", lambda self: (calls.append(1), real(self))[1])
    monkeypatch.setattr(gpr.Exact, "loss", lambda self: pytest.fail("the LML loss was evaluated under objective='loo'"))
    losses, _ = mm.train(method=method, iters=3, lr=1e-3, objective="loo")
    assert len(calls) >= 4 and np.all(np.isfinite(losses[:4]))


def test_the_default_objective_is_the_marginal_likelihood(monkeypatch):
    """objective='lml', spelled out, reproduces the family's Adam golden; train() without it is checked by the families' own tests"""
    import inspect
    assert inspect.signature(mogptk_amd.Model.train).parameters["objective"].default == "lml"
    loo_twin.install(monkeypatch)
    real = mogptk_amd.Model.train
    monkeypatch.setattr(mogptk_amd.Model, "train", lambda self, *a, **k: real(self, *a, objective="lml", **k))
    check_adam_trace("stationary")
