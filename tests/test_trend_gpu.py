"""
LinearKernel, PolynomialKernel and SincKernel on the device (csrc/gram.hip: the dot-product row, kind 7, and the sinc profile, kind 6, in the
radial instantiations of the Gram and moment kernels; the per-point diagonal in the relative jitter and the prediction) against the
reference (tests/golden/trend.npz, written by tests/golden/gen_trend.py from the models of tests/trend_cases.py): Gram matrices, LML, loss,
every raw gradient, predictions, both schedules of the smallest dataflow size, bitwise repeatability, a short Adam trace, and neutrality of
the models that carry neither kind.  Tolerances: those of test_product_gpu.py, relative to max(1, max |want|).
"""
import os
import numpy as np
import pytest

import mogptk_amd
from mogptk_amd import gpr
from mogptk_amd.gpr.kernel import KIND_TIMES
import trend_cases as pc
import stationary_cases as sc
from helpers import load
from test_trend_cpu import golden_K
from test_stationary_cpu import with_reference_raw

pytestmark = pytest.mark.gpu


def err(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return np.max(np.abs(a - b)) / max(1.0, np.max(np.abs(b)))


def check_value_and_gradients(m, fx, pre):
    ps = with_reference_raw(m, fx, pre)
    lml = float(m.log_marginal_likelihood())
    e = err(lml, float(fx[pre + "lml"]))
    print(pre, "lml", e)
    assert e <= 1e-9, (lml, float(fx[pre + "lml"]))
    loss = float(m.loss())
    e = err(loss, float(fx[pre + "loss"]))
    print(pre, "loss", e)
    assert e <= 1e-9
    for i, p in enumerate(ps):
        e = err(p.grad, fx["%sp%d_grad" % (pre, i)])
        print(pre, p._name, "grad", e)
        assert e <= 1e-7, (p._name, p.grad, fx["%sp%d_grad" % (pre, i)])


@pytest.mark.parametrize("case", pc.FULL_CASES)
def test_gram_matrices_match_the_reference(case):
    fx = load("trend.npz")
    pre = case + "__"
    m = pc.exact(gpr, case)
    with_reference_raw(m, fx, pre)
    X, Xs = fx[pre + "X"], fx[pre + "Xs"]
    for name, got, want in (("K", m.kernel(X), golden_K(case)), ("K12", m.kernel(X, Xs), fx[pre + "K12"]), ("Kdiag", m.kernel.K_diag(X), fx[pre + "Kdiag"])):
        e = err(got, want)
        print(pre, name, e)
        assert e <= 1e-12, name


@pytest.mark.parametrize("case", pc.FULL_CASES)
def test_lml_loss_and_every_gradient_match_reference_autograd(case):
    check_value_and_gradients(pc.exact(gpr, case), load("trend.npz"), case + "__")


@pytest.mark.parametrize("case", pc.FULL_CASES)
def test_predictions_match_the_reference(case):
    fx = load("trend.npz")
    pre = case + "__"
    m = pc.exact(gpr, case)
    with_reference_raw(m, fx, pre)
    Xs = fx[pre + "Xs"]
    mu, var = m.predict_f(Xs)
    mu2, cov = m.predict_f(Xs, full=True)
    ymu, yvar = m.predict_y(Xs)[:2]
    for name, got, want in (("mu", mu, fx[pre + "mu"]), ("var", var, fx[pre + "var"]), ("mu(full)", mu2, fx[pre + "mu"]), ("cov", cov, fx[pre + "cov"]),
                            ("ymu", ymu, fx[pre + "ymu"]), ("yvar", yvar, fx[pre + "yvar"])):
        e = err(np.asarray(got).reshape(np.shape(want)), want)
        print(pre, name, e)
        assert e <= 1e-9, name


def test_dataflow_size_under_both_schedules():
    """N = 1100: nine 128-row tiles, the Gram build split into its head and tail launches; MOGP_FLOW is read per evaluation"""
    fx = load("trend.npz")
    old = {k: os.environ.get(k) for k in ("MOGP_FLOW", "MOGP_FLOW_MIN")}
    try:
        os.environ.pop("MOGP_FLOW", None); os.environ.pop("MOGP_FLOW_MIN", None)
        m = pc.exact(gpr, "big")
        check_value_and_gradients(m, fx, "big__")
        assert m._handle.schedule()["dataflow"], m._handle.schedule()
        os.environ["MOGP_FLOW"] = "0"
        m = pc.exact(gpr, "big")
        check_value_and_gradients(m, fx, "big__")
        assert not m._handle.schedule()["dataflow"]
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


@pytest.mark.parametrize("case", ["imo", "lmc"])
def test_repeated_gradient_evaluations_are_bit_identical(case):
    fx = load("trend.npz")
    m = pc.exact(gpr, case)
    ps = with_reference_raw(m, fx, case + "__")
    first = None
    for _ in range(30):
        loss = float(m.loss())
        got = [np.float64(loss).tobytes()] + [p.grad.tobytes() for p in ps]
        if first is None:
            first = got
        assert got == first


def test_adam_trace_through_model_train():
    fx = load("trend.npz")
    X, y, _ = pc.data(pc.ADAM_CASE)
    mm = mogptk_amd.Model(mogptk_amd.DataSet(mogptk_amd.Data(X[:, 0], y, name="a")),
                          gpr.IndependentMultiOutputKernel(pc.kernel(gpr, pc.ADAM_CASE), output_dims=1), inference=mogptk_amd.Exact(variance=pc.NOISE))
    losses, _ = mm.train(method="Adam", iters=pc.ADAM_ITERS, lr=pc.ADAM_LR, verbose=False)
    want = fx["adam__losses"]
    e = err(np.asarray(losses, dtype=np.float64), want)
    print("adam trace", e)
    assert e <= 1e-7
    final = np.concatenate([np.asarray(p.data, dtype=np.float64).reshape(-1) for p in mm.gpr.parameters()])
    assert err(final, fx["adam__final"]) <= 1e-7


def test_models_without_the_new_kinds_are_untouched():
    """Neutrality.  A SpectralMixtureKernel model makes no set_kinds call at all (the Gaussian instantiations are the parent's, instruction
    for instruction: profiles/stationary_kernels.txt) and supplies no per-point diagonal.  The stationary `sum` model of stationary_cases.py
    sends kinds 0 and 3 only: its loss still matches the reference, and repeating it gives the same bits."""
    rng = np.random.default_rng(3)
    X = np.sort(rng.uniform(0, 10, (300, 1)), axis=0)
    y = np.sin(X[:, 0]) + 0.1 * rng.standard_normal(300)
    k = gpr.SpectralMixtureKernel(Q=3, input_dims=1)
    k.magnitude.assign([0.9, 0.5, 0.7]); k.mean.assign([[0.1], [0.25], [0.4]]); k.variance.assign([[0.05], [0.02], [0.08]])
    calls, diag_calls = [], []
    real, real_diag = mogptk_amd._lib.ExactHandle.set_kinds, mogptk_amd._lib.ExactHandle.set_point_diag
    mogptk_amd._lib.ExactHandle.set_kinds = lambda self, *a: (calls.append(a), real(self, *a))[1]
    mogptk_amd._lib.ExactHandle.set_point_diag = lambda self, *a: (diag_calls.append(a), real_diag(self, *a))[1]
    try:
        m = gpr.Exact(k, X, y, variance=0.1)
        l0 = float(m.loss())
        assert not calls and np.isfinite(l0)                    # all-Gaussian, no product: not one extra call
        fx = load("stationary.npz")
        m = sc.exact(gpr, "sum")
        ps = with_reference_raw(m, fx, "sum__")
        l1 = float(m.loss())
        g1 = [p.grad.copy() for p in ps]
        assert len(calls) == 1 and not np.any(calls[0][0] & KIND_TIMES) and calls[0][0][0, 0].tolist() == [0, 3, 0]
        assert err(l1, float(fx["sum__loss"])) <= 1e-9
        l2 = float(m.loss())                                    # the same kinds again: the same bits
        assert np.float64(l1).tobytes() == np.float64(l2).tobytes() and all(g.tobytes() == p.grad.tobytes() for g, p in zip(g1, ps))
    finally:
        mogptk_amd._lib.ExactHandle.set_kinds, mogptk_amd._lib.ExactHandle.set_point_diag = real, real_diag
    assert not diag_calls
