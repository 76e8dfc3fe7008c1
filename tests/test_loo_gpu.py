"""
The leave-one-out predictive likelihood on the device (mogp_exact_loo: csrc/loo.hip, the dense symmetric form of the radial moment kernel in
csrc/gram.hip) against the reference-side goldens (tests/golden/loo.npz, gen_loo.py) over the cases of tests/loo_cases.py: value, per-point
mean and variance 1e-9, every raw gradient 1e-7, relative to max(1, max |want|).  The numpy twin's own error against the same
goldens is printed beside each case: it is the float64 floor, and a case whose floor is above a tenth of a tolerance is a badly
conditioned case, not a loose kernel.  Then: bitwise repeatability, both schedules of the smallest dataflow size, the completeness of the
inverse where the marginal likelihood's gradient forms a band of it, no state left behind for the marginal likelihood, the workspace's
ownership, and a short Adam trace on the LOO loss.
"""
import os
import numpy as np
import pytest

from mogptk_amd import gpr, _lib
import kernel_family as kf
import loo_cases
import loo_twin
from helpers import load
from test_loo_cpu import FX, check_case, check_loo_adam_trace, model_at_reference_raw

pytestmark = pytest.mark.gpu


def twin_floor(case):
    """the twin's largest error against the case's goldens: (value / mu / var, gradients)"""
    with pytest.MonkeyPatch.context() as mp:
        loo_twin.install(mp, loo_cases.twin_kind(case))
        m, ps = model_at_reference_raw(case)
        pre = case + "__"
        ev = kf.err(float(m.loo_loss()), float(FX[pre + "loss"]))
        if not loo_cases.CASES[case].get("light"):
            mu, var = m.loo()
            ev = max(ev, kf.err(mu.reshape(-1), FX[pre + "mu"]), kf.err(var.reshape(-1), FX[pre + "var"]))
        eg = max(kf.err(p.grad, FX["%sp%d_grad" % (pre, i)]) for i, p in enumerate(ps))
    return ev, eg


@pytest.mark.parametrize("case", list(loo_cases.CASES))
def test_value_predictions_and_every_gradient_match_the_reference(case):
    ev, eg = twin_floor(case)
    print(case, "float64 floor (numpy twin against the goldens): value", ev, "gradients", eg, "cond", float(FX[case + "__cond"]))
    assert ev <= 1e-10 and eg <= 1e-8, "the case is too badly conditioned for the tolerances: change its inputs"
    m = check_case(case, 1e-9, 1e-7)
    assert isinstance(m._handle, _lib.ExactHandle)
    assert m._handle.inverse_fraction() == 1.0


def test_repeated_evaluations_are_bit_identical():
    m, ps = model_at_reference_raw("three")
    first = None
    for _ in range(30):
        loss = float(m.loo_loss())
        got = [np.float64(loss).tobytes()] + [p.grad.tobytes() for p in ps]
        first = first or got
        assert got == first
    mu, var = m.loo()
    mu2, var2 = m.loo()
    assert mu.tobytes() == mu2.tobytes() and var.tobytes() == var2.tobytes()


def test_dataflow_size_under_both_schedules():
    """N = 1100; MOGP_FLOW is read per evaluation"""
    old = {k: os.environ.get(k) for k in ("MOGP_FLOW", "MOGP_FLOW_MIN")}
    try:
        os.environ.pop("MOGP_FLOW", None); os.environ.pop("MOGP_FLOW_MIN", None)
        m = check_case("big", 1e-9, 1e-7)
        assert m._handle.schedule()["dataflow"], m._handle.schedule()
        os.environ["MOGP_FLOW"] = "0"
        m = check_case("big", 1e-9, 1e-7)
        assert not m._handle.schedule()["dataflow"]
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


def test_the_inverse_is_complete_where_the_marginal_likelihood_forms_a_band():
    m = loo_cases.banded(gpr)
    m.loss()
    h = m._handle
    assert h.inverse_fraction() < 1.0, "the case no longer has a banded inverse: lengthen the series"
    m.loo_loss()
    assert h.inverse_fraction() == 1.0
    got = h.fetch(1)
    with pytest.MonkeyPatch.context() as mp:
        loo_twin.install(mp)
        t = loo_cases.banded(gpr)
        t.loo_log_likelihood()
        want = t._handle.fetch(1)
    e = kf.err(got, want)
    print("complete inverse", e, "largest entry", np.max(np.abs(want)))
    assert e <= 1e-9
    m.loss()                                     # and the band is back for the marginal likelihood
    assert h.inverse_fraction() < 1.0


@pytest.mark.parametrize("case", ["sum", "mosm", "big"])
def test_loo_leaves_no_state_behind_for_the_marginal_likelihood(case):
    m, ps = model_at_reference_raw(case)

    def lml_bits():
        loss = float(m.loss())
        return [np.float64(loss).tobytes()] + [p.grad.tobytes() for p in ps]

    before = lml_bits()
    m.loo_loss()
    assert lml_bits() == before
    m.loo_log_likelihood()
    assert lml_bits() == before
    mu, var = m.predict_f(m.X[:7])
    m.loo_loss()
    mu2, var2 = m.predict_f(m.X[:7])
    assert mu.tobytes() == mu2.tobytes() and var.tobytes() == var2.tobytes()


def test_the_workspace_belongs_to_handles_that_ask_for_it():
    m, _ = model_at_reference_raw("sum")
    m.loss(); m.predict_f(m.X[:5]); m.log_marginal_likelihood()
    h = m._handle
    assert h.loo_bytes() == 0
    m.loo_log_likelihood()
    vectors = h.loo_bytes()
    assert 0 < vectors < 8 * 256 * 256                         # without gradients: the per-point vectors alone
    m.loo_loss()
    assert h.loo_bytes() == vectors + 8 * 256 * 256            # N = 150 pads to 256: one N x N matrix
    m.loo_loss()
    assert h.loo_bytes() == vectors + 8 * 256 * 256


def test_mean_gradient_vector_is_minus_rho():
    """mogp_model_fetch(3) after a LOO gradient evaluation: dL/dr, which a user mean's backward takes"""
    m, _ = model_at_reference_raw("m32")
    m.loo_loss()
    got = m._handle.fetch(3)
    with pytest.MonkeyPatch.context() as mp:
        loo_twin.install(mp)
        t, _ = model_at_reference_raw("m32")
        t.loo_loss()
        want = t._handle.fetch(3)
    assert kf.err(got, want) <= 1e-9
    m.loo_log_likelihood()                                     # any later evaluation ends it
    with pytest.raises(_lib.MogpError):
        m._handle.fetch(3)


def test_adam_trace_on_the_loo_loss():
    check_loo_adam_trace()
