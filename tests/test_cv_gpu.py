"""
Leave-fold-out cross-validation on the device (mogp_exact_cv: csrc/lfo.hip, with csrc/loo.hip's adjoint and moment pass behind it) against the
reference-side goldens (tests/golden/cv.npz, gen_cv.py) over the cases and fold layouts of tests/cv_cases.py: value, held-out mean and variance
1e-9, every raw gradient 1e-7, relative to max(1, max |want|) (the leave-one-out figures).  The numpy twin's own error against the
same goldens is printed beside each case: it is the float64 floor.  Then: both schedules of the smallest dataflow size, bitwise repeatability,
no state left behind for the marginal likelihood, the workspace's ownership, one-point folds against mogp_exact_loo, and the device's own
refusal of folds the host would never send.
"""
import os
import numpy as np
import pytest

from mogptk_amd import _lib
import kernel_family as kf
import cv_cases
import cv_twin
import loo_cases
from test_cv_cpu import FX, check_case, check_cv_adam_trace, model_at_reference_raw

pytestmark = pytest.mark.gpu


def twin_floor(case, name):
    """the twin's largest error against the goldens of (case, layout): (value / mu / var, gradients)"""
    with pytest.MonkeyPatch.context() as mp:
        cv_twin.install(mp, loo_cases.twin_kind(case))
        _, ev, eg = check_case(case, name, 1e-9, 1e-9)
    return ev, eg


def check_on_device(case, name):
    ev, eg = twin_floor(case, name)
    print(case, name, "float64 floor (numpy twin against the goldens): value", ev, "gradients", eg, "cond", float(FX["%s__%s__cond" % (case, name)]))
    m, dv, dg = check_case(case, name, 1e-9, 1e-7)
    print(case, name, "device against the goldens: value", dv, "gradients", dg)
    assert isinstance(m._handle, _lib.ExactHandle)
    assert m._handle.inverse_fraction() == 1.0
    return m


@pytest.mark.parametrize("case,name", [p for p in cv_cases.PAIRS if p[0] != "big"])
def test_value_predictions_and_every_gradient_match_the_reference(case, name):
    check_on_device(case, name)


def test_dataflow_size_under_both_schedules():
    """N = 1100, 22 blocks of 50 points; MOGP_FLOW is read per evaluation"""
    old = {k: os.environ.get(k) for k in ("MOGP_FLOW", "MOGP_FLOW_MIN")}
    try:
        os.environ.pop("MOGP_FLOW", None); os.environ.pop("MOGP_FLOW_MIN", None)
        m = check_on_device("big", "blocks")
        assert m._handle.schedule()["dataflow"], m._handle.schedule()
        os.environ["MOGP_FLOW"] = "0"
        m = check_on_device("big", "blocks")
        assert not m._handle.schedule()["dataflow"]
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


def test_repeated_evaluations_are_bit_identical():
    m, ps = model_at_reference_raw("m32")
    lab = cv_cases.labels("m32", "wide", m)
    first = None
    for _ in range(20):
        loss = float(m.cv_loss(lab))
        got = [np.float64(loss).tobytes()] + [p.grad.tobytes() for p in ps]
        first = first or got
        assert got == first
    mu, var = m.cv(lab)
    mu2, var2 = m.cv(lab)
    assert mu.tobytes() == mu2.tobytes() and var.tobytes() == var2.tobytes()


def test_cv_leaves_no_state_behind_for_the_marginal_likelihood():
    m, ps = model_at_reference_raw("mosm")
    lab = cv_cases.labels("mosm", "across", m)

    def lml_bits():
        loss = float(m.loss())
        return [np.float64(loss).tobytes()] + [p.grad.tobytes() for p in ps]

    before = lml_bits()
    m.cv_loss(lab)
    assert lml_bits() == before
    m.cv_log_likelihood(lab)
    assert lml_bits() == before
    loo = np.float64(m.loo_loss()).tobytes()
    m.cv_loss(lab)
    assert np.float64(m.loo_loss()).tobytes() == loo          # nor for leave-one-out, whose vectors and adjoint buffer it shares


def test_the_workspace_belongs_to_handles_that_ask_for_it():
    m, _ = model_at_reference_raw("m32")
    lab = cv_cases.labels("m32", "wide", m)
    m.loss(); m.predict_f(m.X[:5]); m.log_marginal_likelihood()
    h = m._handle
    assert h.loo_bytes() == 0
    m.cv_log_likelihood(lab)
    small = h.loo_bytes()
    assert 0 < small < 8 * 256 * 256                          # without gradients: vectors and fold lists alone
    m.cv_loss(lab)
    factors = 8 * (128 * 128 + 1 + 8 * 8)                      # sum of |B|^2 doubles: packed, not 128^2 per fold
    assert h.loo_bytes() == small + 8 * 256 * 256 + factors    # N = 150 pads to 256: the one N x N matrix it shares with leave-one-out
    m.cv_loss(lab); m.loo_loss()
    assert h.loo_bytes() == small + 8 * 256 * 256 + factors


def test_one_point_folds_are_leave_one_out_on_the_device():
    m, ps = model_at_reference_raw("m32")
    lab = cv_cases.labels("m32", "singletons", m)
    mu, var = m.cv(lab)
    mu1, var1 = m.loo()
    assert kf.err(mu, mu1) <= 1e-12 and kf.err(var, var1) <= 1e-12
    loss = float(m.cv_loss(lab))
    grads = [p.grad.copy() for p in ps]
    assert kf.err(loss, float(m.loo_loss())) <= 1e-12
    for g, p in zip(grads, ps):
        assert kf.err(g, p.grad) <= 1e-10, p._name            # two orders of summation of the same N^3 product


def test_the_library_names_a_fold_it_cannot_take():
    """what gpr.Exact refuses on the host, sent past it: an empty fold, a fold of 129 points, a label out of range"""
    m, _ = model_at_reference_raw("m32")
    m.loss()
    h, N = m._handle, m.X.shape[0]
    nv = m._noise_var()
    lab = np.where(np.arange(N) < 5, 0, -1).astype(np.int32)
    with pytest.raises(_lib.MogpError, match="fold 1 holds 0 points"):
        h.cv(nv, m.jitter, lab, 2, grad=False)
    with pytest.raises(_lib.MogpError, match="fold 0 holds 129 points"):
        h.cv(nv, m.jitter, np.where(np.arange(N) < 129, 0, -1).astype(np.int32), 1, grad=False)
    with pytest.raises(_lib.MogpError, match="fold label 3"):
        h.cv(nv, m.jitter, np.where(np.arange(N) < 5, 3, -1).astype(np.int32), 2, grad=False)
    assert np.isfinite(h.cv(nv, m.jitter, lab, 1, grad=False)["cv"])


def test_adam_trace_on_the_cv_loss():
    check_cv_adam_trace()
