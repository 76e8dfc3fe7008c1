"""
The stationary kernels on the device (csrc/gram.hip: the radial instantiations of the general Gram and moment kernels) against the
reference (tests/golden/stationary.npz, written by tests/golden/gen_family.py from the models of tests/stationary_cases.py): Gram
matrices, LML, loss, every raw gradient, predictions, both schedules of the smallest dataflow size, bitwise repeatability, a short Adam
trace, and bitwise neutrality of an all-Gaussian kinds call.  The bodies, shared with the other kernel families, and the tolerances are in
tests/kernel_family.py.
"""
import numpy as np
import pytest

import mogptk_amd
from mogptk_amd import gpr
import kernel_family as kf
from family_cases import exact, full_cases
from helpers import load

pytestmark = pytest.mark.gpu
FAMILY = "stationary"


@pytest.mark.parametrize("case", full_cases(FAMILY))
def test_gram_matrices_match_the_reference(case):
    kf.check_gram_matrices(FAMILY, case)


@pytest.mark.parametrize("case", full_cases(FAMILY))
def test_lml_loss_and_every_gradient_match_reference_autograd(case):
    kf.check_value_and_gradients(exact(FAMILY, gpr, case), load(FAMILY + ".npz"), case + "__")


@pytest.mark.parametrize("case", full_cases(FAMILY))
def test_predictions_match_the_reference(case):
    kf.check_predictions(FAMILY, case)


def test_dataflow_size_under_both_schedules():
    kf.check_both_schedules(FAMILY)


@pytest.mark.parametrize("case", ["imo", "lmc"])
def test_repeated_gradient_evaluations_are_bit_identical(case):
    kf.check_bit_identical_repeats(FAMILY, case)


def test_adam_trace_through_model_train():
    kf.check_adam_trace(FAMILY)


def test_all_gaussian_kinds_call_changes_nothing():
    """a SpectralMixtureKernel model, the new entry point never called, then an explicit all-zero kinds call: the same bits"""
    rng = np.random.default_rng(3)
    X = np.sort(rng.uniform(0, 10, (300, 1)), axis=0)
    y = np.sin(X[:, 0]) + 0.1 * rng.standard_normal(300)

    def build():
        k = gpr.SpectralMixtureKernel(Q=3, input_dims=1)
        k.magnitude.assign([0.9, 0.5, 0.7]); k.mean.assign([[0.1], [0.25], [0.4]]); k.variance.assign([[0.05], [0.02], [0.08]])
        return gpr.Exact(k, X, y, variance=0.1)

    calls = []
    real = mogptk_amd._lib.ExactHandle.set_kinds
    mogptk_amd._lib.ExactHandle.set_kinds = lambda self, *a: (calls.append(a), real(self, *a))[1]
    try:
        m = build()
        l0 = float(m.loss())
        g0 = [p.grad.copy() for p in m.parameters()]
        assert not calls                                     # all-zero kinds: not one extra call
        h = m._handle
        h.set_kinds(np.zeros((1, 1, h.T), dtype=np.int32), np.zeros((1, 1, h.T)))
        l1 = float(m.loss())
        assert np.float64(l0).tobytes() == np.float64(l1).tobytes()
        for g, p in zip(g0, m.parameters()):
            assert g.tobytes() == p.grad.tobytes()
    finally:
        mogptk_amd._lib.ExactHandle.set_kinds = real
