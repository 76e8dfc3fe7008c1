"""
LinearKernel, PolynomialKernel and SincKernel on the device (csrc/gram.hip: the dot-product row, kind 7, and the sinc profile, kind 6, in the
radial instantiations of the Gram and moment kernels; the per-point diagonal in the relative jitter and the prediction) against the
reference (tests/golden/trend.npz, written by tests/golden/gen_family.py from the models of tests/trend_cases.py): Gram matrices, LML, loss,
every raw gradient, predictions, both schedules of the smallest dataflow size, bitwise repeatability, a short Adam trace, and neutrality of
the models that carry neither kind.  The bodies, shared with the other kernel families, and the tolerances are in tests/kernel_family.py.
"""
import pytest

from mogptk_amd import gpr
import kernel_family as kf
from family_cases import exact, full_cases
from helpers import load

pytestmark = pytest.mark.gpu
FAMILY = "trend"


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


def test_models_without_the_new_kinds_are_untouched():
    kf.check_models_without_the_new_kinds_are_untouched()
