"""
ChangePointsKernel on the device (csrc/gram.hip: the gate row, kind 8, staged per point in the radial instantiations of the Gram and moment
kernels; the per-point diagonal in the relative jitter and the prediction) against the reference (tests/golden/changepoint.npz, written by
tests/golden/gen_family.py from the models of tests/changepoint_cases.py): Gram matrices, LML, loss, every raw gradient, predictions, both
schedules of the smallest dataflow size, bitwise repeatability, a short Adam trace, neutrality of the models that carry no such row, and
the row through the raw C ABI.  The bodies, shared with the other kernel families, and the tolerances are in tests/kernel_family.py.
"""
import numpy as np
import pytest

from mogptk_amd import gpr, _lib
from mogptk_amd.gpr.kernel import KIND_TIMES
import kernel_family as kf
from family_cases import exact, full_cases
from helpers import load

pytestmark = pytest.mark.gpu
FAMILY = "changepoint"


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


@pytest.mark.parametrize("case", ["three", "lmc"])
def test_repeated_gradient_evaluations_are_bit_identical(case):
    kf.check_bit_identical_repeats(FAMILY, case)


def test_adam_trace_through_model_train():
    kf.check_adam_trace(FAMILY)


def test_models_without_the_new_kinds_are_untouched():
    kf.check_models_without_the_new_kinds_are_untouched()


def _sigmoid(z):
    e = np.exp(-np.abs(z))
    return np.where(z >= 0, 1.0, e) / (1.0 + e)


def test_gate_only_groups_through_mogp_gram_kinds():
    """a gate row alone, and a group of nothing but gate rows (a window: rising at 3, falling at 7, the second one saturated), square and
    rectangular, against numpy; 150 points: three tile rows, the last ragged"""
    rng = np.random.default_rng(8)
    X1 = np.concatenate([np.zeros((150, 1)), rng.uniform(0, 10, (150, 1))], axis=1)
    X2 = np.concatenate([np.zeros((70, 1)), rng.uniform(-1, 11, (70, 1))], axis=1)
    for rows, kind in (([[1.3, 0.0, 1.7, 4.2, 0.0]], [8]), ([[0.8, 0.0, 2.5, 3.0, 0.0], [1.0, 0.0, -40.0, 7.0, 0.0]], [8 | KIND_TIMES, 8])):
        table, kind = np.array(rows)[None, None], np.array(kind, dtype=np.int32)[None, None]
        for Xb in (None, X2):
            xa, xb = X1[:, 1], (X1 if Xb is None else Xb)[:, 1]
            want = np.prod([r[0] * _sigmoid(r[2] * (xa - r[3]))[:, None] * _sigmoid(r[2] * (xb - r[3]))[None, :] for r in rows], axis=0)
            got = _lib.gram(gpr.config.device, 1, 1, table, X1, Xb, kind, np.zeros(kind.shape))
            e = kf.err(got, want)
            print("gate rows", len(rows), "rectangular" if Xb is not None else "square", e)
            assert e <= 1e-12


def test_set_kinds_refuses_a_gate_row_in_two_dimensions_and_kind_nine():
    rng = np.random.default_rng(9)
    for D, kind in ((2, 8), (1, 9), (1, 9 | KIND_TIMES)):
        h = _lib.ExactHandle(gpr.config.device, np.concatenate([np.zeros((40, 1)), rng.uniform(0, 10, (40, D))], axis=1), rng.standard_normal(40), 1)
        T = 2 if kind & KIND_TIMES else 1
        table = np.zeros((1, 1, T, 2 + 3 * D))
        table[..., 0] = 1.0
        h.set_terms(table)
        kd = np.zeros((1, 1, T), dtype=np.int32)
        kd[0, 0, 0] = kind
        with pytest.raises(_lib.MogpError) as e:
            h.set_kinds(kd, np.zeros((1, 1, T)))
        assert e.value.code == _lib.MOGP_EINVAL, str(e.value)
        assert ("one input dimension" if D == 2 else "unknown kind") in str(e.value)
    h = _lib.ExactHandle(gpr.config.device, np.concatenate([np.zeros((40, 1)), rng.uniform(0, 10, (40, 1))], axis=1), rng.standard_normal(40), 1)
    h.set_terms(np.array([[[[1.0, 0.0, 2.0, 4.0, 0.0]]]]))
    h.set_kinds(np.full((1, 1, 1), 8, dtype=np.int32), np.zeros((1, 1, 1)))      # D = 1: a gate row may stand alone


def test_moments_of_a_gate_row_with_an_amplitude_of_its_own(monkeypatch):
    """the raw ABI with A != 1 on a gate row, alone and behind a Matern row: the device's moments leave the row's own amplitude out (m1_0 and
    m3_0 are d/dbeta and d/dl of h_a h_b; include/mogp_hip.h), as the numpy twin's do; LML 1e-9, moments at the gradients' 1e-7"""
    import changepoint_twin as twin
    import oracle.table_model as tm
    monkeypatch.setattr(tm, "row_parts", twin.row_parts)
    rng = np.random.default_rng(12)
    X = np.concatenate([np.zeros((150, 1)), rng.uniform(0, 10, (150, 1))], axis=1)
    y = np.sin(X[:, 1]) + 0.1 * rng.standard_normal(150)
    table = np.array([[[[0.9, 0.0, 2.0, 0.0, 0.0], [1.3, 0.0, -2.5, 6.1, 0.0], [0.7, 0.0, 1.7, 4.2, 0.0]]]])
    kind, shape = np.array([[[3 | KIND_TIMES, 8, 8]]], dtype=np.int32), np.zeros((1, 1, 3))
    got, want = [], []
    for cls, out in ((_lib.ExactHandle, got), (twin.GateTableDevice, want)):
        h = cls(gpr.config.device, X, y, 1)
        h.set_terms(table)
        h.set_kinds(kind, shape)
        out.append(h.eval(np.array([0.1]), 1e-8, grad=True))
    got, want = got[0], want[0]
    assert kf.err(got["lml"], want["lml"]) <= 1e-9
    e = kf.err(got["moments"], want["moments"])
    print("gate moments, A = 1.3 and 0.7", e)
    assert e <= 1e-7 and np.all(np.asarray(got["moments"])[0, 1:, [1, 3]] == 0.0)
