"""
FunctionKernel and WhiteKernel on the device (csrc/gram.hip: the weighted-dot row, kind 9, over input columns that carry the basis
functions' values, and the white row, kind 10, the identity by index, in the flagged instantiations of the radial Gram and moment kernels
for D = 1, 2, 3 and the generic one; periodic and sinc rows beside feature columns) against the reference (tests/golden/function.npz,
written by tests/golden/gen_function.py from the models of tests/function_cases.py): Gram matrices, LML, loss, every raw gradient,
predictions, both schedules of the smallest dataflow size, bitwise repeatability, a short Adam trace, neutrality of the models that carry
no such row, and the rows through the raw C ABI.  The bodies, shared with the other kernel families, and the tolerances are in
tests/kernel_family.py.
"""
import numpy as np
import pytest

from mogptk_amd import gpr, _lib
from mogptk_amd.gpr.kernel import KIND_TIMES
import kernel_family as kf
from family_cases import exact, full_cases
from helpers import load

pytestmark = pytest.mark.gpu
FAMILY = "function"
X_ = KIND_TIMES


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


@pytest.mark.parametrize("case", ["white_f", "lmc"])
def test_repeated_gradient_evaluations_are_bit_identical(case):
    kf.check_bit_identical_repeats(FAMILY, case)


def test_adam_trace_through_model_train():
    kf.check_adam_trace(FAMILY)


def test_models_without_the_new_kinds_are_untouched():
    kf.check_models_without_the_new_kinds_are_untouched()


def _inputs(rng, n, lo=0.0, hi=10.0):
    """a channel column and three input columns of order one"""
    return np.concatenate([np.zeros((n, 1)), rng.uniform(lo, hi, (n, 1)), rng.uniform(-1.0, 1.0, (n, 2))], axis=1)


def test_weighted_dot_rows_through_mogp_gram_kinds():
    """kind 9 alone and in a group with a Gaussian row, both with A != 1, D = 3, square (150 x 150: three tile rows, the last ragged) and
    rectangular (150 x 70), against numpy"""
    rng = np.random.default_rng(8)
    X1, X2 = _inputs(rng, 150), _inputs(rng, 70, -1.0, 11.0)
    wd = [1.3, 0.0, 0.0, 0.6, 0.9, 0, 0, 0, 0, 0, 0]
    ga = [0.8, 0.0, 0.7, 0.0, 0.0, 0, 0, 0, 0, 0, 0]
    for rows, kind in (([wd], [9]), ([ga, wd], [0 | X_, 9]), ([wd, ga], [9 | X_, 0])):
        table, kd = np.array(rows, dtype=np.float64)[None, None], np.array(kind, dtype=np.int32)[None, None]
        for Xb in (None, X2):
            xa, xb = X1[:, 1:], (X1 if Xb is None else Xb)[:, 1:]
            want = 1.3 * np.einsum("d,ad,bd->ab", np.array(wd[2:5]), xa, xb)
            if len(rows) == 2:
                want = want * 0.8 * np.exp(-0.5 * 0.7 * (xa[:, None, 0] - xb[None, :, 0]) ** 2)
            got = _lib.gram(gpr.config.device, 1, 3, table, X1, Xb, kd, np.zeros(kd.shape))
            e = kf.err(got, want)
            print("weighted-dot rows", kind, "rectangular" if Xb is not None else "square", e)
            assert e <= 1e-12


def test_white_rows_through_mogp_gram_kinds():
    """kind 10: the square call is A I although two inputs coincide; a rectangular call with X2 a copy of X1 is all zeros; White x k is
    diag(A k(x, x)); D = 1 (the white row alone: a weighted-dot row needs a feature column) and D = 3"""
    rng = np.random.default_rng(9)
    for D in (1, 3):
        X = _inputs(rng, 150)[:, :1 + D]
        X[97] = X[13]
        W = 2 + 3 * D
        white = np.zeros(W); white[0] = 0.37
        wd = np.zeros(W); wd[0] = 1.3; wd[2:2 + D] = [0.6, 0.9, 0.4][:D]
        kd, sh = np.array([[[10]]], dtype=np.int32), np.zeros((1, 1, 1))
        K = _lib.gram(gpr.config.device, 1, D, white[None, None, None], X, None, kd, sh)
        assert np.array_equal(K, 0.37 * np.eye(150)) and K[13, 97] == 0.0
        assert not np.any(_lib.gram(gpr.config.device, 1, D, white[None, None, None], X, X.copy(), kd, sh))
        if D == 1:
            continue
        kd, sh = np.array([[[10 | X_, 9]]], dtype=np.int32), np.zeros((1, 1, 2))
        K = _lib.gram(gpr.config.device, 1, D, np.array([white, wd])[None, None], X, None, kd, sh)
        want = np.diag(0.37 * 1.3 * np.sum(wd[2:2 + D] * X[:, 1:] ** 2, axis=1))
        assert kf.err(K, want) <= 1e-12 and np.array_equal(K != 0.0, np.eye(150, dtype=bool))
        assert not np.any(_lib.gram(gpr.config.device, 1, D, np.array([white, wd])[None, None], X, X.copy(), kd, sh))


def test_moments_of_weighted_dot_and_white_rows_with_amplitudes_of_their_own(monkeypatch):
    """the raw ABI with A != 1 on a kind-9 row, alone and in a group with a white row and a Matern row: the device's moments leave the row's
    own amplitude out (include/mogp_hip.h), as the numpy twin's do; LML 1e-9, moments at the gradients' 1e-7.  D = 3: one input column,
    two feature columns"""
    import function_twin as twin
    twin.install(monkeypatch)
    rng = np.random.default_rng(12)
    X = _inputs(rng, 150)
    X[97] = X[13]
    y = np.sin(X[:, 1]) + 0.1 * rng.standard_normal(150)
    wd = [1.3, 0.0, 0.0, 0.6, 0.9, 0, 0, 0, 0, 0, 0]
    for rows, kind in (([wd], [9]), ([[0.4] + [0.0] * 10, wd, [0.9, 0.0, 2.0, 0.0, 0.0, 0, 0, 0, 0, 0, 0], [0.7, 0.0, 0.5, 0.0, 0.0, 0, 0, 0, 0, 0, 0]], [10 | X_, 9 | X_, 3, 0])):
        table, kd = np.array(rows, dtype=np.float64)[None, None], np.array(kind, dtype=np.int32)[None, None]
        got, want = [], []
        for cls, out in ((_lib.ExactHandle, got), (twin.FunctionTableDevice, want)):
            h = cls(gpr.config.device, X, y, 1)
            h.set_terms(table)
            h.set_kinds(kd, np.zeros(kd.shape))
            out.append(h.eval(np.array([0.1]), 1e-8, grad=True))
        got, want = got[0], want[0]
        assert kf.err(got["lml"], want["lml"]) <= 1e-9
        e = kf.err(got["moments"], want["moments"])
        print("moments of", kind, e)
        assert e <= 1e-7
        t = [k & 0xff for k in kind].index(9)
        assert np.all(np.asarray(got["moments"])[0, t, [1, 5, 6, 7, 8, 9, 10]] == 0.0)
        if 10 in [k & 0xff for k in kind]:
            assert np.all(np.asarray(got["moments"])[0, 0, 1:] == 0.0) and np.asarray(got["moments"])[0, 0, 0] != 0.0


def test_set_kinds_accepts_a_periodic_row_in_two_dimensions_and_refuses_kind_eleven():
    rng = np.random.default_rng(13)
    X = _inputs(rng, 150)[:, :3]
    row = np.array([0.8, 0.0, 1.4, 0.0, 0.3, 0.0, 0.0, 0.0])             # [A, Psi, V_0, V_1, M_0, M_1, Delta_0, Delta_1]
    kd, sh = np.array([[[5]]], dtype=np.int32), np.zeros((1, 1, 1))
    h = _lib.ExactHandle(gpr.config.device, X, rng.standard_normal(150), 1)
    h.set_terms(row[None, None, None])
    h.set_kinds(kd, sh)
    th = 2.0 * np.pi * 0.3 * (X[:, None, 1] - X[None, :, 1])
    got = _lib.gram(gpr.config.device, 1, 2, row[None, None, None], X, None, kd, sh)
    want = 0.8 * np.exp(1.4 * (np.cos(th) - 1.0))
    assert kf.err(got, want) <= 1e-12
    for kind in (11, 11 | X_, 200):
        T = 2 if kind & X_ else 1
        table = np.zeros((1, 1, T, 8))
        table[..., 0] = 1.0
        h.set_terms(table)
        bad = np.zeros((1, 1, T), dtype=np.int32)
        bad[0, 0, 0] = kind
        with pytest.raises(_lib.MogpError) as e:
            h.set_kinds(bad, np.zeros((1, 1, T)))
        assert e.value.code == _lib.MOGP_EINVAL and "unknown kind" in str(e.value)
    for kind in (9, 10):                                                 # the two new kinds are known where there is more than one column
        table = np.zeros((1, 1, 1, 8))
        table[..., 0] = 1.0
        h.set_terms(table)
        h.set_kinds(np.full((1, 1, 1), kind, dtype=np.int32), np.zeros((1, 1, 1)))
    # one column: a white row is at home there; a weighted-dot row has no feature column to stand over and stays the unknown kind it was
    h = _lib.ExactHandle(gpr.config.device, X[:, :2], rng.standard_normal(150), 1)
    h.set_terms(np.array([[[[1.0, 0.0, 0.0, 0.0, 0.0]]]]))
    h.set_kinds(np.full((1, 1, 1), 10, dtype=np.int32), np.zeros((1, 1, 1)))
    with pytest.raises(_lib.MogpError) as e:
        h.set_kinds(np.full((1, 1, 1), 9, dtype=np.int32), np.zeros((1, 1, 1)))
    assert e.value.code == _lib.MOGP_EINVAL and "unknown kind" in str(e.value) and "feature column" in str(e.value)


def test_a_device_mean_table_gets_zero_slopes_on_the_feature_columns():
    """LinearMean under `trend` (three device columns, one of them the model's own): the loss is the mean-free model's on y - m(X), the kernel's
    gradients are the same, and the mean's own gradients are the loss's central differences"""
    import function_cases as fc
    X, y, _ = fc.data("trend")
    mean = gpr.LinearMean(input_dims=1)
    mean.bias.assign(0.3); mean.slope.assign([0.12])
    m = gpr.Exact(fc.kernel(gpr, "trend"), X, y, variance=fc.NOISE, mean=mean)
    m0 = gpr.Exact(fc.kernel(gpr, "trend"), X, y - (0.3 + 0.12 * X[:, 0]), variance=fc.NOISE)
    l, l0 = float(m.loss()), float(m0.loss())
    assert kf.err(l, l0) <= 1e-9
    for p, p0 in zip(m.kernel.parameters(), m0.kernel.parameters()):
        assert kf.err(p.grad, p0.grad) <= 1e-7, p._name
    for p in (mean.bias, mean.slope):
        g, raw, h = np.asarray(p.grad, dtype=np.float64).reshape(-1)[0], np.array(p.data, copy=True), 1e-5
        p.data = raw + h
        up = float(m.log_marginal_likelihood())
        p.data = raw - h
        dn = float(m.log_marginal_likelihood())
        p.data = raw
        assert abs(g - (dn - up) / (2 * h)) <= 1e-5 * max(1.0, abs(g)), (p._name, g, (dn - up) / (2 * h))


def test_a_white_row_beside_gate_rows_in_one_dimension():
    """kinds 8 and 10 in one launch (ChangePointsKernel + WhiteKernel): the D = 1 instantiation that carries all three rows; a Matern 3/2 row
    under a rising gate, plus a white row, against numpy"""
    rng = np.random.default_rng(14)
    X = np.concatenate([np.zeros((150, 1)), rng.uniform(0, 10, (150, 1))], axis=1)
    X[97] = X[13]
    table = np.array([[[[0.9, 0.0, 2.0, 0.0, 0.0], [1.0, 0.0, 1.7, 4.2, 0.0], [0.37, 0.0, 0.0, 0.0, 0.0]]]])
    kd = np.array([[[3 | X_, 8, 10]]], dtype=np.int32)
    x = X[:, 1]
    h = 1.0 / (1.0 + np.exp(-1.7 * (x - 4.2)))
    r = np.sqrt(3.0 * 2.0) * np.abs(x[:, None] - x[None, :])
    want = 0.9 * (1.0 + r) * np.exp(-r) * h[:, None] * h[None, :] + 0.37 * np.eye(150)
    got = _lib.gram(gpr.config.device, 1, 1, table, X, None, kd, np.zeros((1, 1, 3)))
    assert kf.err(got, want) <= 1e-12 and got[13, 97] == got[97, 13] and abs(got[13, 13] - got[13, 97] - 0.37) <= 1e-12
    got = _lib.gram(gpr.config.device, 1, 1, table, X, X.copy(), kd, np.zeros((1, 1, 3)))
    assert kf.err(got, want - 0.37 * np.eye(150)) <= 1e-12
