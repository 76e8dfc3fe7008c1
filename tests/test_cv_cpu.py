"""
Leave-fold-out cross-validation without a device: gpr.Exact's CV path -- folds to labels, push, kinds, per-point diagonal,
moments -> table gradient, the jitter term, noise and mean -- over the numpy twin (tests/cv_twin.py) against the reference-side goldens
(tests/golden/cv.npz, gen_cv.py: conditional Gaussians formed directly from Kj), and the public surface.  Tolerances: DESIGN 8, relative to
max(1, max |want|) -- 1e-9 for the value, the predictions and every gradient on the twin.
"""
import numpy as np
import pytest

import mogptk_amd
from mogptk_amd import gpr
from mogptk_amd.gpr.config import config

import cv_cases
import cv_twin
import loo_cases
from family_cases import cases
from helpers import load
from kernel_family import err, with_reference_raw

FX = load("cv.npz")


def model_at_reference_raw(case):
    m, (fx, pre) = loo_cases.exact(gpr, case)
    return m, with_reference_raw(m, fx, pre)


def err_held_out(got, want):
    """err over the held-out points; the points in no fold are NaN on both sides"""
    got, want = np.asarray(got, dtype=np.float64).reshape(-1), np.asarray(want, dtype=np.float64).reshape(-1)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    return err(got[~np.isnan(want)], want[~np.isnan(want)])


def check_case(case, name, tol_value, tol_grad):
    """value, held-out predictions and every gradient of (case, layout) on whatever device handle the model gets; -> (model, largest value error, largest gradient error)"""
    pre = "%s__%s__" % (case, name)
    m, ps = model_at_reference_raw(case)
    lab = cv_cases.labels(case, name, m)
    L = float(m.cv_log_likelihood(lab))
    ev = err(L, float(FX[pre + "cv"]))
    print(pre, "cv", ev)
    assert ev <= tol_value, (L, float(FX[pre + "cv"]))
    if not loo_cases.CASES[case].get("light"):
        mu, var = m.cv(lab)
        assert mu.shape == var.shape == (m.X.shape[0], 1) and mu.dtype == var.dtype == config.dtype
        assert np.array_equal(np.isnan(mu.reshape(-1)), lab < 0)
        for what, got in (("mu", mu), ("var", var)):
            e = err_held_out(got, FX[pre + what])
            print(pre, what, e)
            assert e <= tol_value, what
            ev = max(ev, e)
    loss = float(m.cv_loss(lab))
    e = err(loss, float(FX[pre + "loss"]))
    print(pre, "loss", e)
    assert e <= tol_value
    ev, eg = max(ev, e), 0.0
    for i, p in enumerate(ps):
        g = FX["%sp%d_grad" % (pre, i)]
        e = err(p.grad, g)
        print(pre, p._name, "grad", e)
        assert e <= tol_grad, (p._name, p.grad, g)
        eg = max(eg, e)
    return m, ev, eg


@pytest.mark.parametrize("case,name", cv_cases.PAIRS)
def test_twin_matches_the_reference(case, name, monkeypatch):
    cv_twin.install(monkeypatch, loo_cases.twin_kind(case))
    m, _, _ = check_case(case, name, 1e-9, 1e-9)
    assert isinstance(m._handle, cv_twin.CvTableDevice)


def test_the_layouts_hold_what_they_are_there_for():
    sizes, none, two_channels, every_tile = set(), False, False, False
    for case, name in cv_cases.PAIRS:
        m, _ = loo_cases.exact(gpr, case)
        X = cv_cases.model_inputs(m)
        lab = cv_cases.labels(case, name, m)
        order = np.argsort(X[:, 0], kind="stable")            # the channel sort of the device
        pos = np.empty(len(lab), dtype=np.int64); pos[order] = np.arange(len(lab))
        assert m._fold_labels(lab)[1] == lab.max() + 1         # the host's own check takes every layout
        none |= bool(np.any(lab < 0))
        for f in range(lab.max() + 1):
            B = np.flatnonzero(lab == f)
            sizes.add(B.size)
            two_channels |= np.unique(X[B, 0]).size > 1
            every_tile |= B.size <= 17 and len(lab) > 128 and np.unique(pos[B] // 64).size == (len(lab) + 63) // 64
            if B.size == 128:
                assert pos[B].min() < 128 <= pos[B].max()
                assert (case, pos[B].min(), pos[B].max()) == ("m32", 11, 138)
    assert {1, 17, 50, 128} <= sizes and none and two_channels and every_tile
    m, _ = loo_cases.exact(gpr, "m32")
    assert sorted(cv_cases.labels("m32", "singletons", m)) == list(range(150))
    m, _ = loo_cases.exact(gpr, "big")
    assert np.array_equal(np.bincount(cv_cases.labels("big", "blocks", m)), np.full(22, 50))


def test_one_point_folds_are_leave_one_out(monkeypatch):
    cv_twin.install(monkeypatch)
    m, ps = model_at_reference_raw("m32")
    lab = cv_cases.labels("m32", "singletons", m)
    mu, var = m.cv(lab)
    mu1, var1 = m.loo()
    assert err(mu, mu1) <= 1e-12 and err(var, var1) <= 1e-12
    assert err(float(m.cv_log_likelihood(lab)), float(m.loo_log_likelihood())) <= 1e-12
    loss = float(m.cv_loss(lab))
    grads = [p.grad.copy() for p in ps]
    assert err(loss, float(m.loo_loss())) <= 1e-12
    for g, p in zip(grads, ps):
        assert err(g, p.grad) <= 1e-12, p._name


def test_labels_and_index_arrays_are_the_same_folds(monkeypatch):
    cv_twin.install(monkeypatch)
    m, ps = model_at_reference_raw("three")
    lab = cv_cases.labels("three", "mixed", m)
    a = float(m.cv_loss(lab))
    ga = [p.grad.copy() for p in ps]
    b = float(m.cv_loss(cv_cases.index_arrays(lab)))
    assert a == b and all(np.array_equal(g, p.grad) for g, p in zip(ga, ps))
    assert float(m.cv_loss([list(ix) for ix in cv_cases.index_arrays(lab)])) == a
    assert float(m.cv_loss(lab.astype(np.int64).tolist())) == a


def test_loss_is_unchanged_and_cv_leaves_nothing_behind(monkeypatch):
    """the marginal likelihood's loss and gradients against the family's own golden, bit for bit before and after CV evaluations on the same model"""
    cv_twin.install(monkeypatch)
    m, ps = model_at_reference_raw("m32")
    lab = cv_cases.labels("m32", "wide", m)
    fx = load("stationary.npz")

    def lml_loss():
        loss = float(m.loss())
        assert err(loss, float(fx["m32__loss"])) <= 1e-9
        for i, p in enumerate(ps):
            assert err(p.grad, fx["m32__p%d_grad" % i]) <= 1e-9
        return [np.float64(loss).tobytes()] + [p.grad.tobytes() for p in ps]

    before = lml_loss()
    m.cv_loss(lab); m.cv(lab); m.cv_log_likelihood(lab)
    assert lml_loss() == before


def test_cv_loss_zeroes_the_gradients_first(monkeypatch):
    cv_twin.install(monkeypatch)
    m, ps = model_at_reference_raw("m32")
    lab = cv_cases.labels("m32", "wide", m)
    m.cv_loss(lab)
    first = [p.grad.copy() for p in ps]
    m.cv_loss(lab)
    assert all(np.array_equal(a, p.grad) for a, p in zip(first, ps))


class NoDevice:
    def __init__(self, *a, **k):
        raise AssertionError("a device handle was created")


def test_bad_folds_are_refused_by_name_before_any_device_call(monkeypatch):
    from mogptk_amd import _lib
    monkeypatch.setattr(_lib, "ExactHandle", NoDevice)
    m, _ = loo_cases.exact(gpr, "m32")
    N = m.X.shape[0]
    ok = np.arange(10)
    bad = [
        ([ok, np.arange(9, 15)], r"folds 0 and 1 overlap"),
        ([ok, np.array([], dtype=np.int64)], r"fold 1 is empty"),
        ([ok, np.arange(10, 139)], r"fold 1 holds 129 points: the limit is 128 points per fold, larger folds are not on the device"),
        ([ok, np.array([20, N])], r"fold 1: index %d is out of range" % N),
        ([ok, np.array([-1, 20])], r"fold 1: index -1 is out of range"),
        (np.zeros(N - 1, dtype=np.int64), r"one label per training point: %d labels for %d points" % (N - 1, N)),
        (np.where(np.arange(N) < 5, 0, np.where(np.arange(N) < 9, 2, -1)), r"fold 1 is empty"),
        (np.where(np.arange(N) < 129, 0, -1), r"fold 0 holds 129 points"),
        (np.full(N, -1), r"no folds"),
    ]
    for folds, message in bad:
        for call in (m.cv, m.cv_log_likelihood, m.cv_loss):
            with pytest.raises(ValueError, match=message):
                call(folds)


def test_sharded_evaluation_is_refused_before_any_device_call(monkeypatch):
    from mogptk_amd import _lib
    monkeypatch.setattr(_lib, "ExactHandle", NoDevice)
    monkeypatch.setattr(config, "comm", type("Comm", (), dict(world=2, rank=0, force=False, native=True))(), raising=False)
    m, _ = loo_cases.exact(gpr, "m32")
    for call in (m.cv, m.cv_log_likelihood, m.cv_loss):
        with pytest.raises(NotImplementedError, match="sharded"):
            call(np.arange(m.X.shape[0]) // 10)


def adam_model():
    c = loo_cases.CASES[cv_cases.ADAM_CASE]
    sc = cases(c["family"])
    X, y, _ = sc.data(c["case"])
    return mogptk_amd.Model(mogptk_amd.DataSet(mogptk_amd.Data(X[:, 0], y, name="a")), gpr.IndependentMultiOutputKernel(sc.kernel(gpr, c["case"]), output_dims=1),
                            inference=mogptk_amd.Exact(variance=sc.NOISE))


def test_other_models_have_no_cv():
    sc = cases("stationary")
    X, y, _ = sc.data("se0")
    for m in (gpr.Titsias(sc.kernel(gpr, "se0"), X, y, Z=5), gpr.Snelson(sc.kernel(gpr, "se0"), X, y, Z=5),
              gpr.OpperArchambeau(sc.kernel(gpr, "se0"), X, y), gpr.Hensman(sc.kernel(gpr, "se0"), X, y)):
        for name in ("cv", "cv_log_likelihood", "cv_loss"):
            assert not hasattr(m, name), (m.name(), name)
    mm = mogptk_amd.Model(mogptk_amd.DataSet(mogptk_amd.Data(X[:, 0], y, name="a")), gpr.IndependentMultiOutputKernel(sc.kernel(gpr, "se0"), output_dims=1),
                          inference=mogptk_amd.Titsias(inducing_points=5))
    folds = mm.block_folds(10)
    with pytest.raises(ValueError, match="exact inference"):
        mm.train(method="Adam", iters=1, objective="cv", folds=folds)
    with pytest.raises(ValueError, match="exact inference"):
        mm.cv_log_likelihood(folds)


def test_train_takes_folds_with_the_cv_objective_only(monkeypatch):
    cv_twin.install(monkeypatch)
    mm = adam_model()
    folds = mm.block_folds(10)
    for objective in ("lml", "loo"):
        with pytest.raises(ValueError, match="folds"):
            mm.train(method="Adam", iters=1, objective=objective, folds=folds)
    with pytest.raises(ValueError, match="folds"):
        mm.train(method="Adam", iters=1, objective="cv")
    with pytest.raises(ValueError, match="objective"):
        mm.train(method="Adam", iters=1, objective="elbo")


def test_block_folds():
    mm = adam_model()
    lab = mm.block_folds(10)
    X = np.asarray(mm.gpr.X, dtype=np.float64)
    assert lab.shape == (150,) and np.array_equal(lab, FX["adam__labels"]) and np.array_equal(lab, cv_cases.block_labels(X, 10))
    order = np.argsort(X[:, 1], kind="stable")
    assert np.array_equal(lab[order], np.arange(150) // 10)   # runs of 10 in input order
    assert np.array_equal(np.bincount(mm.block_folds(128)), [128, 22]) and np.array_equal(np.sort(mm.block_folds(1)), np.arange(150))
    assert np.array_equal(np.bincount(mm.block_folds(40)), [40, 40, 40, 30])
    for size in (0, 129, -3):
        with pytest.raises(ValueError, match="size"):
            mm.block_folds(size)
    # two channels of 7 and 4 points given out of input order: per channel, in input order, numbered on from channel to channel
    rng = np.random.default_rng(3)
    xa, xb = rng.permutation(7).astype(float), rng.permutation(4).astype(float)
    m2 = mogptk_amd.Model(mogptk_amd.DataSet(mogptk_amd.Data(xa, np.sin(xa), name="a"), mogptk_amd.Data(xb, np.cos(xb), name="b")),
                          gpr.IndependentMultiOutputKernel(gpr.SquaredExponentialKernel(), gpr.SquaredExponentialKernel(), output_dims=2),
                          inference=mogptk_amd.Exact())
    lab = m2.block_folds(3)
    X2 = np.asarray(m2.gpr.X, dtype=np.float64)
    for c, first, n in ((0, 0, 7), (1, 3, 4)):
        rows = np.flatnonzero(X2[:, 0] == c)
        assert rows.size == n and np.array_equal(lab[rows], first + np.floor(np.argsort(np.argsort(X2[rows, 1])) / 3).astype(int))
    assert np.array_equal(np.bincount(lab), [3, 3, 1, 3, 1])
    x2d = rng.uniform(0, 1, (9, 2))
    m3 = mogptk_amd.Model(mogptk_amd.DataSet(mogptk_amd.Data(x2d, x2d[:, 0], name="a")),
                          gpr.IndependentMultiOutputKernel(gpr.SquaredExponentialKernel(input_dims=2), output_dims=1), inference=mogptk_amd.Exact())
    with pytest.raises(ValueError, match="one input dimension"):
        m3.block_folds(3)


def check_cv_adam_trace():
    mm = adam_model()
    folds = mm.block_folds(cv_cases.ADAM_BLOCK)
    losses, _ = mm.train(method="Adam", iters=cv_cases.ADAM_ITERS, lr=cv_cases.ADAM_LR, verbose=False, objective="cv", folds=folds)
    want = FX["adam__losses"]
    e = err(np.asarray(losses, dtype=np.float64), want)
    print("cv adam trace", e)
    assert e <= 1e-7
    assert losses[-1] < losses[0]
    final = np.concatenate([np.asarray(p.data, dtype=np.float64).reshape(-1) for p in mm.gpr.parameters()])
    assert err(final, FX["adam__final"]) <= 1e-7


def test_train_with_the_cv_objective_follows_the_reference_side_trace(monkeypatch):
    cv_twin.install(monkeypatch)
    check_cv_adam_trace()


@pytest.mark.parametrize("method", ["LBFGS", "SGD", "AdaGrad"])
def test_every_optimiser_takes_the_cv_closure(method, monkeypatch):
    cv_twin.install(monkeypatch)
    mm = adam_model()
    calls = []
    real = gpr.Exact.cv_loss
    monkeypatch.setattr(gpr.Exact, "cv_loss", lambda self, folds: (calls.append(1), real(self, folds))[1])
    monkeypatch.setattr(gpr.Exact, "loss", lambda self: pytest.fail("the LML loss was evaluated under objective='cv'"))
    monkeypatch.setattr(gpr.Exact, "loo_loss", lambda self: pytest.fail("the LOO loss was evaluated under objective='cv'"))
    losses, _ = mm.train(method=method, iters=3, lr=1e-3, objective="cv", folds=mm.block_folds(25))
    assert len(calls) >= 4 and np.all(np.isfinite(losses[:4]))
