"""
The rolling-origin forecast without a device: gpr.Exact's forecast path -- order and cuts checked, push, kinds, per-point diagonal, the
mean -- over the numpy twin (tests/forecast_twin.py: direct conditional solves on the twin's Kj) against the reference-side goldens
(tests/golden/forecast.npz, gen_forecast.py), Model.forecast_origins, the Model-level surface, and every refusal before a device call.
Tolerance: 1e-9 relative to max(1, max |want|) for mean, variance and score (what 1c, 1d and 1f hold predictions to).
"""
import numpy as np
import pytest

import mogptk_amd
from mogptk_amd import gpr
from mogptk_amd.gpr.config import config

import cv_cases
import forecast_cases as fc
import forecast_twin
import loo_cases
from family_cases import cases
from helpers import load
from kernel_family import err, with_reference_raw

FX = load("forecast.npz")
TOL = 1e-9


def model_at_reference_raw(case):
    m, (fx, pre) = loo_cases.exact(gpr, case)
    return m, with_reference_raw(m, fx, pre)


def shape_model_at_reference_raw(shape):
    m, (fx, pre) = fc.shape_model(gpr, shape)
    return m, with_reference_raw(m, fx, pre)


def err_scored(got, want):
    """err over the scored points; the skipped ones are NaN on both sides"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape and np.array_equal(np.isnan(got), np.isnan(want))
    return err(got[~np.isnan(want)], want[~np.isnan(want)])


def check_case(case, name, tol=TOL):
    """score, mean and variance of (case, layout) on whatever device handle the model gets, against the goldens; -> (model, largest error)"""
    pre = "%s__%s__" % (case, name)
    m, _ = model_at_reference_raw(case)
    order, cut = fc.layout(case, name, m)
    score = m.forecast_log_likelihood(order, cut)
    assert score.shape == (cut.shape[0],)
    worst = err(score, FX[pre + "score"])
    print(pre, "score", worst)
    assert worst <= tol, (score, FX[pre + "score"])
    if not loo_cases.CASES[case].get("light"):
        mu, var = m.forecast(order, cut)
        assert mu.shape == var.shape == cut.shape and mu.dtype == var.dtype == config.dtype
        skipped = np.empty(cut.shape, dtype=bool)
        skipped[:, order] = cut < 0                              # the outputs are in the model's row order
        assert np.array_equal(np.isnan(mu), skipped)
        for what, got in (("mu", mu), ("var", var)):
            e = err_scored(got, FX[pre + what])
            print(pre, what, e)
            assert e <= tol, what
            worst = max(worst, e)
    return m, worst


@pytest.mark.parametrize("case,name", fc.PAIRS)
def test_twin_matches_the_reference(case, name, monkeypatch):
    forecast_twin.install(monkeypatch, loo_cases.twin_kind(case))
    m, _ = check_case(case, name)
    assert isinstance(m._handle, forecast_twin.ForecastTableDevice)


def test_the_layouts_hold_what_they_are_there_for():
    Hs, cuts, skipped, interleaved, shuffled = set(), set(), False, False, False
    for case, name in fc.PAIRS:
        m, _ = loo_cases.exact(gpr, case)
        X = cv_cases.model_inputs(m)
        order, cut = fc.layout(case, name, m)
        assert m._forecast_args(order, cut)[1].shape == cut.shape          # the host's own check takes every layout
        Hs.add(cut.shape[0])
        cuts |= set(np.unique(cut).tolist()) & {0, 127, 128, 129}
        skipped |= bool(np.any(cut < 0))
        in_time = np.array_equal(order, np.argsort(X[:, -1], kind="stable"))
        shuffled |= not in_time
        interleaved |= in_time and np.unique(X[:, 0]).size == 3 and int(np.sum(np.diff(X[order, 0]) != 0)) > 30
    assert {1, 5, 8} <= Hs and cuts == {0, 127, 128, 129} and skipped and interleaved and shuffled
    m, _ = loo_cases.exact(gpr, "m32")
    order, cut = fc.layout("m32", "marks", m)
    assert np.array_equal(cut[4], np.arange(150)) and cut[2, 149] == 128 and cut[1, 3] == -1
    assert not np.array_equal(order, np.arange(150))             # the rows of the single-channel cases are not in time order either


@pytest.mark.parametrize("case,name", [("m32", "chain"), ("lmc", "shuffled"), ("linmean", "chain"), ("mosm", "chain")])
def test_the_chain_rule_sums_to_the_marginal_likelihood(case, name, monkeypatch):
    forecast_twin.install(monkeypatch, loo_cases.twin_kind(case))
    m, _ = model_at_reference_raw(case)
    order, cut = fc.layout(case, name, m)
    lml = float(m.log_marginal_likelihood())
    assert err(lml, float(FX["%s__%s__lml" % (case, name)])) <= TOL
    assert err(float(m.forecast_log_likelihood(order, cut[0])), lml) <= TOL


def test_a_one_dimensional_cut_gives_one_dimensional_results(monkeypatch):
    forecast_twin.install(monkeypatch)
    m, _ = model_at_reference_raw("m32")
    order, cut = fc.layout("m32", "marks", m)
    mu, var = m.forecast(order, cut)
    mu1, var1 = m.forecast(order, cut[1])
    assert mu1.shape == var1.shape == (150,) and np.array_equal(mu1, mu[1], equal_nan=True) and np.array_equal(var1, var[1], equal_nan=True)
    s1 = m.forecast_log_likelihood(order, cut[1])
    assert np.ndim(s1) == 0 and s1 == m.forecast_log_likelihood(order, cut)[1]


def test_a_fixed_mean_function_is_added_on_the_host(monkeypatch):
    """a callable that is no gpr.Mean: the device holds y - m(X), the forecast's mean gets m(X) back"""
    forecast_twin.install(monkeypatch)
    sc = cases("stationary")
    X, y, _ = sc.data("m32")
    shift = lambda Z: 0.5 + 0.1 * np.asarray(Z)[:, -1]
    plain = gpr.Exact(sc.kernel(gpr, "m32"), X, y - shift(X), variance=sc.NOISE)
    meant = gpr.Exact(sc.kernel(gpr, "m32"), X, y, variance=sc.NOISE, mean=shift)
    order, cut = fc.marks(np.concatenate([np.zeros((150, 1)), X], axis=1))
    mu0, var0 = plain.forecast(order, cut)
    mu1, var1 = meant.forecast(order, cut)
    assert err_scored(mu1, mu0 + shift(X).reshape(1, -1)) <= 1e-12 and err_scored(var1, var0) <= 1e-12
    assert err(meant.forecast_log_likelihood(order, cut), plain.forecast_log_likelihood(order, cut)) <= 1e-12


# ---- Model.forecast_origins ---------------------------------------------------------------------------------------------------------------
def two_channel_model(xa, xb, inference=None):
    return mogptk_amd.Model(mogptk_amd.DataSet(mogptk_amd.Data(xa, np.sin(xa), name="a"), mogptk_amd.Data(xb, np.cos(xb), name="b")),
                            gpr.IndependentMultiOutputKernel(gpr.SquaredExponentialKernel(), gpr.SquaredExponentialKernel(), output_dims=2),
                            inference=inference or mogptk_amd.Exact(variance=0.1))


def test_forecast_origins_on_a_grid_with_ties_across_channels():
    """two channels on the same 0.1-step grid, the second given backwards: ties in time, and x - 0.1 that is not a grid value in floating point"""
    xa = 0.1 * np.arange(12)
    xb = xa[::-1].copy()
    mm = two_channel_model(xa, xb)
    order, cut = mm.forecast_origins([0.1, 0.3])
    X = np.asarray(mm.gpr.X, dtype=np.float64)
    assert np.array_equal(order, fc.horizons((0.1, 0.3))(X)[0]) and np.array_equal(cut, fc.horizons((0.1, 0.3))(X)[1])
    assert np.array_equal(order, np.argsort(X[:, 1], kind="stable"))
    assert np.array_equal(X[order, 0], np.tile([0.0, 1.0], 12))              # a tie keeps the model's row order: channel a first
    step = np.round(X[order, 1] / 0.1).astype(int)
    # horizon 0.1: both points of every earlier grid step, none of the point's own step, whatever rounding does to x - 0.1
    assert np.array_equal(cut[0], np.where(step >= 1, 2 * step, -1))
    assert np.array_equal(cut[1], np.where(step >= 3, 2 * (step - 2), -1))
    assert np.all(cut <= np.arange(24))
    order1, cut1 = mm.forecast_origins(0.1, min_train=5)
    assert cut1.shape == (1, 24) and np.array_equal(cut1[0], np.where(step >= 3, 2 * step, -1))       # 2 and 4 earlier points are fewer than 5
    assert np.array_equal(mm.forecast_origins(0.1, min_train=0)[1][0], 2 * step)                     # the prior predictive is a forecast too


def test_forecast_origins_refuses_what_it_cannot_order():
    xa = 0.1 * np.arange(12)
    mm = two_channel_model(xa, xa)
    for bad in (0.0, -1.0, [0.1, 1e-12]):
        with pytest.raises(ValueError, match="horizon"):
            mm.forecast_origins(bad)
    with pytest.raises(ValueError, match="horizons"):
        mm.forecast_origins([])
    with pytest.raises(ValueError, match="min_train"):
        mm.forecast_origins(0.1, min_train=-1)
    x2d = np.random.default_rng(3).uniform(0, 1, (9, 2))
    m3 = mogptk_amd.Model(mogptk_amd.DataSet(mogptk_amd.Data(x2d, x2d[:, 0], name="a")),
                          gpr.IndependentMultiOutputKernel(gpr.SquaredExponentialKernel(input_dims=2), output_dims=1), inference=mogptk_amd.Exact())
    for call in (lambda: m3.forecast_origins(0.1), lambda: m3.backtest(0.1), lambda: m3.forecast_error(0.1), lambda: m3.forecast_log_likelihood(0.1)):
        with pytest.raises(ValueError, match="one input dimension"):
            call()


# ---- refusals, all before any device call -------------------------------------------------------------------------------------------------
class NoDevice:
    def __init__(self, *a, **k):
        raise AssertionError("a device handle was created")


def test_bad_orders_and_cuts_are_refused_by_name_before_any_device_call(monkeypatch):
    from mogptk_amd import _lib
    monkeypatch.setattr(_lib, "ExactHandle", NoDevice)
    m, _ = loo_cases.exact(gpr, "m32")
    N = m.X.shape[0]
    order, p = np.arange(N), np.arange(N)
    twice = order.copy(); twice[5] = 4
    over = p.copy(); over[7] = 8
    under = np.stack([p, p]); under[1, 9] = -2
    bad = [
        (order[:-1], p, r"order must hold one integer row index per training point"),
        (order.astype(np.float64), p, r"order must hold one integer row index"),
        (twice, p, r"order is not a permutation of 0 \.\. 149"),
        (order + 1, p, r"order is not a permutation"),
        (order, p[:-1], r"cut must hold one integer per training point"),
        (order, p.astype(np.float64), r"cut must hold one integer per training point"),
        (order, np.zeros((9, N), dtype=np.int64), r"cut holds 9 horizons: one call takes 1 \.\. 8"),
        (order, np.zeros((0, N), dtype=np.int64), r"cut holds 0 horizons"),
        (order, over, r"cut\[0, 7\] = 8"),
        (order, under, r"cut\[1, 9\] = -2"),
    ]
    for o, c, message in bad:
        for call in (m.forecast, m.forecast_log_likelihood):
            with pytest.raises(ValueError, match=message):
                call(o, c)


def test_sharded_evaluation_is_refused_before_any_device_call(monkeypatch):
    from mogptk_amd import _lib
    monkeypatch.setattr(_lib, "ExactHandle", NoDevice)
    monkeypatch.setattr(config, "comm", type("Comm", (), dict(world=2, rank=0, force=False, native=True))(), raising=False)
    m, _ = loo_cases.exact(gpr, "m32")
    N = m.X.shape[0]
    for call in (m.forecast, m.forecast_log_likelihood):
        with pytest.raises(NotImplementedError, match="rolling-origin forecast is not carried through the sharded"):
            call(np.arange(N), np.arange(N))


def test_other_models_have_no_forecast(monkeypatch):
    from mogptk_amd import _lib
    monkeypatch.setattr(_lib, "ExactHandle", NoDevice)
    sc = cases("stationary")
    X, y, _ = sc.data("se0")
    for m in (gpr.Titsias(sc.kernel(gpr, "se0"), X, y, Z=5), gpr.Snelson(sc.kernel(gpr, "se0"), X, y, Z=5),
              gpr.OpperArchambeau(sc.kernel(gpr, "se0"), X, y), gpr.Hensman(sc.kernel(gpr, "se0"), X, y)):
        for name in ("forecast", "forecast_log_likelihood"):
            assert not hasattr(m, name), (m.name(), name)
    xa = 0.1 * np.arange(12)
    mm = two_channel_model(xa, xa, inference=mogptk_amd.Titsias(inducing_points=5))
    for call in (lambda: mm.forecast_log_likelihood(0.1), lambda: mm.backtest(0.1), lambda: mm.forecast_error(0.1)):
        with pytest.raises(ValueError, match="exact inference"):
            call()


# ---- the Model-level surface against gpr.Exact.forecast, assembled by hand ----------------------------------------------------------------
def transformed_model():
    """two channels of different lengths, interleaved in time, each with a Y transformer of its own"""
    rng = np.random.default_rng(17)
    xa, xb = np.sort(rng.uniform(0, 10, 40)), np.sort(rng.uniform(0, 10, 27))
    a = mogptk_amd.Data(xa, 3.0 + np.sin(xa) + 0.05 * rng.standard_normal(40), name="a")
    b = mogptk_amd.Data(xb, np.exp(0.2 * xb + 0.05 * rng.standard_normal(27)), name="b")
    a.transform(mogptk_amd.TransformDetrend(degree=1))
    b.transform(mogptk_amd.TransformLog())
    return mogptk_amd.Model(mogptk_amd.DataSet(a, b),
                            gpr.IndependentMultiOutputKernel(gpr.SquaredExponentialKernel(), gpr.MaternKernel(nu=1.5), output_dims=2),
                            inference=mogptk_amd.Exact(variance=0.05))


def check_model_surface():
    mm = transformed_model()
    hs = [0.25, 1.0, 2.5]
    order, cut = mm.forecast_origins(hs, min_train=4)
    assert np.any(cut < 0) and cut.shape == (3, 67)
    mu, var = mm.gpr.forecast(order, cut)
    rows = [slice(0, 40), slice(40, 67)]
    Xtrain, Ytrain = mm.dataset.get_train_data()
    y = np.asarray(mm.gpr.y, dtype=np.float64).reshape(1, -1)
    terms = -0.5 * np.log(2.0 * np.pi * var) - 0.5 * np.square(y - mu) / var

    assert err(mm.forecast_log_likelihood(hs, min_train=4), mm.gpr.forecast_log_likelihood(order, cut)) <= 1e-12
    per = mm.forecast_log_likelihood(hs, min_train=4, per_channel=True)
    assert per.shape == (3, 2) and err(per, np.stack([np.nansum(terms[:, r], axis=1) for r in rows], axis=1)) <= 1e-12

    X, bmu, lo, up = mm.backtest(hs, sigma=3, min_train=4)
    Xt, tmu, tlo, tup = mm.backtest(hs, sigma=3, min_train=4, transformed=True)
    s = 3.0 * np.sqrt(var)
    for j, r in enumerate(rows):
        assert np.array_equal(X[j], Xtrain[j]) and bmu[j].shape == lo[j].shape == up[j].shape == (3, r.stop - r.start)
        back = mm.dataset[j].Y_transformer.backward
        for got, raw, want in ((bmu[j], tmu[j], mu[:, r]), (lo[j], tlo[j], (mu - s)[:, r]), (up[j], tup[j], (mu + s)[:, r])):
            assert np.array_equal(raw, want, equal_nan=True)
            for h in range(3):
                assert np.array_equal(got[h], np.reshape(back(want[h], Xtrain[j]), -1), equal_nan=True)
    assert np.array_equal(np.isnan(bmu[0]), np.isnan(mu[:, rows[0]]))

    pred = np.concatenate([np.stack([np.reshape(mm.dataset[j].Y_transformer.backward(mu[h, r], Xtrain[j]), -1) for h in range(3)]) for j, r in enumerate(rows)], axis=1)
    truth = np.concatenate(Ytrain)
    for method, f in (("MAE", lambda t, q: np.mean(np.abs(t - q))), ("rmse", lambda t, q: np.sqrt(np.mean((t - q) ** 2)))):
        got = mm.forecast_error(hs, method=method, min_train=4)
        want = [f(truth[~np.isnan(mu[h])], pred[h][~np.isnan(mu[h])]) for h in range(3)]
        assert got.shape == (3,) and err(got, np.array(want)) <= 1e-12
    with pytest.raises(ValueError, match="MAE, MAPE"):
        mm.forecast_error(hs, method="nope")
    # more horizons than one device call takes: chunks, same numbers
    many = np.linspace(0.2, 3.0, 11)
    o11, c11 = mm.forecast_origins(many)
    want = np.concatenate([mm.gpr.forecast_log_likelihood(o11, c11[:8]), mm.gpr.forecast_log_likelihood(o11, c11[8:])])
    assert err(mm.forecast_log_likelihood(many), want) <= 1e-12
    return mm


def test_model_backtest_error_and_likelihood_are_assembled_from_the_forecast(monkeypatch):
    forecast_twin.install(monkeypatch)
    mm = check_model_surface()
    assert isinstance(mm.gpr._handle, forecast_twin.ForecastTableDevice)
    # a single channel gives bare arrays, as predict does
    sc = cases("stationary")
    X, y, _ = sc.data("m32")
    one = mogptk_amd.Model(mogptk_amd.DataSet(mogptk_amd.Data(X[:, 0], y, name="a")), gpr.IndependentMultiOutputKernel(sc.kernel(gpr, "m32"), output_dims=1),
                           inference=mogptk_amd.Exact(variance=sc.NOISE))
    Xo, mu, lo, up = one.backtest(0.5)
    assert Xo.shape[0] == 150 and mu.shape == lo.shape == up.shape == (1, 150)
