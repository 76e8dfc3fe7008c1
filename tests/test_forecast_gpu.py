"""
The rolling-origin forecast on the device (mogp_exact_forecast: csrc/forecast.hip behind the gathered, refined factorisation of csrc/exact.hip)
against the reference-side goldens (tests/golden/forecast.npz, gen_forecast.py) over the cases and cut layouts of tests/forecast_cases.py, and
against the numpy twin (tests/forecast_twin.py: direct conditional solves) at the sizes where the device code takes another path: mean, variance
and score to 1e-9 relative to max(1, max |want|).  Then: the chain rule against the device's own marginal likelihood, H cuts in one call
against H calls and repeated calls bit for bit, nothing left behind for the marginal likelihood, mogp_model_fetch, the library's own refusals, and
the Model-level surface.
"""
import numpy as np
import pytest

from mogptk_amd import _lib
import forecast_cases as fc
import forecast_twin
import loo_cases
from kernel_family import err
from test_forecast_cpu import (FX, TOL, check_case, check_model_surface, err_scored, model_at_reference_raw, shape_model_at_reference_raw)

pytestmark = pytest.mark.gpu


def on_the_twin(build, order, cut, kind=None):
    """(mu, var, score, lml) of the same model on the numpy twin"""
    with pytest.MonkeyPatch.context() as mp:
        forecast_twin.install(mp, kind)
        m, _ = build()
        mu, var = m.forecast(order, cut)
        return mu, var, m.forecast_log_likelihood(order, cut), float(m.log_marginal_likelihood())


@pytest.mark.parametrize("case,name", fc.PAIRS)
def test_score_mean_and_variance_match_the_reference_and_the_twin(case, name):
    with pytest.MonkeyPatch.context() as mp:
        forecast_twin.install(mp, loo_cases.twin_kind(case))
        _, floor = check_case(case, name)
    print(case, name, "float64 floor (numpy twin against the goldens)", floor, "cond", float(FX["%s__%s__cond" % (case, name)]))
    m, e = check_case(case, name)
    print(case, name, "device against the goldens", e)
    assert isinstance(m._handle, _lib.ExactHandle)
    if not loo_cases.CASES[case].get("light"):
        order, cut = fc.layout(case, name, m)
        mu, var, score, _ = on_the_twin(lambda: model_at_reference_raw(case), order, cut, loo_cases.twin_kind(case))
        dmu, dvar = m.forecast(order, cut)
        assert err_scored(dmu, mu) <= TOL and err_scored(dvar, var) <= TOL and err(m.forecast_log_likelihood(order, cut), score) <= TOL


def shape_layout(N):
    """H = 6 over N points in time order: the chain (above 300 points an origin every 16, which keeps the twin's direct solves to a second: the chain
    itself is held to the LML), the prefixes around column 128 (the chain below it), the prior predictive, every fifth point skipped"""
    p = np.arange(N)
    cut = np.stack([p if N <= 300 else 16 * (p // 16), np.minimum(p, 127), np.minimum(p, 128), np.minimum(p, 129), np.zeros(N, dtype=np.int64), np.where(p % 5 == 2, -1, p // 3)])
    return cut


@pytest.mark.parametrize("shape", list(fc.SHAPES))
def test_shapes_where_the_kernels_can_go_wrong(shape):
    """one partial tile, no padding, a ragged last tile, two outer blocks of the factorisation, three channels interleaved over three tiles: against
    the twin's direct solves, and the chain against the device's own LML, in time order and under a seeded permutation"""
    m, _ = shape_model_at_reference_raw(shape)
    N = m.X.shape[0]
    X = np.asarray(m.X, dtype=np.float64)
    order = np.argsort(X[:, -1], kind="stable")
    cut = shape_layout(N)
    mu, var, score, lml_twin = on_the_twin(lambda: shape_model_at_reference_raw(shape), order, cut)
    dmu, dvar = m.forecast(order, cut)
    dscore = m.forecast_log_likelihood(order, cut)
    errs = (err_scored(dmu, mu), err_scored(dvar, var), err(dscore, score))
    print(shape, "N", N, "device against the twin: mu %.2e var %.2e score %.2e" % errs)
    assert max(errs) <= TOL
    lml = float(m.log_marginal_likelihood())
    assert err(lml, lml_twin) <= TOL
    assert err(float(m.forecast_log_likelihood(order, np.arange(N))), lml) <= TOL          # (a) the time order
    shuffled = np.random.default_rng(3).permutation(N)
    assert err(float(m.forecast_log_likelihood(shuffled, np.arange(N))), lml) <= TOL       # (b) any order


@pytest.mark.parametrize("case,name", [("m32", "chain"), ("lmc", "shuffled"), ("mosm", "chain"), ("linmean", "chain")])
def test_the_chain_rule_reproduces_the_marginal_likelihood(case, name):
    m, _ = model_at_reference_raw(case)
    order, cut = fc.layout(case, name, m)
    lml = float(m.log_marginal_likelihood())
    assert err(float(m.forecast_log_likelihood(order, cut[0])), lml) <= TOL
    N = len(order)
    assert err(float(m.forecast_log_likelihood(np.random.default_rng(8).permutation(N), np.arange(N))), lml) <= TOL


@pytest.mark.parametrize("build,name", [(lambda: model_at_reference_raw("gate"), "gate"), (lambda: shape_model_at_reference_raw("n700"), "n700")])
def test_eight_cuts_in_one_call_are_eight_calls_bit_for_bit(build, name):
    m, _ = build()
    X = np.asarray(m.X, dtype=np.float64).reshape(m.X.shape[0], -1)
    order, cut = fc.eight(X)
    mu, var = m.forecast(order, cut)
    score = m.forecast_log_likelihood(order, cut)
    again = m.forecast(order, cut)
    assert mu.tobytes() == again[0].tobytes() and var.tobytes() == again[1].tobytes()
    assert score.tobytes() == m.forecast_log_likelihood(order, cut).tobytes()
    for h in range(8):
        mu1, var1 = m.forecast(order, cut[h])
        assert mu1.tobytes() == mu[h].tobytes() and var1.tobytes() == var[h].tobytes(), h
        assert np.float64(m.forecast_log_likelihood(order, cut[h])).tobytes() == np.float64(score[h]).tobytes(), h
    for H in (2, 3, 5):                                           # every width of the row kernel
        muH, varH = m.forecast(order, cut[:H])
        assert muH.tobytes() == mu[:H].tobytes() and varH.tobytes() == var[:H].tobytes(), H


def test_a_forecast_leaves_nothing_behind_for_the_marginal_likelihood():
    """N = 1100 takes the dataflow schedule: loss() and every gradient bit for bit before and after"""
    m, ps = model_at_reference_raw("big")
    order, cut = fc.layout("big", "origins", m)

    def lml_bits():
        loss = float(m.loss())
        return [np.float64(loss).tobytes()] + [p.grad.tobytes() for p in ps]

    before = lml_bits()
    assert m._handle.schedule()["dataflow"], m._handle.schedule()
    m.forecast_log_likelihood(order, cut)
    assert lml_bits() == before
    m.forecast(order, cut)
    m.predict_f(m.X[:5])
    assert lml_bits() == before


def test_fetch_reports_nothing_after_a_forecast():
    m, _ = model_at_reference_raw("m32")
    order, cut = fc.layout("m32", "chain", m)
    m.loss()
    h = m._handle
    assert h.fetch(0).shape == (150, 150)
    m.forecast(order, cut)
    for which in (0, 1, 2):
        with pytest.raises(_lib.MogpError, match="mogp_model_fetch"):
            h.fetch(which)
    m.loss()
    assert h.fetch(0).shape == (150, 150)


def test_the_library_names_what_it_cannot_take():
    """what gpr.Exact refuses on the host, sent past it"""
    m, _ = model_at_reference_raw("m32")
    m.loss()
    h, N = m._handle, m.X.shape[0]
    nv = m._noise_var()
    order, p = np.arange(N), np.arange(N)[None, :]
    twice = order.copy(); twice[5] = 4
    with pytest.raises(_lib.MogpError, match=r"order\[5\] = 4 appears twice"):
        h.forecast(nv, m.jitter, twice, p)
    away = order.copy(); away[7] = N
    with pytest.raises(_lib.MogpError, match=r"order\[7\] = 150 is out of range"):
        h.forecast(nv, m.jitter, away, p)
    cut = np.repeat(p, 3, axis=0); cut[2, 11] = 12
    with pytest.raises(_lib.MogpError, match=r"cut\[h = 2, p = 11\] = 12"):
        h.forecast(nv, m.jitter, order, cut)
    cut[2, 11] = -2
    with pytest.raises(_lib.MogpError, match=r"cut\[h = 2, p = 11\] = -2"):
        h.forecast(nv, m.jitter, order, cut)
    with pytest.raises(_lib.MogpError, match=r"H = 9 cuts per point, and a call takes 1 \.\. 8"):
        h.forecast(nv, m.jitter, order, np.repeat(p, 9, axis=0))
    assert np.all(np.isfinite(h.forecast(nv, m.jitter, order, p)["score"]))


def test_model_backtest_error_and_likelihood_on_the_device():
    mm = check_model_surface()
    assert isinstance(mm.gpr._handle, _lib.ExactHandle)
