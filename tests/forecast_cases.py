"""
The cases of tests/golden/forecast.npz (the rolling-origin forecast): models of tests/loo_cases.py -- nothing new is defined, no data and
no parameters -- each with one or two deterministic cut layouts.  A layout is a function of the model's inputs in kernel format (channel column
first: cv_cases.model_inputs) and returns (order, cut): order (N,) the model's row at every time position, cut (H, N) per horizon and time position
p the number of leading points the point's prediction may use, 0 .. p, or -1 (skipped).  numpy only; used by the generator (gen_forecast.py) and by
the tests on either side.

What the layouts cover between them: the chain rule (cut = p, whose scores sum to the LML) under the time order and under a seeded permutation,
cuts at 0, 127, 128, 129 and p (the prefix ends at, before and behind a 128-column tile edge), skipped points, H = 1, 5 and 8, the horizons
Model.forecast_origins makes (ties across channels included), channels interleaved in time, and 22 origins of 50 points at N = 1100.

The shape models (shape_model) are cut out of the N = 1100 case's own data for the sizes at which the device code takes another path; they have
no golden, the numpy twin's direct solves are their yardstick.
"""
import numpy as np

import loo_cases
import stationary_cases
from helpers import load

CASES = ("m32", "three", "gate", "wdot", "white", "imo", "lmc", "mosm", "mohsm", "linmean", "datavar", "big")
MAXH = 8


def time_order(X):
    return np.argsort(X[:, -1], kind="stable")


def chain(X):
    """every point from all the points before it in time: the terms of the chain rule of the joint density"""
    N = X.shape[0]
    return time_order(X), np.arange(N)[None, :]


def shuffled_chain(seed):
    def layout(X):
        N = X.shape[0]
        return np.random.default_rng(seed).permutation(N), np.arange(N)[None, :]
    return layout


def marks(X):
    """H = 5: the prior predictive, the prefixes that end one before, at and one behind column 128, and the chain; every seventh point skipped in rows 1 and 3"""
    N = X.shape[0]
    p = np.arange(N)
    cut = np.stack([np.zeros(N, dtype=np.int64), np.minimum(p, 127), np.minimum(p, 128), np.minimum(p, 129), p])
    cut[1, p % 7 == 3] = -1
    cut[3, p % 7 == 5] = -1
    return time_order(X), cut


def horizons(hs, min_train=1):
    """what Model.forecast_origins(hs, min_train) returns for inputs X in kernel format"""
    def layout(X):
        x = X[:, -1]
        order = time_order(X)
        xs = x[order]
        tol = 1e-9 * (x.max() - x.min())
        cut = np.stack([np.searchsorted(xs, xs - h + tol, side="right") for h in hs]).astype(np.int64)
        cut[cut < min_train] = -1
        return order, cut
    return layout


def eight(X):
    """H = 8: the chain, three lags counted in points, two seeded rows of cuts drawn from -1 .. p, the prior predictive, and half the history"""
    N = X.shape[0]
    p = np.arange(N)
    rng = np.random.default_rng(31)
    draw = lambda: np.floor(rng.random(N) * (p + 2)).astype(np.int64) - 1
    cut = np.stack([p, np.maximum(p - 1, 0), np.maximum(p - 5, 0), np.where(p >= 20, p - 20, -1), draw(), draw(), np.zeros(N, dtype=np.int64), p // 2])
    return time_order(X), cut


def origins_of_50(X):
    """a refit every 50 points: point p from the first 50 floor(p / 50)"""
    N = X.shape[0]
    return time_order(X), (50 * (np.arange(N) // 50))[None, :]


LAYOUTS = {
    "m32":     dict(chain=chain, marks=marks),
    "three":   dict(horizons=horizons((0.1, 0.5, 2.0), 5)),
    "gate":    dict(eight=eight),
    "wdot":    dict(horizons=horizons((0.3, 1.5))),
    "white":   dict(chain=chain),
    "imo":     dict(chain=chain, horizons=horizons((0.2, 1.0), 3)),
    "lmc":     dict(shuffled=shuffled_chain(13)),
    "mosm":    dict(chain=chain, eight=eight),
    "mohsm":   dict(horizons=horizons((0.25, 1.0, 3.0))),
    "linmean": dict(chain=chain, horizons=horizons((0.5,), 2)),
    "datavar": dict(marks=marks),
    "big":     dict(origins=origins_of_50),
}
PAIRS = [(case, name) for case in CASES for name in LAYOUTS[case]]
assert set(LAYOUTS) == set(CASES) and all(case in loo_cases.CASES for case in CASES)


def check_layout(order, cut, N):
    order, cut = np.asarray(order, dtype=np.int64), np.asarray(cut, dtype=np.int64)
    assert order.shape == (N,) and np.array_equal(np.sort(order), np.arange(N))
    assert cut.ndim == 2 and cut.shape[1] == N and 1 <= cut.shape[0] <= MAXH
    assert cut.min() >= -1 and np.all(cut <= np.arange(N))
    return order, cut


def layout(case, name, m):
    """the layout's (order, cut) for the model m of the case, checked"""
    import cv_cases
    X = cv_cases.model_inputs(m)
    return check_layout(*LAYOUTS[case][name](X), X.shape[0])


# ---- the shape models: rows of the N = 1100 case, no golden -------------------------------------------------------------------------
SHAPES = {
    "n50":     dict(n=50),                      # one partial tile
    "n256":    dict(n=256),                     # no padding
    "n150":    dict(n=150),                     # a ragged last tile
    "n700":    dict(n=700),                     # two 512-column outer blocks of the factorisation
    "c3_n300": dict(n=300, channels=3),         # three channels interleaved in time over three tiles: the gather crosses every channel-pair tile
}


def shape_model(G, shape):
    """-> (Exact model built with G, (fixture, key prefix) of its raw parameters): the first n rows of the `big` case under its own kernel, or -- three
    channels -- the same rows dealt to the channels in turn under the MOSM fixture's kernel"""
    s = SHAPES[shape]
    X, y, _ = stationary_cases.data("big")
    X, y = X[:s["n"]], y[:s["n"]]
    if s.get("channels", 1) == 1:
        return G.Exact(stationary_cases.kernel(G, "big"), X, y, variance=stationary_cases.NOISE), (load("stationary.npz"), "big__")
    fx = load("lml_mosm_c3q2.npz")
    C, Q, D = [int(v) for v in fx["meta"][:3]]
    assert C == s["channels"] and D == 1
    Xc = np.concatenate([(np.arange(s["n"]) % C).astype(np.float64)[:, None], X], axis=1)
    scale = fx["p%d_cons" % (len(fx["names"]) - 1)]
    return G.Exact(loo_cases.spectral_kernel(G, "mosm", C, Q, D), Xc, y, variance=np.square(scale), jitter=float(fx["jitter"])), (fx, "")
