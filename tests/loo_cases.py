"""
The models of tests/golden/loo.npz (the leave-one-out predictive likelihood), built the same way on either side: `G` is the
reference's `mogptk.gpr` (tests/golden/gen_loo.py) or this package's `mogptk_amd.gpr` (tests/test_loo_*.py).  Nothing new is defined where an
existing case fits: a case names a case of a family's module (stationary_cases, product_cases, trend_cases, changepoint_cases,
function_cases: built through family_cases.exact; the raw parameters are the family fixture's), of mean_cases, or a spectral fixture
(tests/golden/lml_<name>.npz: inputs, targets, jitter and raw parameters, as gen_golden.py wrote them).  numpy only.

Shapes: N = 150 is three ragged 64-point moment tiles and two 128-row factor tiles; two channels of 70 and 45 points give tiles that stop at
a channel boundary; N = 1100 takes the dataflow schedule.  cond(Kj) stays below 1e5 (the generator asserts it).
"""
import numpy as np
import family_cases
import mean_cases
from helpers import load

CASES = {
    # family cases: (family, case)
    "m32":      dict(family="stationary", case="m32"),           # one profile row
    "sum":      dict(family="stationary", case="sum"),           # a Gaussian, a Matern and a spectral row
    "m12_per":  dict(family="product", case="m12_per"),          # the r = 0 entry inside a group
    "three":    dict(family="product", case="three"),            # a three-row group
    "lin_se":   dict(family="trend", case="lin_se"),             # a dot-product row: the per-point diagonal in the jitter term
    "gate":     dict(family="changepoint", case="two"),          # gate rows
    "wdot":     dict(family="function", case="trend"),           # a weighted-dot row, three device columns
    "white":    dict(family="function", case="white"),
    "imo":      dict(family="stationary", case="imo"),           # two channels
    "lmc":      dict(family="stationary", case="lmc"),
    "big":      dict(family="stationary", case="big", light=True),      # N = 1100: the value and the gradients only, on both schedules
    # spectral fixtures
    "mosm":     dict(spectral="mosm_c3q2"),                      # three channels, Q = 2: the Gaussian dense moments
    "mohsm":    dict(spectral="mohsm_c3q2"),                     # enveloped rows of width 2 + 5 D
    # a trainable mean
    "linmean":  dict(mean="lin_mosm2_d1"),
    # per-point variances beside the trained one
    "datavar":  dict(family="stationary", case="se0", data_variance=True),
}
ADAM_CASE, ADAM_ITERS, ADAM_LR = "m32", 20, 0.05                 # Model.train('Adam', objective='loo'): the recorded trace
BRUTE_CASE = "m32"                                               # the closed form against N refits, in the generator
BANDED = dict(N=1100, span=300.0, lengthscale=0.5)               # a long series under a short squared-exponential kernel: the LML gradient's inverse is banded


def twin_kind(case):
    """which family twin carries the case's row kinds in front of the oracle's (None: the oracle's own)"""
    return {"changepoint": "changepoint", "function": "function"}.get(CASES[case].get("family"))


def data_variance(case):
    c = CASES[case]
    if not c.get("data_variance"):
        return None
    X, _, _ = family_cases.cases(c["family"]).data(c["case"])
    return np.random.default_rng(41).uniform(0.01, 0.1, X.shape[0])


def spectral_kernel(G, kind, C, Q, D):
    if kind == "mosm":
        return G.MultiOutputSpectralMixtureKernel(Q=Q, output_dims=C, input_dims=D)
    if kind == "mohsm":
        return G.MixtureKernel(G.MultiOutputHarmonizableSpectralKernel(output_dims=C, input_dims=D), Q)
    raise ValueError(kind)


def exact(G, case):
    """-> (the case's Exact model built with G, (fixture, key prefix) of the raw parameters that go in)"""
    c = CASES[case]
    if "family" in c:
        kw = {}
        dv = data_variance(case)
        if dv is not None:
            kw["data_variance"] = dv
        return family_cases.exact(c["family"], G, c["case"], **kw), (load(c["family"] + ".npz"), c["case"] + "__")
    if "mean" in c:
        return mean_cases.exact(G, c["mean"]), (load("mean.npz"), c["mean"] + "__")
    fx = load("lml_%s.npz" % c["spectral"])
    C, Q, D = [int(v) for v in fx["meta"][:3]]
    scale = fx["p%d_cons" % (len(fx["names"]) - 1)]
    m = G.Exact(spectral_kernel(G, str(fx["kind"]), C, Q, D), fx["X"], fx["y"], variance=np.square(scale), jitter=float(fx["jitter"]))
    return m, (fx, "")


def banded(G):
    """the inverse-completeness case of the device tests: no golden, the twin's float64 inverse is the yardstick"""
    rng = np.random.default_rng(77)
    X = np.sort(rng.uniform(0.0, BANDED["span"], (BANDED["N"], 1)), axis=0)
    y = np.sin(X[:, 0]) + 0.1 * rng.standard_normal(BANDED["N"])
    k = G.SquaredExponentialKernel(order=0, input_dims=1)
    k.magnitude.assign(1.0)
    k.lengthscale.assign(BANDED["lengthscale"])
    return G.Exact(k, X, y, variance=0.1)
