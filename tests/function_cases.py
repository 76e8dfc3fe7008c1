"""
The models of tests/golden/function.npz, built the same way on either side: `G` is the reference's `mogptk.gpr` (tests/golden/gen_family.py)
or this package's `mogptk_amd.gpr` (tests/test_function_*.py, tests/kernel_family.py).  Only seeded numpy inputs go in.

Shapes as in the other families: N = 150 is three 64-point tile rows with a ragged last one; two channels of 70 and 45 points give tiles that
stop at a channel boundary; N = 1100 is the smallest size that takes the dataflow schedule.  Inputs over [0, 10], noise variance 0.1.  In
every case rows 13 and 97 coincide and one test row equals a training row: that is what tells a white kernel that is the identity by
index from one that is the identity by distance.  The feature maps are defined once, by name (FEATURES), and built with torch for the
reference and with numpy for this package; their values stay of order one over [0, 10].  The generator asserts cond(K + s2 I) < 1e5, so the
exact model's accurate-mode repeat never engages.
"""
from functools import partial
import numpy as np
import family_cases
from family_cases import top

NOISE = 0.1
ADAM_CASE, ADAM_ITERS, ADAM_LR = "trend", 20, 0.05
CASES = {
    # 1. single output, N = 150
    "alone":       dict(kern="f2", N=150),                  # kind 9 on its own
    "trend":       dict(kern="f2+se", N=150),               # three device columns
    "modulated":   dict(kern="fs*se", N=150),               # kind 9 as a factor of a group
    "four":        dict(kern="f4+m32", N=150),              # five device columns: the generic instantiation
    "seasonal":    dict(kern="f2+per", N=150),              # a periodic row beside feature columns
    "bandlimited": dict(kern="f2+sinc", N=150),             # a sinc row beside feature columns
    "white":       dict(kern="white+se", N=150),            # kind 10 in a sum
    "white_f":     dict(kern="white*f2+se", N=150),         # kind 10 multiplying kind 9
    "white_se":    dict(kern="white*se+se", N=150),         # kind 10 multiplying a profile
    # 2. two channels of 70 and 45 points
    "imo": dict(kern="imo", n=(70, 45)),                    # different rows per channel
    "lmc": dict(kern="lmc", n=(70, 45)),                    # amplitude scaling of kinds 9 and 10
    # 3. seven single rows, then fs * se: T = 9, the group would straddle the 8-row chunk
    "straddle": dict(kern="straddle", N=150),
    # 4. the dataflow schedule: LML and gradients only
    "big": dict(kern="f2+se+white", N=1100, light=True),
}

# basis functions by name, of the first input column t
FEATURES = {"f2": ("one", "lin"), "fs": ("sin", "cos"), "f4": ("one", "lin", "sin", "cos")}


def feature_map(G, name):
    """phi of FEATURES[name]: tensors in, tensors out for the reference; arrays for this package"""
    if G.__name__.split(".")[0] == "mogptk":
        import torch as lib
    else:
        lib = np
    cols = FEATURES[name]

    def phi(x):
        t = x[:, 0]
        col = {"one": lambda: lib.ones_like(t), "lin": lambda: t / 10.0, "sin": lambda: lib.sin(t / 2.0), "cos": lambda: lib.cos(t / 2.0)}
        return lib.stack([col[c]() for c in cols], 1)
    return phi


def data(case, seed=11):
    c = CASES[case]
    rng = np.random.default_rng(seed + sum(map(ord, case)))
    if "n" in c:
        n = c["n"]
        xs = np.concatenate([rng.uniform(0, 10, (k, 1)) for k in n])
        ch = np.concatenate([np.full(k, float(j)) for j, k in enumerate(n)])
        xs[97] = xs[13]                                     # (rows 13 and 97: channels 0 and 1)
        y = np.sin(xs[:, 0] * (1.0 + 0.4 * ch)) + 0.15 * xs[:, 0] + 0.3 * ch + 0.1 * rng.standard_normal(len(ch))
        X = np.concatenate([ch[:, None], xs], axis=1)
        Xs = np.concatenate([np.concatenate([np.full((20, 1), float(j)), rng.uniform(-0.5, 10.5, (20, 1))], axis=1) for j in range(len(n))])
        Xs[3] = X[13]                                       # a test row that is a training row
        return X, y, Xs
    N = c["N"]
    X = rng.uniform(0, 10, (N, 1))
    X[97] = X[13]                                           # rows of different tiles
    y = np.sin(X[:, 0]) + 0.15 * X[:, 0] + 0.5 * np.cos(X[:, 0] / 2.0) + 0.1 * rng.standard_normal(N)      # a trend, a slow wave, a fast one
    Xs = rng.uniform(-0.5, 10.5, (40, 1))
    Xs[3] = X[13]
    return X, y, Xs


def single(G, kern, D, rng):
    if kern in FEATURES:
        k = G.FunctionKernel(feature_map(G, kern), input_dims=D)
        k.magnitude.assign(rng.uniform(0.3, 1.0, len(FEATURES[kern])))
        return k
    if kern == "white":
        k = G.WhiteKernel(input_dims=D)
        k.magnitude.assign(rng.uniform(0.05, 0.2))
        return k
    if kern == "cos":
        k = G.CosineKernel(input_dims=D)
        k.magnitude.assign(rng.uniform(0.6, 1.4))
        k.lengthscale.assign(rng.uniform(2.0, 5.0, D))
        return k
    if kern == "per":
        k = G.PeriodicKernel(order=0, input_dims=D)
        k.magnitude.assign(rng.uniform(0.6, 1.4))
        k.period.assign(rng.uniform(2.0, 4.0, D))
        k.lengthscale.assign(rng.uniform(0.7, 1.5, D))
        return k
    if kern == "sinc":
        k = G.SincKernel(input_dims=D)
        k.magnitude.assign(rng.uniform(0.6, 1.4))
        k.frequency.assign(rng.uniform(0.1, 0.3, D))
        k.bandwidth.assign(rng.uniform(0.5, 1.5, D))
        return k
    if kern == "se":
        k = G.SquaredExponentialKernel(order=0, input_dims=D)
    elif kern == "rq":
        k = G.RationalQuadraticKernel(alpha=0.7, order=0, input_dims=D)
    else:
        k = G.MaternKernel(nu={"m12": 0.5, "m32": 1.5, "m52": 2.5}[kern], input_dims=D)
    k.magnitude.assign(rng.uniform(0.6, 1.4))
    k.lengthscale.assign(rng.uniform(0.3, 1.0, tuple(k.lengthscale().shape)))
    return k


parse = partial(family_cases.parse, single)


def kernel(G, case, seed=31):
    c = CASES[case]
    rng = np.random.default_rng(seed + sum(map(ord, case)))
    kern = c["kern"]
    if kern == "straddle":
        return G.AddKernel(*[single(G, e, 1, rng) for e in ("se", "m32", "cos", "rq", "m52", "per", "m12")], parse(G, "fs*se", 1, rng))
    if kern == "imo":
        return G.IndependentMultiOutputKernel(parse(G, "f2+se", 1, rng), parse(G, "white+m32", 1, rng), output_dims=2)
    if kern == "lmc":
        k = G.LinearModelOfCoregionalizationKernel(single(G, "f2", 1, rng), single(G, "white", 1, rng), single(G, "se", 1, rng),
                                                   output_dims=2, input_dims=1, Rq=2)
        k.weight.assign(rng.uniform(0.4, 1.1, (2, 3, 2)))
        return k
    return top(G, parse(G, kern, 1, rng))


def checkpoint_kernels(G):
    """(tag, channels, points per channel, kernel) of function_checkpoints.npz: a white kernel in a sum, and one under LMC.  A FunctionKernel
    holds code and is not written to checkpoints."""
    return [("wm", 1, 40, G.AddKernel(G.WhiteKernel(), G.MaternKernel(nu=1.5))),
            ("lmc", 2, 30, G.LinearModelOfCoregionalizationKernel(G.WhiteKernel(), G.SquaredExponentialKernel(), output_dims=2, Rq=2))]


def shake_range(G, module, name):
    """the range a checkpoint model's parameter `name` of `module` is drawn from"""
    return (0.05, 0.3) if isinstance(module, G.WhiteKernel) else (0.4, 1.2)
