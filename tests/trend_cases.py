"""
The models of tests/golden/trend.npz, built the same way on either side: `G` is the reference's `mogptk.gpr` (tests/golden/gen_family.py) or
this package's `mogptk_amd.gpr` (tests/test_trend_*.py, tests/kernel_family.py).  Only seeded numpy inputs go in.

Shapes as in product_cases.py: N = 150 is three 64-point tile rows with a ragged last one; two channels of 70 and 45 points give tiles that
stop at a channel boundary; N = 1100 is the smallest size that takes the dataflow schedule.  Inputs over [0, 10], noise variance 0.1.  In
every single-channel case rows 13 and 97 coincide (r = 0 off the diagonal: the sinc series) and one test row equals a training row.
Dot-product magnitudes in [0.01, 0.03] and biases in [0.2, 0.8] keep (mag x x' + bias)^n of order one over [0, 10]; sinc bandwidth 0.7 and
frequency 0.3, Matern and squared-exponential lengthscale 0.6, period 3.  The generator asserts cond(K + s2 I) < 1e5, so the exact model's
accurate-mode repeat never engages.
"""
from functools import partial
import numpy as np
import family_cases
from family_cases import top

NOISE = 0.1
ADAM_CASE, ADAM_ITERS, ADAM_LR = "lin_per", 20, 0.05
CASES = {
    # 1. single output, D = 1, N = 150
    "lin":      dict(kern="lin", N=150),
    "poly2":    dict(kern="poly2", N=150),
    "poly3":    dict(kern="poly3", N=150),
    "lin_se":   dict(kern="lin+se", N=150),                 # a trend beside a stationary kernel
    "lin_per":  dict(kern="lin*per", N=150),                # growing amplitude: the dot-product row first in its group
    "poly2_m32": dict(kern="poly2*m32", N=150),
    "sinc":     dict(kern="sinc", N=150),                   # kind 6 alone
    "sinc_lin": dict(kern="sinc*lin", N=150),               # the dot-product row last in its group
    # 2. input_dims = 2
    "lin_d2":   dict(kern="lin", N=150, D=2),
    # 3. two channels of 70 and 45 points
    "imo": dict(kern="imo", n=(70, 45)),
    "lmc": dict(kern="lmc", n=(70, 45)),
    # 4. seven single rows, then a two-row group with the dot-product row: T = 9, the group would straddle the 8-term chunk
    "straddle": dict(kern="straddle", N=150),
    # 5. the dataflow schedule: LML and gradients only
    "big": dict(kern="big", N=1100, light=True),
}


def data(case, seed=7):
    c = CASES[case]
    rng = np.random.default_rng(seed + sum(map(ord, case)))
    D = c.get("D", 1)
    if "n" in c:
        n = c["n"]
        xs = np.concatenate([rng.uniform(0, 10, (k, D)) for k in n])
        ch = np.concatenate([np.full(k, float(j)) for j, k in enumerate(n)])
        y = np.sin(xs[:, 0] * (1.0 + 0.4 * ch)) + 0.1 * xs[:, 0] + 0.3 * ch + 0.1 * rng.standard_normal(len(ch))
        X = np.concatenate([ch[:, None], xs], axis=1)
        Xs = np.concatenate([np.concatenate([np.full((20, 1), float(j)), rng.uniform(-0.5, 10.5, (20, D))], axis=1) for j in range(len(n))])
        Xs[3] = X[13]                                       # a test row that is a training row
        return X, y, Xs
    N = c["N"]
    X = rng.uniform(0, 10, (N, D))
    X[97] = X[13]                                           # rows of different tiles
    y = np.sin(X[:, 0]) + 0.15 * X[:, 0] + 0.3 * np.cos(2.0 * X[:, -1]) + 0.1 * rng.standard_normal(N)
    Xs = rng.uniform(-0.5, 10.5, (40, D))
    Xs[3] = X[13]                                           # r = 0 in the rectangular Gram too
    return X, y, Xs


def single(G, kern, D, rng):
    if kern in ("lin", "poly2", "poly3"):
        k = G.LinearKernel(input_dims=D) if kern == "lin" else G.PolynomialKernel(int(kern[-1]), input_dims=D)
        k.magnitude.assign(rng.uniform(0.01, 0.03))
        k.bias.assign(rng.uniform(0.2, 0.8))
        return k
    if kern == "sinc":
        k = G.SincKernel(input_dims=D)
        k.magnitude.assign(rng.uniform(0.6, 1.4))
        k.bandwidth.assign(np.full(D, 0.7))
        k.frequency.assign(np.full(D, 0.3))
        return k
    if kern == "per":
        k = G.PeriodicKernel(order=0, input_dims=D)
        k.magnitude.assign(rng.uniform(0.6, 1.4))
        k.period.assign(np.full(D, 3.0))
        k.lengthscale.assign(np.full(D, 1.0))
        return k
    k = G.SquaredExponentialKernel(order=0, input_dims=D) if kern == "se" else G.MaternKernel(nu=1.5, input_dims=D)
    k.magnitude.assign(rng.uniform(0.6, 1.4))
    k.lengthscale.assign(np.full(D, 0.6))
    return k


parse = partial(family_cases.parse, single)


def kernel(G, case, seed=29):
    c = CASES[case]
    rng = np.random.default_rng(seed + sum(map(ord, case)))
    D = c.get("D", 1)
    kern = c["kern"]
    if kern == "straddle":
        return parse(G, "se+m32+sinc+se+m32+per+sinc+lin*per", D, rng)
    if kern == "big":
        return parse(G, "lin*per+m32", D, rng)
    if kern == "imo":
        return G.IndependentMultiOutputKernel(parse(G, "lin*per", D, rng), single(G, "sinc", D, rng), output_dims=2)
    if kern == "lmc":
        k = G.LinearModelOfCoregionalizationKernel(single(G, "lin", D, rng), single(G, "m32", D, rng), output_dims=2, input_dims=D, Rq=2)
        k.weight.assign(rng.uniform(0.4, 1.1, (2, 2, 2)))
        return k
    return top(G, parse(G, kern, D, rng))


def checkpoint_kernels(G):
    """(tag, channels, points per channel, kernel) of trend_checkpoints.npz: linear, polynomial and sinc kernels inside AddKernel, MulKernel
    and LMC"""
    return [("trend", 1, 40, G.AddKernel(G.MulKernel(G.LinearKernel(), G.PeriodicKernel()), G.PolynomialKernel(2), G.SincKernel())),
            ("lmc", 2, 30, G.LinearModelOfCoregionalizationKernel(G.LinearKernel(), G.MulKernel(G.SincKernel(), G.PolynomialKernel(3)), output_dims=2, Rq=2))]


def shake_range(G, module, name):
    """the range a checkpoint model's parameter `name` of `module` is drawn from: (mag x x' + bias)^n stays of order one"""
    small = name == "magnitude" and isinstance(module, (G.LinearKernel, G.PolynomialKernel))
    return (0.01, 0.03) if small else (0.4, 1.2)
