"""
The models of tests/golden/product.npz, built the same way on either side: `G` is the reference's `mogptk.gpr` (tests/golden/gen_family.py)
or this package's `mogptk_amd.gpr` (tests/test_product_*.py, tests/kernel_family.py).  Only seeded numpy inputs go in.

Shapes as in stationary_cases.py: N = 150 is three 64-point tile rows with a ragged last one; two channels of 70 and 45 points give tiles
that stop at a channel boundary; N = 1100 is the smallest size that takes the dataflow schedule.  Inputs over [0, 10], noise variance 0.1,
magnitudes <= 1.4: the generator asserts cond(K + s2 I) < 1e5, so the exact model's accurate-mode repeat never engages.
"""
from functools import partial
import numpy as np
import family_cases
from family_cases import top

NOISE = 0.1
ADAM_CASE, ADAM_ITERS, ADAM_LR = "m32_cos", 20, 0.05
CASES = {
    # 1. single output, D = 1, N = 150
    "se_cos":   dict(kern="se*cos", N=150),
    "m32_cos":  dict(kern="m32*cos", N=150),                # quasi-periodic
    "m12_per":  dict(kern="m12*per", N=150, dup=True),      # two coincident inputs: the r = 0 entry inside a group
    "const_rq": dict(kern="const*rq", N=150),               # a scaled kernel
    "per":      dict(kern="per", N=150),                    # kind 5 alone
    "locper":   dict(kern="locper", N=150),
    "cos":      dict(kern="cos", N=150),                    # an ordinary table: no kinds travel
    "const_se": dict(kern="const+se", N=150),
    "dist":     dict(kern="(se+m52)*cos", N=150),           # (a + b) c = a c + b c: the cosine row is used twice
    "three":    dict(kern="se*cos*per", N=150),
    "straddle": dict(kern="straddle", N=150),               # seven single rows, then a two-row group: T = 9, the group would straddle the 8-term chunk
    "lowmag":   dict(kern="lowmag", N=150),                 # one factor's magnitude at its lower bound
    # 2. input_dims = 2
    "se_cos_d2":   dict(kern="se*cos", N=150, D=2),
    "rq_const_d2": dict(kern="rq*const", N=150, D=2),
    # 3. two channels of 70 and 45 points
    "imo": dict(kern="imo", n=(70, 45)),
    "lmc": dict(kern="lmc", n=(70, 45)),
    # 4. the dataflow schedule: LML and gradients only
    "big": dict(kern="big", N=1100, light=True),
}
PRODUCT_CASES = [c for c in CASES if c not in ("per", "cos", "const_se")]      # MulKernel or LocallyPeriodicKernel inside: product groups


def data(case, seed=7):
    c = CASES[case]
    rng = np.random.default_rng(seed + sum(map(ord, case)))
    D = c.get("D", 1)
    if "n" in c:
        n = c["n"]
        xs = np.concatenate([rng.uniform(0, 10, (k, D)) for k in n])
        ch = np.concatenate([np.full(k, float(j)) for j, k in enumerate(n)])
        y = np.sin(xs[:, 0] * (1.0 + 0.4 * ch)) + 0.3 * ch + 0.1 * rng.standard_normal(len(ch))
        X = np.concatenate([ch[:, None], xs], axis=1)
        Xs = np.concatenate([np.concatenate([np.full((20, 1), float(j)), rng.uniform(-0.5, 10.5, (20, D))], axis=1) for j in range(len(n))])
        return X, y, Xs
    N = c["N"]
    X = rng.uniform(0, 10, (N, D))
    if c.get("dup"):
        X[97] = X[13]                                   # rows of different tiles
    y = np.sin(X[:, 0]) + 0.3 * np.cos(2.0 * X[:, -1]) + 0.1 * rng.standard_normal(N)
    Xs = rng.uniform(-0.5, 10.5, (40, D))
    if c.get("dup"):
        Xs[3] = X[13]                                   # r = 0 in the rectangular Gram too
    return X, y, Xs


def single(G, kern, D, rng):
    if kern == "const":
        k = G.ConstantKernel(input_dims=D)
        k.magnitude.assign(rng.uniform(0.6, 1.4))
        return k
    if kern == "cos":
        k = G.CosineKernel(input_dims=D)
        k.magnitude.assign(rng.uniform(0.6, 1.4))
        k.lengthscale.assign(rng.uniform(2.0, 5.0, D))
        return k
    if kern in ("per", "locper"):
        k = (G.PeriodicKernel if kern == "per" else G.LocallyPeriodicKernel)(order=0, input_dims=D)
        k.magnitude.assign(rng.uniform(0.6, 1.4))
        k.period.assign(rng.uniform(2.0, 4.0, D))
        k.lengthscale.assign(rng.uniform(0.7, 1.5, D))
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


def kernel(G, case, seed=29):
    c = CASES[case]
    rng = np.random.default_rng(seed + sum(map(ord, case)))
    D = c.get("D", 1)
    kern = c["kern"]
    if kern == "straddle":
        return parse(G, "se+m32+cos+rq+m52+per+m12+se*cos", D, rng)
    if kern == "lowmag":
        k = parse(G, "se*cos+m32", D, rng)
        cos = k.kernels[0].kernels[1]
        cos.magnitude.assign(float(np.asarray(cos.magnitude.lower).reshape(-1)[0]))
        return k
    if kern == "big":
        return parse(G, "se*cos+m32", D, rng)
    if kern == "imo":
        return G.IndependentMultiOutputKernel(parse(G, "se*cos", D, rng), parse(G, "m52*per", D, rng), output_dims=2)
    if kern == "lmc":
        k = G.LinearModelOfCoregionalizationKernel(parse(G, "se*cos", D, rng), single(G, "m32", D, rng), output_dims=2, input_dims=D, Rq=2)
        k.weight.assign(rng.uniform(0.4, 1.1, (2, 2, 2)))
        return k
    return top(G, parse(G, kern, D, rng))


def checkpoint_kernels(G):
    """(tag, channels, points per channel, kernel) of product_checkpoints.npz: product, cosine, constant and periodic kernels inside
    AddKernel and LMC"""
    return [("mul", 1, 40, G.AddKernel(G.MulKernel(G.SquaredExponentialKernel(order=-1), G.CosineKernel()), G.LocallyPeriodicKernel(order=-1),
                                       G.MulKernel(G.ConstantKernel(), G.PeriodicKernel()))),
            ("lmc", 2, 30, G.LinearModelOfCoregionalizationKernel(G.MulKernel(G.MaternKernel(nu=1.5), G.CosineKernel()), G.ConstantKernel(), output_dims=2, Rq=2))]


def shake_range(G, module, name):
    """the range a checkpoint model's parameter `name` of `module` is drawn from"""
    return 0.4, 1.2
