"""
The models of tests/golden/stationary.npz, built the same way on either side: `G` is the reference's `mogptk.gpr`
(tests/golden/gen_family.py) or this package's `mogptk_amd.gpr` (tests/test_stationary_*.py, tests/kernel_family.py).  Only seeded numpy inputs go in.

Shapes: N = 150 is three 64-point tile rows with a ragged last one (diagonal and off-diagonal tiles); two channels of 70 and 45 points give
tiles that stop at a channel boundary; N = 1100 is the smallest size that takes the dataflow schedule.  Inputs over [0, 10], lengthscales
0.3 - 1 and a noise variance of 0.1 keep cond(K + s2 I) at a few hundred to a few thousand (the generator asserts < 1e5), so the exact model's
accurate-mode repeat never engages.
"""
import numpy as np

NOISE = 0.1
ADAM_CASE, ADAM_ITERS, ADAM_LR = "m32", 20, 0.05        # Model.train('Adam') on a case-1 model: the recorded loss trace
CASES = {
    # 1. single output, D = 1, N = 150
    "se0":   dict(kern="se0", N=150),
    "sem1":  dict(kern="sem1", N=150),
    "rq":    dict(kern="rq", N=150),
    "m12":   dict(kern="m12", N=150, dup=True),        # two coincident inputs: the r = 0 entry off the diagonal
    "m32":   dict(kern="m32", N=150),
    "m52":   dict(kern="m52", N=150),
    "exp":   dict(kern="exp", N=150, dup=True),
    "sum":   dict(kern="sum", N=150),                  # SE + Matern 3/2 + SpectralKernel: mixed kinds in one launch, one term with M != 0
    # 2. ARD, input_dims = 2
    "se_d2": dict(kern="se0", N=150, D=2),
    "rq_d2": dict(kern="rq", N=150, D=2),
    # 3. two channels of 70 and 45 points
    "imo":   dict(kern="imo", n=(70, 45)),             # different kinds at the same t
    "lmc":   dict(kern="lmc", n=(70, 45)),
    # 4. the dataflow schedule: LML and gradients only
    "big":   dict(kern="big", N=1100, light=True),
}


def data(case, seed=5):
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


def _single(G, kern, D, rng):
    if kern == "se0":
        k = G.SquaredExponentialKernel(order=0, input_dims=D)
    elif kern == "sem1":
        k = G.SquaredExponentialKernel(order=-1, input_dims=D)
    elif kern == "rq":
        k = G.RationalQuadraticKernel(alpha=0.7, order=0, input_dims=D)
    elif kern in ("m12", "m32", "m52"):
        k = G.MaternKernel(nu={"m12": 0.5, "m32": 1.5, "m52": 2.5}[kern], input_dims=D)
    elif kern == "exp":
        k = G.ExponentialKernel(input_dims=D)
    elif kern == "spec":
        k = G.SpectralKernel(input_dims=D)
        k.magnitude.assign(rng.uniform(0.3, 0.8))
        k.mean.assign(rng.uniform(0.1, 0.3, D))
        k.variance.assign(rng.uniform(0.02, 0.08, D))
        return k
    k.magnitude.assign(rng.uniform(0.6, 1.4))
    shape = tuple(k.lengthscale().shape)                 # () for order = -1
    ls = rng.uniform(0.3, 1.0, shape if shape else None)
    k.lengthscale.assign(0.5 * ls if kern == "exp" else ls)       # exp(-|tau| / (2 l)): half the lengthscale for the same decay
    return k


def kernel(G, case, seed=23):
    c = CASES[case]
    rng = np.random.default_rng(seed + sum(map(ord, case)))
    D = c.get("D", 1)
    kern = c["kern"]
    if kern == "sum":
        return G.AddKernel(_single(G, "se0", D, rng), _single(G, "m32", D, rng), _single(G, "spec", D, rng))
    if kern == "big":
        return G.AddKernel(_single(G, "se0", D, rng), _single(G, "m32", D, rng))
    if kern == "imo":
        return G.IndependentMultiOutputKernel(_single(G, "rq", D, rng), _single(G, "m52", D, rng), output_dims=2)
    if kern == "lmc":
        k = G.LinearModelOfCoregionalizationKernel(_single(G, "se0", D, rng), _single(G, "m32", D, rng), output_dims=2, input_dims=D, Rq=2)
        k.weight.assign(rng.uniform(0.4, 1.1, (2, 2, 2)))
        return k
    return _single(G, kern, D, rng)


def checkpoint_kernels(G):
    """(tag, channels, points per channel, kernel) of stationary_checkpoints.npz: the four kernels inside AddKernel,
    IndependentMultiOutputKernel and LMC"""
    return [("add", 1, 40, G.AddKernel(G.SquaredExponentialKernel(order=-1), G.MaternKernel(nu=1.5), G.RationalQuadraticKernel(alpha=0.7), G.ExponentialKernel())),
            ("imo", 2, 30, G.IndependentMultiOutputKernel(G.RationalQuadraticKernel(alpha=1.3), G.MaternKernel(nu=2.5), output_dims=2)),
            ("lmc", 2, 30, G.LinearModelOfCoregionalizationKernel(G.SquaredExponentialKernel(), G.ExponentialKernel(), G.MaternKernel(nu=0.5), output_dims=2, Rq=2))]


def shake_range(G, module, name):
    """the range a checkpoint model's parameter `name` of `module` is drawn from"""
    return 0.4, 1.2
