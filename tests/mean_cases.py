"""
The models of tests/golden/mean.npz, built the same way on either side: `G` is the reference's `mogptk.gpr` (tests/golden/gen_mean.py)
or this package's `mogptk_amd.gpr` (tests/test_mean_*.py).  Only seeded numpy inputs go in, so both sides construct the same model.
"""
import numpy as np

CASES = {
    "const_sm":     dict(kern="sm",   C=1, Q=2, D=1, N=60, mean="const"),
    "const_mosm3":  dict(kern="mosm", C=3, Q=2, D=1, N=72, mean="const"),
    "lin_mosm2_d1": dict(kern="mosm", C=2, Q=2, D=1, N=64, mean="lin"),
    "lin_mosm2_d2": dict(kern="mosm", C=2, Q=1, D=2, N=64, mean="lin"),
    "mom_shuf":     dict(kern="mosm", C=2, Q=2, D=1, N=70, mean="mom", shuffle=True),
    "poly_mosm2":   dict(kern="mosm", C=2, Q=1, D=1, N=60, mean="poly"),
    "lin_mosm3_n300": dict(kern="mosm", C=3, Q=2, D=1, N=300, mean="lin"),      # three 128-row tiles: the multi-block schedules
}
SPARSE_CASES = {                       # (model, case): Titsias / Snelson with a mean, 4 inducing points per channel
    "titsias_lin": ("Titsias", "lin_mosm2_d1"),
    "titsias_mom": ("Titsias", "mom_shuf"),
    "snelson_lin": ("Snelson", "lin_mosm2_d1"),
    "snelson_mom": ("Snelson", "mom_shuf"),
    "titsias_poly": ("Titsias", "poly_mosm2"),     # a user's Mean on the sparse models: the host route through dp/dr (mogp_model_fetch 3)
    "snelson_poly": ("Snelson", "poly_mosm2"),
}


def poly_mean(G):
    """the polynomial mean of the reference's tutorial 06 (a user's Mean subclass): m(x) = c0 + c1 x + c2 x^2 on the last input column.
    `mean` is the same expression under torch and numpy; `backward` is what this package asks of a trainable user mean."""

    class PolynomialMean(G.Mean):
        def __init__(self):
            super().__init__()
            self.coefficients = G.Parameter([0.0, 0.0, 0.0])

        def mean(self, X):
            c = self.coefficients()
            x = X[:, -1]
            return (c[0] + c[1] * x + c[2] * x ** 2).reshape(-1, 1)

        def backward(self, X, dmu):
            x = X[:, -1]
            d = np.reshape(dmu, -1)
            self.coefficients.accumulate_grad(np.array([np.sum(d), np.sum(d * x), np.sum(d * x * x)]))

    return PolynomialMean()


def data(case, seed=7):
    c = CASES[case]
    rng = np.random.default_rng(seed)
    C, D, N = c["C"], c["D"], c["N"]
    n = [N // C + (1 if j < N % C else 0) for j in range(C)]
    x = [rng.uniform(0, 10, (n[j], D)) for j in range(C)]
    ch = np.concatenate([np.full(n[j], float(j)) for j in range(C)])
    xs = np.concatenate(x)
    y = np.sin(xs[:, 0]) + 0.5 + 0.2 * xs[:, -1] + 0.3 * ch + 0.1 * rng.standard_normal(N)
    X = xs if c["kern"] == "sm" else np.concatenate([ch[:, None], xs], axis=1)
    if c.get("shuffle"):
        p = rng.permutation(N)
        X, y = X[p], y[p]
    Xs = np.concatenate([np.concatenate([np.full((9, 1), float(j)), np.linspace(-1, 11, 9 * D).reshape(9, D)], axis=1) for j in range(C)])
    if c["kern"] == "sm":
        Xs = Xs[:, 1:]
    return X, y, Xs


def kernel(G, case, seed=11):
    c = CASES[case]
    rng = np.random.default_rng(seed)
    C, Q, D = c["C"], c["Q"], c["D"]
    if c["kern"] == "sm":
        k = G.SpectralMixtureKernel(Q=Q, input_dims=D)
        k.magnitude.assign(rng.uniform(0.5, 1.5, Q))
        k.mean.assign(rng.uniform(0.05, 0.3, (Q, D)))
        k.variance.assign(rng.uniform(0.01, 0.1, (Q, D)))
        return k
    k = G.MultiOutputSpectralMixtureKernel(Q=Q, output_dims=C, input_dims=D)
    k.weight.assign(rng.uniform(0.5, 1.5, (C, Q)))
    k.mean.assign(rng.uniform(0.05, 0.3, (C, Q, D)))
    k.variance.assign(rng.uniform(0.01, 0.1, (C, Q, D)))
    k.delay.assign(rng.normal(0, 0.1, (C, Q, D)))
    k.phase.assign(rng.normal(0, 0.1, (C, Q)))
    return k


def mean(G, case):
    c = CASES[case]
    kind, D = c["mean"], c["D"]
    if kind == "const":
        m = G.ConstantMean()
        m.bias.assign(0.3)
    elif kind == "lin":
        m = G.LinearMean(D + (0 if c["kern"] == "sm" else 1))        # the channel column too under a multi-output kernel
        m.bias.assign(0.2)
        m.slope.assign(np.linspace(0.25, -0.05, m.slope.shape[0]))
    elif kind == "mom":
        a, b = G.ConstantMean(), G.LinearMean(D)
        a.bias.assign(0.4)
        b.bias.assign(-0.1)
        b.slope.assign(np.full(D, 0.05))
        m = G.MultiOutputMean(a, b)
    else:
        m = poly_mean(G)
        m.coefficients.assign([0.1, 0.05, -0.01])
    return m


def exact(G, case, **kw):
    X, y, _ = data(case)
    return G.Exact(kernel(G, case), X, y, variance=0.1, mean=mean(G, case), **kw)


def sparse(G, name):
    model, case = SPARSE_CASES[name]
    X, y, _ = data(case)
    return getattr(G, model)(kernel(G, case), X, y, Z=4, variance=0.1, mean=mean(G, case))


def sub_means(m):
    """the sub-means of a MultiOutputMean (Q8: not among the model's parameters), else []"""
    return list(getattr(m.mean, "means", []))
