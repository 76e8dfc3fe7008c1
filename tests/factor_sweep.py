"""
The generator and the reference of the factorisation sweep (tests/test_factor_sweep_cpu.py, tests/test_factor_sweep_gpu.py, whose device
side is tests/factor_sweep_child.py): exact MOSM models (C = 3, Q = 2, D = 1, through the project's own term table) at the sizes where the
schedules of the exact path take another set of launches -- the tile-row count modulo the outer block of 4 (csrc/potri.hip, csrc/flow.hip,
csrc/sweep.hip: `rem > 0`, `k0 > 0`, `Kd == 4 * MOGP_TILE`, the identity padding, the 64-row variants of a partial block), a last tile with
ONE valid row, and the edges 512 and 1024 themselves.  Seeded numpy only; no device is asked anywhere in this file.

Hyper-parameters and data are drawn as tests/test_gpu_parity.py:test_exact_entry_points_share_one_handle draws them, x uniform on
[0, 10 N / 1100] so that every size has that test's point density; ragged channels, the caller's rows shuffled.  N = 256 has the channels
(128, 128, 0): an empty one, and the other two exactly a tile each; N = 300 has a channel of one point.

The two banded cases are for the planned inverse (csrc/exact.hip: kinv_plan), drawn as test_gradient_with_only_the_needed_tiles_of_the_inverse
draws its own: two channels interleaved in x order, spectral variances 0.5 .. 1.5, x uniform on [0, 600].

The reference is numpy / scipy in float64: Kj from oracle.table_model.TableDevice._Kj, permuted into the library's order
(np.argsort(X[:, 0], kind="stable")), L by Cholesky, W by a triangular solve against I, Kj^-1 = W^T W, alpha, the range of diag(L) and the
log-determinant from them; LML, moments, diagG, trG, jitter_abs and the predictions are TableDevice's as they stand.  W is returned in the
sorted order, everything else in the caller's (include/mogp_hip.h: mogp_model_fetch).  Built once per case; treat as read-only.
"""
import functools
import types
import numpy as np

from mogptk_amd import gpr
from oracle.table_model import TableDevice

TILE, OUTER, GT = 128, 4, 64
C, Q = 3, 2
JITTER = 1e-8

# N -> (tile rows, outer blocks)
SIZES = {100: (1, (1,)), 256: (2, (2,)), 300: (3, (3,)), 512: (4, (4,)), 513: (5, (4, 1)), 800: (7, (4, 3)), 1024: (8, (4, 4)),
         1025: (9, (4, 4, 1)), 1200: (10, (4, 4, 2)), 1400: (11, (4, 4, 3)), 1537: (13, (4, 4, 4, 1))}
FIXED_CHANNELS = {256: (128, 128, 0), 300: (1, 170, 129)}     # an empty channel next to two of exactly a tile; a channel of one point
BANDED = {"b600x700": ((600, 700), 11, (4, 4, 3)), "b700x837": ((700, 837), 13, (4, 4, 4, 1))}
CASES = ["n%d" % n for n in SIZES]
ALL = CASES + list(BANDED)
NEWTON_MAX_N = 640                                            # no np.longdouble product above (one takes a minute at 1537)

# the prediction: tile rows of the training set -> nothing; every S with every size.  S -> channel sizes of the test set (one with an
# empty channel; S = 1 has two); Srow = Spad + 128 is 2, 2, 3 and 4 tile rows
PREDICT_CASES = ["n513", "n1024", "n1025", "n1537"]
TEST_SETS = {1: (0, 1, 0), 128: (50, 0, 78), 129: (43, 43, 43), 300: (101, 99, 100)}
FULL_COV_S = 129
ACCURATE_PREDICT = ("n1025", 129)


def tile_rows(N):
    return -(-N // TILE)


def outer_blocks(nb):
    return tuple(min(OUTER, nb - k) for k in range(0, nb, OUTER))


def _mosm(rng, nch, v_lo, v_hi):
    k = gpr.MultiOutputSpectralMixtureKernel(Q=Q, output_dims=nch, input_dims=1)
    k.weight.assign(rng.uniform(0.5, 1.5, (nch, Q))); k.mean.assign(rng.uniform(0.02, 0.4, (nch, Q, 1)))
    k.variance.assign(rng.uniform(v_lo, v_hi, (nch, Q, 1))); k.delay.assign(rng.normal(0, 0.3, (nch, Q, 1))); k.phase.assign(rng.normal(0, 0.3, (nch, Q)))
    return k


@functools.lru_cache(maxsize=None)
def case(name):
    c = types.SimpleNamespace(name=name, jitter=JITTER, banded=name in BANDED)
    if c.banded:
        sizes, c.nb, c.blocks = BANDED[name]
        c.C, c.N = 2, int(sum(sizes))
        rng = np.random.default_rng([5] + list(sizes))
        X = np.concatenate([np.stack([np.full(s, float(ch)), rng.uniform(0, 600, s)], axis=1) for ch, s in enumerate(sizes)])
        c.X = X[np.argsort(X[:, 1])]                          # interleaved, each channel in the order of its series: a 64-point block is local in x
        c.y = rng.standard_normal(c.N)
        c.kernel = _mosm(rng, c.C, 0.5, 1.5)
        c.xmax = 600.0
    else:
        c.N = int(name[1:])
        c.nb, c.blocks = SIZES[c.N]
        c.C = C
        rng = np.random.default_rng(c.N)
        sizes = FIXED_CHANNELS.get(c.N)
        if sizes is None:
            sizes = tuple(int(s) for s in rng.multinomial(c.N - C, np.ones(C) / C) + 1)
        c.xmax = 10.0 * c.N / 1100.0
        c.X = np.concatenate([np.stack([np.full(s, float(ch)), rng.uniform(0, c.xmax, s)], axis=1) for ch, s in enumerate(sizes)])[rng.permutation(c.N)]
        c.y = rng.standard_normal(c.N)
        c.kernel = _mosm(rng, c.C, 0.05, 0.5)
    c.sizes = tuple(sizes)
    c.table, c.kss = np.array(c.kernel._spectral_terms(1)), np.array(c.kernel._spectral_diag(1))
    c.noise = rng.uniform(0.05, 0.2, c.C)
    c.order = np.argsort(c.X[:, 0], kind="stable")
    return c


@functools.lru_cache(maxsize=None)
def test_points(name, S):
    """S test points in shuffled order, a little beyond the range of the data on either side"""
    c = case(name)
    rng = np.random.default_rng([77, c.N, S])
    Xs = np.concatenate([np.stack([np.full(s, float(ch)), rng.uniform(-1.0, c.xmax + 1.0, s)], axis=1) for ch, s in enumerate(TEST_SETS[S])])
    return Xs[rng.permutation(S)]


def twin(c):
    h = TableDevice(0, c.X, c.y, c.C)
    h.set_terms(c.table)
    return h


@functools.lru_cache(maxsize=None)
def reference(name):
    """-> dict: Kj (caller order), W (sorted order), Kinv, alpha (caller order), lmin, lmax, logdet, and TableDevice's lml, moments, diagG, trG,
    jitter_abs of the gradient evaluation"""
    from scipy.linalg import solve_triangular
    c = case(name)
    h = twin(c)
    ref = dict(h.eval(c.noise, c.jitter, grad=True))
    Kj, _ = h._Kj(c.noise, c.jitter, None)
    o = c.order
    L = np.linalg.cholesky(Kj[np.ix_(o, o)])
    W = solve_triangular(L, np.eye(c.N), lower=True)
    Kinv = np.empty((c.N, c.N))
    Kinv[np.ix_(o, o)] = W.T @ W
    d = np.diagonal(L)
    ref.update(Kj=Kj, W=W, Kinv=Kinv, alpha=Kinv @ c.y, lmin=float(np.min(d)), lmax=float(np.max(d)), logdet=float(2.0 * np.sum(np.log(d))))
    return ref


@functools.lru_cache(maxsize=None)
def reference_predictions(name):
    """-> {S: (mu, var)} and {"cov": S x S at FULL_COV_S}: TableDevice.predict as it stands, once over all test sets of the case (mean and
    variance of a point do not depend on the other test points) and once more for the full covariance"""
    c = case(name)
    h = twin(c)
    sets = [test_points(name, S) for S in TEST_SETS]
    mu, var = h.predict(c.noise, c.jitter, c.kss, np.concatenate(sets))
    out, at = {}, 0
    for S in TEST_SETS:
        out[S] = (mu[at:at + S].reshape(-1, 1), var[at:at + S].reshape(-1, 1))
        at += S
    out["cov"] = h.predict(c.noise, c.jitter, c.kss, test_points(name, FULL_COV_S), full=True)[1]
    return out


def newton_inverse(K, X0, steps=2):
    """X <- X (2 I - K X) in np.longdouble from the float64 inverse X0: every step squares the residual, two take 1e-12 below the last digit"""
    Kl, X = K.astype(np.longdouble), X0.astype(np.longdouble)
    I2 = 2.0 * np.eye(K.shape[0], dtype=np.longdouble)
    for _ in range(steps):
        X = X @ (I2 - Kl @ X)
    return X


def planned_fraction(c):
    """numpy restatement of kinv_plan (csrc/exact.hip): the fraction of the lower 128 x 128 tiles of Kj^-1 that some 64-point block pair needs,
    a pair being needed unless every term's exponent is beyond 52 at the closest approach of the two blocks' ranges; diagonal tiles always"""
    x = c.X[c.order, 1]
    ch = c.X[c.order, 0].astype(np.int64)
    off = np.concatenate([[0], np.cumsum(np.bincount(ch, minlength=c.C))])
    blocks = [(i, off[i] + b, min(GT, off[i + 1] - off[i] - b)) for i in range(c.C) for b in range(0, off[i + 1] - off[i], GT)]
    cen = [0.5 * (np.min(x[r0:r0 + n]) + np.max(x[r0:r0 + n])) for _, r0, n in blocks]
    half = [0.5 * (np.max(x[r0:r0 + n]) - np.min(x[r0:r0 + n])) for _, r0, n in blocks]
    nb = tile_rows(c.N)
    need = np.eye(nb, dtype=bool)
    for rb, (i, r0, nr) in enumerate(blocks):
        for cb, (j, c0, nc) in enumerate(blocks):
            if j > i or (i == j and cb > rb):
                continue
            rows = c.table[i, j]                              # T x [A, Psi, V, M, Delta]
            sd = (cen[rb] - cen[cb]) + rows[:, 4]
            mu = np.maximum(0.0, np.abs(sd) - half[rb] - half[cb])
            if np.all(0.5 * rows[:, 2] * mu * mu > 52.0):
                continue
            for ti in range(r0 // TILE, (r0 + nr - 1) // TILE + 1):
                for tj in range(c0 // TILE, (c0 + nc - 1) // TILE + 1):
                    if tj <= ti:
                        need[ti, tj] = True
    return float(np.sum(np.tril(need)) / (nb * (nb + 1) / 2))
