"""
The cases of tests/golden/cv.npz (leave-fold-out cross-validation): models of tests/loo_cases.py -- nothing new is defined, no data
and no parameters -- each with one or two deterministic fold layouts.  A layout is a function of the model's inputs in kernel format (channel
column first: model_inputs) and returns one label per training point in the model's row order: -1 (never held out) or the fold's number.  numpy only; used
by the generator (gen_cv.py) and by the tests on either side.

What the layouts cover between them: a fold of exactly 128 points across row 128 of the channel-sorted order (two factor tiles), a one-point
fold, a fold of 17 points (no multiple of 16), a fold whose points lie in every tile, folds with points of two channels, points in no fold,
22 blocks of 50 points at N = 1100, and every point its own fold (which is leave-one-out).
"""
import numpy as np

import loo_cases

FOLD_MAX = 128


def model_inputs(m):
    """a model's inputs in kernel format (channel column first; zeros under a single-output kernel), as numpy -- of either package"""
    X = m.X
    X = np.asarray(X.detach().cpu().numpy() if hasattr(X, "detach") else X, dtype=np.float64)
    return np.concatenate([np.zeros((X.shape[0], 1)), X], axis=1) if m.kernel.output_dims is None else X


def _channels(X):
    return X[:, 0].astype(np.int64)


def wide(X):
    """rows 11 .. 138 of a single-channel model: 128 points over the boundary of the first two 128-row tiles; a one-point fold; a short block"""
    N = X.shape[0]
    assert N >= 148 and np.all(_channels(X) == 0)
    lab = np.full(N, -1)
    lab[11:139] = 0
    lab[3] = 1
    lab[140:148] = 2
    return lab


def singletons(X):
    """every point its own fold, numbered by a seeded permutation"""
    return np.random.default_rng(5).permutation(X.shape[0])


def mixed(X):
    """a block of 17 points, 17 points spread over the whole range (every tile of 64 has some), and seeded blocks of 1 .. 9 points elsewhere"""
    N = X.shape[0]
    lab = np.full(N, -1)
    spread = np.unique(np.round(np.linspace(1, N - 2, 17)).astype(np.int64))
    assert spread.size == 17 and np.unique(spread // 64).size == (N + 63) // 64
    lab[spread] = 1
    lab[np.flatnonzero(lab < 0)[20:37]] = 0                      # the block steps over the spread points inside it
    rng = np.random.default_rng(9)
    free = np.flatnonzero(lab < 0)
    at, f = 0, 2
    while at < free.size:
        n = int(rng.integers(1, 10))
        if rng.random() < 0.7:                                   # the rest stays in no fold
            lab[free[at:at + n]] = f
            f += 1
        at += n
    return lab


def seeded(seed, nfolds, p_out=0.25):
    """labels drawn point by point: in no fold with probability p_out, else one of nfolds folds (scattered over all rows and channels)"""
    def layout(X):
        rng = np.random.default_rng(seed)
        N = X.shape[0]
        lab = rng.integers(0, nfolds, N)
        lab[rng.random(N) < p_out] = -1
        used = np.unique(lab[lab >= 0])
        assert used.size == nfolds and np.max(np.bincount(lab[lab >= 0])) <= FOLD_MAX
        return lab
    return layout


def across_channels(X):
    """per channel boundary one fold of the last 6 points of a channel and the first 9 of the next (rows as the model has them); a block of 30 inside
    the first channel; one point of the last"""
    c = _channels(X)
    N = X.shape[0]
    lab = np.full(N, -1)
    f = 0
    for k in range(int(c.max())):
        a, b = np.flatnonzero(c == k), np.flatnonzero(c == k + 1)
        lab[a[-6:]] = f
        lab[b[:9]] = f
        f += 1
    first = np.flatnonzero(c == 0)
    lab[first[2:32]] = f
    lab[np.flatnonzero(c == c.max())[-1]] = f + 1
    return lab


def held_out_range(X):
    """a range of 40 consecutive points and one more point: where a white kernel's identity by index meets a held-out block"""
    N = X.shape[0]
    lab = np.full(N, -1)
    lab[N // 3:N // 3 + 40] = 0
    lab[N - 2] = 1
    return lab


def blocks_of_50(X):
    N = X.shape[0]
    assert N == 1100
    return np.arange(N) // 50


def block_labels(X, size):
    """what Model.block_folds(size) returns for inputs X in kernel format: per channel, runs of `size` points in input order"""
    c = _channels(X)
    lab = np.empty(X.shape[0], dtype=np.int64)
    first = 0
    for k in np.unique(c):
        rows = np.flatnonzero(c == k)
        rows = rows[np.argsort(X[rows, -1], kind="stable")]
        lab[rows] = first + np.arange(rows.size) // size
        first += -(-rows.size // size)
    return lab


LAYOUTS = {
    "m32":     dict(wide=wide, singletons=singletons),
    "three":   dict(mixed=mixed),
    "gate":    dict(seeded=seeded(21, 5)),
    "white":   dict(range=held_out_range),
    "imo":     dict(across=across_channels),
    "mosm":    dict(across=across_channels),
    "mohsm":   dict(seeded=seeded(23, 7)),
    "linmean": dict(seeded=seeded(25, 6)),
    "datavar": dict(seeded=seeded(27, 4, p_out=0.5)),
    "big":     dict(blocks=blocks_of_50),
}
PAIRS = [(case, name) for case, ls in LAYOUTS.items() for name in ls]
assert all(case in loo_cases.CASES for case in LAYOUTS)
ADAM_CASE, ADAM_ITERS, ADAM_LR, ADAM_BLOCK = loo_cases.ADAM_CASE, 20, 0.05, 10       # Model.train('Adam', objective='cv', folds=block_folds(10))


def labels(case, name, m):
    """the layout's labels for the model m of the case, checked: int32, every fold 1 .. 128 points, numbered without gaps"""
    X = model_inputs(m)
    lab = np.asarray(LAYOUTS[case][name](X), dtype=np.int32)
    sizes = np.bincount(lab[lab >= 0])
    assert lab.shape == (X.shape[0],) and lab.min() >= -1 and sizes.min() >= 1 and sizes.max() <= FOLD_MAX
    return lab


def index_arrays(lab):
    """the same folds as a sequence of index arrays"""
    return [np.flatnonzero(lab == f) for f in range(int(lab.max()) + 1)]
