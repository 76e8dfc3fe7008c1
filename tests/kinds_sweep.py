"""
The generator of the kinds sweep (tests/test_kinds_sweep_cpu.py, tests/test_kinds_sweep_gpu.py): row programs that reach every radial
instantiation of k_gram / k_moments (csrc/gram.hip: DT in {1, 2, 3, generic}, GATE in {0, 1, 2}), random tables for them with a phase, a
delay and a frequency on the off-diagonal channel pairs, and point sets of the channel sizes at which the tile lists, the permutation to
caller order and the store paths change.  Seeded numpy only; a case is a function of (program, sizes) and is built once.

Arbitrary cross pairs are not positive semi-definite by construction.  The amplitude of the row that closes each group is therefore scaled
on every off-diagonal pair by 0.25 * 2^-k, with the smallest k for which the TWIN's lambda_min(Kj) >= 0.1 (`Case.k`): the device is not
asked.  tests/test_kinds_sweep_cpu.py asserts the conditions every case has to meet.
"""
import contextlib
import functools
import types
import numpy as np
import pytest

import kinds_twin

X_ = 1 << 8                                                 # MOGP_KIND_TIMES
MASK = 0xff
RQ, M12, M32, M52, PERIODIC, SINC, DOT, GATE, WDOT, WHITE = 1, 2, 3, 4, 5, 6, 7, 8, 9, 10
POINT_KINDS = (DOT, GATE, WDOT)
PROFILES = (0, RQ, M12, M32, M52)                            # what an off-diagonal pair may exchange for one another
JITTER = 1e-8
LAMBDA_MIN = 0.1

PROGRAMS = {                                                # name -> (D, kinds)
    "profiles_d1": (1, [1, 2, 3, 4, 0, 6, 5]),
    "groups_d1": (1, [3 | X_, 0, 5 | X_, 0, 7 | X_, 5, 4 | X_, 0 | X_, 6 | X_, 1]),
    "gates_d1": (1, [8 | X_, 3, 8 | X_, 8 | X_, 4 | X_, 0, 10, 7 | X_, 8 | X_, 2]),
    "profiles_d3": (3, [1, 2, 3, 4, 0, 6, 5, 7, 7 | X_, 3]),
    "features_d3": (3, [9, 9 | X_, 0, 10 | X_, 9, 10, 5 | X_, 9, 3]),
    "generic_d5": (5, [4, 1 | X_, 0, 7 | X_, 2, 6, 5]),
    "features_d8": (8, [9, 9 | X_, 3, 10, 0 | X_, 9 | X_, 5]),
}
SINGLE = [(1,), (2,), (63,), (64,), (65,), (127,), (128,), (129,)]
SEVERAL = [(1, 70, 0, 45), (65, 1, 63), (71, 129, 33), (255, 130), (193, 5, 187, 132)]
SIZES = SINGLE + SEVERAL
DATAFLOW_SIZES = (367, 400, 333)
DATAFLOW_PROGRAMS = ("groups_d1", "features_d3")
SWEEP = [(p, s) for p in PROGRAMS for s in SIZES] + [(p, DATAFLOW_SIZES) for p in DATAFLOW_PROGRAMS]


def case_id(v):
    return "x".join(str(s) for s in v) if isinstance(v, tuple) else str(v)


@contextlib.contextmanager
def installed():
    """`with installed():` -- the composed twin in place for the block, nothing of it afterwards"""
    with pytest.MonkeyPatch.context() as mp:
        kinds_twin.install(mp)
        yield mp


def draw_row(rng, kd, D, cross):
    """one table row [A, Psi, V_d, M_d, Delta_d] of kind `kd` and its shape; cross: an off-diagonal pair (Psi, Delta drawn)"""
    row, shape = np.zeros(2 + 3 * D), 0.0
    row[0] = rng.uniform(0.6, 1.3)
    if kd == WHITE:
        row[0] = rng.uniform(0.1, 0.4)
        return row, shape
    if kd == DOT:
        row[0] = rng.uniform(0.015, 0.025)
        row[1] = rng.uniform(0.3, 1.0)                      # the bias rides in the Psi slot
        return row, float(rng.integers(1, 4))
    if kd == GATE:
        row[2] = rng.uniform(0.5, 3.0) * rng.choice([-1.0, 1.0])
        row[3] = rng.uniform(2.0, 8.0)
        return row, shape
    if kd == WDOT:
        row[3:2 + D] = rng.uniform(0.0, 0.05, D - 1)        # weights on the feature columns, 0 on the input column
        return row, shape
    row[2:2 + D] = (rng.uniform(0.05, 0.3, D) if kd == SINC else rng.uniform(0.5, 3.0, D)) / D
    if kd == PERIODIC:
        row[2] *= D                                         # the periodic profile reads V_0 alone
        row[2 + D] = rng.uniform(0.05, 0.2)
        if rng.random() < 0.5:
            row[3 + D:2 + 2 * D] = rng.uniform(0.02, 0.2, D - 1)
    elif rng.random() < 0.5:
        row[2 + D:2 + 2 * D] = rng.uniform(0.02, 0.2, D)
    if kd == RQ:
        shape = rng.uniform(0.5, 2.0)
    if cross:
        row[1] = rng.uniform(-0.25, 0.25)
        if rng.random() < 0.5:                              # the other half keeps r = 0 reachable on a cross pair
            row[2 + 2 * D:2 + 3 * D] = rng.uniform(-1.0, 1.0, D) * np.where(np.arange(D) == 0, 0.5, 0.2)
    return row, shape


def draw_table(rng, kinds, D, C, like=None):
    """(table, kind, shape) C x C x T (x W): Psi = Delta = 0 on diagonal pairs; [j][i] is the mirror of [i][j], the same block seen from
    the other side (u -> -u: Psi and Delta change sign where a row reads them).  like = (kind, shape): new values for these very kinds"""
    T = len(kinds)
    table, kind, shape = np.zeros((C, C, T, 2 + 3 * D)), np.zeros((C, C, T), dtype=np.int32), np.zeros((C, C, T))
    for i in range(C):
        for j in range(i + 1):
            for t, k in enumerate(kinds):
                kd = k & MASK
                if like is not None:
                    kd = int(like[0][i, j, t]) & MASK
                elif i != j and kd in PROFILES and rng.random() < 0.5:
                    kd = int(rng.choice(PROFILES))          # another profile under the same flag
                table[i, j, t], shape[i, j, t] = draw_row(rng, kd, D, i != j)
                kind[i, j, t] = kd | (k & X_)
            if like is not None:
                shape[i, j] = like[1][i, j]
            if i != j:
                table[j, i], kind[j, i], shape[j, i] = table[i, j], kind[i, j], shape[i, j]
                reads = ~np.isin(kind[i, j] & MASK, (DOT, GATE, WDOT, WHITE))
                table[j, i, reads, 1] *= -1.0
                table[j, i, reads, 2 + 2 * D:] *= -1.0
    return table, kind, shape


def closing_rows(kinds):
    return [t for t, k in enumerate(kinds) if not (k & X_)]


def scale_cross(table, kind, shape, factor):
    """the amplitude of every group's closing row times `factor` on the off-diagonal pairs; a dot-product row: its A by the factor and its
    bias by the factor's degree-th root"""
    out = table.copy()
    C = table.shape[0]
    for i in range(C):
        for j in range(C):
            if i == j:
                continue
            for t in closing_rows(kind[i, j]):
                out[i, j, t, 0] *= factor
                if (kind[i, j, t] & MASK) == DOT:
                    out[i, j, t, 1] *= factor ** (1.0 / shape[i, j, t])
    return out


def draw_points(rng, sizes, D, duplicate=True, shuffle=True):
    """channel column, one input column on [0, 10], the others on [-1, 1]; one point's inputs copied onto another's; shuffled"""
    N = int(sum(sizes))
    X = np.concatenate([np.repeat(np.arange(len(sizes), dtype=np.float64), sizes)[:, None], rng.uniform(0.0, 10.0, (N, 1)),
                        rng.uniform(-1.0, 1.0, (N, D - 1))], axis=1)
    if duplicate and N > 3:
        X[N // 2, 1:] = X[1, 1:]
    return X[rng.permutation(N)] if shuffle else X


def twin_device(c, X=None, y=None):
    """the composed twin's device with the case's table and kinds; call under `installed()`"""
    X = c.X if X is None else X
    h = kinds_twin.KindsTableDevice(0, X, c.y if y is None else y, c.C)
    h.set_terms(c.table)
    h.set_kinds(c.kind, c.shape)
    return h


def make_case(name, D, kinds, sizes, seed, points=None, like=None):
    """a table of `kinds` for channels of `sizes` points, with inputs, targets and noise of its own or those of `points` (another case), and
    the cross pairs scaled until the twin's Kj is positive definite enough; like: another case whose kinds and shapes the table is drawn for"""
    rng = np.random.default_rng(seed)
    C = len(sizes)
    c = types.SimpleNamespace(program=name, sizes=sizes, D=D, C=C, T=len(kinds), N=int(sum(sizes)), jitter=JITTER)
    base, c.kind, c.shape = draw_table(rng, kinds, D, C, None if like is None else (like.kind, like.shape))
    if points is None:
        c.X = draw_points(rng, sizes, D)
        c.y = rng.standard_normal(c.N)
        c.noise = rng.uniform(0.2, 0.4, C)
    else:
        assert points.sizes == sizes and points.D == D
        c.X, c.y, c.noise = points.X, points.y, points.noise
    c.point_rows = bool(np.any(np.isin(c.kind & MASK, POINT_KINDS)))
    with installed():
        for c.k in range(12):
            c.table = scale_cross(base, c.kind, c.shape, 0.25 * 2.0 ** -c.k)
            Kj, _ = twin_device(c)._Kj(c.noise, c.jitter, None)
            ev = np.linalg.eigvalsh(Kj)
            if ev[0] >= LAMBDA_MIN or C == 1:
                break
    c.lambda_min, c.cond = float(ev[0]), float(ev[-1] / ev[0])
    ch = c.X[:, 0]
    off = ch[:, None] != ch[None, :]
    c.cross_ratio = float(np.max(np.abs(Kj[off])) / np.max(np.diagonal(Kj))) if np.any(off) else None
    return c


@functools.lru_cache(maxsize=None)
def case(program, sizes):
    D, kinds = PROGRAMS[program]
    return make_case(program, D, kinds, sizes, [list(PROGRAMS).index(program)] + list(sizes))


def kss_diag(c, Xs):
    """what mogp_exact_predict takes beside the test points, from the twin: K(x, x) per test point where a row's diagonal follows the point,
    per channel otherwise; call under `installed()`"""
    if c.point_rows:
        return np.diagonal(kinds_twin.gram_from_table(c.table, Xs, None, c.kind, c.shape)).copy()
    out = np.zeros(c.C)
    for ch in range(c.C):
        x = np.concatenate([[float(ch)], np.zeros(c.D)])[None]
        out[ch] = kinds_twin.gram_from_table(c.table, x, None, c.kind, c.shape)[0, 0]
    return out
