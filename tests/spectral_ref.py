"""
The reference of the spectral sweep (tests/test_spectral_sweep_cpu.py, tests/test_spectral_sweep_gpu.py): the term formula of the unified
table, restated in np.longdouble with the differences taken FIRST,

    u_d = (x_a,d - x_b,d) + Delta_d,      k_t = A exp(-1/2 sum_d V_d u_d^2) cos(2 pi (sum_d M_d u_d + Psi)),

times exp(-1/2 sum_d L_d ((x_a,d + x_b,d) / 2 - c_d)^2) for rows of width 2 + 5 D; per channel pair from the table, the lower pairs
mirrored for the square form.  It shares no code with oracle/table_model.py, and nothing with the device's split into per-point phases
p_a = sum_d M_d (x_a,d + Delta_d) + Psi, q_b = sum_d M_d x_b,d and tile-centred Gaussian factors.  Where np.longdouble is only 64 bits wide the
same difference-first code is still the reference (`EPS` says which it is; the CPU module prints it once).
"""
import numpy as np

LD = np.longdouble
EPS = np.finfo(LD).eps
TWO_PI = 2 * LD("3.14159265358979323846264338327950288")


def pair_block(rows, x1, x2):
    """one channel-pair block: rows (T, W) of a table, x1 (n1, D), x2 (n2, D) -> (n1, n2) in longdouble"""
    rows, x1, x2 = np.asarray(rows, dtype=LD), np.asarray(x1, dtype=LD), np.asarray(x2, dtype=LD)
    D = x1.shape[1]
    out = np.zeros((x1.shape[0], x2.shape[0]), dtype=LD)
    for r in rows:
        arg = np.zeros_like(out)
        ph = np.full_like(out, r[1])
        for d in range(D):
            u = (x1[:, None, d] - x2[None, :, d]) + r[2 + 2 * D + d]
            arg += r[2 + d] * u * u
            ph += r[2 + D + d] * u
            if len(r) > 2 + 3 * D:
                a = (x1[:, None, d] + x2[None, :, d]) / 2 - r[2 + 4 * D + d]
                arg += r[2 + 3 * D + d] * a * a
        out += r[0] * np.exp(-arg / 2) * np.cos(TWO_PI * ph)
    return out


def gram(table, X1, X2=None):
    """K(X1[, X2]) in the callers' row order, longdouble; X: (n, 1 + D) with the channel in column 0.  Square form: the pairs i >= j from the
    table, the others their mirror"""
    C = table.shape[0]
    Xc = X1 if X2 is None else X2
    c1, c2 = X1[:, 0].astype(np.int64), Xc[:, 0].astype(np.int64)
    K = np.zeros((len(X1), len(Xc)), dtype=LD)
    for i in range(C):
        r1 = np.nonzero(c1 == i)[0]
        for j in range(C if X2 is not None else i + 1):
            r2 = np.nonzero(c2 == j)[0]
            if len(r1) == 0 or len(r2) == 0:
                continue
            B = pair_block(table[i, j], X1[r1, 1:], Xc[r2, 1:])
            K[np.ix_(r1, r2)] = B
            if X2 is None and i != j:
                K[np.ix_(r2, r1)] = B.T
    return K


def kj(table, X, noise, jitter, data_var=None):
    """(Kj, jitter_abs): K + noise (+ data_var) + jitter * mean(diagonal) on the diagonal, caller order, longdouble"""
    K = gram(table, X)
    n = len(X)
    d = np.diagonal(K) + np.asarray(noise, dtype=LD)[X[:, 0].astype(np.int64)]
    if data_var is not None:
        d = d + np.asarray(data_var, dtype=LD)
    jit = LD(jitter) * np.sum(d) / n
    K[np.arange(n), np.arange(n)] = d + jit
    return K, jit


def sorted_order(X):
    """the device's channel-sorted order: a stable sort by channel"""
    return np.argsort(X[:, 0], kind="stable")


def phase_magnitude(table, X):
    """P = max over (pair, term) of sum_d |M_d| max_a |x_a,d + Delta_d| + |Psi|: the size of the per-point phases the device forms from
    absolute inputs (the rounding term of the far case's bound)"""
    D = X.shape[1] - 1
    rows = table.reshape(-1, table.shape[3])
    lo, hi, dl = np.min(X[:, 1:], axis=0)[None, :], np.max(X[:, 1:], axis=0)[None, :], rows[:, 2 + 2 * D:2 + 3 * D]
    reach = np.maximum(np.abs(lo + dl), np.abs(hi + dl))
    return float(np.max(np.sum(np.abs(rows[:, 2 + D:2 + 2 * D]) * reach, axis=1) + np.abs(rows[:, 1])))
