"""
The numpy twin of the weighted-dot row (kind 9), the white row (kind 10) and the periodic row beside further input columns (kind 5, D > 1)
for the tests of the function family.  oracle/table_model.py carries kinds 0 - 7 and the periodic row for D = 1; the twins live
here and are put in their place by `install(monkeypatch)`.  Written from the definitions
    kind 9:   k = sum_d V_d x_a,d x_b,d                       (times the row's amplitude)
    kind 10:  k = 1 where row and column are the same point of the same set, 0 elsewhere
    kind 5:   k = exp(V_0 (cos theta - 1)),  theta = 2 pi (sum_d M_d u_d + Psi)
independently of mogptk_amd/gpr.  The white row is an identity by INDEX and only on symmetric calls: the oracle's walk over channel pairs
says which block pairs a point set with itself (`gram_from_table` without X2, `moments_dense` with sym, on the blocks i == j).
"""
import numpy as np
from scipy.linalg import solve_triangular

import oracle.table_model as tm

KIND_PERIODIC, KIND_WDOT, KIND_WHITE = 5, 9, 10
TWO_PI = 2.0 * np.pi
_STATE = dict(symmetric=False, same=False)      # the call in progress has one point set; the block in progress pairs it with itself


def wdot_row_parts(row, x1, x2):
    """(sum_d V_d x_a,d x_b,d, the integrands of [m0, m4, m1_d, m2_d, m3_d]): m0 = d/dA, m1_d = d/dV_d over the row's amplitude"""
    D = x1.shape[1]
    xx = x1[:, None, :] * x2[None, :, :]
    k = np.sum(row[2:2 + D] * xx, axis=2)
    zero = np.zeros_like(k)
    return k, [k, zero] + [xx[..., d] for d in range(D)] + [zero] * (2 * D)


def white_row_parts(row, x1, x2):
    """(the identity by index on a block that pairs a point set with itself, zeros on every other block; m0 alone)"""
    D = x1.shape[1]
    if _STATE["same"]:
        assert x1.shape == x2.shape
        k = np.eye(x1.shape[0])
    else:
        k = np.zeros((x1.shape[0], x2.shape[0]))
    return k, [k] + [np.zeros_like(k)] * (1 + 3 * D)


def periodic_row_parts(row, x1, x2):
    """the periodic row for any D: V_0 and the row's phase; m4 = d/dPsi, m1_0 = d/dV_0 and m3_0 = d/dM_0 over their chain-rule factors"""
    D = x1.shape[1]
    u = x1[:, None, :] - x2[None, :, :] + row[2 + 2 * D:2 + 3 * D]
    th = TWO_PI * (np.sum(row[2 + D:2 + 2 * D] * u, axis=2) + row[1])
    E = np.exp(row[2] * (np.cos(th) - 1.0))
    zero = np.zeros_like(E)
    return E, ([E, E * row[2] * np.sin(th), E * 2.0 * (1.0 - np.cos(th))] + [zero] * (D - 1) + [zero] * D
               + [E * row[2] * u[..., 0] * np.sin(th)] + [zero] * (D - 1))


_oracle = dict(row_parts=tm.row_parts, gram_block=tm._gram_block, gram_from_table=tm.gram_from_table, moments_dense=tm.moments_dense)


def row_parts(row, kind, shape, x1, x2):
    if kind == KIND_WDOT:
        return wdot_row_parts(row, x1, x2)
    if kind == KIND_WHITE:
        return white_row_parts(row, x1, x2)
    if kind == KIND_PERIODIC and x1.shape[1] > 1:
        return periodic_row_parts(row, x1, x2)
    return _oracle["row_parts"](row, kind, shape, x1, x2)


def gram_from_table(table, X1, X2=None, kind=None, shape=None):
    _STATE["symmetric"] = X2 is None
    try:
        return _oracle["gram_from_table"](table, X1, X2, kind, shape)
    finally:
        _STATE["symmetric"] = _STATE["same"] = False


def _gram_block(table, kind, shape, i, j, x1, x2):
    _STATE["same"] = _STATE["symmetric"] and i == j
    return _oracle["gram_block"](table, kind, shape, i, j, x1, x2)


def moments_dense(table, G, X1, X2, sym, kind=None, shape=None):
    """the oracle's walk over channel pairs for tables with kinds, saying per block whether it pairs the point set with itself"""
    kd, sh = tm._kinds(kind, shape)
    if kd is None:
        return _oracle["moments_dense"](table, G, X1, X2, sym, kind, shape)
    C, T = table.shape[0], table.shape[2]
    D = X1.shape[1] - 1
    c1, c2 = X1[:, 0].astype(np.int64), X2[:, 0].astype(np.int64)
    out = np.zeros(((C * (C + 1) // 2) if sym else C * C, T, table.shape[3]))
    try:
        for i in range(C):
            ri = np.nonzero(c1 == i)[0]
            for j in range((i + 1) if sym else C):
                rj = np.nonzero(c2 == j)[0]
                if len(ri) == 0 or len(rj) == 0:
                    continue
                g = G[np.ix_(ri, rj)] * (2.0 if (sym and i != j) else 1.0)
                m = out[i * (i + 1) // 2 + j] if sym else out[i * C + j]
                _STATE["same"] = bool(sym and i == j)
                m[:] = tm.kinds_block(table[i, j], kd[i, j], sh[i, j], X1[ri, 1:], X2[rj, 1:], g)[1]
                if sym and i == j:                          # odd-in-tau moments cancel over the full symmetric block
                    m[:, 1] = 0.0
                    m[:, 2 + D:2 + 2 * D] = 0.0
    finally:
        _STATE["same"] = False
    return out


class FunctionTableDevice(tm.TableDevice):
    """TableDevice whose `predict` treats weighted-dot rows per point (the oracle's knows dot-product rows only)"""

    def predict(self, noise_var, jitter, kss_diag, Xs, full=False, data_var=None):
        wdot = self.kind is not None and np.any((np.asarray(self.kind) & tm.KIND_MASK) == KIND_WDOT)
        if full or not wdot:
            return super().predict(noise_var, jitter, kss_diag, Xs, full=full, data_var=data_var)
        K, _ = self._Kj(noise_var, jitter, data_var)
        L = np.linalg.cholesky(K)
        Kfs = self._gram(self.X, Xs)
        alpha = solve_triangular(L.T, solve_triangular(L, self.y, lower=True), lower=False)
        v = solve_triangular(L, Kfs, lower=True)
        kdiag = np.asarray(kss_diag, dtype=np.float64).reshape(-1)
        assert kdiag.shape == (Xs.shape[0],), "with a weighted-dot row kss_diag holds one value per test point"
        return Kfs.T @ alpha, (kdiag - np.sum(v * v, axis=0)).reshape(-1, 1)


def install(monkeypatch):
    """kinds 9, 10 and the D-general kind 5 into the oracle's walk over rows, the same-set flag into its walks over channel pairs, and the
    per-point prediction into the scaffold's device twin"""
    import kernel_family as kf
    monkeypatch.setattr(tm, "row_parts", row_parts)
    monkeypatch.setattr(tm, "_gram_block", _gram_block)
    monkeypatch.setattr(tm, "gram_from_table", gram_from_table)
    monkeypatch.setattr(tm, "moments_dense", moments_dense)
    monkeypatch.setattr(kf, "gram_from_table", gram_from_table)
    monkeypatch.setattr(kf, "TableDevice", FunctionTableDevice)
