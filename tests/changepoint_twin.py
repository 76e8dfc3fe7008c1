"""
The numpy twin of the gate row (kind 8) for the tests of the change-point family.  oracle/table_model.py carries kinds 0 - 7; the
twin of kind 8 lives here and is put in its place by `install(monkeypatch)`: `row_parts` with the gate row in front of the oracle's own, and
a `TableDevice` whose prediction takes the diagonal per test point when a gate row is present, as the library does.  Written from the
definition h(x) = sigmoid(beta (x - l)), independently of mogptk_amd/gpr.
"""
import numpy as np
from scipy.linalg import solve_triangular

import oracle.table_model as tm

KIND_GATE = 8


def sigmoid(z):
    """1 / (1 + exp(-z)), no overflow for any finite z"""
    e = np.exp(-np.abs(z))
    return np.where(z >= 0, 1.0, e) / (1.0 + e)


def gate_row_parts(row, x1, x2):
    """(h_a h_b, the integrands of [m0, m4, m1_0, m2_0, m3_0]) of a gate row [A, 0, beta, l, 0] at x1 (n1, 1), x2 (n2, 1): m1_0 = d/dbeta,
    m3_0 = d/dl, raw; the complement 1 - h is sigmoid(-z)"""
    beta, loc = row[2], row[3]
    a, b = x1[:, 0] - loc, x2[:, 0] - loc
    ha, hb, ca, cb = sigmoid(beta * a), sigmoid(beta * b), sigmoid(-beta * a), sigmoid(-beta * b)
    k = ha[:, None] * hb[None, :]
    zero = np.zeros_like(k)
    return k, [k, zero, k * ((ca * a)[:, None] + (cb * b)[None, :]), zero, -beta * k * (ca[:, None] + cb[None, :])]


_oracle_row_parts = tm.row_parts


def row_parts(row, kind, shape, x1, x2):
    if kind == KIND_GATE:
        assert x1.shape[1] == 1, "a gate row takes one input dimension"
        return gate_row_parts(row, x1, x2)
    return _oracle_row_parts(row, kind, shape, x1, x2)


class GateTableDevice(tm.TableDevice):
    """TableDevice whose `predict` treats gate rows per point (the oracle's knows dot-product rows only)"""

    def predict(self, noise_var, jitter, kss_diag, Xs, full=False, data_var=None):
        gates = self.kind is not None and np.any((np.asarray(self.kind) & tm.KIND_MASK) == KIND_GATE)
        if full or not gates:
            return super().predict(noise_var, jitter, kss_diag, Xs, full=full, data_var=data_var)
        K, _ = self._Kj(noise_var, jitter, data_var)
        L = np.linalg.cholesky(K)
        Kfs = self._gram(self.X, Xs)
        alpha = solve_triangular(L.T, solve_triangular(L, self.y, lower=True), lower=False)
        v = solve_triangular(L, Kfs, lower=True)
        kdiag = np.asarray(kss_diag, dtype=np.float64).reshape(-1)
        assert kdiag.shape == (Xs.shape[0],), "with a gate row kss_diag holds one value per test point"
        return Kfs.T @ alpha, (kdiag - np.sum(v * v, axis=0)).reshape(-1, 1)


def install(monkeypatch):
    """kind 8 into the oracle's walk over rows, and the per-point prediction into the scaffold's device twin"""
    import kernel_family as kf
    monkeypatch.setattr(tm, "row_parts", row_parts)
    monkeypatch.setattr(kf, "TableDevice", GateTableDevice)
