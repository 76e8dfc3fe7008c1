"""
The numpy twin of mogp_exact_predict_grad (include/mogp_hip.h, csrc/exact.hip, csrc/gram.hip:k_gram_dx) for the tests of the posterior of
df/dx: parts_twin's device with `predict_grad` written from the formulas
    dmu_d = J_d Kj^-1 r,   dvar_d = kappa_d - colsum((L^-1 J_d^T)^2),   J_d[a, b] = dK(x*_a, x_b)/dx*_a,d,
Kj, r and the jitter the whole model's (`_Kj`, `_residual`).  The Jacobian of Gaussian and enveloped rows is the oracle's `_jr_block`; for
tables with kinds it is written here over the oracle's `row_parts` / `profiles`, row by row and group by group (the product rule with the
other rows' values recomputed).  The twin also holds the ABI's refusals: kinds 2, 8, 9 and 10.
"""
import numpy as np
from scipy.linalg import solve_triangular

import oracle.table_model as tm
import parts_twin
from mogptk_amd import _lib

KIND_PERIODIC, KIND_DOT = 5, 7
REFUSED = {2: "Matern 1/2", 8: "gate", 9: "weighted-dot", 10: "white"}


def row_jacobian(row, kind, shape, x1, x2):
    """(the row's value as `kinds_block` multiplies it -- amplitude included --, d value / d x1 (n1, n2, D))"""
    D = x1.shape[1]
    A = row[0]
    if kind == KIND_DOT:
        n = int(shape)
        b = A * (x1 @ x2.T) + row[1]
        db = n * b ** (n - 1) if n > 1 else np.ones_like(b)
        return b ** n, (db * A)[:, :, None] * x2[None, :, :]
    Psi, V, M = row[1], row[2:2 + D], row[2 + D:2 + 2 * D]
    u = x1[:, None, :] - x2[None, :, :] + row[2 + 2 * D:2 + 3 * D]
    th = tm.TWO_PI * (np.sum(M * u, axis=2) + Psi)
    if kind == KIND_PERIODIC:
        E = np.exp(V[0] * (np.cos(th) - 1.0))
        return A * E, (-A * V[0] * np.sin(th) * E)[:, :, None] * (tm.TWO_PI * M)
    phi, psi = tm.profiles(kind, shape, np.sum(V * u * u, axis=2))
    J = -(psi * np.cos(th))[:, :, None] * (V * u) - (phi * np.sin(th))[:, :, None] * (tm.TWO_PI * M)
    return A * phi * np.cos(th), A * J


def kinds_jacobian(tab, kind, shape, x1, x2):
    """d (one channel-pair block of a table with kinds) / d x1: (n1, n2, D)"""
    T, D = tab.shape[0], x1.shape[1]
    kd = kind & tm.KIND_MASK
    rows = [row_jacobian(tab[t], int(kd[t]), shape[t], x1, x2) for t in range(T)]
    J = np.zeros((x1.shape[0], x2.shape[0], D))
    t0 = 0
    for t in range(T):
        if (int(kind[t]) & tm.KIND_TIMES) and t < T - 1:
            continue
        for h in range(t0, t + 1):
            others = np.prod([rows[g][0] for g in range(t0, t + 1) if g != h] + [np.ones((x1.shape[0], x2.shape[0]))], axis=0)
            J += rows[h][1] * others[:, :, None]
        t0 = t + 1
    return J


def jacobian_from_table(table, Xs, X, kind=None, shape=None):
    """J (S, N, D): d K(Xs, X) / d Xs, channel pair by channel pair"""
    kind, shape = tm._kinds(kind, shape)
    C, D = table.shape[0], Xs.shape[1] - 1
    c1, c2 = Xs[:, 0].astype(np.int64), X[:, 0].astype(np.int64)
    J = np.zeros((Xs.shape[0], X.shape[0], D))
    for i in range(C):
        r1 = np.nonzero(c1 == i)[0]
        for j in range(C):
            r2 = np.nonzero(c2 == j)[0]
            if len(r1) == 0 or len(r2) == 0:
                continue
            x1, x2 = Xs[r1, 1:], X[r2, 1:]
            J[np.ix_(r1, r2)] = tm._jr_block(table[i, j], x1, x2) if kind is None else kinds_jacobian(table[i, j], kind[i, j], shape[i, j], x1, x2)
    return J


class DerivTableDevice(parts_twin.PartsTableDevice):
    def predict_grad(self, noise_var, jitter, dkss_diag, Xs, data_var=None):
        if self.kind is not None:
            for k, name in REFUSED.items():
                if np.any((np.asarray(self.kind) & tm.KIND_MASK) == k):
                    raise _lib.MogpError(_lib.MOGP_EINVAL, "mogp_exact_predict_grad: a %s row (kind %d)" % (name, k))
        S = Xs.shape[0]
        kappa = np.asarray(dkss_diag, dtype=np.float64)
        assert kappa.shape == (self.D, S), kappa.shape
        K, _ = self._Kj(noise_var, jitter, data_var)
        L = np.linalg.cholesky(K)
        alpha = solve_triangular(L.T, solve_triangular(L, self._residual(), lower=True), lower=False)
        J = jacobian_from_table(self.table, np.asarray(Xs, dtype=np.float64), self.X, self.kind, self.shape)
        dmu, dvar = np.empty((self.D, S)), np.empty((self.D, S))
        for d in range(self.D):
            v = solve_triangular(L, J[:, :, d].T, lower=True)
            dmu[d] = (J[:, :, d] @ alpha).reshape(-1)
            dvar[d] = kappa[d] - np.sum(v * v, axis=0)
        return dmu, dvar


def install(monkeypatch, which=None):
    """the twin in the device handle's place, as parts_twin.install does"""
    parts_twin.install(monkeypatch, which)
    monkeypatch.setattr(_lib, "ExactHandle", DerivTableDevice)
