"""
The numpy twin of mogp_exact_predict_grad_cov (include/mogp_hip.h, csrc/exact.hip, csrc/gram.hip:k_gram_dxdx) for the tests of the joint
posterior covariance of df/dx: deriv_twin's device whose `predict_grad` takes `full=True`,
    dcov[a, d, b, e] = H_de[a][b] - (L^-1 J_d(x*_a))^T (L^-1 J_e(x*_b)),   H_de[a][b] = d^2 K(x_a, x_b) / dx_a,d dx_b,e,
Kj, L, J and the jitter those of deriv_twin.  H is written here from the formulas of the issue, row by row -- every row brings its value, its two
first derivatives and its mixed second derivative -- and a product group is the EXPLICIT double sum
    sum_h H_h prod_{g != h} k_g + sum_{h != g} (d_a k_h)(d_b k_g) prod_{f != h, g} k_f
with the other rows' values multiplied up again for every term (the device carries the product rule forward instead).  The third profile function
chi = -2 dpsi/ds is written here in closed form, with sinc's series summed term by term from factorials.
"""
import math
import numpy as np
from scipy.linalg import solve_triangular

import oracle.table_model as tm
import deriv_twin
from mogptk_amd import _lib

KIND_PERIODIC, KIND_DOT = deriv_twin.KIND_PERIODIC, deriv_twin.KIND_DOT
ROWS_MAX = 8192


def chi_profile(kind, shape, s):
    """chi(s) = -2 dpsi/ds; returned as 0 where Matern 3/2 has r = 0 (chi ~ 1/r there, and the product u_d u_e chi it enters is O(r))"""
    r = np.sqrt(s)
    if kind == tm.KIND_RQ:
        return (shape + 1.0) / shape * (1.0 + s / (2.0 * shape)) ** (-shape - 2.0)
    if kind == tm.KIND_MATERN32:
        pos = r > 0
        return np.where(pos, 9.0 * np.exp(-tm.SQ3 * r) / np.where(pos, tm.SQ3 * r, 1.0), 0.0)
    if kind == tm.KIND_MATERN52:
        return (25.0 / 3.0) * np.exp(-tm.SQ5 * r)
    if kind == tm.KIND_SINC:                                # (3 psi - pi^2 phi) / s, and 2 pi^4 sum_j (-x)^j (j + 1)(2j + 4) / (2j + 5)! for x = pi^2 s <= 1
        phi, psi = tm.profiles(kind, shape, s)
        x = np.pi ** 2 * s
        series = 2.0 * np.pi ** 4 * sum((-x) ** j * (j + 1) * (2 * j + 4) / math.factorial(2 * j + 5) for j in range(12))
        small = x <= 1.0
        return np.where(small, series, (3.0 * psi - np.pi ** 2 * phi) / np.where(small, 1.0, s))
    return np.exp(-0.5 * s)


def row_hessian(row, kind, shape, x1, x2):
    """(k, d k / d x1 (n1, n2, D), d k / d x2 (n1, n2, D), d^2 k / d x1_d d x2_e (n1, n2, D, D)) of one table row, amplitude included"""
    D = x1.shape[1]
    A = row[0]
    eye = np.eye(D)
    if kind == KIND_DOT:
        n = int(shape)
        b = A * (x1 @ x2.T) + row[1]
        p1 = n * b ** (n - 1) if n > 1 else np.ones_like(b)
        p2 = n * (n - 1) * b ** (n - 2) if n > 1 else np.zeros_like(b)
        xa, xb = x1[:, None, :] + 0.0 * x2[None, :, :], x2[None, :, :] + 0.0 * x1[:, None, :]
        H = (p2 * A * A)[:, :, None, None] * xb[:, :, :, None] * xa[:, :, None, :] + (p1 * A)[:, :, None, None] * eye
        return b ** n, (p1 * A)[:, :, None] * xb, (p1 * A)[:, :, None] * xa, H
    Psi, V, M = row[1], row[2:2 + D], row[2 + D:2 + 2 * D]
    u = x1[:, None, :] - x2[None, :, :] + row[2 + 2 * D:2 + 3 * D]
    th = tm.TWO_PI * (np.sum(M * u, axis=2) + Psi)
    c, sn = np.cos(th), np.sin(th)
    w = tm.TWO_PI * M
    if kind == KIND_PERIODIC:
        E = A * np.exp(V[0] * (c - 1.0))
        ku = (-E * V[0] * w[0] * sn)[:, :, None]
        return E, ku, -ku, (E * V[0] * w[0] ** 2 * (c - V[0] * sn * sn))[:, :, None, None]
    s = np.sum(V * u * u, axis=2)
    phi, psi = tm.profiles(kind, shape, s)
    chi = chi_profile(kind, shape, s)
    Vu = V * u
    ku = A * (-(psi * c)[:, :, None] * Vu - (phi * sn)[:, :, None] * w)
    outer = Vu[:, :, :, None] * Vu[:, :, None, :]
    cross = Vu[:, :, :, None] * w[None, None, None, :] + w[None, None, :, None] * Vu[:, :, None, :]
    H = A * ((psi[:, :, None, None] * (eye * V) - chi[:, :, None, None] * outer + phi[:, :, None, None] * np.outer(w, w)) * c[:, :, None, None]
             - (psi * sn)[:, :, None, None] * cross)
    return A * phi * c, ku, -ku, H


def kinds_hessian(tab, kind, shape, x1, x2):
    """the mixed second derivative of one channel-pair block of a table with kinds: (n1, n2, D, D)"""
    T, D = tab.shape[0], x1.shape[1]
    kd = kind & tm.KIND_MASK
    rows = [row_hessian(tab[t], int(kd[t]), shape[t], x1, x2) for t in range(T)]
    one = np.ones((x1.shape[0], x2.shape[0]))
    H = np.zeros((x1.shape[0], x2.shape[0], D, D))
    t0 = 0
    for t in range(T):
        if (int(kind[t]) & tm.KIND_TIMES) and t < T - 1:
            continue
        grp = range(t0, t + 1)
        for h in grp:
            H += rows[h][3] * np.prod([rows[f][0] for f in grp if f != h] + [one], axis=0)[:, :, None, None]
            for g in grp:
                if g != h:
                    rest = np.prod([rows[f][0] for f in grp if f != h and f != g] + [one], axis=0)
                    H += rows[h][1][:, :, :, None] * rows[g][2][:, :, None, :] * rest[:, :, None, None]
        t0 = t + 1
    return H


def gauss_hessian(tab, x1, x2):
    """the same of a table without kinds: Gaussian rows, with the envelope on the midpoint where the rows carry one"""
    D = x1.shape[1]
    A, V, M = tab[:, 0], tab[:, 2:2 + D], tab[:, 2 + D:2 + 2 * D]
    Ec, Es, u, a = tm.table_block(tab, x1, x2, with_mid=True)             # (T, n1, n2): g E cos, g E sin; u, a (T, n1, n2, D)
    eye = np.eye(D)
    H = np.zeros((x1.shape[0], x2.shape[0], D, D))
    for t in range(tab.shape[0]):
        Vu, w = V[t] * u[t], tm.TWO_PI * M[t]
        hd = -(Ec[t][:, :, None] * Vu + Es[t][:, :, None] * w)                      # g dh/du_d  (without the amplitude)
        hde = (Vu[:, :, :, None] * Vu[:, :, None, :] - eye * V[t] - np.outer(w, w)) * Ec[t][:, :, None, None] \
            + (Vu[:, :, :, None] * w[None, None, None, :] + w[None, None, :, None] * Vu[:, :, None, :]) * Es[t][:, :, None, None]
        Ht = -hde
        if a is not None:
            Lv = tab[t, 2 + 3 * D:2 + 4 * D]
            gd = -Lv * a[t]                                                         # (dg/dm_d) / g
            gde = gd[:, :, :, None] * gd[:, :, None, :] - eye * Lv
            Ht = Ht + 0.5 * hd[:, :, :, None] * gd[:, :, None, :] - 0.5 * gd[:, :, :, None] * hd[:, :, None, :] + 0.25 * gde * Ec[t][:, :, None, None]
        H += A[t] * Ht
    return H


def hessian_from_table(table, Xa, Xb, kind=None, shape=None):
    """H (Sa, D, Sb, D): d^2 K(Xa, Xb) / d Xa_d d Xb_e, channel pair by channel pair"""
    kind, shape = tm._kinds(kind, shape)
    C, D = table.shape[0], Xa.shape[1] - 1
    c1, c2 = Xa[:, 0].astype(np.int64), Xb[:, 0].astype(np.int64)
    H = np.zeros((Xa.shape[0], Xb.shape[0], D, D))
    for i in range(C):
        r1 = np.nonzero(c1 == i)[0]
        for j in range(C):
            r2 = np.nonzero(c2 == j)[0]
            if len(r1) == 0 or len(r2) == 0:
                continue
            x1, x2 = Xa[r1, 1:], Xb[r2, 1:]
            H[np.ix_(r1, r2)] = gauss_hessian(table[i, j], x1, x2) if kind is None else kinds_hessian(table[i, j], kind[i, j], shape[i, j], x1, x2)
    return H.transpose(0, 2, 1, 3)


class DcovTableDevice(deriv_twin.DerivTableDevice):
    def predict_grad(self, noise_var, jitter, dkss_diag, Xs, data_var=None, full=False):
        if not full:
            return super().predict_grad(noise_var, jitter, dkss_diag, Xs, data_var=data_var)
        assert dkss_diag is None
        S = Xs.shape[0]
        if self.D * S > ROWS_MAX:
            raise _lib.MogpError(_lib.MOGP_EINVAL, "mogp_exact_predict_grad_cov: D * S = %d stacked rows, limited to %d" % (self.D * S, ROWS_MAX))
        if self.kind is not None:
            for k, name in deriv_twin.REFUSED.items():
                if np.any((np.asarray(self.kind) & tm.KIND_MASK) == k):
                    raise _lib.MogpError(_lib.MOGP_EINVAL, "mogp_exact_predict_grad_cov: a %s row (kind %d)" % (name, k))
        Xs = np.asarray(Xs, dtype=np.float64)
        K, _ = self._Kj(noise_var, jitter, data_var)
        L = np.linalg.cholesky(K)
        alpha = solve_triangular(L.T, solve_triangular(L, self._residual(), lower=True), lower=False)
        J = deriv_twin.jacobian_from_table(self.table, Xs, self.X, self.kind, self.shape)      # (S, N, D)
        Jrows = J.transpose(0, 2, 1).reshape(S * self.D, -1)                                    # row a * D + d
        V = solve_triangular(L, Jrows.T, lower=True)
        H = hessian_from_table(self.table, Xs, Xs, self.kind, self.shape)
        dcov = H.reshape(S * self.D, S * self.D) - V.T @ V
        dmu = (Jrows @ alpha).reshape(S, self.D).T
        return np.ascontiguousarray(dmu), dcov.reshape(S, self.D, S, self.D)


def install(monkeypatch, which=None):
    """the twin in the device handle's place, as deriv_twin.install does"""
    deriv_twin.install(monkeypatch, which)
    monkeypatch.setattr(_lib, "ExactHandle", DcovTableDevice)
