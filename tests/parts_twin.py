"""
The numpy twin of mogp_exact_predict_parts (include/mogp_hip.h, csrc/exact.hip) for the tests of the posterior by kernel part: a
TableDevice (oracle/table_model.py; through loo_twin's, which carries the affine mean table) with `predict_parts` written from the formulas
    mu_p = K_p(Xs, X) Kj^-1 r,   var_p = kss_diag_p - colsum((L^-1 K_p(X, Xs))^2)   (full: K_p(Xs, Xs) - V^T V),
Kj, r and the jitter the whole model's (`_Kj`, `_residual`), K_p the oracle's Gram walk over part p's table.  `predict` is the same
arithmetic with the model's own table as the one part, so a model predicts through one code path here as on the device.  The twin also
holds the ABI's rule on part tables: only amplitudes, and the bias of dot-product rows, may differ from the table last set.  Row kinds the
oracle does not carry come from the family twins, as in loo_twin: `install(monkeypatch, which)`.
"""
import numpy as np
from scipy.linalg import solve_triangular

import oracle.table_model as tm
import loo_twin
from mogptk_amd import _lib

KIND_DOT, POINT_KINDS = 7, (7, 8, 9)


class PartsTableDevice(loo_twin.LooTableDevice):
    def _check_part_tables(self, tabs):
        assert tabs.ndim == 5 and tabs.shape[1:] == self.table.shape, (tabs.shape, self.table.shape)
        free = np.zeros(self.table.shape, dtype=bool)
        free[..., 0] = True
        if self.kind is not None:
            free[..., 1] = (np.asarray(self.kind) & tm.KIND_MASK) == KIND_DOT
        same = (tabs == self.table[None]) | free[None]
        assert np.all(same), "a part table differs from the model's outside the amplitudes and dot-product biases at %s" % (np.argwhere(~same)[0],)

    def predict_parts(self, noise_var, jitter, part_tables, kss_diag, Xs, full=False, data_var=None):
        tabs = np.asarray(part_tables, dtype=np.float64)
        self._check_part_tables(tabs)
        P, S = tabs.shape[0], Xs.shape[0]
        K, _ = self._Kj(noise_var, jitter, data_var)
        L = np.linalg.cholesky(K)
        alpha = solve_triangular(L.T, solve_triangular(L, self._residual(), lower=True), lower=False)
        kinds = None if self.kind is None else np.asarray(self.kind) & tm.KIND_MASK
        per_point = self.table.shape[3] > 2 + 3 * self.D or (kinds is not None and bool(np.any(np.isin(kinds, POINT_KINDS))))
        kss = np.asarray(kss_diag, dtype=np.float64)
        assert kss.shape == (P, S if per_point else self.C), (kss.shape, per_point)
        cs = Xs[:, 0].astype(np.int64)
        mu, var = np.empty((P, S, 1)), np.empty((P, S, S) if full else (P, S, 1))
        for p in range(P):
            Kfs = tm.gram_from_table(tabs[p], self.X, Xs, self.kind, self.shape)
            v = solve_triangular(L, Kfs, lower=True)
            mu[p] = Kfs.T @ alpha
            if full:
                var[p] = tm.gram_from_table(tabs[p], Xs, None, self.kind, self.shape) - v.T @ v
            else:
                var[p, :, 0] = (kss[p] if per_point else kss[p][cs]) - np.sum(v * v, axis=0)
        return mu, var

    def predict(self, noise_var, jitter, kss_diag, Xs, full=False, data_var=None):
        mu, var = self.predict_parts(noise_var, jitter, self.table[None], np.asarray(kss_diag, dtype=np.float64).reshape(1, -1), Xs, full=full, data_var=data_var)
        return mu[0], var[0]


def install(monkeypatch, which=None):
    """the twin in the device handle's place; which = 'changepoint' / 'function': that family's row kinds in front of the oracle's"""
    loo_twin.install(monkeypatch, which)
    monkeypatch.setattr(_lib, "ExactHandle", PartsTableDevice)
