"""
The numpy twin of mogp_exact_loo (include/mogp_hip.h, csrc/loo.hip) for the tests of the leave-one-out likelihood: a TableDevice
(oracle/table_model.py) with `loo()` written from the formulas of Rasmussen & Williams 5.4.2,
    kappa = diag Kj^-1, alpha = Kj^-1 r:   mu = y - alpha / kappa,  var = 1 / kappa,  L = sum 1/2 log kappa - alpha^2 / (2 kappa) - 1/2 log 2 pi
    a = 1/2 / kappa + alpha^2 / (2 kappa^2),  b = alpha / kappa,  rho = Kj^-1 b:   dL/dKj = -Kj^-1 diag(a) Kj^-1 + 1/2 (alpha rho^T + rho alpha^T),  dL/dr = -rho
and the oracle's own walks for what surrounds them: `_Kj` for the matrix, `moments_dense` (which takes kinds) for the moments of the dense
symmetric adjoint.  The row kinds the oracle does not carry come from the family twins (changepoint_twin, function_twin), which put their
`row_parts` in front of the oracle's: `install(monkeypatch, which)`.  The affine mean table of csrc/mean.hip is twinned here too (the
oracle's device has none): residual, its gradient table, and dp/dr for `fetch(3)`.
"""
import numpy as np

import oracle.table_model as tm
from mogptk_amd import _lib


class LooTableDevice(tm.TableDevice):
    mean_table = None

    def set_mean(self, coef):
        self.mean_table = None if coef is None else np.array(coef, dtype=np.float64)

    def _residual(self):
        if self.mean_table is None:
            return self.y
        c = self.X[:, 0].astype(np.int64)
        return self.y - (self.mean_table[c, 0] + np.sum(self.mean_table[c, 1:] * self.X[:, 1:], axis=1)).reshape(-1, 1)

    def mean_grad(self):
        """g[c] = sum_{k in c} dp/dr_k [1, x_k]"""
        c = self.X[:, 0].astype(np.int64)
        ext = np.concatenate([np.ones((self.N, 1)), self.X[:, 1:]], axis=1)
        return np.array([np.sum(self._dpdr[c == k, None] * ext[c == k], axis=0) for k in range(self.C)])

    def eval(self, noise_var, jitter, grad=True, data_var=None):
        raw, self.y = self.y, self._residual()
        try:
            res = super().eval(noise_var, jitter, grad=grad, data_var=data_var)
        finally:
            self.y = raw
        self._dpdr = -self._last[1].reshape(-1)              # dLML/dr = -alpha
        return res

    def loo(self, noise_var, jitter, grad=True, data_var=None):
        K, jit = self._Kj(noise_var, jitter, data_var, check_diag=True)
        Kinv = np.linalg.inv(K)
        Kinv = 0.5 * (Kinv + Kinv.T)
        r = self._residual().reshape(-1)
        alpha = Kinv @ r
        kappa = np.diagonal(Kinv).copy()
        mu = self.y.reshape(-1) - alpha / kappa               # the targets as they were given: under a mean table, the raw ones
        var = 1.0 / kappa
        L = float(np.sum(0.5 * np.log(kappa) - 0.5 * alpha * alpha / kappa - 0.5 * np.log(tm.TWO_PI)))
        self._last = (K, alpha.reshape(-1, 1))
        self._Kinv = Kinv
        out = dict(loo=L, mu=mu, var=var, moments=None, diagG=None, trG=0.0, jitter_abs=jit)
        if not grad:
            return out
        a = 0.5 / kappa + 0.5 * alpha * alpha / (kappa * kappa)
        b = alpha / kappa
        rho = Kinv @ b
        G = -(Kinv * a) @ Kinv + 0.5 * (np.outer(alpha, rho) + np.outer(rho, alpha))
        G = 0.5 * (G + G.T)
        self._dpdr = -rho
        c = self.X[:, 0].astype(np.int64)
        dG = np.diagonal(G)
        out.update(moments=tm.moments_dense(self.table, G, self.X, self.X, sym=True, kind=self.kind, shape=self.shape),
                   diagG=np.array([np.sum(dG[c == k]) for k in range(self.C)]), trG=float(np.sum(dG)))
        return out

    def fetch(self, which):
        if which == 3:
            return self._dpdr.copy()
        if which == 1 and getattr(self, "_Kinv", None) is not None:
            return self._Kinv.copy()
        return super().fetch(which)


def install(monkeypatch, which=None):
    """the twin in the device handle's place; which = 'changepoint' / 'function': that family's row kinds in front of the oracle's"""
    if which == "changepoint":
        import changepoint_twin
        changepoint_twin.install(monkeypatch)
    elif which == "function":
        import function_twin
        function_twin.install(monkeypatch)
    monkeypatch.setattr(_lib, "ExactHandle", LooTableDevice)
