"""
The numpy twin of mogp_exact_cv (include/mogp_hip.h, csrc/lfo.hip) for the tests of leave-fold-out cross-validation: loo_twin's LooTableDevice
with `cv()` written from the block formulas -- P = Kj^-1, alpha = P r and, per fold B,
    Sigma_B = (P_BB)^-1,  b_B = Sigma_B alpha_B:   mu_B = y_B - b_B,  var_B = diag Sigma_B,
    log p(y_B | y_-B) = -1/2 alpha_B^T b_B + 1/2 log det P_BB - |B|/2 log 2 pi
    E_B = 1/2 Sigma_B + 1/2 b_B b_B^T,  rho = P b:   dL/dKj = -P E P + 1/2 (alpha rho^T + rho alpha^T),  dL/dr = -rho
-- with numpy's own inverse, solve and slogdet per block (the device factors P_BB = L L^T and works with L^-1: the two agree through the
mathematics, not through shared steps).  Everything around it -- the matrix, the moments of the dense symmetric adjoint for every row kind, the
mean table -- is loo_twin's and the oracle's.
"""
import numpy as np

import oracle.table_model as tm
from mogptk_amd import _lib
import loo_twin


class CvTableDevice(loo_twin.LooTableDevice):
    def cv(self, noise_var, jitter, fold, nfolds, grad=True, data_var=None):
        fold = np.asarray(fold)
        assert fold.shape == (self.N,) and fold.dtype == np.int32 and fold.min() >= -1 and fold.max() == nfolds - 1
        K, jit = self._Kj(noise_var, jitter, data_var, check_diag=True)
        P = np.linalg.inv(K)
        P = 0.5 * (P + P.T)
        r = self._residual().reshape(-1)
        alpha = P @ r
        mu, var = np.full(self.N, np.nan), np.full(self.N, np.nan)
        b = np.zeros(self.N)
        E = np.zeros((self.N, self.N))
        L = 0.0
        for f in range(nfolds):
            B = np.flatnonzero(fold == f)
            assert 1 <= B.size <= 128
            PBB = P[np.ix_(B, B)]
            S = np.linalg.inv(PBB)
            S = 0.5 * (S + S.T)
            bB = np.linalg.solve(PBB, alpha[B])
            sign, logdet = np.linalg.slogdet(PBB)
            assert sign > 0
            L += -0.5 * alpha[B] @ bB + 0.5 * logdet - 0.5 * B.size * np.log(tm.TWO_PI)
            mu[B] = self.y.reshape(-1)[B] - bB                 # the targets as they were given: under a mean table, the raw ones
            var[B] = np.diagonal(S)
            b[B] = bB
            E[np.ix_(B, B)] = 0.5 * S + 0.5 * np.outer(bB, bB)
        self._last = (K, alpha.reshape(-1, 1))
        self._Kinv = P
        out = dict(cv=float(L), mu=mu, var=var, moments=None, diagG=None, trG=0.0, jitter_abs=jit)
        if not grad:
            return out
        rho = P @ b
        G = -P @ E @ P + 0.5 * (np.outer(alpha, rho) + np.outer(rho, alpha))
        G = 0.5 * (G + G.T)
        self._dpdr = -rho
        c = self.X[:, 0].astype(np.int64)
        dG = np.diagonal(G)
        out.update(moments=tm.moments_dense(self.table, G, self.X, self.X, sym=True, kind=self.kind, shape=self.shape),
                   diagG=np.array([np.sum(dG[c == k]) for k in range(self.C)]), trG=float(np.sum(dG)))
        return out


def install(monkeypatch, which=None):
    """the twin in the device handle's place; which = 'changepoint' / 'function': that family's row kinds in front of the oracle's"""
    loo_twin.install(monkeypatch, which)
    monkeypatch.setattr(_lib, "ExactHandle", CvTableDevice)
