"""
The numpy twin of mogp_exact_forecast (include/mogp_hip.h, csrc/forecast.hip) for the tests of the rolling-origin forecast: cv_twin's CvTableDevice
with `forecast()` written from the DEFINITION -- for the point at time position p and the cut c, with A = order[:c] the rows the prediction may use,
    mu = m_p + Kj[p, A] Kj[A, A]^-1 r_A,    var = Kj[p, p] - Kj[p, A] Kj[A, A]^-1 Kj[A, p],    log N(y_p; mu, var)
by one direct solve with Kj[A, A] per distinct cut (numpy's LU), never through a factor of the whole matrix: the device reads these numbers off
the rows of one Cholesky factor, and the two agree only if both are right.  Everything around it -- the matrix, the mean table -- is loo_twin's and
the oracle's.
"""
import numpy as np

from mogptk_amd import _lib
import cv_twin
import loo_twin


def conditionals(Kj, r, m0, order, cut):
    """mu, var (H, N) in the row order of Kj (NaN where cut = -1) of every point given the `cut` rows in front of it in `order`; m0: the mean at every row"""
    N = Kj.shape[0]
    H = cut.shape[0]
    mu, var = np.full((H, N), np.nan), np.full((H, N), np.nan)
    for h in range(H):
        for c in np.unique(cut[h]):
            if c < 0:
                continue
            rows = order[np.flatnonzero(cut[h] == c)]
            if c == 0:
                mu[h, rows], var[h, rows] = m0[rows], np.diagonal(Kj)[rows]
                continue
            A = order[:c]
            sol = np.linalg.solve(Kj[np.ix_(A, A)], np.concatenate([r[A].reshape(-1, 1), Kj[np.ix_(A, rows)]], axis=1))
            mu[h, rows] = m0[rows] + Kj[np.ix_(rows, A)] @ sol[:, 0]
            var[h, rows] = np.diagonal(Kj)[rows] - np.einsum("ia,ai->i", Kj[np.ix_(rows, A)], sol[:, 1:])
    return mu, var


def scores(y, mu, var):
    return np.nansum(-0.5 * np.log(2.0 * np.pi * var) - 0.5 * np.square(y.reshape(1, -1) - mu) / var, axis=1)


class ForecastTableDevice(cv_twin.CvTableDevice):
    def forecast(self, noise_var, jitter, order, cut, data_var=None):
        order, cut = np.asarray(order), np.asarray(cut)
        assert order.shape == (self.N,) and np.array_equal(np.sort(order), np.arange(self.N))
        assert cut.ndim == 2 and cut.shape[1] == self.N and 1 <= cut.shape[0] <= 8 and cut.min() >= -1 and np.all(cut <= np.arange(self.N))
        K, jit = self._Kj(noise_var, jitter, data_var, check_diag=True)
        r = self._residual().reshape(-1)
        y = self.y.reshape(-1)                                  # the targets as they were given: under a mean table, the raw ones
        mu, var = conditionals(K, r, y - r, order, cut)
        return dict(score=scores(y, mu, var), mu=mu, var=var, jitter_abs=jit)


def install(monkeypatch, which=None):
    """the twin in the device handle's place; which = 'changepoint' / 'function': that family's row kinds in front of the oracle's"""
    loo_twin.install(monkeypatch, which)
    monkeypatch.setattr(_lib, "ExactHandle", ForecastTableDevice)
