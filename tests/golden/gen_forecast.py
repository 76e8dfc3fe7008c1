"""
Golden vectors of the rolling-origin forecast in tests/golden/forecast.npz.  Runs only where the reference (GAMES-UChile/mogptk) is
importable, like gen_cv.py; the fixture is data only.  The reference has no such score: what it contributes is the model -- kernel, noise, mean,
data variance, relative jitter.  Per case and cut layout of tests/forecast_cases.py: the reference's Exact model at the raw parameters of the
fixture the case comes from, Kj formed as its log_marginal_likelihood forms it (gpr/model.py:438-442, :244), then in float64 torch, for every
distinct cut c of a row of the layout, the conditional Gaussian of the points with that cut given the rows A = order[:c] DIRECTLY from Kj
    mu = m + Kj[., A] Kj[A, A]^-1 r_A,   var = diag(Kj[., .] - Kj[., A] Kj[A, A]^-1 Kj[A, .]),   log N(y; mu, var)
-- one Cholesky factorisation of Kj[A, A] per cut, never a factor of the whole matrix: the identity the device uses (the rows of ONE factor in time
order) does not appear in its yardstick.  cond(Kj) is asserted below 1e5, and every layout with cut = p is held to the reference's own
log_marginal_likelihood (the chain rule of the joint density).
Re-run:  python tests/golden/gen_forecast.py [path to the reference]
"""
import os
import sys
import types
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
ip, disp = types.ModuleType("IPython"), types.ModuleType("IPython.display")
disp.display = lambda *a, **k: None
disp.HTML = lambda s: s
ip.display = disp
sys.modules["IPython"] = ip
sys.modules["IPython.display"] = disp
sys.path.insert(0, sys.argv[1] if len(sys.argv) > 1 else os.environ.get("MOGPTK_REFERENCE", "reference"))
import torch                  # noqa: E402
import mogptk                 # noqa: E402
import loo_cases              # noqa: E402
import forecast_cases         # noqa: E402
from gen_loo import at_fixture_raw, N_      # noqa: E402

G = mogptk.gpr
torch.set_default_dtype(torch.float64)


def joint(m):
    """(Kj, r, y) of a reference Exact model"""
    Kff = m.kernel.K(m.X) + m._index_channel(m.likelihood.scale().square(), m.X) * m.eye
    if m.data_variance is not None:
        Kff = Kff + m.data_variance
    Kj = Kff + (m.jitter * Kff.diagonal().mean()).repeat(Kff.shape[0]).diagflat()
    y = m.y.reshape(-1)
    r = y if m.mean is None else y - m.mean(m.X).reshape(-1)
    return Kj, r, y


def forecast(Kj, r, y, order, cut):
    N, H = Kj.shape[0], cut.shape[0]
    mu, var = torch.full((H, N), float("nan")), torch.full((H, N), float("nan"))
    for h in range(H):
        for c in np.unique(cut[h]):
            if c < 0:
                continue
            B = torch.tensor(order[np.flatnonzero(cut[h] == c)])
            if c == 0:
                mu[h, B], var[h, B] = (y - r)[B], Kj.diagonal()[B]
                continue
            A = torch.tensor(order[:c])
            La = torch.linalg.cholesky(Kj[A][:, A])
            sol = torch.cholesky_solve(torch.cat([r[A].reshape(-1, 1), Kj[A][:, B]], dim=1), La)
            mu[h, B] = (y - r)[B] + Kj[B][:, A] @ sol[:, 0]
            var[h, B] = Kj.diagonal()[B] - torch.sum(Kj[B][:, A] * sol[:, 1:].T, dim=1)
    terms = -0.5 * torch.log(2.0 * np.pi * var) - 0.5 * (y.reshape(1, -1) - mu) ** 2 / var
    return mu, var, torch.nansum(terms, dim=1)


def main():
    out = {}
    for case, name in forecast_cases.PAIRS:
        pre = "%s__%s__" % (case, name)
        m, (fx, fpre) = loo_cases.exact(G, case)
        at_fixture_raw(m, fx, fpre)
        order, cut = forecast_cases.layout(case, name, m)
        with torch.no_grad():
            Kj, r, y = joint(m)
            mu, var, score = forecast(Kj, r, y, order, cut)
            lml = float(m.log_marginal_likelihood())
        cond = float(np.linalg.cond(N_(Kj)))
        assert cond < 1e5, (case, cond)
        assert bool(torch.all(var[~torch.isnan(var)] > 0))
        for h in range(cut.shape[0]):
            if np.array_equal(cut[h], np.arange(len(order))):          # the chain rule: the reference's own LML
                assert abs(float(score[h]) - lml) <= 1e-10 * max(1.0, abs(lml)), (case, name, float(score[h]), lml)
        out[pre + "score"] = N_(score)
        out[pre + "lml"] = np.array(lml)
        out[pre + "cond"] = np.array(cond)
        if not loo_cases.CASES[case].get("light"):
            out[pre + "mu"], out[pre + "var"] = N_(mu), N_(var)
        print("%-8s %-9s N = %4d  H = %d  skipped = %4d  cond(Kj) = %.3g  LML = %.6f  scores = %s"
              % (case, name, Kj.shape[0], cut.shape[0], int(np.sum(cut < 0)), cond, lml, np.array2string(N_(score), precision=4)))
    path = os.path.join(HERE, "forecast.npz")
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) < 1 << 20
    print("wrote forecast.npz", os.path.getsize(path), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
