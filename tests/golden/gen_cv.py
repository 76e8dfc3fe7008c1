"""
Golden vectors of leave-fold-out cross-validation in tests/golden/cv.npz.  Runs only where the reference (GAMES-UChile/mogptk) is
importable, like gen_loo.py; the fixture is data only.  The reference has no such score: what it contributes is the model -- kernel, noise,
mean, data variance, relative jitter -- and autograd.  Per case and fold layout of tests/cv_cases.py: the reference's Exact model at the raw
parameters of the fixture the case comes from, Kj formed as its log_marginal_likelihood forms it (gpr/model.py:438-442, :244), then in
float64 torch, fold by fold, the conditional Gaussian of y_B given every other point DIRECTLY from Kj (O: the points outside B)
    mu_B = m_B + Kj_BO Kj_OO^-1 r_O,   Sigma_B = Kj_BB - Kj_BO Kj_OO^-1 Kj_OB,   log N(y_B; mu_B, Sigma_B)
-- one Cholesky factorisation of Kj_OO per fold, no block of Kj^-1 anywhere: the identities the device and its numpy twin use do not appear
in their yardstick -- and the autograd gradient of -L - log prior with respect to every raw parameter, with cond(Kj), asserted below 1e5.
One case also records the trace of 20 Adam steps on the CV loss over blocks of 10 points.
Re-run:  python tests/golden/gen_cv.py [path to the reference]
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
import family_cases           # noqa: E402
import loo_cases              # noqa: E402
import cv_cases               # noqa: E402
from gen_loo import at_fixture_raw, N_      # noqa: E402

G = mogptk.gpr
torch.set_default_dtype(torch.float64)
HALF_LOG_2PI = 0.5 * np.log(2.0 * np.pi)


def cv_parts(m, lab):
    """(Kj, L, mu, var) of a reference Exact model under the fold labels lab, differentiable; mu and var NaN outside the folds"""
    Kff = m.kernel.K(m.X) + m._index_channel(m.likelihood.scale().square(), m.X) * m.eye
    if m.data_variance is not None:
        Kff = Kff + m.data_variance
    Kj = Kff + (m.jitter * Kff.diagonal().mean()).repeat(Kff.shape[0]).diagflat()
    y = m.y.reshape(-1)
    r = y if m.mean is None else y - m.mean(m.X).reshape(-1)
    n = Kj.shape[0]
    mu = torch.full((n,), float("nan"))
    var = torch.full((n,), float("nan"))
    L = torch.zeros(())
    for f in range(int(lab.max()) + 1):
        B = torch.tensor(np.flatnonzero(lab == f))
        O = torch.tensor(np.flatnonzero(lab != f))
        Lo = torch.linalg.cholesky(Kj[O][:, O])
        sol = torch.cholesky_solve(torch.cat([r[O].reshape(-1, 1), Kj[O][:, B]], dim=1), Lo)
        mean_r = Kj[B][:, O] @ sol[:, 0]                       # of the residual; the targets' mean adds m_B = y_B - r_B
        S = Kj[B][:, B] - Kj[B][:, O] @ sol[:, 1:]
        S = 0.5 * (S + S.T)
        Ls = torch.linalg.cholesky(S)
        z = torch.linalg.solve_triangular(Ls, (r[B] - mean_r).reshape(-1, 1), upper=False)
        L = L - 0.5 * torch.sum(z * z) - torch.sum(torch.log(Ls.diagonal())) - len(B) * HALF_LOG_2PI
        mu = mu.index_put((B,), (y[B] - r[B]) + mean_r)
        var = var.index_put((B,), S.diagonal())
    return Kj, L, mu, var


def cv_loss(m, lab):
    m.zero_grad(set_to_none=True)
    loss = -cv_parts(m, lab)[1] - m.log_prior()
    loss.backward()
    return loss


def main():
    out = {}
    for case, name in cv_cases.PAIRS:
        pre = "%s__%s__" % (case, name)
        m, (fx, fpre) = loo_cases.exact(G, case)
        ps = at_fixture_raw(m, fx, fpre)
        lab = cv_cases.labels(case, name, m)
        loss = cv_loss(m, lab)
        with torch.no_grad():
            Kj, L, mu, var = cv_parts(m, lab)
        cond = float(np.linalg.cond(N_(Kj)))
        assert cond < 1e5, (case, cond)
        out[pre + "cv"] = np.array(float(L))
        out[pre + "loss"] = np.array(float(loss.detach()))
        out[pre + "cond"] = np.array(cond)
        for i, p in enumerate(ps):
            assert p.grad is not None and bool(torch.all(torch.isfinite(p.grad))), (case, p._name)
            out["%sp%d_grad" % (pre, i)] = N_(p.grad)
        if not loo_cases.CASES[case].get("light"):
            out[pre + "mu"], out[pre + "var"] = N_(mu), N_(var)
        sizes = np.bincount(lab[lab >= 0])
        print("%-8s %-10s N = %4d  folds = %3d (%d .. %d points, %d in none)  cond(Kj) = %.3g  L = %.6f"
              % (case, name, Kj.shape[0], sizes.size, sizes.min(), sizes.max(), int(np.sum(lab < 0)), cond, float(L)))

    # 20 Adam steps on the CV loss over blocks of 10 points, the loop of the reference's Model.train (mogptk/model.py:556-566) with the CV loss in its place
    sc = family_cases.cases(loo_cases.CASES[cv_cases.ADAM_CASE]["family"])
    acase = loo_cases.CASES[cv_cases.ADAM_CASE]["case"]
    X, y, _ = sc.data(acase)
    mm = mogptk.Model(mogptk.DataSet(mogptk.Data(X[:, 0], y, name="a")), G.IndependentMultiOutputKernel(sc.kernel(G, acase), output_dims=1),
                      inference=mogptk.Exact(variance=sc.NOISE))
    lab = cv_cases.block_labels(cv_cases.model_inputs(mm.gpr), cv_cases.ADAM_BLOCK)
    opt = torch.optim.Adam(mm.gpr.parameters(), lr=cv_cases.ADAM_LR)
    losses = []
    for _ in range(cv_cases.ADAM_ITERS):
        losses.append(float(cv_loss(mm.gpr, lab).detach()))
        opt.step()
    losses.append(float(cv_loss(mm.gpr, lab).detach()))
    assert losses[-1] < losses[0]
    out["adam__losses"] = np.array(losses, dtype=np.float64)
    out["adam__final"] = np.concatenate([N_(p.data).reshape(-1) for p in mm.gpr.parameters()])
    out["adam__labels"] = lab.astype(np.int32)
    print("adam: %.6f -> %.6f" % (losses[0], losses[-1]))

    path = os.path.join(HERE, "cv.npz")
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) < 1 << 20
    print("wrote cv.npz", os.path.getsize(path), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
