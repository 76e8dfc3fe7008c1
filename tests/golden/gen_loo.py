"""
Golden vectors of the leave-one-out predictive likelihood (Rasmussen & Williams 5.4.2) in tests/golden/loo.npz.  Runs only where the reference
(GAMES-UChile/mogptk) is importable, like gen_family.py; the fixture is data only.  The reference has no such score: what it contributes
is the model -- kernel, noise, mean, data variance, relative jitter -- and autograd.  Per case of tests/loo_cases.py: the reference's Exact
model at the raw parameters of the fixture the case comes from (they are not repeated here), Kj formed as its log_marginal_likelihood forms it
(gpr/model.py:438-442, :244), then in float64 torch
    Kinv = Kj^-1, alpha = Kinv r, kappa = diag Kinv:   mu = y - alpha / kappa,  var = 1 / kappa,
    L = sum_i 1/2 log kappa_i - alpha_i^2 / (2 kappa_i) - 1/2 log 2 pi
and the autograd gradient of -L - log prior with respect to every raw parameter, with cond(Kj) -- asserted below 1e5, the families' bound.
On one N = 150 case the closed form is checked against N refits (numpy, 1e-10).  One case also records the trace of 20 Adam steps on the
LOO loss (torch.optim.Adam over the raw parameters, as the reference's Model.train runs it on its own loss).
Re-run:  python tests/golden/gen_loo.py [path to the reference]
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

G = mogptk.gpr
torch.set_default_dtype(torch.float64)
N_ = lambda t: t.detach().cpu().numpy().astype(np.float64)
HALF_LOG_2PI = 0.5 * np.log(2.0 * np.pi)


def at_fixture_raw(m, fx, pre):
    """the model's parameters at the raw values of the fixture the case comes from (same names, same order)"""
    ps = list(m.parameters())
    assert [p._name for p in ps] == [str(n) for n in fx[pre + "names"]], pre
    with torch.no_grad():
        for i, p in enumerate(ps):
            raw = torch.tensor(np.asarray(fx["%sp%d_raw" % (pre, i)], dtype=np.float64))
            assert tuple(raw.shape) == tuple(p.data.shape), p._name
            p.data.copy_(raw)
    return ps


def loo_parts(m):
    """(Kj, residual, L, mu, var) of a reference Exact model, differentiable"""
    Kff = m.kernel.K(m.X) + m._index_channel(m.likelihood.scale().square(), m.X) * m.eye
    if m.data_variance is not None:
        Kff = Kff + m.data_variance
    Kj = Kff + (m.jitter * Kff.diagonal().mean()).repeat(Kff.shape[0]).diagflat()
    r = m.y if m.mean is None else m.y - m.mean(m.X).reshape(-1, 1)
    Kinv = torch.cholesky_inverse(torch.linalg.cholesky(Kj))
    alpha = (Kinv @ r).reshape(-1)
    kappa = Kinv.diagonal()
    mu = m.y.reshape(-1) - alpha / kappa
    L = torch.sum(0.5 * torch.log(kappa) - 0.5 * alpha * alpha / kappa - HALF_LOG_2PI)
    return Kj, r, L, mu, 1.0 / kappa


def loo_loss(m):
    m.zero_grad(set_to_none=True)
    loss = -loo_parts(m)[2] - m.log_prior()
    loss.backward()
    return loss


def brute_force(Kj, r, y):
    """N refits: the prediction of point i from the others under the same Kj"""
    n = Kj.shape[0]
    mu, var = np.zeros(n), np.zeros(n)
    for i in range(n):
        o = np.arange(n) != i
        sol = np.linalg.solve(Kj[np.ix_(o, o)], np.stack([r[o], Kj[o, i]], axis=1))
        mu[i] = (y[i] - r[i]) + Kj[i, o] @ sol[:, 0]
        var[i] = Kj[i, i] - Kj[i, o] @ sol[:, 1]
    return mu, var, float(np.sum(-0.5 * np.log(2.0 * np.pi * var) - 0.5 * (y - mu) ** 2 / var))


def main():
    out = {}
    for case, c in loo_cases.CASES.items():
        pre = case + "__"
        m, (fx, fpre) = loo_cases.exact(G, case)
        ps = at_fixture_raw(m, fx, fpre)
        loss = loo_loss(m)
        Kj, r, L, mu, var = loo_parts(m)
        cond = float(np.linalg.cond(N_(Kj)))
        assert cond < 1e5, (case, cond)
        out[pre + "loo"] = np.array(float(L.detach()))
        out[pre + "loss"] = np.array(float(loss.detach()))
        out[pre + "cond"] = np.array(cond)
        for i, p in enumerate(ps):
            assert p.grad is not None and bool(torch.all(torch.isfinite(p.grad))), (case, p._name)
            out["%sp%d_grad" % (pre, i)] = N_(p.grad)
        if not c.get("light"):
            out[pre + "mu"], out[pre + "var"] = N_(mu), N_(var)
        print("%-8s N = %4d  cond(Kj) = %.3g  L = %.6f" % (case, Kj.shape[0], cond, float(L.detach())))
        if case == loo_cases.BRUTE_CASE:
            bmu, bvar, bL = brute_force(N_(Kj), N_(r).reshape(-1), N_(m.y).reshape(-1))
            errs = (np.max(np.abs(bmu - N_(mu))), np.max(np.abs(bvar - N_(var))), abs(bL - float(L.detach())) / max(1.0, abs(bL)))
            print("         closed form against %d refits: mu %.2e  var %.2e  L %.2e" % ((Kj.shape[0],) + errs))
            assert max(errs) <= 1e-10, errs

    # 20 Adam steps on the LOO loss, the loop of the reference's Model.train (mogptk/model.py:556-566) with the LOO loss in its place
    sc = family_cases.cases(loo_cases.CASES[loo_cases.ADAM_CASE]["family"])
    acase = loo_cases.CASES[loo_cases.ADAM_CASE]["case"]
    X, y, _ = sc.data(acase)
    mm = mogptk.Model(mogptk.DataSet(mogptk.Data(X[:, 0], y, name="a")), G.IndependentMultiOutputKernel(sc.kernel(G, acase), output_dims=1),
                      inference=mogptk.Exact(variance=sc.NOISE))
    opt = torch.optim.Adam(mm.gpr.parameters(), lr=loo_cases.ADAM_LR)
    losses = []
    for _ in range(loo_cases.ADAM_ITERS):
        losses.append(float(loo_loss(mm.gpr).detach()))
        opt.step()
    losses.append(float(loo_loss(mm.gpr).detach()))
    assert losses[-1] < losses[0]
    out["adam__losses"] = np.array(losses, dtype=np.float64)
    out["adam__final"] = np.concatenate([N_(p.data).reshape(-1) for p in mm.gpr.parameters()])
    print("adam: %.6f -> %.6f" % (losses[0], losses[-1]))

    path = os.path.join(HERE, "loo.npz")
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) < 1 << 20
    print("wrote loo.npz", os.path.getsize(path), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
