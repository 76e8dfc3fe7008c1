"""
Golden vectors of the posterior of df/dx in tests/golden/deriv.npz.  Runs only where the reference (GAMES-UChile/mogptk) is
importable, like gen_parts.py; the fixture is data only.  The reference has no such call: what it contributes is the model -- kernel, noise,
mean, relative jitter -- and its own kernel objects in float64.  Per case of tests/deriv_cases.py: Kj, L and alpha formed as the reference's
predict_f forms them (gpr/model.py:455-472, :244), and
    J[a, b, d] = d kernel(Xs, X)[a, b] / d Xs[a, d]                          by torch autograd,
    kappa[a, d] = d^2 kernel(x, x') / dx_d dx'_d at x = x' = Xs[a]           by autograd in both arguments where the kernel is smooth through
                  tau = 0 in torch (`smooth`), else by an extrapolated second central difference of the reference kernel (Neville's
                  tableau over h = 0.1 / 2^i; a kernel through |tau| has odd powers of h in its error, so every power is eliminated),
    dmu_d = J_d alpha (+ the slope of a LinearMean),   dvar_d = kappa_d - colsum((L^-1 J_d^T)^2).
Asserted here, not by the device: both routes to kappa agree to 1e-7 where both apply; dmu is the central difference of the reference's own
predict_f mean to 1e-6 relative; cond(Kj) < 1e5; dvar_d >= 1e-3 kappa_d at every stored point; the coincident test point of `m32cos` has
J = 0 at its training point.  Stored: dmu, dvar, kappa (S, D), the first KROWS rows of J, the raw parameters, cond(Kj).
Re-run:  python tests/golden/gen_deriv.py [path to the reference]
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
import deriv_cases            # noqa: E402

G = mogptk.gpr
torch.set_default_dtype(torch.float64)
N_ = lambda t: t.detach().cpu().numpy().astype(np.float64)


def split(Xs, multi):
    """(channel columns without a gradient, input columns with one, the two joined as the kernel takes them)"""
    t = torch.tensor(Xs, dtype=torch.float64)
    x = t[:, 1:].clone().requires_grad_(True) if multi else t.clone().requires_grad_(True)
    return x, (torch.cat([t[:, :1], x], dim=1) if multi else x)


def jacobian(kernel, Xs, X, multi):
    x, full = split(Xs, multi)
    K = kernel.K(full, X)
    J = np.empty((Xs.shape[0], X.shape[0], x.shape[1]))
    for b in range(X.shape[0]):                              # row a of K depends on Xs[a] alone
        J[:, b, :] = N_(torch.autograd.grad(K[:, b].sum(), x, retain_graph=True)[0])
    return J


def kappa_autograd(kernel, Xs, multi):
    xa, fa = split(Xs, multi)
    xb, fb = split(Xs, multi)
    g = torch.autograd.grad(kernel.K(fa, fb).diagonal().sum(), xa, create_graph=True)[0]
    out = np.empty(tuple(xa.shape))
    for d in range(xa.shape[1]):
        out[:, d] = N_(torch.autograd.grad(g[:, d].sum(), xb, retain_graph=True)[0])[:, d]
    return out


def kappa_difference(kernel, Xs, multi, levels=7):
    off = 1 if multi else 0
    S, D = Xs.shape[0], Xs.shape[1] - off
    kd = lambda A, B: N_(kernel.K(torch.tensor(A), torch.tensor(B)).diagonal())
    out = np.empty((S, D))
    for d in range(D):
        T = []
        for i in range(levels):
            h = 0.1 / 2 ** i                                # down to 1.6e-3: the rounding of a kernel value, 1e-16 / 4 h^2, stays near 1e-11
            P, M = Xs.copy(), Xs.copy()
            P[:, off + d] += h
            M[:, off + d] -= h
            with torch.no_grad():
                T.append([(kd(P, P) - kd(P, M) - kd(M, P) + kd(M, M)) / (4.0 * h * h)])
            for j in range(1, i + 1):                       # Neville: the value at h = 0 of the polynomial through h_{i-j} .. h_i
                T[i].append(T[i][j - 1] + (T[i][j - 1] - T[i - 1][j - 1]) / (2.0 ** j - 1.0))
        diag = np.stack([T[i][i] for i in range(levels)])
        best = np.argmin(np.abs(np.diff(diag, axis=0)), axis=0) + 1      # per point: where two successive extrapolations agree best
        out[:, d] = diag[best, np.arange(S)]
    return out


def main():
    out = {}
    for case, c in deriv_cases.CASES.items():
        pre = case + "__"
        m = deriv_cases.exact(G, case)
        _, _, Xs = deriv_cases.data(case)
        multi = "n" in c
        ps = list(m.parameters())
        out[pre + "names"] = np.array([p._name for p in ps])
        for i, p in enumerate(ps):
            out["%sp%d_raw" % (pre, i)] = N_(p.data)
        with torch.no_grad():
            Kff = m.kernel.K(m.X) + m._index_channel(m.likelihood.scale().square(), m.X) * m.eye
            Kj = Kff + (m.jitter * Kff.diagonal().mean()).repeat(Kff.shape[0]).diagflat()
            r = m.y if m.mean is None else m.y - m.mean(m.X).reshape(-1, 1)
            L = torch.linalg.cholesky(Kj)
            alpha = N_(torch.cholesky_solve(r, L)).reshape(-1)
            cond = float(np.linalg.cond(N_(Kj)))
            assert cond < 1e5, (case, cond)
        J = jacobian(m.kernel, Xs, m.X, multi)
        assert np.all(np.isfinite(J)), case
        if c.get("coincide"):
            assert np.all(J[3, 13] == 0.0), (case, J[3, 13])
        kap = kappa_difference(m.kernel, Xs, multi)
        how = "difference"
        if c.get("smooth"):
            ka = kappa_autograd(m.kernel, Xs, multi)
            e = np.max(np.abs(ka - kap)) / max(1.0, np.max(np.abs(ka)))
            assert e <= 1e-7, (case, "the two routes to kappa disagree", e)
            kap, how = ka, "autograd (difference within %.1e)" % e
        S, D = kap.shape
        dmu, dvar = np.empty((S, D)), np.empty((S, D))
        for d in range(D):
            V = N_(torch.linalg.solve_triangular(L, torch.tensor(J[:, :, d].T.copy()), upper=False))
            dmu[:, d] = J[:, :, d] @ alpha
            dvar[:, d] = kap[:, d] - np.sum(V * V, axis=0)
        if m.mean is not None:
            dmu += deriv_cases.SLOPE
        assert np.all(dvar >= 1e-3 * kap), (case, float(np.min(dvar / kap)))
        # the central difference of the reference's own predictive mean (Richardson over h and h / 2)
        off = 1 if multi else 0
        fd = np.empty((S, D))
        with torch.no_grad():
            mean_at = lambda A: N_(m.predict_f(torch.tensor(A))[0]).reshape(-1)
            for d in range(D):
                est = []
                for h in (2e-4, 1e-4):
                    P, M = Xs.copy(), Xs.copy()
                    P[:, off + d] += h
                    M[:, off + d] -= h
                    est.append((mean_at(P) - mean_at(M)) / (2.0 * h))
                fd[:, d] = (4.0 * est[1] - est[0]) / 3.0
        e_fd = np.max(np.abs(fd - dmu)) / max(1.0, np.max(np.abs(dmu)))
        assert e_fd <= 1e-6, (case, "dmu is not the slope of predict_f's mean", e_fd)
        out[pre + "cond"] = np.array(cond)
        out[pre + "dmu"], out[pre + "dvar"], out[pre + "kappa"], out[pre + "J"] = dmu, dvar, kap, J[:deriv_cases.KROWS]
        print("%-8s N = %3d  S = %2d  D = %d  cond(Kj) = %.3g  min dvar / kappa = %.3g  dmu vs difference %.1e  kappa by %s"
              % (case, Kj.shape[0], S, D, cond, float(np.min(dvar / kap)), e_fd, how))

    path = os.path.join(HERE, "deriv.npz")
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) < 1000000
    print("wrote deriv.npz", os.path.getsize(path), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
