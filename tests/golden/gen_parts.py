"""
Golden vectors of the posterior by kernel part in tests/golden/parts.npz.  Runs only where the reference (GAMES-UChile/mogptk) is
importable, like gen_loo.py and gen_family.py; the fixture is data only.  The reference has no such call: what it contributes is the model --
kernel, noise, mean, data variance, relative jitter -- and its own kernel objects, ONE PER PART.  Per case of tests/parts_cases.py: the
reference's Exact model, Kj and L formed as its predict_f forms them (gpr/model.py:455-472, :244), and for every part p of the default
partition the part's own reference kernel (parts_cases.part_kernels: the sub-kernel, or a kernel of the same class holding the part's slice of
the parameters), evaluated in float64:
    K_p(Xs, X),  K_p(Xs, Xs),   mu_p = K_p(Xs, X) Kj^-1 r,   cov_p = K_p(Xs, Xs) - V^T V,  V = L^-1 K_p(X, Xs),   var_p = diag cov_p.
Stored: mu (P, S), var (P, S), the first KROWS rows of K_p(Xs, X) (the whole of it would not fit the size limit of a committed file), cov_p for
the cases marked `full`, the raw parameters, cond(Kj) -- asserted below 1e5, the families' bound.  Asserted here: the parts' cross-Grams sum to
the whole kernel's (1e-12), and sum_p mu_p + mean(Xs) is the reference's own predict_f mean (1e-9).  For `big` only mu and var are stored.
Re-run:  python tests/golden/gen_parts.py [path to the reference]
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
import parts_cases            # noqa: E402

G = mogptk.gpr
torch.set_default_dtype(torch.float64)
N_ = lambda t: t.detach().cpu().numpy().astype(np.float64)


def main():
    out = {}
    for case, c in parts_cases.CASES.items():
        pre = case + "__"
        m = parts_cases.exact(G, case)
        _, _, Xs = parts_cases.data(case)
        Xs_t = torch.tensor(Xs, dtype=torch.float64)
        ps = list(m.parameters())
        out[pre + "names"] = np.array([p._name for p in ps])
        for i, p in enumerate(ps):
            out["%sp%d_raw" % (pre, i)] = N_(p.data)
        with torch.no_grad():
            Kff = m.kernel.K(m.X) + m._index_channel(m.likelihood.scale().square(), m.X) * m.eye
            if m.data_variance is not None:
                Kff = Kff + m.data_variance
            Kj = Kff + (m.jitter * Kff.diagonal().mean()).repeat(Kff.shape[0]).diagflat()
            r = m.y if m.mean is None else m.y - m.mean(m.X).reshape(-1, 1)
            L = torch.linalg.cholesky(Kj)
            alpha = torch.cholesky_solve(r, L)
            cond = float(np.linalg.cond(N_(Kj)))
            assert cond < 1e5, (case, cond)
            parts = parts_cases.part_kernels(G, m.kernel)
            mus, vars_, covs, Ksx = [], [], [], []
            for pk in parts:
                Ks = pk.K(Xs_t, m.X)
                Kss = pk.K(Xs_t)
                V = torch.linalg.solve_triangular(L, Ks.T, upper=False)
                cov = Kss - V.T @ V
                mus.append(N_(Ks @ alpha).reshape(-1))
                vars_.append(N_(cov.diagonal()))
                covs.append(N_(cov))
                Ksx.append(N_(Ks))
            whole = N_(m.kernel.K(Xs_t, m.X))
            err = np.max(np.abs(sum(Ksx) - whole)) / max(1.0, np.max(np.abs(whole)))
            assert err <= 1e-12, (case, "the parts do not sum to the kernel", err)
            mu_ref, _ = m.predict_f(Xs_t)
            total = sum(mus) + (0.0 if m.mean is None else N_(m.mean(Xs_t)).reshape(-1))
            err_mu = np.max(np.abs(total - N_(mu_ref).reshape(-1))) / max(1.0, np.max(np.abs(N_(mu_ref))))
            assert err_mu <= 1e-9, (case, "the parts' means do not sum to predict_f's", err_mu)
        out[pre + "cond"] = np.array(cond)
        out[pre + "mu"], out[pre + "var"] = np.stack(mus), np.stack(vars_)
        if not c.get("light"):
            out[pre + "Ksx"] = np.stack(Ksx)[:, :parts_cases.KROWS]
        if c.get("full"):
            out[pre + "cov"] = np.stack(covs)
        print("%-8s N = %4d  S = %3d  P = %d  cond(Kj) = %.3g  parts sum %.1e  means sum %.1e" % (case, Kj.shape[0], Xs.shape[0], len(parts), cond, err, err_mu))

    path = os.path.join(HERE, "parts.npz")
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) < 1000000
    print("wrote parts.npz", os.path.getsize(path), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
