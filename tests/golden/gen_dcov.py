"""
Golden vectors of the JOINT posterior covariance of df/dx in tests/golden/dcov.npz.  Runs only where the reference
(GAMES-UChile/mogptk) is importable, like gen_deriv.py, whose helpers it uses; the fixture is data only.  Per case of tests/deriv_cases.py, with
its S = 24 test points:
    H[a, d, b, e] = d^2 kernel(Xs, Xs)[a, b] / d Xs[a, d] d Xs'[b, e]      by double autograd through the reference's own kernel objects, the two
                    arguments of the kernel being separate leaves.  For a != b it is asserted finite (no pair of test points coincides); for
                    a = b it is kept where the case is `smooth`, else (all such cases are D = 1) replaced by gen_deriv.py's extrapolated difference,
    dcov = H - V^T V,   V = L^-1 [J_d(x*_a)]^T over the stacked rows (a, d),   L formed as the reference's predict_f forms it.
Asserted here, not by the device: both routes to the diagonal of H agree to 1e-7 where both apply; diag(dcov) is the dvar stored in deriv.npz to
1e-9 relative; dcov is symmetric (1e-12 of its largest entry) and lambda_min(dcov) >= -1e-10 max diag -- the last wherever the reference's kernel over
[X; Xs] is itself positive semi-definite to that figure, which `mohsm`'s is not (see main).  Stored: dcov (S, D, S, D) per case; the
raw parameters, dmu and dvar of the same models are deriv.npz's.
Re-run:  python tests/golden/gen_dcov.py [path to the reference]
"""
import os
import numpy as np

import gen_deriv as gd        # (sets the import path to the reference and the tests, float64 as torch's default)
import torch                  # noqa: E402
import deriv_cases            # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
N_ = gd.N_


def hessian(kernel, Xs, multi):
    """H (S, D, S, D) by double autograd: the first derivative of column b with the graph kept, then one backward pass per (a, d)"""
    xa, fa = gd.split(Xs, multi)
    xb, fb = gd.split(Xs, multi)
    K = kernel.K(fa, fb)
    S, D = xa.shape
    H = np.empty((S, D, S, D))
    for b in range(S):
        g = torch.autograd.grad(K[:, b].sum(), xa, create_graph=True)[0]      # g[a, d] = d K[a, b] / d xa[a, d]: row a of K depends on xa[a] alone
        for a in range(S):
            for d in range(D):
                H[a, d, b, :] = N_(torch.autograd.grad(g[a, d], xb, retain_graph=True)[0])[b]
    return H


def main():
    FX = np.load(os.path.join(HERE, "deriv.npz"))
    out = {}
    for case, c in deriv_cases.CASES.items():
        pre = case + "__"
        m = deriv_cases.exact(gd.G, case)
        _, _, Xs = deriv_cases.data(case)
        multi = "n" in c
        for i, p in enumerate(m.parameters()):                 # the same bits as deriv.npz's models
            assert np.array_equal(N_(p.data), FX["%sp%d_raw" % (pre, i)]), (case, i)
        with torch.no_grad():
            Kff = m.kernel.K(m.X) + m._index_channel(m.likelihood.scale().square(), m.X) * m.eye
            Kj = Kff + (m.jitter * Kff.diagonal().mean()).repeat(Kff.shape[0]).diagflat()
            L = torch.linalg.cholesky(Kj)
        J = gd.jacobian(m.kernel, Xs, m.X, multi)               # (S, N, D)
        S, _, D = J.shape
        H = hessian(m.kernel, Xs, multi)
        off = ~np.eye(S, dtype=bool)
        assert np.all(np.isfinite(H.transpose(0, 2, 1, 3)[off])), (case, "a pair of test points coincides")
        idx = np.arange(S)
        kap = gd.kappa_difference(m.kernel, Xs, multi)          # (S, D): the d = e entries at a = b
        how = "difference"
        if c.get("smooth"):
            ka = np.stack([H[idx, d, idx, d] for d in range(D)], axis=1)
            e = np.max(np.abs(ka - kap)) / max(1.0, np.max(np.abs(ka)))
            assert e <= 1e-7, (case, "the two routes to the diagonal of H disagree", e)
            how = "autograd (difference within %.1e)" % e
        else:
            assert D == 1, case
            H[idx, 0, idx, 0] = kap[:, 0]
        assert np.all(np.isfinite(H)), case
        rows = J.transpose(0, 2, 1).reshape(S * D, -1)          # row a * D + d
        V = N_(torch.linalg.solve_triangular(L, torch.tensor(rows.T.copy()), upper=False))
        dcov = H.reshape(S * D, S * D) - V.T @ V
        diag = np.diagonal(dcov).reshape(S, D)
        e_diag = np.max(np.abs(diag - FX[pre + "dvar"]) / np.abs(FX[pre + "dvar"]))
        assert e_diag <= 1e-9, (case, "diag(dcov) is not deriv.npz's dvar", e_diag)
        e_sym = np.max(np.abs(dcov - dcov.T)) / np.max(np.abs(dcov))
        assert e_sym <= 1e-12, (case, "dcov is not symmetric", e_sym)
        lam = np.linalg.eigvalsh(0.5 * (dcov + dcov.T))[0]
        with torch.no_grad():                                   # the reference's kernel over training and test points together
            Z = np.concatenate([N_(m.X), Xs])
            KZ = N_(m.kernel.K(torch.tensor(Z)))
        lam_k = np.linalg.eigvalsh(0.5 * (KZ + KZ.T))[0] / np.max(np.diagonal(KZ))
        # a posterior covariance is positive semi-definite when the prior is.  The reference's harmonizable kernel with two channels of different
        # lengthscales is not (`mohsm`: lambda_min(K) = -4e-2 max diag over these very points), and then no correct dcov can be either: the bound is
        # asserted wherever the kernel itself meets it, and the case's figure is printed
        if lam_k >= -1e-10:
            assert lam >= -1e-10 * np.max(diag), (case, lam)
        else:
            assert case == "mohsm", (case, lam_k)
        out[pre + "dcov"] = dcov.reshape(S, D, S, D)
        print("%-8s S = %2d  D = %d  diag vs dvar %.1e  asymmetry %.1e  lambda_min / max diag %.2e (the kernel's own: %.2e)  diagonal of H by %s"
              % (case, S, D, e_diag, e_sym, lam / np.max(diag), lam_k, how))

    path = os.path.join(HERE, "dcov.npz")
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) < 1000000
    print("wrote dcov.npz", os.path.getsize(path), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
