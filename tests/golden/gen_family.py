"""
Golden vectors of a kernel family -- stationary, product or trend (tests/family_cases.py) -- in tests/golden/<family>.npz,
<family>_gram_[ab].npz and <family>_checkpoints.npz.  Runs only where the reference (GAMES-UChile/mogptk) is importable, like gen_mean.py; the
fixtures are data only.  The models come from tests/<family>_cases.py, built with the reference's `mogptk.gpr`.  Per case: inputs, targets,
parameter names and constrained / raw values, K(X) (its packed lower triangle, in two files of their own: a committed file stays under
1 MiB), K(X, Xs), K_diag, LML, loss, the autograd gradient of every raw parameter, predict_f (diagonal and full), predict_y, and
cond(K + s2 I) -- asserted below 1e5.  One case also records the loss trace of 20 Adam steps through Model.train.  Everything float64.
Re-run:  python tests/golden/gen_family.py <family> [path to the reference]
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
FAMILY = sys.argv[1]
sys.path.insert(0, sys.argv[2] if len(sys.argv) > 2 else os.environ.get("MOGPTK_REFERENCE", "reference"))
import torch                  # noqa: E402
import mogptk                 # noqa: E402
import family_cases           # noqa: E402

sc = family_cases.cases(FAMILY)
G = mogptk.gpr
torch.set_default_dtype(torch.float64)
N_ = lambda t: t.detach().cpu().numpy().astype(np.float64)
T_ = lambda a: torch.tensor(np.asarray(a, dtype=np.float64))


def main():
    out, grams = {}, [{}, {}]
    for n, case in enumerate(sc.CASES):
        pre = case + "__"
        light = sc.CASES[case].get("light", False)
        m = family_cases.exact(FAMILY, G, case)
        X, y, Xs = sc.data(case)
        ps = list(m.parameters())
        out[pre + "names"] = np.array([p._name for p in ps])
        out[pre + "lml"] = np.array(float(m.log_marginal_likelihood().detach()))
        out[pre + "loss"] = np.array(float(m.loss()))
        for i, p in enumerate(ps):
            out["%sp%d_raw" % (pre, i)] = N_(p.data)
            out["%sp%d_cons" % (pre, i)] = N_(p.constrained)
            out["%sp%d_grad" % (pre, i)] = N_(p.grad)
        K = N_(m.kernel(T_(X)))
        s2 = sc.NOISE
        cond = float(np.linalg.cond(K + s2 * np.eye(K.shape[0])))
        assert cond < 1e5, (case, cond)
        assert all(np.all(np.isfinite(N_(p.grad))) for p in ps), case
        out[pre + "cond"] = np.array(cond)
        print("%-12s N = %4d  cond(K + s2 I) = %.3g  lml = %.6f" % (case, K.shape[0], cond, float(out[pre + "lml"])))
        if light:
            continue
        out[pre + "X"], out[pre + "y"], out[pre + "Xs"] = X, y, Xs
        assert np.array_equal(K, K.T)
        grams[n % 2][pre + "K_tril"] = K[np.tril_indices(K.shape[0])]
        out[pre + "K12"] = N_(m.kernel(T_(X), T_(Xs)))
        out[pre + "Kdiag"] = N_(m.kernel.K_diag(T_(X)))
        mu, var = m.predict_f(Xs)
        out[pre + "mu"], out[pre + "var"] = N_(mu), N_(var)
        _, cov = m.predict_f(Xs, full=True)
        out[pre + "cov"] = N_(cov)
        res = m.predict_y(Xs)
        out[pre + "ymu"], out[pre + "yvar"] = N_(res[0]), N_(res[1])
    # Model.train('Adam') on a case-1 model: the losses it records
    X, y, _ = sc.data(sc.ADAM_CASE)
    mm = mogptk.Model(mogptk.DataSet(mogptk.Data(X[:, 0], y, name="a")), G.IndependentMultiOutputKernel(sc.kernel(G, sc.ADAM_CASE), output_dims=1),
                      inference=mogptk.Exact(variance=sc.NOISE))
    losses, _ = mm.train(method="Adam", iters=sc.ADAM_ITERS, lr=sc.ADAM_LR, verbose=False)
    out["adam__losses"] = np.array(losses, dtype=np.float64)
    out["adam__final"] = np.concatenate([N_(p.data).reshape(-1) for p in mm.gpr.parameters()])
    np.savez_compressed(os.path.join(HERE, FAMILY + ".npz"), **out)
    for tag, g in zip("ab", grams):
        np.savez_compressed(os.path.join(HERE, "%s_gram_%s.npz" % (FAMILY, tag)), **g)
    for f in (FAMILY + ".npz", FAMILY + "_gram_a.npz", FAMILY + "_gram_b.npz"):
        size = os.path.getsize(os.path.join(HERE, f))
        assert size < 1 << 20, (f, size)
        print("wrote", f, size, "bytes")
    gen_checkpoints()


def gen_checkpoints():
    """Files written by the reference's Model.save() with the family's kernels inside the compositions of `checkpoint_kernels`, stored as
    bytes next to what the reference computes on the loaded object (constrained values, loss, gradients, predictions)."""
    import tempfile
    rng = np.random.default_rng(91)
    out = {}

    def dataset(C, n):
        ds = mogptk.DataSet()
        for c in range(C):
            x = np.sort(rng.uniform(0, 10, n))
            d = mogptk.Data(x, np.sin(x * (1 + 0.5 * c)) + 0.1 * rng.standard_normal(n), name="ch%d" % c)
            d.set_prediction_data(np.linspace(0, 11, 7))
            ds.append(d)
        return ds

    def shake(k):
        for m in k.modules():                               # (torch modules: every kernel of the composition, each parameter once)
            for name, p in m._parameters.items():
                lo, hi = sc.shake_range(G, m, name)
                p.assign(rng.uniform(lo, hi, tuple(p().shape)) if p().ndim else rng.uniform(lo, hi))
        return k

    def record(tag, model):
        with tempfile.TemporaryDirectory() as d:
            model.save(os.path.join(d, "m"))
            raw = open(os.path.join(d, "m.npy"), "rb").read()
            loaded = mogptk.LoadModel(os.path.join(d, "m"))
        out[tag + "_file"] = np.frombuffer(raw, dtype=np.uint8)
        ps = list(loaded.gpr.parameters())
        out[tag + "_names"] = np.array([p._name for p in ps])
        for i, p in enumerate(ps):
            out["%s_p%d" % (tag, i)] = N_(p.constrained)
        out[tag + "_loss"] = np.array(float(loaded.loss()))
        for i, p in enumerate(ps):
            out["%s_g%d" % (tag, i)] = np.zeros(0) if p.grad is None else N_(p.grad)
        _, mu, _, _ = loaded.predict(transformed=False)
        out[tag + "_mu"] = np.concatenate([np.asarray(m).reshape(-1) for m in mu])

    for tag, C, n, k in sc.checkpoint_kernels(G):           # data first, then the parameters: the order of the draws
        ds = dataset(C, n)
        k = shake(k)
        record(tag, mogptk.Model(ds, G.IndependentMultiOutputKernel(k, output_dims=1) if C == 1 else k, inference=mogptk.Exact()))
    np.savez_compressed(os.path.join(HERE, FAMILY + "_checkpoints.npz"), **out)
    print("wrote %s_checkpoints.npz" % FAMILY, len(out), "arrays")


if __name__ == "__main__":
    main()
