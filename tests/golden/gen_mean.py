"""
Golden vectors of the trainable mean functions (tests/golden/mean.npz).  Runs only where the reference (GAMES-UChile/mogptk) is
importable, like gen_golden.py; the fixture is data only.  The models come from tests/mean_cases.py, built with the reference's
`mogptk.gpr`.  Per case: parameter names, raw values, LML, loss and the autograd gradient of every parameter (and of the sub-means of a
MultiOutputMean, quirk Q8), predict_f (diagonal and full) and predict_y; the same for Titsias / Snelson with a mean; an Adam trace in
tutorial 06's phases (mean only, kernel only, both), by hand and
through Model.train('Adam').  mean_checkpoints.npz: files the reference's Model.save() wrote with each built-in mean, and what it computes
after loading them.  Re-run:  python tests/golden/gen_mean.py [path to the reference]
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
import torch          # noqa: E402
import mogptk         # noqa: E402
import mean_cases     # noqa: E402

G = mogptk.gpr
torch.set_default_dtype(torch.float64)
N_ = lambda t: t.detach().cpu().numpy().astype(np.float64)


def params(out, pre, m):
    ps = list(m.parameters())
    out[pre + "names"] = np.array([p._name for p in ps])
    for i, p in enumerate(ps):
        out["%sp%d_raw" % (pre, i)] = N_(p.data)
        out["%sp%d_grad" % (pre, i)] = N_(p.grad) if p.grad is not None else np.array(np.nan)
    for j, s in enumerate(mean_cases.sub_means(m)):
        for i, p in enumerate(s.parameters()):
            out["%ssub%d_p%d_name" % (pre, j, i)] = np.array(p._name)
            out["%ssub%d_p%d_grad" % (pre, j, i)] = N_(p.grad)


def main():
    out = {}
    for case in mean_cases.CASES:
        pre = case + "__"
        m = mean_cases.exact(G, case)
        out[pre + "lml"] = float(m.log_marginal_likelihood().detach())
        out[pre + "loss"] = float(m.loss())
        params(out, pre, m)
        _, _, Xs = mean_cases.data(case)
        mu, var = m.predict_f(Xs)
        out[pre + "mu"], out[pre + "var"] = N_(mu), N_(var)
        _, cov = m.predict_f(Xs, full=True)
        out[pre + "cov"] = N_(cov)
        res = m.predict_y(Xs)
        out[pre + "ymu"], out[pre + "yvar"] = N_(res[0]), N_(res[1])
    for name in mean_cases.SPARSE_CASES:
        pre = name + "__"
        m = mean_cases.sparse(G, name)
        out[pre + "lml"] = float(m.log_marginal_likelihood().detach())
        out[pre + "loss"] = float(m.loss())
        params(out, pre, m)
        _, _, Xs = mean_cases.data(mean_cases.SPARSE_CASES[name][1])
        mu, var = m.predict_f(Xs)
        out[pre + "mu"], out[pre + "var"] = N_(mu), N_(var)
    # tutorial 06's phases with an SM kernel (IMO) in place of its periodic kernel: mean only, kernel only, both; Adam, lr 0.05, 8 steps each
    # (each phase is a train() call of its own: a fresh Adam over the parameters whose train flag is on, as mogptk's Model.train builds it)
    m = mean_cases.exact(G, "poly_mosm2")
    trace = []
    for phase in ((True, False), (False, True), (True, True)):
        m.mean.train, m.kernel.train = phase
        opt = torch.optim.Adam([p for p in m.parameters() if p.train], lr=0.05)
        for _ in range(8):
            opt.zero_grad()
            loss = m.loss()
            opt.step()
            trace.append(float(loss))
    out["adam__trace"] = np.array(trace)
    out["adam__final"] = np.concatenate([N_(p.data).reshape(-1) for p in m.parameters()])
    # the same three phases through Model.train('Adam') of a mogptk Model (one train() call per phase): the losses it records
    X, y, _ = mean_cases.data("poly_mosm2")
    ds = mogptk.DataSet(*[mogptk.Data(X[X[:, 0] == c, 1], y[X[:, 0] == c], name="ch%d" % c) for c in range(2)])
    mm = mogptk.Model(ds, mean_cases.kernel(G, "poly_mosm2"), inference=mogptk.Exact(variance=0.1), mean=mean_cases.mean(G, "poly_mosm2"))
    for k, phase in enumerate(((True, False), (False, True), (True, True))):
        mm.gpr.mean.train, mm.gpr.kernel.train = phase
        losses, _ = mm.train(method="Adam", iters=8, lr=0.05, verbose=False)
        out["train__losses%d" % k] = np.array(losses, dtype=np.float64)
    out["train__final"] = np.concatenate([N_(p.data).reshape(-1) for p in mm.gpr.parameters()])
    np.savez_compressed(os.path.join(HERE, "mean.npz"), **out)
    print("wrote", os.path.join(HERE, "mean.npz"), len(out), "arrays")
    gen_checkpoints()


def gen_checkpoints():
    """Files written by the reference's Model.save() with each built-in mean (a trained ConstantMean, a LinearMean on the channel column with a
    bounded bias and a fixed slope, a MultiOutputMean under Exact and under Titsias), stored as bytes next to what the reference computes on
    the loaded object: constrained values, train flags, loss, gradients, the sub-means' values and gradients (Q8), predictions."""
    import tempfile
    rng = np.random.default_rng(78)
    out = {}

    def dataset(C, n):
        ds = mogptk.DataSet()
        for c in range(C):
            x = np.sort(rng.uniform(0, 10, n))
            d = mogptk.Data(x, np.sin(x * (1 + 0.5 * c)) + 0.5 + 0.1 * x + 0.1 * rng.standard_normal(n), name="ch%d" % c)
            d.set_prediction_data(np.linspace(0, 11, 7))
            ds.append(d)
        return ds

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
            out["%s_train%d" % (tag, i)] = np.array(bool(p.train))
        out[tag + "_loss"] = np.array(float(loaded.loss()))
        for i, p in enumerate(ps):
            out["%s_g%d" % (tag, i)] = np.zeros(0) if p.grad is None else N_(p.grad)
        for j, sm in enumerate(getattr(loaded.gpr.mean, "means", [])):
            for i, p in enumerate(sm.parameters()):
                out["%s_sub%d_p%d" % (tag, j, i)] = N_(p.constrained)
                out["%s_sub%d_g%d" % (tag, j, i)] = N_(p.grad)
        _, mu, _, _ = loaded.predict(transformed=False)
        out[tag + "_mu"] = np.concatenate([np.asarray(m).reshape(-1) for m in mu])

    m = mogptk.MOSM(dataset(2, 30), Q=1, mean=G.ConstantMean())
    m.gpr.mean.bias.assign(0.4)
    m.train(method="Adam", lr=0.01, iters=3, verbose=False)
    record("const", m)
    mean = G.LinearMean(2)
    mean.bias.assign(0.2, lower=-1.0, upper=1.0)
    mean.slope.assign([0.1, 0.05], train=False)
    m = mogptk.MOSM(dataset(2, 30), Q=1, mean=mean)
    record("linear", m)
    a, b = G.ConstantMean(), G.LinearMean(1)
    a.bias.assign(0.3); b.bias.assign(-0.2); b.slope.assign([0.07])
    record("mom", mogptk.MOSM(dataset(2, 30), Q=1, mean=G.MultiOutputMean(a, b)))
    a, b = G.ConstantMean(), G.LinearMean(1)
    a.bias.assign(0.1); b.bias.assign(0.2); b.slope.assign([-0.03])
    record("mom_titsias", mogptk.MOSM(dataset(2, 40), Q=1, inference=mogptk.Titsias(inducing_points=6), mean=G.MultiOutputMean(a, b)))
    np.savez_compressed(os.path.join(HERE, "mean_checkpoints.npz"), **out)
    print("wrote", os.path.join(HERE, "mean_checkpoints.npz"), len(out), "arrays")


if __name__ == "__main__":
    main()
