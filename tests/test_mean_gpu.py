"""
Trainable mean functions on the device (csrc/mean.hip): the residual y - m(X) and the mean's gradient of the exact, Titsias and Snelson
models against the reference's autograd (tests/golden/mean.npz, written by tests/golden/gen_mean.py from the models of
tests/mean_cases.py), every gradient schedule, a short Adam trace in the phases of the reference's tutorial 06, bitwise neutrality of a
zero mean, and the device reduction at configs[1]'s size against numpy.
"""
import numpy as np
import pytest

from mogptk_amd import gpr, synth
import mean_cases
from helpers import load

pytestmark = pytest.mark.gpu


def close(a, b, tol):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.max(np.abs(a - b)) <= tol * max(1.0, np.max(np.abs(b)))


def with_reference_raw(m, fx, pre):
    """the reference's raw parameter values (same registration order: test_mean_cpu checks the names)"""
    ps = list(m.parameters())
    assert [p._name for p in ps] == [str(n) for n in fx[pre + "names"]]
    for i, p in enumerate(ps):
        p.data = np.array(fx["%sp%d_raw" % (pre, i)], dtype=p.data.dtype).reshape(p.data.shape)
    return ps


def check_value_and_gradients(m, fx, pre, lml_tol=1e-9, grad_tol=1e-7):
    ps = with_reference_raw(m, fx, pre)
    lml = float(m.log_marginal_likelihood())
    assert abs(lml - float(fx[pre + "lml"])) <= lml_tol * abs(float(fx[pre + "lml"])), (lml, float(fx[pre + "lml"]))
    loss = float(m.loss())
    assert abs(loss - float(fx[pre + "loss"])) <= lml_tol * abs(float(fx[pre + "loss"]))
    for i, p in enumerate(ps):
        g = fx["%sp%d_grad" % (pre, i)]
        assert close(p.grad, g, grad_tol), (pre, p._name, p.grad, g)
    for j, s in enumerate(mean_cases.sub_means(m)):             # Q8: the sub-means are not parameters, but their .grad is filled
        for i, p in enumerate(s.parameters()):
            assert p._name == str(fx["%ssub%d_p%d_name" % (pre, j, i)])
            assert close(p.grad, fx["%ssub%d_p%d_grad" % (pre, j, i)], grad_tol), (pre, j, p._name)
    return ps


@pytest.mark.parametrize("case", list(mean_cases.CASES))
def test_exact_lml_loss_and_every_gradient_match_reference_autograd(case):
    fx = load("mean.npz")
    m = mean_cases.exact(gpr, case)
    check_value_and_gradients(m, fx, case + "__")


@pytest.mark.parametrize("case", list(mean_cases.CASES))
def test_exact_prediction_with_a_mean_matches_reference(case):
    fx = load("mean.npz")
    pre = case + "__"
    m = mean_cases.exact(gpr, case)
    with_reference_raw(m, fx, pre)
    _, _, Xs = mean_cases.data(case)
    mu, var = m.predict_f(Xs)
    assert close(mu, fx[pre + "mu"], 1e-9) and close(var, fx[pre + "var"], 1e-9)
    mu2, cov = m.predict_f(Xs, full=True)
    assert close(mu2, fx[pre + "mu"], 1e-9) and close(cov, fx[pre + "cov"], 1e-9)
    ym, yv = m.predict_y(Xs)[:2]
    assert close(ym, fx[pre + "ymu"], 1e-9) and close(yv, fx[pre + "yvar"], 1e-9)


@pytest.mark.parametrize("name", list(mean_cases.SPARSE_CASES))
def test_sparse_bound_gradients_and_prediction_with_a_mean(name):
    """Titsias (w = -s2^-1 (r - s2^-1 v^T t1)) and Snelson (w = -(Qff + Lambda)^-1 r): bound, kernel / noise / Z / mean gradients,
    predict_f, at the tolerances of the existing sparse tests"""
    fx = load("mean.npz")
    pre = name + "__"
    m = mean_cases.sparse(gpr, name)
    check_value_and_gradients(m, fx, pre, lml_tol=1e-9, grad_tol=1e-6)
    _, _, Xs = mean_cases.data(mean_cases.SPARSE_CASES[name][1])
    mu, var = m.predict_f(Xs)
    assert close(mu, fx[pre + "mu"], 1e-8) and close(var, fx[pre + "var"], 1e-8)


def test_adam_trace_in_tutorial_phases():
    """mean only, kernel only, both (the reference's tutorial 06 switches mean.train / kernel.train between train() calls); per phase a
    fresh torch.optim.Adam (lr 0.05) over the parameters whose train flag is on"""
    fx = load("mean.npz")
    m = mean_cases.exact(gpr, "poly_mosm2")
    ps = list(m.parameters())
    trace = []
    lr, b1, b2, eps = 0.05, 0.9, 0.999, 1e-8
    for phase in ((True, False), (False, True), (True, True)):
        m.mean.train, m.kernel.train = phase
        state = {id(p): [0, np.zeros_like(p.data), np.zeros_like(p.data)] for p in ps}      # a fresh optimiser per phase (one train() call each)
        for _ in range(8):
            trace.append(float(m.loss()))
            for p in ps:
                if not p.train or p.grad is None:
                    continue
                s = state[id(p)]
                s[0] += 1
                s[1] = b1 * s[1] + (1 - b1) * p.grad
                s[2] = b2 * s[2] + (1 - b2) * p.grad * p.grad
                mh = s[1] / (1 - b1 ** s[0])
                p.data = p.data - lr * mh / (np.sqrt(s[2] / (1 - b2 ** s[0])) + eps)
    assert close(trace, fx["adam__trace"], 1e-7), (np.array(trace), fx["adam__trace"])
    assert close(np.concatenate([p.data.reshape(-1) for p in ps]), fx["adam__final"], 1e-7)


def test_model_train_adam_in_tutorial_phases():
    """the same three phases through the package's own Model.train('Adam') (its flat Adam state over gpr.parameters(), one train() call per
    phase) against the losses the reference's Model.train recorded"""
    import mogptk_amd
    fx = load("mean.npz")
    X, y, _ = mean_cases.data("poly_mosm2")
    ds = mogptk_amd.DataSet(*[mogptk_amd.Data(X[X[:, 0] == c, 1], y[X[:, 0] == c], name="ch%d" % c) for c in range(2)])
    m = mogptk_amd.Model(ds, mean_cases.kernel(gpr, "poly_mosm2"), inference=mogptk_amd.Exact(variance=0.1), mean=mean_cases.mean(gpr, "poly_mosm2"))
    for k, phase in enumerate(((True, False), (False, True), (True, True))):
        m.gpr.mean.train, m.gpr.kernel.train = phase
        losses, _ = m.train(method="Adam", iters=8, lr=0.05, verbose=False)
        assert close(losses, fx["train__losses%d" % k], 1e-7), (k, np.asarray(losses), fx["train__losses%d" % k])
    assert close(np.concatenate([p.data.reshape(-1) for p in m.gpr.parameters()]), fx["train__final"], 1e-7)


@pytest.mark.parametrize("tag", ["const", "linear", "mom", "mom_titsias"])
def test_reference_checkpoint_with_a_mean_on_device(tag, tmp_path):
    """a file the reference wrote with a built-in mean, loaded without it: loss, every gradient, the sub-means' gradients (Q8), predictions"""
    import mogptk_amd
    fx = load("mean_checkpoints.npz")
    (tmp_path / "ref.npy").write_bytes(fx[tag + "_file"].tobytes())
    m = mogptk_amd.LoadModel(str(tmp_path / "ref"))
    loss = float(m.loss())
    assert abs(loss - float(fx[tag + "_loss"])) <= 1e-8 * max(1.0, abs(float(fx[tag + "_loss"])))
    tol = 1e-6 if tag == "mom_titsias" else 1e-7
    for i, p in enumerate(m.gpr.parameters()):
        assert close(p.grad, fx["%s_g%d" % (tag, i)], tol), (tag, p._name)
    for j, s in enumerate(mean_cases.sub_means(m.gpr)):
        for i, p in enumerate(s.parameters()):
            assert close(p.grad, fx["%s_sub%d_g%d" % (tag, j, i)], tol), (tag, j, p._name)
    _, mu, _, _ = m.predict(transformed=False)
    assert close(np.concatenate([np.asarray(v).reshape(-1) for v in mu]), fx[tag + "_mu"], 1e-7)


@pytest.mark.parametrize("path", ["phases", "fused"])
def test_mean_gradient_with_only_the_needed_tiles_of_the_inverse(path):
    """where the suite asserts two evaluations bit for bit equal -- only the tiles of Kj^-1 the gradient reads against every tile
    (MOGP_FULL_INVERSE=1), test_gpu_parity.py::test_gradient_with_only_the_needed_tiles_of_the_inverse -- the mean's gradient is the same bits too"""
    import os, subprocess, sys, tempfile, textwrap
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = textwrap.dedent('''
        import sys, numpy as np
        sys.path.insert(0, %r)
        from mogptk_amd import gpr, _lib
        N, C, Q = 3000, 2, 2
        rng = np.random.default_rng(5)
        sizes = [1400, 1600]
        X = np.concatenate([np.stack([np.full(s, float(c)), rng.uniform(0, 900, s)], axis=1) for c, s in enumerate(sizes)])
        X = X[np.argsort(X[:, 1])]
        y = rng.standard_normal(N)
        k = gpr.MultiOutputSpectralMixtureKernel(Q=Q, output_dims=C, input_dims=1)
        k.weight.assign(rng.uniform(0.5, 1.5, (C, Q))); k.mean.assign(rng.uniform(0.02, 0.4, (C, Q, 1)))
        k.variance.assign(rng.uniform(0.5, 1.5, (C, Q, 1))); k.delay.assign(rng.normal(0, 0.3, (C, Q, 1))); k.phase.assign(rng.normal(0, 0.3, (C, Q)))
        dev = _lib.ExactHandle(0, X, y, C)
        dev.set_terms(k._spectral_terms(1))
        dev.set_mean(np.array([[0.3, 0.001], [-0.2, 0.002]]))
        a = dev.eval(rng.uniform(0.05, 0.2, C), 1e-8, grad=True)
        g = dev.mean_grad()
        alpha = dev.fetch(2)
        want = np.array([[-alpha[X[:, 0] == c].sum(), -(alpha * X[:, 1])[X[:, 0] == c].sum()] for c in range(C)])
        assert np.allclose(g, want, rtol=1e-10, atol=1e-12), (g, want)
        if sys.argv[1] != "-":
            np.save(sys.argv[1], g)
            print("FULL", dev.inverse_fraction())
        else:
            f = np.load(sys.argv[2])
            assert dev.inverse_fraction() < 0.5
            assert np.array_equal(g, f), (g, f)
            print("MEAN_PLAN_OK", dev.inverse_fraction())
    ''') % root
    with tempfile.TemporaryDirectory() as tmp:
        full = os.path.join(tmp, "full.npy")
        r1 = subprocess.run([sys.executable, "-c", code, full], capture_output=True, text=True, timeout=600,
                            env=dict(os.environ, MOGP_GRAD_PATH=path, MOGP_FULL_INVERSE="1", MOGP_FLOW="0"))
        assert r1.returncode == 0, r1.stdout[-1500:] + r1.stderr[-3000:]
        r2 = subprocess.run([sys.executable, "-c", code, "-", full], capture_output=True, text=True, timeout=600,
                            env=dict({k_: v for k_, v in os.environ.items() if k_ != "MOGP_FULL_INVERSE"}, MOGP_GRAD_PATH=path))
        assert "MEAN_PLAN_OK" in r2.stdout, r2.stdout[-1500:] + r2.stderr[-3000:]


def test_fetch_dp_dr_ends_with_the_next_call():
    """mogp_model_fetch(which = 3) belongs to the gradient evaluation that formed it: a later evaluation or prediction clears it"""
    from mogptk_amd import _lib
    m = mean_cases.exact(gpr, "poly_mosm2")
    m.loss()
    h = m._handle
    w = h.fetch(3)
    assert np.array_equal(w, -h.fetch(2))
    m.log_marginal_likelihood()
    with pytest.raises(_lib.MogpError):
        h.fetch(3)
    m.loss()
    _, _, Xs = mean_cases.data("poly_mosm2")
    m.predict_f(Xs)
    with pytest.raises(_lib.MogpError):
        h.fetch(3)


def test_model_train_moves_the_mean():
    m = mean_cases.exact(gpr, "lin_mosm2_d1")
    b0 = m.mean.bias.data.copy()
    l0 = float(m.loss())
    opt = list(m.parameters())                          # what the optimisers of Model.train step: the mean's parameters are among them
    assert any(p is m.mean.bias for p in opt)
    for _ in range(5):
        m.loss()
        for p in opt:
            if p.train:
                p.data = p.data - 1e-4 * p.grad
    assert not np.array_equal(m.mean.bias.data, b0) and float(m.loss()) < l0


def test_zero_constant_mean_is_bitwise_neutral():
    X, y, _ = mean_cases.data("const_mosm3")
    a = gpr.Exact(mean_cases.kernel(gpr, "const_mosm3"), X, y, variance=0.1)
    mean = gpr.ConstantMean()
    mean.train = False
    b = gpr.Exact(mean_cases.kernel(gpr, "const_mosm3"), X, y, variance=0.1, mean=mean)
    la, lb = float(a.loss()), float(b.loss())
    assert la == lb
    for p, q in zip(a.parameters(), [q for q in b.parameters() if not q._name.startswith("ConstantMean")]):
        assert p._name == q._name and np.array_equal(p.grad, q.grad)


def test_device_mean_gradient_at_cfg1_size_and_repeatability():
    """N = 8192 (MOSM C=4 Q=3, configs[1]'s draw) with a MultiOutputMean of LinearMeans: the device reduction equals
    -sum_{k in c} alpha_k [1, x_k] from numpy, and 50 identical evaluations give one result with no dataflow time-out"""
    C, Q, N = 4, 3, 8192
    X, y = synth.make_data(N, C)
    h = synth.mosm_hypers(C, Q)
    k = gpr.MultiOutputSpectralMixtureKernel(Q=Q, output_dims=C)
    for n in ("weight", "mean", "variance", "delay", "phase"):
        getattr(k, n).assign(h[n])
    means = [gpr.LinearMean(1) for _ in range(C)]
    for c, mm in enumerate(means):
        mm.bias.assign(0.1 * c); mm.slope.assign([0.01 * (c - 1.5)])
    m = gpr.Exact(k, X, y, variance=h["scale"] ** 2, mean=gpr.MultiOutputMean(means))
    m.likelihood.scale.assign(h["scale"])
    m.loss()
    hd = m._handle
    g = hd.mean_grad()
    alpha = hd.fetch(2)
    ch = X[:, 0].astype(int)
    want, size = np.zeros((C, 2)), np.zeros((C, 2))
    for c in range(C):
        a, x = alpha[ch == c], X[ch == c, 1]
        want[c] = -np.sum(a), -np.sum(a * x)
        size[c] = np.sum(np.abs(a)), np.sum(np.abs(a * x))        # relative to the sum of the magnitudes: the two summation orders differ
    assert np.all(np.abs(g - want) <= 1e-12 * size), (g, want)
    assert np.array_equal(hd.fetch(3), -alpha)
    seen = set()
    for _ in range(50):
        m.loss()
        seen.add(hd.mean_grad().tobytes())
    assert len(seen) == 1
    assert hd.schedule()["dataflow_timeouts"] == 0


@pytest.mark.parametrize("path", ["sweep", "phases", "fused", "fused-streams"])
def test_every_gradient_schedule_and_accurate_mode_with_a_mean(path):
    """each schedule (and the backward-stable mode) against the same golden vectors, in a fresh process: the schedule is chosen once per process"""
    import os, subprocess, sys, textwrap
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = textwrap.dedent('''
        import sys, numpy as np
        sys.path.insert(0, %r); sys.path.insert(0, %r)
        from helpers import load
        import mean_cases
        from test_mean_gpu import check_value_and_gradients
        from mogptk_amd import gpr
        fx = load("mean.npz")
        for case in ("const_mosm3", "lin_mosm2_d2", "mom_shuf", "poly_mosm2", "lin_mosm3_n300"):
            check_value_and_gradients(mean_cases.exact(gpr, case), fx, case + "__")
            m = mean_cases.exact(gpr, case)
            m._device_handle().set_accurate(True); m._handle.accurate_mode = True
            check_value_and_gradients(m, fx, case + "__")
        print("MEAN_SCHEDULE_OK")
    ''') % (root, os.path.join(root, "tests"))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600,
                         env=dict(os.environ, MOGP_GRAD_PATH=path.split("-")[0], MOGP_FLOW="0" if path == "fused-streams" else "1", MOGP_FLOW_MIN="2"))
    assert "MEAN_SCHEDULE_OK" in out.stdout, out.stdout[-2000:] + out.stderr[-3000:]
