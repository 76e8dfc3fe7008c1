"""
Host logic on CPU: the term tables, the chain rule table -> raw parameters, the optimiser loop and the driver
semantics of the product package, with the device replaced by the numpy table model (oracle/table_model.py).
The native library is NOT exercised here (see tests/test_gpu_parity.py for that); results are compared with the
reference's own outputs in tests/golden/.
"""
import os
import pickle
import numpy as np
import pytest

import mogptk_amd
from mogptk_amd import gpr
import mogptk_amd._lib as L
from helpers import load, fixture_params, product_exact, product_kernel, load_raw, relerr
from oracle.table_model import TableDevice, gram_from_table


@pytest.fixture(autouse=True)
def fake_device(monkeypatch):
    monkeypatch.setattr(L, "ExactHandle", TableDevice)
    monkeypatch.setattr(L, "gram", lambda device, C, D, table, X1, X2=None: gram_from_table(np.asarray(table), X1, X2))


@pytest.mark.parametrize("fixture", ["kernels.npz", "kernels_8f2.npz", "kernels_mohsm.npz"])
def test_term_tables_reproduce_reference_kernels(fixture):
    fx = load(fixture)
    for n in range(int(fx["ncases"])):
        pre = "c%d_" % n
        C, Q, D, Rq = [int(v) for v in fx[pre + "meta"]]
        k = product_kernel(str(fx[pre + "kind"]), C, Q, D, Rq)
        load_raw(k.parameters(), fixture_params(fx, pre))
        X, X2 = fx[pre + "X"], fx[pre + "X2"]
        assert relerr(k.K(X), fx[pre + "K"]) < 1e-13
        assert relerr(k(X, X2), fx[pre + "K12"]) < 1e-13
        assert relerr(k.K_diag(X), fx[pre + "Kdiag"]) < 1e-14


LML = ["mosm_c3q2", "mosm_c2q3_shuf", "mosm_c3q2_d2", "mosm_c1q2", "mosm_scalarvar", "sm_c1q3", "sm_c2q2_d2",
       "csm_c3q2", "csm_c2q2r2",
       "mosk_c3q2", "mosk_c2q1_d2", "umosm_c3q2", "umosm_c2q2_d2", "lmc_c3q2r2", "lmc_c2q3_d2", "lmcsm_c2q2", "conv_c3q2", "conv_c2q1_d2",          # same term table, other parameter algebra
       "mohsm_c3q2", "mohsm_c2q1_d2", "mohsm_c1q2"]                                # ... and the enveloped (2 + 5 D) rows of MOHSM


@pytest.mark.parametrize("name", LML)
def test_loss_and_chain_rule_match_reference_autograd(name):
    fx = load("lml_%s.npz" % name)
    m, fp = product_exact(fx)
    assert abs(float(m.log_marginal_likelihood()) - float(fx["lml"])) < 1e-9 * abs(float(fx["lml"]))
    loss = m.loss()
    assert abs(float(loss) - float(fx["loss"])) < 1e-9 * abs(float(fx["loss"]))
    for p, f in zip(m.parameters(), fp):
        if f["grad"] is None:
            assert p.grad is None, p._name      # same graph membership as the reference
        else:
            assert p.grad is not None, p._name
            assert np.max(np.abs(p.grad - f["grad"])) <= 1e-8 * max(1.0, np.max(np.abs(f["grad"]))), (p._name, p.grad, f["grad"])


def test_predict_matches_reference():
    fx = load("predict.npz")
    for n in range(int(fx["ncases"])):
        pre = "c%d_" % n
        m, fp = product_exact(fx, pre)
        Xs = fx[pre + "Xs"]
        mu, var = m.predict_f(Xs)
        assert mu.shape == (Xs.shape[0], 1) and var.shape == (Xs.shape[0], 1)
        assert relerr(mu, fx[pre + "mu"]) < 1e-9 and np.max(np.abs(var - fx[pre + "var"])) < 1e-9
        _, cov = m.predict_f(Xs, full=True)
        assert np.max(np.abs(cov - fx[pre + "cov"])) < 1e-9
        ymu, lo, up = m.predict_y(Xs, sigma=2.0)
        assert relerr(lo, fx[pre + "lower"]) < 1e-9 and relerr(up, fx[pre + "upper"]) < 1e-9   # quirk Q4 branch


def test_single_output_kernel_without_channel_column():
    fx = load("predict.npz")
    k = gpr.SpectralMixtureKernel(Q=2, input_dims=1)
    m = gpr.Exact(k, fx["so_X"], fx["so_y"], variance=0.04)
    load_raw(m.parameters(), fixture_params(fx, "so_"))
    assert abs(float(m.log_marginal_likelihood()) - float(fx["so_lml"])) < 1e-9
    mu, var = m.predict_f(fx["so_Xs"])
    assert relerr(mu, fx["so_mu"]) < 1e-9 and np.max(np.abs(var - fx["so_var"])) < 1e-9
    _, lo, up = m.predict_y(fx["so_Xs"], sigma=2.0)
    assert relerr(lo, fx["so_lower"]) < 1e-9 and relerr(up, fx["so_upper"]) < 1e-9           # single-output CI branch


def _airline_model():
    fx = load("adam_cfg1.npz")
    data = mogptk_amd.Data(fx["X"][:, 1], fx["y"][:, 0], name="airline")      # already transformed by the reference
    model = mogptk_amd.SM(data, Q=3)
    load_raw(model.gpr.parameters(), fixture_params(fx, "init_"))
    return fx, model


def test_train_adam_trajectory_and_driver_semantics():
    fx, model = _airline_model()
    assert abs(model.log_marginal_likelihood() - float(fx["lml0"])) < 1e-9
    iters = 30
    losses, errors = model.train("Adam", iters=iters, lr=float(fx["lr"]))
    assert losses.shape == (iters + 1,) and errors.shape == (iters + 1,)        # iters+1 evaluations (model.py:563-566)
    assert relerr(losses, fx["losses"][:iters + 1]) < 1e-8
    assert model.times.shape == (iters + 1,) and model.iters == iters
    # a second train() call continues the traces but starts a NEW optimiser (model.py:501-509, :557)
    losses2, _ = model.train("adam", iters=5, lr=float(fx["lr"]))
    assert losses2.shape == (iters + 5 + 1,) and model.iters == iters + 5
    assert np.allclose(losses2[:iters], losses[:iters])
    with pytest.raises(ValueError):
        model.train("nope")


def test_train_lbfgs_trajectories_match_reference():
    """train('LBFGS') (reference model.py:541-553): losses indexed by function evaluation, model.iters = number of evaluations,
    fixed-step torch defaults and lr / history_size overrides -- against traces recorded from the reference."""
    fx = load("lbfgs_cfg1.npz")
    for tag, kw in (("fixed", {}), ("fixed_lr", dict(lr=0.5, history_size=5))):
        _, model = _airline_model()
        losses, errors = model.train("LBFGS", iters=int(fx[tag + "_max_iter"]), **kw)
        ref = fx[tag + "_losses"]
        assert model.iters == int(fx[tag + "_iters"]) and model.losses.shape == ref.shape
        assert relerr(model.losses[:15], ref[:15]) < 1e-8                       # measured 1e-12 .. 4e-10: the same algorithm
        assert relerr(model.losses, ref) < 1e-4                                  # later the curvature pairs amplify rounding (measured 3e-5)
        for p, f in zip(model.gpr.parameters(), fixture_params(fx, tag + "_final_")):
            assert np.max(np.abs(p.data - f["raw"])) < 1e-3 * max(1.0, np.max(np.abs(f["raw"]))), p._name   # measured 2e-4
    for alias in ("l-bfgs", "lbfgsb", "L-BFGS-B"):
        _, model = _airline_model()
        model.train(alias, iters=3)
        assert model.iters == 3


def test_lbfgs_matches_torch_on_a_test_function():
    """the numpy optimiser against torch.optim.LBFGS itself (the semantics the reference relies on), with and without the strong-Wolfe
    line search, on the 6-dimensional Rosenbrock function: same iterates, same number of function evaluations"""
    import torch
    from mogptk_amd.model import _LBFGS
    from mogptk_amd.gpr import Parameter

    def rosen(x):
        return ((1.0 - x[:-1]) ** 2).sum() + 100.0 * ((x[1:] - x[:-1] ** 2) ** 2).sum()

    x0 = np.array([-1.2, 1.0, 0.5, -0.3, 0.8, 1.5])
    for kw in (dict(max_iter=25), dict(max_iter=40, line_search_fn="strong_wolfe"), dict(max_iter=30, lr=0.3, history_size=4),
               dict(max_iter=60, max_eval=70, line_search_fn="strong_wolfe", tolerance_grad=1e-12, tolerance_change=1e-14)):
        xt = torch.tensor(x0, dtype=torch.float64, requires_grad=True)
        opt = torch.optim.LBFGS([xt], **kw)
        trace_t = []

        def closure_t():
            opt.zero_grad()
            f = rosen(xt)
            f.backward()
            trace_t.append(float(f))
            return f
        opt.step(closure_t)

        p = Parameter(x0.copy())
        p.data = x0.copy()
        mine = _LBFGS([p], **kw)
        trace_m = []

        def closure_m():
            x = torch.tensor(p.data, dtype=torch.float64, requires_grad=True)
            f = rosen(x)
            f.backward()
            p.grad = x.grad.numpy().copy()
            trace_m.append(float(f))
            return float(f)
        mine.step(closure_m)
        assert len(trace_m) == len(trace_t) == mine.state["func_evals"], (kw, len(trace_m), len(trace_t))
        assert relerr(trace_m, trace_t) < 1e-6, (kw, relerr(trace_m, trace_t))      # same evaluation count; values agree to rounding amplification
        assert np.max(np.abs(p.data - xt.detach().numpy())) < 1e-6, kw


def test_predict_return_shapes_and_pickle_roundtrip(tmp_path):
    fx, model = _airline_model()
    xs = fx["pred_X"]
    X, mu, lo, up = model.predict(xs)
    assert isinstance(mu, np.ndarray) and mu.shape == (len(xs),)               # bare arrays for one channel (model.py:662-664)
    model.save(str(tmp_path / "m"))
    m2 = mogptk_amd.LoadModel(str(tmp_path / "m"))
    assert m2.gpr._handle is None                                              # device handles are not pickled
    assert abs(m2.log_marginal_likelihood() - model.log_marginal_likelihood()) < 1e-12
    t = np.linspace(0, 10, 30)
    ds = mogptk_amd.DataSet(t, [np.sin(t), np.cos(t)])
    mm = mogptk_amd.MOSM(ds, Q=2)
    Xl, Mu, Lo, Up = mm.predict([np.linspace(0, 12, 7), np.linspace(0, 12, 9)])
    assert isinstance(Mu, list) and Mu[0].shape == (7,) and Mu[1].shape == (9,)


def test_quirks_q1_q2_q3():
    fx = load("quirks.npz")
    p = gpr.Parameter(1.0, lower=1e-8)
    assert np.allclose(p(), fx["q1_readback"], rtol=1e-15) and np.allclose(p.data, fx["q1_raw"], rtol=1e-15)
    p = gpr.Parameter(fx["sp_vals"], lower=1e-8)
    assert np.allclose(p.data, fx["sp_raw"], rtol=1e-14) and np.allclose(p(), fx["sp_cons"], rtol=1e-14)
    p = gpr.Parameter(fx["sp_vals"], lower=1e-8, upper=300.0)
    assert np.allclose(p.data, fx["sg_raw"], rtol=1e-13) and np.allclose(p(), fx["sg_cons"], rtol=1e-14)
    t = np.linspace(0, 10, 20)
    ds = mogptk_amd.DataSet(t, [np.sin(t), np.cos(t)])
    m = mogptk_amd.MOSM(ds, Q=2)
    assert np.array_equal(m.gpr.kernel.mean(), fx["q2_mean"])                   # Q2: collapsed to the lower bound
    assert np.all(np.isneginf(m.gpr.kernel.mean.data)) == np.all(np.isneginf(fx["q2_mean_raw"]))
    assert np.allclose(m.gpr.kernel.mean.upper, fx["q2_upper"])
    # Q3: train=False only changes num_parameters(); the optimiser still moves the tensor
    n0 = m.num_parameters()
    m.gpr.kernel.weight.train = False
    assert m.num_parameters() == n0 - m.gpr.kernel.weight.num_parameters
    w0 = m.gpr.kernel.weight.data.copy()
    m.gpr.kernel.mean.assign(np.full((2, 2, 1), 0.1))
    m.train("Adam", iters=2, lr=0.1)
    assert not np.allclose(m.gpr.kernel.weight.data, w0)
    with pytest.raises(AttributeError):
        m.gpr.kernel.weight = gpr.Parameter(1.0)


def test_sm_lmc_wrapper_matches_reference():
    """SM_LMC (reference models/sm_lmc.py): constructor state -- bounds, train flags, pegged magnitudes, Nyquist re-bounding with quirk
    Q2 --, then loss, gradient and an Adam trace at explicit parameter values"""
    fx = load("sm_lmc.npz")
    ds = mogptk_amd.DataSet(fx["t"], [fx["Y"][j] for j in range(3)])
    m = mogptk_amd.SM_LMC(ds, Q=int(fx["Q"]), Rq=int(fx["Rq"]))
    params = list(m.gpr.parameters())
    ctor = fixture_params(fx, "ctor_")
    assert [p._name for p in params] == [str(n) for n in fx["ctor_names"]]
    assert [bool(p.train) for p in params] == [bool(b) for b in fx["ctor_train"]]
    assert m.num_parameters() == int(fx["num_parameters"])
    for p, f in zip(params, ctor):
        for mine, ref in ((p.lower, f["lower"]), (p.upper, f["upper"])):
            assert (mine is None) == (ref is None), p._name
            if ref is not None:
                assert np.allclose(np.broadcast_to(mine, np.shape(ref)), ref, rtol=1e-12), p._name
        if p._name.endswith("magnitude") or p._name.endswith("mean"):          # not random: pegged to 1 / collapsed by quirk Q2
            assert np.allclose(p(), f["cons"], rtol=1e-12), p._name
    fp = fixture_params(fx)
    load_raw(params, fp)
    assert abs(m.log_marginal_likelihood() - float(fx["lml"])) < 1e-9 * abs(float(fx["lml"]))
    assert abs(float(m.gpr.loss()) - float(fx["loss"])) < 1e-9 * abs(float(fx["loss"]))
    for p, f in zip(params, fp):
        if f["grad"] is None:
            assert p.grad is None, p._name
        else:
            assert np.max(np.abs(p.grad - f["grad"])) <= 1e-8 * max(1.0, np.max(np.abs(f["grad"]))), p._name
    losses, _ = m.train("Adam", iters=10, lr=0.05)
    assert relerr(losses, fx["adam_losses"]) < 1e-8


def test_init_parameters_ls_matches_reference():
    """Lomb-Scargle peak estimates (data.py:946-1002) and init_parameters('LS') of the four wrappers against the reference"""
    fx = load("init_ls.npz")
    chans = [(fx["x%d" % j], fx["y%d" % j]) for j in range(int(fx["nchan"]))]
    ds = mogptk_amd.DataSet(*[mogptk_amd.Data(x, y) for x, y in chans])
    assert np.allclose(np.stack(ds.get_nyquist_estimation()), fx["nyquist"], rtol=1e-13)
    A, B, C = ds.get_ls_estimation(Q=3)
    assert relerr(np.stack(A), fx["ls_A"]) < 1e-10 and relerr(np.stack(B), fx["ls_B"]) < 1e-12 and relerr(np.stack(C), fx["ls_C"]) < 1e-9
    for tag, make in (("mosm", lambda: mogptk_amd.MOSM(ds, Q=2)), ("sm", lambda: mogptk_amd.SM(ds, Q=3)),
                      ("csm", lambda: mogptk_amd.CSM(ds, Q=2, Rq=2)), ("smlmc", lambda: mogptk_amd.SM_LMC(ds, Q=2, Rq=2))):
        m = make()
        m.init_parameters("LS")
        fp = fixture_params(fx, tag + "_")
        for p, f in zip(m.gpr.parameters(), fp):
            random_in_reference = tag in ("mosm",) and (p._name.endswith("delay") or p._name.endswith("phase"))
            random_in_reference |= tag == "csm" and p._name.endswith("shift")
            if random_in_reference:
                continue                                    # drawn from torch.rand by the constructor, untouched by init_parameters
            assert np.allclose(p(), f["cons"], rtol=1e-8, atol=1e-12), (tag, p._name, p(), f["cons"])
        if tag in ("sm", "smlmc"):                          # nothing random left: the whole model state is reproduced
            assert abs(m.log_marginal_likelihood() - float(fx[tag + "_lml"])) < 1e-7 * abs(float(fx[tag + "_lml"]))
    with pytest.raises(ValueError):
        mogptk_amd.MOSM(ds, Q=2).init_parameters("nope")
    # the 'SM' method: a spectral mixture fitted per channel on the device (here: its numpy twin), then handed to MOSM
    m = mogptk_amd.MOSM(mogptk_amd.DataSet(*[mogptk_amd.Data(x[:40], y[:40]) for x, y in chans[:2]]), Q=2)
    m.init_parameters("SM", iters=5)
    assert np.all(np.isfinite(m.gpr.kernel.mean())) and np.isfinite(m.log_marginal_likelihood())


def test_bnse_matches_reference():
    """BNSE (reference init.py): the GP fit (Adam, lr = 2) runs through the device path, the spectrum posterior uses the factor the
    device hands back; spectra, peak estimates and MOSM.init_parameters('BNSE') against the reference"""
    fx = load("bnse.npz")
    w, mu, var = mogptk_amd.BNSE(fx["x"].copy(), fx["y"], n=150, iters=60)
    assert relerr(w, fx["w"]) < 1e-13
    assert relerr(mu, fx["mu"]) < 1e-6 and relerr(var, fx["var"]) < 1e-6
    w2, mu2, var2 = mogptk_amd.BNSE(fx["x"].copy(), fx["y"], y_err=fx["yerr"], max_freq=0.9, n=120, iters=40)
    assert relerr(mu2, fx["mu2"]) < 1e-6 and relerr(var2, fx["var2"]) < 1e-6
    ds = mogptk_amd.DataSet(mogptk_amd.Data(fx["x"], fx["y"]), mogptk_amd.Data(fx["x1"], fx["y1"]))
    A, B, C = ds.get_bnse_estimation(Q=2, n=400, iters=50)
    assert relerr(np.stack(A), fx["est_A"]) < 1e-5 and relerr(np.stack(B), fx["est_B"]) < 1e-9 and relerr(np.stack(C), fx["est_C"]) < 1e-4
    m = mogptk_amd.MOSM(ds, Q=2)
    m.init_parameters("BNSE", iters=50)
    for p, f in zip(m.gpr.parameters(), fixture_params(fx, "mosm_")):
        if p._name.endswith("delay") or p._name.endswith("phase"):
            continue                                        # random in the reference's constructor
        assert np.allclose(p(), f["cons"], rtol=1e-4, atol=1e-10), (p._name, p(), f["cons"])


def test_transformers_match_reference_and_cfg1_end_to_end():
    """Y transformers (reference transformer.py) alone and chained; and BASELINE.json configs[0] from the raw series: transforms ->
    SM(Q=3) -> init_parameters('LS') reproduces the kernel-format data and the initial parameters of adam_cfg1.npz"""
    fx = load("transformers.npz")
    cases = {"detrend2": [mogptk_amd.TransformDetrend(degree=2)], "linear": [mogptk_amd.TransformLinear(bias=1.5, slope=0.7)],
             "normalize": [mogptk_amd.TransformNormalize], "log": [mogptk_amd.TransformLog], "standard": [mogptk_amd.TransformStandard],
             "chain": [mogptk_amd.TransformDetrend(degree=1), mogptk_amd.TransformLog, mogptk_amd.TransformStandard()]}
    for name, ts in cases.items():
        d = mogptk_amd.Data(fx["x"][:, 0].copy(), fx["y"].copy())
        for t in ts:
            d.transform(t)
        _, yt = d.get_data(transformed=True)
        assert relerr(yt, fx[name + "_fwd"]) < 1e-13, name
        assert relerr(d.Y_transformer.backward(yt + 0.25, d.X), fx[name + "_bwd"]) < 1e-13, name
    with pytest.raises(ValueError):
        mogptk_amd.Transformer([object()])
    d = mogptk_amd.Data(fx["air_x"], fx["air_y"], name="airline")
    d.transform(mogptk_amd.TransformDetrend(degree=2)); d.transform(mogptk_amd.TransformStandard())
    assert relerr(d.get_data(transformed=True)[1], fx["air_yt"]) < 1e-12
    gold = load("adam_cfg1.npz")
    model = mogptk_amd.SM(d, Q=3)
    model.init_parameters("LS")
    assert relerr(model.gpr.y[:, 0], gold["y"][:, 0]) < 1e-12
    for p, f in zip(model.gpr.parameters(), fixture_params(gold, "init_")):
        assert np.allclose(p(), f["cons"], rtol=1e-8, atol=1e-12), p._name
    assert abs(model.log_marginal_likelihood() - float(gold["lml0"])) < 1e-7 * abs(float(gold["lml0"]))
    losses, _ = model.train("Adam", iters=20, lr=float(gold["lr"]))
    assert relerr(losses, gold["losses"][:21]) < 1e-6
    X, mu, lo, up = model.predict(gold["pred_X"])             # back-transformed by default
    assert np.all(np.isfinite(mu)) and mu.shape == (len(gold["pred_X"]),)


def check_single_precision_switch(tol=2e-3):
    """config.use_single_precision() (reference gpr/config.py:20-24, jitter floor gpr/model.py:106-110): float32 host tensors in and
    out, the 1e-6 jitter floor; the device still computes in fp64, so against the reference's own float32 run only float32-level
    agreement can be asked for (its Cholesky runs in float32)."""
    fx = load("fp32.npz")
    C, Q, D, Rq = [int(v) for v in fx["meta"]]
    fp = fixture_params(fx)
    gpr.use_single_precision()
    try:
        k = product_kernel("mosm", C, Q, D, Rq)
        m = gpr.Exact(k, fx["X"], fx["y"], variance=np.square(fp[-1]["cons"]), jitter=1e-8)
        assert m.jitter == float(fx["jitter"]) == 1e-6
        load_raw(m.parameters(), fp)
        assert all(p.data.dtype == np.float32 for p in m.parameters()) and m.X.dtype == np.float32
        loss = m.loss()
        assert loss.dtype == np.float32 and str(fx["loss_dtype"]) == "torch.float32"
        assert abs(float(loss) - float(fx["loss"])) < tol * abs(float(fx["loss"]))
        for p, f in zip(m.parameters(), fp):
            assert p.grad.dtype == np.float32
            assert np.max(np.abs(p.grad - f["grad"])) <= 10 * tol * max(1.0, np.max(np.abs(f["grad"]))), (p._name, p.grad, f["grad"])
        mu, var = m.predict_f(fx["Xs"])
        assert mu.dtype == np.float32 and var.dtype == np.float32
        assert relerr(mu, fx["mu"]) < 10 * tol and np.max(np.abs(var - fx["var"])) < 10 * tol * max(1.0, np.max(np.abs(fx["var"])))
    finally:
        gpr.use_double_precision()
    assert gpr.Parameter(1.0).data.dtype == np.float64


def test_single_precision_switch_matches_reference_semantics():
    check_single_precision_switch()


def test_unsupported_paths_fail_loudly():
    with pytest.raises(NotImplementedError):
        gpr.use_half_precision()
    with pytest.raises(NotImplementedError):
        gpr.use_cpu()
    k = gpr.MultiOutputSpectralMixtureKernel(Q=1, output_dims=2) * gpr.MultiOutputSpectralMixtureKernel(Q=1, output_dims=2)
    with pytest.raises(NotImplementedError):
        k._spectral_terms(1)


def _titsias_from_fixture(fx, pre):
    C, Q, D, Rq = [int(v) for v in fx[pre + "meta"]]
    fp = fixture_params(fx, pre)
    k = gpr.MultiOutputSpectralMixtureKernel(Q=Q, output_dims=C, input_dims=D)
    Zspec = fx[pre + "Zspec"]
    Zspec = int(Zspec[0]) if bool(fx[pre + "Zspec_is_int"]) else [int(z) for z in Zspec]
    m = gpr.Titsias(k, fx[pre + "X"], fx[pre + "y"], Z=Zspec, variance=float(fp[-1]["cons"]) ** 2, jitter=float(fx[pre + "jitter"]))
    return m, fp


def test_titsias_bound_gradient_and_quirks_q5_q6():
    """config 5's model class at fixture size: inducing-point initialisation (int = per channel, float32-rounded grid),
    parameter order (Z first, like torch.nn.Module.parameters()), ELBO, every gradient incl. dZ and dsigma, predict_f"""
    fx = load("titsias.npz")
    for n in range(int(fx["ncases"])):
        pre = "c%d_" % n
        m, fp = _titsias_from_fixture(fx, pre)
        assert [p._name.split(".")[-1] for p in m.parameters()] == [f["name"].split(".")[-1] for f in fp]
        assert np.array_equal(m.Z.data, fp[0]["raw"])                                  # Q5 + Q6
        load_raw(m.parameters(), fp)
        assert abs(float(m.log_marginal_likelihood()) - float(fx[pre + "elbo"])) < 1e-9 * abs(float(fx[pre + "elbo"]))
        assert abs(float(m.loss()) - float(fx[pre + "loss"])) < 1e-9 * abs(float(fx[pre + "loss"]))
        for p, f in zip(m.parameters(), fp):
            if f["grad"] is None:
                assert p.grad is None, p._name
            else:
                assert np.max(np.abs(p.grad - f["grad"])) <= 1e-8 * max(1.0, np.max(np.abs(f["grad"]))), p._name
        assert np.all(m.Z.grad[:, 0] == 0.0)                                            # gradient-free channel column
        mu, var = m.predict_f(fx[pre + "Xs"])
        assert relerr(mu, fx[pre + "mu"]) < 1e-9 and np.max(np.abs(var - fx[pre + "var"])) < 1e-9


def check_titsias_with_enveloped_terms(tol_loss=1e-9, tol_grad=1e-8, tol_pred=1e-9):
    """any kernel under any inference (reference gpr/multioutput.py:340-395 under gpr/model.py:700-724): the Titsias bound with a mixture of
    MultiOutputHarmonizableSpectralKernel -- term rows of width 2 + 5 D, a kernel diagonal that follows the points (per-point K_ff,diag in
    the trace term, K_uu's relative jitter depending on Z), the envelope's share of d/dZ -- against the reference's autograd"""
    fx = load("titsias_mohsm.npz")
    for n in range(int(fx["ncases"])):
        pre = "c%d_" % n
        C, Q, D, _ = [int(v) for v in fx[pre + "meta"]]
        fp = fixture_params(fx, pre)
        k = gpr.MixtureKernel(gpr.MultiOutputHarmonizableSpectralKernel(output_dims=C, input_dims=D), Q)
        s = float(fx[pre + "scale"])
        m = gpr.Titsias(k, fx[pre + "X"], fx[pre + "y"], Z=[int(z) for z in fx[pre + "Zspec"]], variance=s ** 2, jitter=float(fx[pre + "jitter"]))
        assert [p._name.split(".")[-1] for p in m.parameters()] == [f["name"].split(".")[-1] for f in fp]
        load_raw(m.parameters(), fp)
        assert abs(float(m.log_marginal_likelihood()) - float(fx[pre + "elbo"])) < tol_loss * abs(float(fx[pre + "elbo"]))
        assert abs(float(m.loss()) - float(fx[pre + "loss"])) < tol_loss * abs(float(fx[pre + "loss"]))
        for p, f in zip(m.parameters(), fp):
            if f["grad"] is None:
                assert p.grad is None, p._name
            else:
                assert np.max(np.abs(p.grad - f["grad"])) <= tol_grad * max(1.0, np.max(np.abs(f["grad"]))), (n, p._name, p.grad, f["grad"])
        mu, var = m.predict_f(fx[pre + "Xs"])
        assert relerr(mu, fx[pre + "mu"]) < tol_pred and np.max(np.abs(var - fx[pre + "var"])) < tol_pred * max(1.0, np.max(np.abs(fx[pre + "var"])))


def test_titsias_with_enveloped_terms_matches_reference():
    check_titsias_with_enveloped_terms()


def check_snelson_with_enveloped_terms(tol_loss=1e-9, tol_grad=1e-8, tol_pred=1e-9):
    """the FITC model under the same enveloped kernel (reference gpr/multioutput.py:340-395 under gpr/model.py:516-576): K_ff,diag per training
    point inside g_n = K_ff,nn - Q_ff,nn + sigma^2 and dp/dK_ff,nn per point back through it, K_uu's relative jitter depending on Z, scalar
    and per-channel noise -- against the reference's autograd"""
    fx = load("snelson_mohsm.npz")
    for n in range(int(fx["ncases"])):
        pre = "c%d_" % n
        C, Q, D, _ = [int(v) for v in fx[pre + "meta"]]
        fp = fixture_params(fx, pre)
        k = gpr.MixtureKernel(gpr.MultiOutputHarmonizableSpectralKernel(output_dims=C, input_dims=D), Q)
        var = np.asarray(fx[pre + "variance"])
        m = gpr.Snelson(k, fx[pre + "X"], fx[pre + "y"], Z=[int(z) for z in fx[pre + "Zspec"]], variance=(var if var.ndim else float(var)),
                        jitter=float(fx[pre + "jitter"]))
        assert [p._name.split(".")[-1] for p in m.parameters()] == [f["name"].split(".")[-1] for f in fp]
        load_raw(m.parameters(), fp)
        assert abs(float(m.log_marginal_likelihood()) - float(fx[pre + "lml"])) < tol_loss * abs(float(fx[pre + "lml"]))
        assert abs(float(m.loss()) - float(fx[pre + "loss"])) < tol_loss * abs(float(fx[pre + "loss"]))
        for p, f in zip(m.parameters(), fp):
            if f["grad"] is None:
                assert p.grad is None, p._name
            else:
                assert np.max(np.abs(p.grad - f["grad"])) <= tol_grad * max(1.0, np.max(np.abs(f["grad"]))), (n, p._name, p.grad, f["grad"])
        mu, var_p = m.predict_f(fx[pre + "Xs"])
        assert relerr(mu, fx[pre + "mu"]) < tol_pred and np.max(np.abs(var_p - fx[pre + "var"])) < tol_pred * max(1.0, np.max(np.abs(fx[pre + "var"])))


def test_snelson_with_enveloped_terms_matches_reference():
    check_snelson_with_enveloped_terms()


def test_titsias_through_the_model_wrapper():
    t = np.linspace(0, 10, 40)
    ds = mogptk_amd.DataSet(t, [np.sin(t), np.cos(t)])
    m = mogptk_amd.MOSM(ds, Q=2, inference=mogptk_amd.Titsias(inducing_points=5, variance=0.05))
    assert m.gpr.Z().shape == (10, 2)                                                  # 5 per channel (quirk Q5)
    m.gpr.kernel.mean.assign(np.full((2, 2, 1), 0.1))
    losses, _ = m.train("Adam", iters=3, lr=0.05)
    assert losses.shape == (4,) and np.all(np.isfinite(losses))
    assert m.num_parameters() == sum(p.num_parameters for p in m.parameters())        # Z counts without its channel column


# ---- SURVEY 8f-1 remainder: SGD / AdaGrad / error= pinned on traces recorded from the reference (model.py:531-561) -------------
OPT_RUNS = (("sgd", "SGD", dict(iters=12, lr=2e-4)),
            ("sgd_mom", "sgd", dict(iters=12, lr=1e-4, momentum=0.9, nesterov=True, weight_decay=1e-3)),
            ("adagrad", "AdaGrad", dict(iters=12, lr=0.05)),
            ("adagrad_decay", "adagrad", dict(iters=12, lr=0.05, lr_decay=0.1, initial_accumulator_value=0.5)))


def check_opt_traces(tol_loss=1e-9, tol_raw=1e-8):
    fx = load("opt_traces.npz")
    for tag, method, kw in OPT_RUNS:
        _, model = _airline_model()
        losses, errors = model.train(method, **kw)
        assert losses.shape == fx[tag + "_losses"].shape and np.all(errors == 0.0)
        assert relerr(losses, fx[tag + "_losses"]) < tol_loss, (tag, relerr(losses, fx[tag + "_losses"]))
        for p, f in zip(model.gpr.parameters(), fixture_params(fx, tag + "_final_")):
            assert np.max(np.abs(p.data - f["raw"])) < tol_raw * max(1.0, np.max(np.abs(f["raw"]))), (tag, p._name)


def _airline_model_with_test_points(fx, remove=24):
    air = load("transformers.npz")
    data = mogptk_amd.Data(air["air_x"], air["air_y"], name="airline")
    data.remove_range(start=air["air_x"][-remove] - 1e-9)
    data.transform(mogptk_amd.TransformDetrend(degree=2))
    data.transform(mogptk_amd.TransformStandard())
    model = mogptk_amd.SM(data, Q=3)
    assert relerr(model.gpr.X, fx["err_X"]) < 1e-14 and relerr(model.gpr.y, fx["err_y"]) < 1e-12
    load_raw(model.gpr.parameters(), fixture_params(fx, "err_init_"))
    return model


def check_error_path(tol=1e-7):
    """error= evaluates a full predict on the held-out points (or on all data when there are none) at every iteration"""
    fx = load("opt_traces.npz")
    model = _airline_model_with_test_points(fx)
    losses, errors = model.train("Adam", iters=8, lr=0.05, error="MAE")
    assert relerr(model.losses, fx["err_losses"]) < tol and relerr(model.errors, fx["err_errors"]) < tol
    losses, errors = model.train("Adam", iters=5, lr=0.05, error="sMAPE")           # continued call: iter_offset (model.py:501-509)
    assert model.iters == int(fx["err_iters2"]) and errors.shape == fx["err_errors2"].shape
    assert relerr(model.losses, fx["err_losses2"]) < tol and relerr(model.errors, fx["err_errors2"]) < tol
    assert abs(model.error("RMSE", use_all_data=True) - float(fx["err_rmse_all"])) < tol * float(fx["err_rmse_all"])
    _, model = _airline_model()
    air = load("transformers.npz")
    model = None
    data = mogptk_amd.Data(air["air_x"], air["air_y"], name="airline")
    data.transform(mogptk_amd.TransformDetrend(degree=2))
    data.transform(mogptk_amd.TransformStandard())
    model = mogptk_amd.SM(data, Q=3)
    load_raw(model.gpr.parameters(), fixture_params(load("adam_cfg1.npz"), "init_"))
    losses, errors = model.train("Adam", iters=4, lr=0.05, error=lambda yt, yp: float(np.max(np.abs(yt - yp))))
    assert relerr(errors, fx["errall_errors"]) < tol
    with pytest.raises(ValueError):
        model.train("Adam", iters=1, error=lambda yt, yp: "nope")


def test_train_sgd_adagrad_trajectories_match_reference():
    check_opt_traces()


def test_train_error_path_matches_reference():
    check_error_path()


def test_data_removal_semantics():
    """reference data.py:683-705: nothing is removed without n / pct; n must be an integer"""
    d = mogptk_amd.Data(np.arange(20.0), np.arange(20.0))
    d.remove_randomly()
    assert d.mask.all()
    d.remove_randomly(pct=0.25, seed=3)
    assert (~d.mask).sum() == 5
    with pytest.raises(ValueError):
        d.remove_randomly(n=2.5)
    d = mogptk_amd.Data(np.arange(20.0), np.arange(20.0))
    d.remove_range(5, 9)
    assert (~d.mask).sum() == 5 and not d.mask[5] and not d.mask[9] and d.mask[10]


def check_pegged_parameters(tol_loss=1e-9, tol_grad=1e-7):
    """Parameter.peg (reference parameter.py:321-335): the gradient of a pegged parameter goes to the parameter it follows, through
    the peg transform; the pegged tensor keeps grad None"""
    fx = load("peg.npz")
    C, Q, D, Rq = [int(v) for v in fx["meta"]]
    fp = fixture_params(fx)
    k = product_kernel("sm", C, Q, D, Rq)
    m = gpr.Exact(k, fx["X"], fx["y"], variance=np.square(fp[-1]["cons"]), jitter=float(fx["jitter"]))
    load_raw(m.parameters(), fp)
    k[1].mean.peg(k[0].mean, lambda x: 2.0 * x)
    k[1].magnitude.peg(k[0].magnitude)
    assert abs(float(m.log_marginal_likelihood()) - float(fx["lml"])) < tol_loss * abs(float(fx["lml"]))
    assert abs(float(m.loss()) - float(fx["loss"])) < tol_loss * abs(float(fx["loss"]))
    for p, f in zip(m.parameters(), fp):
        if f["grad"] is None:
            assert p.grad is None and p.pegged, p._name
        else:
            assert np.max(np.abs(p.grad - f["grad"])) <= tol_grad * max(1.0, np.max(np.abs(f["grad"]))), (p._name, p.grad, f["grad"])


def test_pegged_parameters_route_gradients_like_autograd():
    check_pegged_parameters()


def check_mohsm_predict_and_wrapper(tol_pred=1e-8, tol_loss=1e-9, tol_grad=1e-8, tol_trace=1e-8):
    """MOHSM (SURVEY 8f-2 remainder): predict_f of a harmonizable mixture (non-constant K_diag -> per-point kss), then the wrapper:
    constructor state, init_parameters('LS'), loss + gradient and an Adam trace against recordings of the reference"""
    fx = load("mohsm.npz")
    m, fp = product_exact(fx)
    mu, var = m.predict_f(fx["Xs"])
    assert relerr(mu, fx["mu"]) < tol_pred and np.max(np.abs(var - fx["var"])) < tol_pred * max(1.0, np.max(np.abs(fx["var"])))
    ds = mogptk_amd.DataSet(fx["w_t"], [fx["w_Y"][j] for j in range(2)])
    w = mogptk_amd.MOHSM(ds, P=1, Q=2)
    params = list(w.gpr.parameters())
    ctor = fixture_params(fx, "w_ctor_")
    assert [p._name for p in params] == [str(n) for n in fx["w_ctor_names"]]
    assert w.num_parameters() == int(fx["w_num_parameters"])
    for p, f in zip(params, ctor):
        for mine, ref in ((p.lower, f["lower"]), (p.upper, f["upper"])):
            assert (mine is None) == (ref is None), p._name
    load_raw(params, ctor)                       # the random draws of the reference's constructor
    w.init_parameters("LS")
    for p, f in zip(params, fixture_params(fx, "w_init_")):
        assert np.max(np.abs(p() - f["cons"])) <= 1e-8 * max(1.0, np.max(np.abs(f["cons"]))), (p._name, p(), f["cons"])
    wp = fixture_params(fx, "w_")
    load_raw(params, wp)
    assert abs(w.log_marginal_likelihood() - float(fx["w_lml"])) < tol_loss * abs(float(fx["w_lml"]))
    assert abs(float(w.gpr.loss()) - float(fx["w_loss"])) < tol_loss * abs(float(fx["w_loss"]))
    for p, f in zip(params, wp):
        if f["grad"] is None:
            assert p.grad is None, p._name
        else:
            assert np.max(np.abs(p.grad - f["grad"])) <= tol_grad * max(1.0, np.max(np.abs(f["grad"]))), (p._name, p.grad, f["grad"])
    losses, _ = w.train("Adam", iters=8, lr=0.05)
    assert relerr(losses, fx["w_adam_losses"]) < tol_trace


def test_mohsm_predict_and_wrapper_match_reference():
    check_mohsm_predict_and_wrapper()


# ---- checkpoints written by the reference's Model.save() load without the reference ----------------------------------
def check_reference_checkpoints(tmp_path, tol_value=1e-12, tol_loss=1e-8, tol_grad=1e-6, tol_pred=1e-6, tags=("mosm", "sm", "csm", "smlmc", "conv", "titsias", "snelson", "hensman", "oa", "hensman_lik")):
    """checkpoints.npz: the bytes of files the reference wrote, and what the reference itself computes after loading them"""
    fx = load("checkpoints.npz")
    for tag in tags:
        path = tmp_path / ("ref_%s" % tag)
        (tmp_path / ("ref_%s.npy" % tag)).write_bytes(fx[tag + "_file"].tobytes())
        m = mogptk_amd.LoadModel(str(path))
        assert type(m).__name__ == {"mosm": "MOSM", "sm": "SM", "csm": "CSM", "smlmc": "SM_LMC", "conv": "CONV", "titsias": "MOSM", "snelson": "MOSM", "hensman": "MOSM", "oa": "MOSM", "hensman_lik": "MOSM"}[tag]
        ps = list(m.gpr.parameters())
        assert [p._name for p in ps] == [str(n) for n in fx[tag + "_names"]]
        for i, p in enumerate(ps):
            ref = fx["%s_p%d" % (tag, i)]
            assert np.max(np.abs(np.asarray(p()) - ref)) <= tol_value * max(1.0, np.max(np.abs(ref))), (tag, p._name)
            assert bool(p.train) == bool(fx["%s_train%d" % (tag, i)])
        assert list(fx[tag + "_history"]) == [m.iters, len(m.times), len(m.losses)]
        loss = m.loss()
        ref_loss = float(fx[tag + "_loss"])
        assert abs(loss - ref_loss) <= tol_loss * max(1.0, abs(ref_loss)), (tag, loss, ref_loss)
        for i, p in enumerate(ps):
            g = fx["%s_g%d" % (tag, i)]
            if g.size == 0:
                assert p.grad is None, (tag, p._name)
            else:
                assert np.max(np.abs(p.grad - g)) <= tol_grad * max(1.0, np.max(np.abs(g))), (tag, p._name)
        if tag == "hensman_lik":
            import torch
            torch.manual_seed(4321)                              # sampled intervals: same generator, same seed, same sequence of draws as the reference
        _, mu, lower, upper = m.predict(transformed=False)
        cat = lambda parts: np.concatenate([np.asarray(v).reshape(-1) for v in (parts if isinstance(parts, list) else [parts])])
        for got, key in ((mu, "_mu"), (lower, "_lower"), (upper, "_upper")):
            ref = fx[tag + key]
            fin = np.isfinite(ref)                               # (the log of a zero Poisson count is -inf on both sides)
            assert np.array_equal(cat(got)[~fin], ref[~fin]) and np.max(np.abs(cat(got)[fin] - ref[fin])) <= tol_pred * max(1.0, np.max(np.abs(ref[fin]))), (tag, key)
        # and back out through this package's own save / load, and through a file in the reference's format
        m.save(str(tmp_path / ("own_%s" % tag)))
        m2 = mogptk_amd.LoadModel(str(tmp_path / ("own_%s" % tag)))
        assert abs(m2.loss() - loss) <= 1e-12 * max(1.0, abs(loss))
        if tag in WRITER_TAGS:
            m.save(str(tmp_path / ("back_%s" % tag)), reference=True)
            m3 = mogptk_amd.LoadModel(str(tmp_path / ("back_%s" % tag)))
            assert type(m3) is type(m) and abs(m3.loss() - loss) <= 1e-12 * max(1.0, abs(loss))


WRITER_TAGS = ("mosm", "sm", "csm", "smlmc", "conv", "titsias")


def _checkpoint_tree(o, pars):
    """a pickled model of the reference, read into state bags, as nested plain data: class names, attribute dictionaries IN ORDER, tensors as
    arrays, each parameter once (pegging refers to it by number)"""
    import torch
    from mogptk_amd import compat
    if isinstance(o, compat._Bag):
        return ("obj", o._mod, o._cls, [(k, _checkpoint_tree(v, pars)) for k, v in o.state().items() if k != "compiled_forward"])
    if isinstance(o, compat._RefParameter):
        if id(o) in pars:
            return ("parameter", pars[id(o)])
        pars[id(o)] = len(pars)
        return ("parameter", pars[id(o)], o.name, o.data, o.lower, o.upper, o.train, o.num_parameters, o.prior,
                _checkpoint_tree(o.pegged_parameter, pars), repr(o.pegged_transform))
    if isinstance(o, torch.nn.ModuleList):
        return ("obj", "torch.nn.modules.container", "ModuleList", [(k, _checkpoint_tree(v, pars)) for k, v in o.__dict__.items()])
    if isinstance(o, torch.Tensor):
        return ("tensor", str(o.dtype), o.detach().numpy())
    if isinstance(o, dict):
        return (type(o).__name__, [(k, _checkpoint_tree(v, pars)) for k, v in o.items()])
    if isinstance(o, (list, tuple)):
        return (type(o).__name__, [_checkpoint_tree(v, pars) for v in o])
    return (type(o).__name__, o)


def _tree_differences(a, b, path, out):
    if type(a) is not type(b):
        out.append((path, type(a).__name__, type(b).__name__))
    elif isinstance(a, (tuple, list)):
        if len(a) != len(b):
            out.append((path, "length", len(a), len(b)))
        for i, (x, y) in enumerate(zip(a, b)):
            _tree_differences(x, y, "%s/%s" % (path, x[0] if isinstance(x, tuple) and x and isinstance(x[0], str) else i), out)
    elif isinstance(a, np.ndarray):
        if a.shape != b.shape or a.dtype != b.dtype or not np.array_equal(a, b, equal_nan=True):
            out.append((path, "array", a.shape, b.shape, a.dtype, b.dtype))
    elif a != b:
        out.append((path, a, b))


def test_written_checkpoints_are_what_the_reference_writes():
    """SURVEY 8f-4, the other direction.  A model read from a file of the reference and written back in the reference's format
    (compat.dump_reference_model, no reference installed) has the same object tree as the reference's own file: the same classes under the
    same module names, the same attributes in the same order, the same tensors (data, the dense identity, the quadrature nodes) and arrays,
    masks, fitted transformers, bounds, train flags, pegging and history -- bit for bit."""
    pytest.importorskip("torch")
    import io
    from mogptk_amd import compat
    fx = load("checkpoints.npz")
    for tag in WRITER_TAGS:
        raw = fx[tag + "_file"].tobytes()
        written = compat.dump_reference_model(compat.load_reference_model(raw))
        assert compat.is_reference_checkpoint(written)
        theirs = _checkpoint_tree(compat._Unpickler(io.BytesIO(raw)).load(), {})
        ours = _checkpoint_tree(compat._Unpickler(io.BytesIO(written)).load(), {})
        out = []
        _tree_differences(theirs, ours, tag, out)
        assert not out, out[:5]


def test_the_writer_says_what_it_does_not_cover(tmp_path):
    pytest.importorskip("torch")
    fx = load("checkpoints.npz")
    from mogptk_amd import compat
    m = compat.load_reference_model(fx["snelson_file"].tobytes())
    (tmp_path / "keep.npy").write_bytes(b"previous file")
    with pytest.raises(NotImplementedError, match="Snelson"):
        m.save(str(tmp_path / "keep"), reference=True)
    assert (tmp_path / "keep.npy").read_bytes() == b"previous file"


@pytest.mark.skipif(not os.path.isdir("/root/reference/mogptk"), reason="needs the reference itself (build container only)")
def test_the_reference_reads_written_checkpoints(tmp_path):
    """the reference's own LoadModel (mogptk/model.py:62-74), in a process of its own, reads the files this package writes and computes the
    loss and the predictions recorded for its own files in checkpoints.npz"""
    pytest.importorskip("torch")
    import subprocess
    import sys
    from mogptk_amd import compat
    fx = load("checkpoints.npz")
    for tag in WRITER_TAGS:
        (tmp_path / ("w_%s.npy" % tag)).write_bytes(compat.dump_reference_model(compat.load_reference_model(fx[tag + "_file"].tobytes())))
    script = """
import sys, types, json
ip, disp = types.ModuleType("IPython"), types.ModuleType("IPython.display")
disp.display = lambda *a, **k: None; disp.HTML = lambda s: s; ip.display = disp
sys.modules["IPython"] = ip; sys.modules["IPython.display"] = disp
sys.path.insert(0, "/root/reference")
import numpy as np, mogptk
out = {}
for tag in sys.argv[2:]:
    m = mogptk.LoadModel(sys.argv[1] + "/w_" + tag)
    loss = float(m.loss())
    X, mu, lower, upper = m.predict(transformed=False)
    m.train(method="Adam", lr=0.01, iters=2, verbose=False)          # and it trains on
    out[tag] = {"cls": type(m).__module__ + "." + type(m).__name__, "loss": loss, "mu": np.concatenate([np.asarray(v).reshape(-1) for v in mu]).tolist(),
                "upper": np.concatenate([np.asarray(v).reshape(-1) for v in upper]).tolist(), "iters": int(m.iters)}
print("RESULT " + json.dumps(out))
"""
    r = subprocess.run([sys.executable, "-c", script, str(tmp_path)] + list(WRITER_TAGS), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    import json
    got = json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
    for tag in WRITER_TAGS:
        g = got[tag]
        assert g["cls"].startswith("mogptk.models.")
        assert abs(g["loss"] - float(fx[tag + "_loss"])) <= 1e-12 * max(1.0, abs(float(fx[tag + "_loss"]))), tag
        assert np.max(np.abs(np.array(g["mu"]) - fx[tag + "_mu"])) <= 1e-10 * max(1.0, np.max(np.abs(fx[tag + "_mu"]))), tag
        assert np.max(np.abs(np.array(g["upper"]) - fx[tag + "_upper"])) <= 1e-10 * max(1.0, np.max(np.abs(fx[tag + "_upper"]))), tag
        assert g["iters"] == int(fx[tag + "_history"][0]) + 2


def test_written_checkpoint_carries_observation_errors_as_the_reference_keeps_them(tmp_path):
    """a model with per-point error bars (Y_err -> Exact's data_variance): the written file holds the N x N diagonal matrix the reference's
    constructor builds (gpr/model.py:423) -- its LML adds the attribute to Kff as it is (:442) --, the reference computes the loss of the
    numpy oracle with those variances on the diagonal, and this package's loader turns the matrix back into the vector"""
    pytest.importorskip("torch")
    import subprocess
    import sys
    import json
    from mogptk_amd import compat
    import mogptk_amd
    rng = np.random.default_rng(5)
    x = np.sort(rng.uniform(0, 10, 24))
    chans = [mogptk_amd.Data(x, np.sin(x + c) + 0.1 * rng.standard_normal(24), Y_err=0.05 + 0.1 * rng.random(24), name="c%d" % c) for c in range(2)]
    m = mogptk_amd.MOSM(mogptk_amd.DataSet(chans), Q=2)
    m.gpr.kernel.mean.assign(0.05 + 0.2 * rng.random((2, 2, 1)))
    dv = np.asarray(m.gpr.data_variance, dtype=np.float64)
    assert dv.shape == (48,) and np.allclose(dv, np.concatenate([c.Y_err for c in chans]) ** 2)
    raw = compat.dump_reference_model(m)
    (tmp_path / "w_err.npy").write_bytes(raw)
    back = compat.load_reference_model(raw)
    assert np.asarray(back.gpr.data_variance).shape == (48,) and np.array_equal(np.asarray(back.gpr.data_variance), dv)
    script = """
import sys, types, json
ip, disp = types.ModuleType("IPython"), types.ModuleType("IPython.display")
disp.display = lambda *a, **k: None; disp.HTML = lambda s: s; ip.display = disp
sys.modules["IPython"] = ip; sys.modules["IPython.display"] = disp
sys.path.insert(0, "/root/reference")
import numpy as np, mogptk
m = mogptk.LoadModel(sys.argv[1] + "/w_err")
dv = m.gpr.data_variance
print("RESULT " + json.dumps({"shape": list(dv.shape), "diag": dv.diagonal().tolist(), "off": float((dv - dv.diagonal().diagflat()).abs().max()), "lml": float(m.gpr.log_marginal_likelihood())}))
"""
    if not os.path.isdir("/root/reference"):
        pytest.skip("the reference is only present in the build container")
    r = subprocess.run([sys.executable, "-c", script, str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    got = json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
    assert got["shape"] == [48, 48] and got["off"] == 0.0 and np.allclose(got["diag"], dv, rtol=0, atol=0)
    # the same number from the numpy oracle with the variances on the diagonal
    X = np.asarray(m.gpr.X, dtype=np.float64)
    K = gram_from_table(np.asarray(m.gpr.kernel._spectral_terms(1)), X)
    Kn = K + np.diag(m.gpr._noise_var()[np.asarray(m.gpr.X)[:, 0].astype(int)]) + np.diag(dv)
    Kj = Kn + m.gpr.jitter * np.mean(np.diag(Kn)) * np.eye(48)
    L = np.linalg.cholesky(Kj)
    y = np.reshape(m.gpr.y, -1)
    z = np.linalg.solve(L, y)
    lml = -0.5 * 48 * np.log(2 * np.pi) - np.sum(np.log(np.diag(L))) - 0.5 * z @ z
    assert abs(got["lml"] - lml) <= 1e-10 * max(1.0, abs(lml))


def test_reference_checkpoints_load_without_the_reference(tmp_path):
    pytest.importorskip("torch")
    import sys
    assert "mogptk" not in sys.modules
    check_reference_checkpoints(tmp_path)


# ---- the Snelson (FITC) model, pinned on the reference (gpr/model.py:485-576) -----------------------------------------
def check_snelson(tol_lml=1e-9, tol_grad=1e-7, tol_pred=1e-8):
    fx = load("snelson.npz")
    for n in range(int(fx["ncases"])):
        pre = "c%d_" % n
        C, Q, D, _ = [int(v) for v in fx[pre + "meta"]]
        fp = fixture_params(fx, pre)
        k = gpr.MultiOutputSpectralMixtureKernel(Q=Q, output_dims=C, input_dims=D)
        var = fx[pre + "variance"]
        m = gpr.Snelson(k, fx[pre + "X"], fx[pre + "y"], Z=fx[pre + "Z"], variance=(var if var.ndim else float(var)), jitter=float(fx[pre + "jitter"]))
        assert [p._name.split(".")[-1] for p in m.parameters()] == [f["name"].split(".")[-1] for f in fp]
        load_raw(m.parameters(), fp)
        lml, ref = float(m.log_marginal_likelihood()), float(fx[pre + "lml"])
        assert abs(lml - ref) < tol_lml * max(1.0, abs(ref)), (n, lml, ref)
        loss, ref = float(m.loss()), float(fx[pre + "loss"])
        assert abs(loss - ref) < tol_lml * max(1.0, abs(ref)), (n, loss, ref)
        for p, f in zip(m.parameters(), fp):
            if f["grad"] is None:
                assert p.grad is None, p._name
            else:
                assert np.max(np.abs(p.grad - f["grad"])) <= tol_grad * max(1.0, np.max(np.abs(f["grad"]))), (n, p._name, p.grad, f["grad"])
        assert np.all(m.Z.grad[:, 0] == 0.0)
        mu, var_p = m.predict_f(fx[pre + "Xs"])
        assert relerr(mu, fx[pre + "mu"]) < tol_pred and np.max(np.abs(var_p - fx[pre + "var"])) < tol_pred, n


def test_snelson_matches_reference():
    check_snelson()


def test_snelson_through_the_model_wrapper():
    t = np.linspace(0, 10, 40)
    ds = mogptk_amd.DataSet(t, [np.sin(t), np.cos(t)])
    m = mogptk_amd.MOSM(ds, Q=2, inference=mogptk_amd.Snelson(inducing_points=5))
    assert type(m.gpr).__name__ == "Snelson" and m.gpr.Z().shape == (10, 2)          # 5 per channel, like the reference (quirk Q5)
    assert m.gpr.likelihood.scale().shape == (2,)                                      # variance None -> one per channel (model.py:114-118)
    m.gpr.kernel.mean.assign(np.full((2, 2, 1), 0.1))
    losses, _ = m.train("Adam", iters=3, lr=0.05)
    assert losses.shape == (4,) and np.all(np.isfinite(losses))
    _, mu, lower, upper = m.predict(transformed=False)
    assert all(np.all(np.isfinite(v)) for v in mu) and all(np.all(lo <= up) for lo, up in zip(lower, upper))


# ---- the Hensman models with the Gaussian likelihood, pinned on the reference (gpr/model.py:767-886) -------------------
def check_hensman(tol_elbo=1e-9, tol_grad=1e-7, tol_pred=1e-8):
    fx = load("hensman.npz")
    for n in range(int(fx["ncases"])):
        pre = "c%d_" % n
        C, Q, D, _ = [int(v) for v in fx[pre + "meta"]]
        fp = fixture_params(fx, pre)
        sparse = bool(fx[pre + "sparse"])
        k = gpr.MultiOutputSpectralMixtureKernel(Q=Q, output_dims=C, input_dims=D)
        lik = gpr.GaussianLikelihood(1.0)
        if sparse:
            m = gpr.SparseHensman(k, fx[pre + "X"], fx[pre + "y"], Z=fx[pre + "Z"], likelihood=lik, jitter=float(fx[pre + "jitter"]))
        else:
            m = gpr.Hensman(k, fx[pre + "X"], fx[pre + "y"], likelihood=lik, jitter=float(fx[pre + "jitter"]))
        assert [p._name.split(".")[-1] for p in m.parameters()] == [f["name"].split(".")[-1] for f in fp]
        load_raw(m.parameters(), fp)
        te, tg, tp = tol_elbo, tol_grad, tol_pred
        elbo, ref = float(m.log_marginal_likelihood()), float(fx[pre + "elbo"])
        assert abs(elbo - ref) < te * max(1.0, abs(ref)), (n, elbo, ref)
        loss, ref = float(m.loss()), float(fx[pre + "loss"])
        assert abs(loss - ref) < te * max(1.0, abs(ref)), (n, loss, ref)
        for p, f in zip(m.parameters(), fp):
            if f["grad"] is None:
                assert p.grad is None, (n, p._name)
            else:
                assert p.grad is not None, (n, p._name)
                assert np.max(np.abs(p.grad - f["grad"])) <= tg * max(1.0, np.max(np.abs(f["grad"]))), (n, p._name, np.max(np.abs(p.grad - f["grad"])))
        mu, var_p = m.predict_f(fx[pre + "Xs"])
        assert relerr(mu, fx[pre + "mu"]) < tp and np.max(np.abs(var_p - fx[pre + "var"])) < tp * max(1.0, np.max(np.abs(fx[pre + "var"]))), n


def test_hensman_matches_reference():
    check_hensman()


def check_hensman_with_enveloped_terms(tol_elbo=1e-9, tol_grad=1e-7, tol_pred=1e-8):
    """SparseHensman (Gaussian, Student-t) and the dense Hensman model under the enveloped MOHSM kernel (reference gpr/multioutput.py:340-395
    under gpr/model.py:767-886): K_diag per training point inside var_n with the likelihood's d/dvar_n going back through it, K_uu's jitter
    through the inducing inputs -- against the reference's autograd"""
    fx = load("hensman_mohsm.npz")
    for n in range(int(fx["ncases"])):
        pre = "c%d_" % n
        C, Q, D, _ = [int(v) for v in fx[pre + "meta"]]
        fp = fixture_params(fx, pre)
        sparse = bool(fx[pre + "sparse"])
        k = gpr.MixtureKernel(gpr.MultiOutputHarmonizableSpectralKernel(output_dims=C, input_dims=D), Q)
        lik = gpr.GaussianLikelihood(1.0) if str(fx[pre + "lik"]) == "gaussian" else gpr.StudentTLikelihood(dof=4, scale=1.0)
        if sparse:
            m = gpr.SparseHensman(k, fx[pre + "X"], fx[pre + "y"], Z=[int(z) for z in fx[pre + "Zspec"]], likelihood=lik, jitter=float(fx[pre + "jitter"]))
        else:
            m = gpr.Hensman(k, fx[pre + "X"], fx[pre + "y"], likelihood=lik, jitter=float(fx[pre + "jitter"]))
        assert [p._name.split(".")[-1] for p in m.parameters()] == [f["name"].split(".")[-1] for f in fp]
        load_raw(m.parameters(), fp)
        elbo, ref = float(m.log_marginal_likelihood()), float(fx[pre + "elbo"])
        assert abs(elbo - ref) < tol_elbo * max(1.0, abs(ref)), (n, elbo, ref)
        loss, ref = float(m.loss()), float(fx[pre + "loss"])
        assert abs(loss - ref) < tol_elbo * max(1.0, abs(ref)), (n, loss, ref)
        for p, f in zip(m.parameters(), fp):
            if f["grad"] is None:
                assert p.grad is None, (n, p._name)
            else:
                assert p.grad is not None, (n, p._name)
                assert np.max(np.abs(p.grad - f["grad"])) <= tol_grad * max(1.0, np.max(np.abs(f["grad"]))), (n, p._name, np.max(np.abs(p.grad - f["grad"])))
        mu, var_p = m.predict_f(fx[pre + "Xs"])
        assert relerr(mu, fx[pre + "mu"]) < tol_pred and np.max(np.abs(var_p - fx[pre + "var"])) < tol_pred * max(1.0, np.max(np.abs(fx[pre + "var"]))), n


def test_hensman_with_enveloped_terms_matches_reference():
    check_hensman_with_enveloped_terms()


def check_oa(tol_elbo=1e-9, tol_grad=1e-7, tol_pred=1e-8):
    fx = load("oa.npz")
    for n in range(int(fx["ncases"])):
        pre = "c%d_" % n
        C, Q, D, _ = [int(v) for v in fx[pre + "meta"]]
        fp = fixture_params(fx, pre)
        k = gpr.MultiOutputSpectralMixtureKernel(Q=Q, output_dims=C, input_dims=D)
        m = gpr.OpperArchambeau(k, fx[pre + "X"], fx[pre + "y"], likelihood=gpr.GaussianLikelihood(1.0), jitter=1e-6)
        assert [p._name.split(".")[-1] for p in m.parameters()] == [f["name"].split(".")[-1] for f in fp]
        load_raw(m.parameters(), fp)
        elbo, ref = float(m.log_marginal_likelihood()), float(fx[pre + "elbo"])
        assert abs(elbo - ref) < tol_elbo * max(1.0, abs(ref)), (n, elbo, ref)
        loss, ref = float(m.loss()), float(fx[pre + "loss"])
        assert abs(loss - ref) < tol_elbo * max(1.0, abs(ref)), (n, loss, ref)
        for p, f in zip(m.parameters(), fp):
            if f["grad"] is None:
                assert p.grad is None, (n, p._name)
            else:
                assert p.grad is not None, (n, p._name)
                assert np.max(np.abs(p.grad - f["grad"])) <= tol_grad * max(1.0, np.max(np.abs(f["grad"]))), (n, p._name, np.max(np.abs(p.grad - f["grad"])))
        mu, var_p = m.predict_f(fx[pre + "Xs"])
        assert relerr(mu, fx[pre + "mu"]) < tol_pred and np.max(np.abs(var_p - fx[pre + "var"])) < tol_pred * max(1.0, np.max(np.abs(fx[pre + "var"]))), n
        mu, cov = m.predict_f(fx[pre + "Xs"], full=True)
        assert relerr(mu, fx[pre + "mu"]) < tol_pred and np.max(np.abs(cov - fx[pre + "cov"])) < tol_pred * max(1.0, np.max(np.abs(fx[pre + "cov"]))), n


def test_opper_archambeau_matches_reference():
    check_oa()


def test_opper_archambeau_through_the_model_wrapper():
    np.random.seed(20251001)          # the wrapper draws its initial weights / means from numpy's global generator (as the reference does from torch's):
    t = np.linspace(0, 10, 30)        # three Adam steps from an unlucky draw need not lower the loss
    ds = mogptk_amd.DataSet(t, [np.sin(t), np.cos(t)])
    m = mogptk_amd.MOSM(ds, Q=1, inference=mogptk_amd.OpperArchambeau())
    assert type(m.gpr).__name__ == "OpperArchambeau" and m.gpr.q_nu().shape == (60, 1) and m.gpr.q_lambda().shape == (60, 1)
    losses, _ = m.train("Adam", iters=3, lr=0.05)
    assert losses.shape == (4,) and np.all(np.isfinite(losses)) and losses[-1] < losses[0]
    _, mu, lower, upper = m.predict(transformed=False)
    assert all(np.all(np.isfinite(v)) for v in mu)


def check_likelihood_models(tol_loss=1e-9, tol_grad=1e-7, tol_pred=1e-8):
    """likelihoods.npz: SparseHensman / Hensman / OpperArchambeau with non-Gaussian likelihoods, pinned on the reference's loss, autograd
    gradients of every parameter (likelihood parameters included), predict_f and the mean of predict_y"""
    fx = load("likelihoods.npz")
    L = gpr
    for tag in [str(t) for t in fx["model_tags"]]:
        pre = tag + "_"
        C, Q, D, _ = [int(v) for v in fx[pre + "meta"]]
        lik = {"svgp_studentt": lambda: L.StudentTLikelihood(dof=4, scale=0.4),
               "svgp_multi": lambda: L.MultiOutputLikelihood(L.PoissonLikelihood(), L.GaussianLikelihood(0.3)),
               "oa_bernoulli": lambda: L.BernoulliLikelihood(),
               "hensman_laplace": lambda: L.LaplaceLikelihood(scale=0.3),
               "oa_gamma": lambda: L.GammaLikelihood(shape=2.0)}[tag]()
        k = gpr.MultiOutputSpectralMixtureKernel(Q=Q, output_dims=C, input_dims=D)
        X, y = fx[pre + "X"], fx[pre + "y"]
        if tag.startswith("svgp"):
            m = gpr.SparseHensman(k, X, y, Z=fx[pre + "Z"], likelihood=lik, jitter=1e-6)
        elif tag.startswith("hensman"):
            m = gpr.Hensman(k, X, y, likelihood=lik, jitter=1e-6)
        else:
            m = gpr.OpperArchambeau(k, X, y, likelihood=lik, jitter=1e-6)
        fp = fixture_params(fx, pre)
        assert [p._name for p in m.parameters()] == [f["name"] for f in fp], tag
        load_raw(m.parameters(), fp)
        loss, ref = float(m.loss()), float(fx[pre + "loss"])
        assert abs(loss - ref) < tol_loss * max(1.0, abs(ref)), (tag, loss, ref)
        for p, f in zip(m.parameters(), fp):
            if f["grad"] is None:
                assert p.grad is None, (tag, p._name)
            else:
                assert p.grad is not None, (tag, p._name)
                assert np.max(np.abs(p.grad - f["grad"])) <= tol_grad * max(1.0, np.max(np.abs(f["grad"]))), (tag, p._name, np.max(np.abs(p.grad - f["grad"])))
        mu, var_p = m.predict_f(fx[pre + "Xs"])
        assert relerr(mu, fx[pre + "mu_f"]) < tol_pred and np.max(np.abs(var_p - fx[pre + "var_f"])) < tol_pred * max(1.0, np.max(np.abs(fx[pre + "var_f"]))), tag
        assert relerr(np.reshape(m.predict_y(fx[pre + "Xs"]), -1), fx[pre + "mu_y"]) < tol_pred, tag


def test_variational_models_with_non_gaussian_likelihoods_match_reference():
    check_likelihood_models()


def test_non_gaussian_likelihood_through_the_model_wrapper():
    rng = np.random.default_rng(5)
    t = np.linspace(0, 10, 40)
    counts = rng.poisson(np.exp(0.8 * np.sin(t))).astype(np.float64)
    ds = mogptk_amd.DataSet(t, [counts, np.cos(t)])
    lik = gpr.MultiOutputLikelihood(gpr.PoissonLikelihood(), gpr.StudentTLikelihood(dof=4, scale=0.3))
    m = mogptk_amd.MOSM(ds, Q=1, inference=mogptk_amd.Hensman(inducing_points=6, likelihood=lik))
    losses, _ = m.train("Adam", iters=5, lr=0.05)
    assert losses.shape == (6,) and np.all(np.isfinite(losses)) and losses[-1] < losses[0]
    _, mu, lower, upper = m.predict(transformed=False)
    assert all(np.all(np.isfinite(v)) for v in mu) and np.all(np.asarray(mu[0]) > 0)          # the Poisson channel predicts a rate
    m.save("/tmp/_mogp_lik_model")
    m2 = mogptk_amd.LoadModel("/tmp/_mogp_lik_model")
    assert abs(m2.loss() - m.loss()) < 1e-12 * abs(m.loss()) and m2.gpr.likelihood.name() == "[PoissonLikelihood,StudentTLikelihood]"


def check_samples(tol=1e-8):
    """samples.npz: sample_f of a multi-output exact model and Model.sample of a single-output one, drawn by the reference under a fixed torch
    seed; this package draws from the same generator with the same calls, so the samples are the same numbers"""
    torch = pytest.importorskip("torch")
    fx = load("samples.npz")
    k = gpr.MultiOutputSpectralMixtureKernel(Q=2, output_dims=2, input_dims=1)
    m = gpr.Exact(k, fx["X"], fx["y"], variance=[0.2, 0.3], jitter=1e-8)
    load_raw(m.parameters(), fixture_params(fx, "exact_"))
    torch.manual_seed(99)
    f1 = m.sample_f(fx["Z"])
    torch.manual_seed(99)
    f4 = m.sample_f(fx["Z"], n=4)
    assert f1.shape == fx["f_single"].shape and f4.shape == (4, 9)
    assert np.max(np.abs(f1 - fx["f_single"])) < tol and np.max(np.abs(f4 - fx["f_many"])) < tol
    with pytest.raises(TypeError):
        m.sample_f(fx["Z"], prior=True)                     # the reference calls a mean function that is not there
    d = mogptk_amd.Data(fx["sm_t"], fx["sm_Y"])
    d.transform(mogptk_amd.TransformDetrend(degree=1))
    d.set_prediction_data(np.linspace(0, 11, 8))
    ms = mogptk_amd.SM(mogptk_amd.DataSet(d), Q=2)
    load_raw(ms.gpr.parameters(), fixture_params(fx, "sm_"))
    torch.manual_seed(7)
    s1 = np.asarray(ms.sample())
    torch.manual_seed(7)
    s2 = np.asarray(ms.sample(transformed=True))
    assert np.max(np.abs(s1 - fx["sm_sample"])) < tol and np.max(np.abs(s2 - fx["sm_sample_transformed"])) < tol


def test_posterior_samples_match_reference():
    check_samples()


def check_sparse_cov(tol=1e-8, tol_sample=1e-6):
    """sparse_cov.npz: predict_f(full=True) of Titsias, SparseHensman and Hensman against the reference, and a posterior sample of f drawn from
    it under the reference's seed"""
    torch = pytest.importorskip("torch")
    fx = load("sparse_cov.npz")
    X, y, Xs, Z = fx["X"], fx["y"], fx["Xs"], fx["Z"]
    for tag in ("titsias", "sparse_hensman", "hensman"):
        k = gpr.MultiOutputSpectralMixtureKernel(Q=2, output_dims=2, input_dims=1)
        if tag == "titsias":
            m = gpr.Titsias(k, X, y, Z=Z, variance=0.09, jitter=1e-6)
        elif tag == "sparse_hensman":
            m = gpr.SparseHensman(k, X, y, Z=Z, likelihood=gpr.GaussianLikelihood(0.3), jitter=1e-6)
        else:
            m = gpr.Hensman(k, X, y, likelihood=gpr.GaussianLikelihood(0.3), jitter=1e-6)
        load_raw(m.parameters(), fixture_params(fx, tag + "_"))
        mu, cov = m.predict_f(Xs, full=True)
        assert cov.shape == (11, 11)
        assert relerr(mu, fx[tag + "_mu"]) < tol and np.max(np.abs(cov - fx[tag + "_cov"])) < tol * max(1.0, np.max(np.abs(fx[tag + "_cov"]))), tag
        mu1, var = m.predict_f(Xs)
        assert np.max(np.abs(np.reshape(var, -1) - np.diagonal(cov))) < tol, tag
        torch.manual_seed(5)
        assert np.max(np.abs(m.sample_f(Xs) - fx[tag + "_sample"])) < tol_sample, tag


def test_sparse_models_full_covariance_matches_reference():
    check_sparse_cov()


def test_hensman_through_the_model_wrapper():
    t = np.linspace(0, 10, 30)
    ds = mogptk_amd.DataSet(t, [np.sin(t), np.cos(t)])
    for inducing in (4, None):                                                          # sparse (4 per channel) and the non-sparse default
        m = mogptk_amd.MOSM(ds, Q=1, inference=mogptk_amd.Hensman(inducing_points=inducing))
        assert type(m.gpr).__name__ == ("SparseHensman" if inducing else "Hensman")
        n = 8 if inducing else 60
        assert m.gpr.q_mu().shape == (n, 1) and m.gpr.q_sqrt().shape == (n, n) and m.gpr.q_sqrt.num_parameters == n * (n + 1) // 2
        losses, _ = m.train("Adam", iters=3, lr=0.05)
        assert losses.shape == (4,) and np.all(np.isfinite(losses)) and losses[-1] < losses[0]
        _, mu, lower, upper = m.predict(transformed=False)
        assert all(np.all(np.isfinite(v)) for v in mu)


def test_reference_checkpoint_loader_refuses_names_a_checkpoint_has_no_use_for(tmp_path):
    """a "reference checkpoint" that names os.system (the reference's plain pickle.load would call it) is refused by class resolution"""
    import pickle
    from mogptk_amd import compat

    class Evil:
        def __reduce__(self):
            import os
            return (os.system, ("true",))
    raw = pickle.dumps({"model": Evil(), "tag": "mogptk.model"})          # contains b"mogptk." -> routed through the reference loader
    assert compat.is_reference_checkpoint(raw)
    import io
    with pytest.raises(pickle.UnpicklingError):
        compat._Unpickler(io.BytesIO(raw)).load()


def test_checkpoint_loaders_refuse_dotted_names_and_module_prefix_tricks(tmp_path):
    """round 3's allow list matched whole modules by prefix, and pickle protocol 4 resolves dotted names attribute by attribute: both
    GLOBAL('torch.serialization', 'os.getcwd') and torch._utils._import_dotted_name('os.getcwd') + REDUCE got through.  Now only exact
    (module, name) pairs resolve -- for the reference's checkpoints and for this package's own -- and a native checkpoint still round-trips."""
    import io, pickle, pickletools
    from mogptk_amd import compat

    def stack_global(module, name, args=b")"):
        # protocol 4: module, name as short unicode strings, STACK_GLOBAL, empty tuple (or `args`), REDUCE, STOP
        def u(s):
            b = s.encode()
            return b"\x8c" + bytes([len(b)]) + b
        return b"\x80\x04" + u(module) + u(name) + b"\x93" + args + b"R."

    payloads = [
        stack_global("torch.serialization", "os.getcwd"),
        stack_global("torch._utils", "_import_dotted_name", b"\x8c\x09os.getcwd\x85"),
        stack_global("torch.nn.modules.module", "Module"),
        stack_global("mogptk_amd.model", "os.getcwd"),
        stack_global("mogptk_amd.model", "pickle"),                 # reachable through the package, not defined in it
        stack_global("builtins", "eval", b"\x8c\x031+1\x85"),
    ]
    for raw in payloads:
        pickletools.dis(raw, out=io.StringIO())                      # well-formed pickles
        for cls in (compat._Unpickler, compat._NativeUnpickler):
            with pytest.raises(pickle.UnpicklingError):
                cls(io.BytesIO(raw)).load()
    # a model of this package still saves and loads through the restricted loader
    import mogptk_amd
    rng = np.random.default_rng(0)
    x = np.sort(rng.uniform(0, 10, 40))
    ds = mogptk_amd.DataSet(mogptk_amd.Data(x, np.sin(x)), mogptk_amd.Data(x, np.cos(x)))
    m = mogptk_amd.MOSM(ds, Q=2)
    path = str(tmp_path / "native")
    m.save(path)
    m2 = mogptk_amd.LoadModel(path)
    for a, b in zip(m.gpr.parameters(), m2.gpr.parameters()):
        assert np.array_equal(a.data, b.data)


class _UserMean:
    """a caller's own mean function: lives in the test module, not in the package"""

    def __init__(self, slope):
        self.slope = slope

    def __call__(self, X):
        return self.slope * np.asarray(X)[:, -1]


class _Outer:
    class NestedMean(_UserMean):
        pass


def test_checkpoint_with_user_code_needs_an_opt_in(tmp_path):
    """a model saved with the caller's own mean function names the caller's module.  The restricted loader refuses it with a
    message that names the opt-in; LoadModel(allow=[...]) admits exactly that class (nested classes too), trusted=True is plain pickle.load;
    a package merely NAMED like this one ('mogptk_amd_x') is not this one."""
    import io
    import pickle
    import mogptk_amd
    from mogptk_amd import compat
    rng = np.random.default_rng(1)
    x = np.sort(rng.uniform(0, 10, 30))
    for mean in (_UserMean(0.3), _Outer.NestedMean(0.3)):
        m = mogptk_amd.SM(mogptk_amd.Data(x, np.sin(x) + 0.3 * x), Q=1, mean=mean)
        path = str(tmp_path / "user_mean")
        m.save(path)
        with pytest.raises(pickle.UnpicklingError) as e:
            mogptk_amd.LoadModel(path)
        assert "allow=" in str(e.value) and "trusted=True" in str(e.value) and type(mean).__name__ in str(e.value)
        for kw in (dict(allow=[type(mean)]), dict(trusted=True)):
            m2 = mogptk_amd.LoadModel(path, **kw)
            assert type(m2.gpr.mean) is type(mean) and m2.gpr.mean.slope == 0.3
            for a, b in zip(m.gpr.parameters(), m2.gpr.parameters()):
                assert np.array_equal(a.data, b.data)
    with pytest.raises(pickle.UnpicklingError):                     # allow= admits the named object only
        mogptk_amd.LoadModel(path, allow=[_UserMean])
    assert not compat._in_package("mogptk_amd_x") and compat._in_package("mogptk_amd.gpr.kernel") and compat._in_package("mogptk_amd")
    # a function of the package that is not on the short list is not callable from a checkpoint
    raw = pickle.dumps(compat.is_reference_checkpoint)
    with pytest.raises(pickle.UnpicklingError):
        compat._NativeUnpickler(io.BytesIO(raw)).load()


# ---- the host side of the exact path's conditioning check (no device: a handle that only reports an estimate) ------------------------
def test_ill_conditioned_models_warn_once_and_switch_to_the_backward_stable_form():
    import warnings
    from oracle.table_model import TableDevice

    class Reporting(TableDevice):
        """the numpy twin plus the two entry points of the device handle the check uses; the estimate is dialled by the test"""
        estimate = 1.0

        def __init__(self, *a):
            super().__init__(*a)
            self.accurate, self.evals = False, []

        def condition_estimate(self):
            return type(self).estimate

        def set_accurate(self, on):
            self.accurate = bool(on)

        def eval(self, *a, **k):
            self.evals.append(self.accurate)
            return super().eval(*a, **k)

    rng = np.random.default_rng(3)
    x = np.sort(rng.uniform(0, 10, 40))
    X = np.c_[np.repeat([0, 1], 20), np.r_[x[:20], x[20:]]]
    y = np.sin(X[:, 1]) + 0.1 * rng.standard_normal(40)
    k = gpr.MultiOutputSpectralMixtureKernel(Q=1, output_dims=2)
    old = L.ExactHandle
    L.ExactHandle = Reporting
    try:
        m = gpr.Exact(k, X, y, variance=0.04)
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            Reporting.estimate = 5e3
            l0 = m.loss()
            assert not w and m._handle.evals == [False] and not getattr(m._handle, "accurate_mode", False)
            Reporting.estimate = 3e6                       # the factor's diagonal says: ill-conditioned
            l1 = m.loss()
            assert len(w) == 1 and issubclass(w[0].category, RuntimeWarning) and "ill-conditioned" in str(w[0].message)
            assert m._handle.accurate_mode and m._handle.evals == [False, False, True]            # the evaluation was repeated in the other form
            m.loss()
            assert len(w) == 1 and m._handle.evals[-1] is True and len(m._handle.evals) == 4      # stays there, says it once
            m.log_marginal_likelihood()                   # (the LML alone does not take part)
            Reporting.estimate = 5e4                       # better, but not by the factor of ten that switches back
            m.loss()
            assert m._handle.accurate_mode
            Reporting.estimate = 5e3
            m.loss()
            assert not m._handle.accurate_mode and m._handle.accurate is False
            n = len(m._handle.evals)
            m.loss()
            assert m._handle.evals[n:] == [False]
        assert l0 == l1                                    # (the twin computes the same thing either way)
        # predict_f takes part in the same way: an ill-conditioned system found by a prediction is said once and predicted again in the refined form
        m3 = gpr.Exact(gpr.MultiOutputSpectralMixtureKernel(Q=1, output_dims=2), X, y, variance=0.04)
        calls = []
        orig = Reporting.predict
        Reporting.predict = lambda self, *a, **k: (calls.append(self.accurate), orig(self, *a, **k))[1]
        try:
            with warnings.catch_warnings(record=True) as w:
                warnings.simplefilter("always")
                Reporting.estimate = 3e6
                mu1, _ = m3.predict_f(X[:5])
                mu2, _ = m3.predict_f(X[:5])
            assert len(w) == 1 and m3._handle.accurate_mode and calls == [False, True, True] and np.array_equal(mu1, mu2)
        finally:
            Reporting.predict = orig
        # the switch that only warns
        gpr.config.accurate_fallback = False
        m2 = gpr.Exact(gpr.MultiOutputSpectralMixtureKernel(Q=1, output_dims=2), X, y, variance=0.04)
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            Reporting.estimate = 3e6
            m2.loss(); m2.loss()
        assert len(w) == 1 and not getattr(m2._handle, "accurate_mode", False) and m2._handle.evals == [False, False]
    finally:
        gpr.config.accurate_fallback = True
        L.ExactHandle = old


# ---- the one Cholesky guard of gpr/model.py: every device call that factorises, loss() and predict_f() of all six models -----------------------
def _guard_models():
    rng = np.random.default_rng(5)
    x = np.sort(rng.uniform(0, 10, 12))
    X = np.c_[np.repeat([0, 1], 6), x]
    y = np.sin(x) + 0.1 * rng.standard_normal(12)
    k = lambda: gpr.MultiOutputSpectralMixtureKernel(Q=1, output_dims=2)
    return X, [gpr.Exact(k(), X, y, variance=0.04), gpr.Titsias(k(), X, y, Z=2, variance=0.04), gpr.Snelson(k(), X, y, Z=2, variance=0.04),
               gpr.OpperArchambeau(k(), X, y), gpr.SparseHensman(k(), X, y, Z=2), gpr.Hensman(k(), X, y)]


_GUARDED = {"Exact": ("eval", "predict"), "Titsias": ("titsias_eval", "titsias_predict"), "Snelson": ("snelson_eval", "snelson_predict"),
            "OpperArchambeau": ("oa_forward", "oa_predict"), "SparseHensman": ("svgp_forward", "svgp_forward"), "Hensman": ("svgp_forward", "svgp_forward")}


def test_not_positive_definite_becomes_cholesky_exception_in_every_model(monkeypatch, capsys):
    """the device reports MOGP_ENOTPD from the call loss() / predict_f() makes: CholeskyException(message, None, model) as the reference raises it
    (gpr/model.py:245-255), `ERROR:` on sys.__stdout__ and the parameter table printed; any other code passes through unchanged"""
    import io
    import sys
    X, models = _guard_models()
    assert [m.Z().shape[0] for m in models[1:3] + models[4:5]] == [4, 4, 4]
    code = [L.MOGP_ENOTPD]

    def fail(self, *a, **k):
        raise L.MogpError(code[0], "matrix is not positive definite at pivot 3")

    for m in models:
        for method, call in zip(_GUARDED[m.name()], (m.loss, lambda: m.predict_f(X[:3]))):
            real_out = io.StringIO()
            with monkeypatch.context() as mp:
                mp.setattr(TableDevice, method, fail)
                mp.setattr(sys, "__stdout__", real_out)
                capsys.readouterr()
                with pytest.raises(gpr.CholeskyException) as e:
                    call()
            assert str(e.value) == e.value.message == "matrix is not positive definite at pivot 3", (m.name(), method)
            assert e.value.model is m and e.value.K is None
            assert real_out.getvalue() == "ERROR: matrix is not positive definite at pivot 3\n"
            table = capsys.readouterr().out.splitlines()
            assert table[0].split() == ["Name", "Value"] and len(table) == 1 + len(list(m.parameters())), (m.name(), method, table)
    code[0] = L.MOGP_EINVAL
    with monkeypatch.context() as mp:
        mp.setattr(TableDevice, "titsias_predict", fail)
        with pytest.raises(L.MogpError) as e:
            models[1].predict_f(X[:3])
    assert e.value.code == L.MOGP_EINVAL and not isinstance(e.value, gpr.CholeskyException)
