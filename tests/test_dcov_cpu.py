"""
The joint posterior covariance of df/dx and slope draws without a device: the numpy twin (tests/dcov_twin.py) against the
reference-side goldens (tests/golden/dcov.npz, gen_dcov.py: double autograd through the reference's own kernel objects), and the host's part of
gpr.Exact.predict_df_cov, sample_df and Model.sample_derivative over the twin -- shapes, symmetry, the default call's bits, the refusals,
the draws.  Tolerance: test_deriv_cpu.TOL, 1e-9 relative to max(1, max |want|).
"""
import numpy as np
import pytest

import mogptk_amd
from mogptk_amd import gpr, _lib
from mogptk_amd.gpr.config import config
from mogptk_amd.gpr.kernel import deriv_diag

import deriv_cases
import dcov_twin
import deriv_twin
import kinds_sweep as ks
import test_deriv_gpu as tdg
from helpers import load
from kernel_family import err
from test_deriv_cpu import FX, TOL, NoDevice, _exact, model

DX = load("dcov.npz")


@pytest.mark.parametrize("case", list(deriv_cases.CASES))
def test_twin_matches_the_reference(case, monkeypatch):
    dcov_twin.install(monkeypatch)
    m, Xs = model(case)
    dmu, dcov = m.predict_df_cov(Xs)
    assert isinstance(m._handle, dcov_twin.DcovTableDevice)
    S, D = len(Xs), deriv_cases.CASES[case]["D"]
    assert dmu.shape == (S, D) and dcov.shape == (S, D, S, D) and dmu.dtype == dcov.dtype == config.dtype
    for name, got, want in (("dmu", dmu, FX[case + "__dmu"]), ("dcov", dcov, DX[case + "__dcov"])):
        e = err(got, want)
        print(case, name, e)
        assert e <= TOL, name


@pytest.mark.parametrize("case", ["mosm2", "trend", "mohsm", "linmean"])
def test_full_covariance_on_the_host(case, monkeypatch):
    """the default call before any full call, the full call, the default call again: the same bits; the full call's diagonal is dvar"""
    dcov_twin.install(monkeypatch)
    m, Xs = model(case)
    dmu0, dvar0 = m.predict_df(Xs)
    dmu, dcov = m.predict_df_cov(Xs)
    dmu1, dvar1 = m.predict_df(Xs)
    assert dmu0.tobytes() == dmu1.tobytes() and dvar0.tobytes() == dvar1.tobytes()
    S, D = dmu0.shape
    flat = dcov.reshape(S * D, S * D)
    assert np.array_equal(flat, flat.T)                      # symmetrised on the host
    assert err(dmu, dmu0) <= TOL
    assert err(np.diagonal(flat).reshape(S, D), dvar0) <= TOL


def test_the_full_call_is_one_device_call_without_kappa(monkeypatch):
    dcov_twin.install(monkeypatch)
    calls = []
    real = dcov_twin.DcovTableDevice.predict_grad
    monkeypatch.setattr(dcov_twin.DcovTableDevice, "predict_grad",
                        lambda self, nv, j, kap, X, **kw: (calls.append((kap, X.shape[0], kw.get("full"))), real(self, nv, j, kap, X, **kw))[1])
    m, Xs = model("sm3")
    m.PART_ROWS = 30                                          # chunks the default call, never the full one
    m.predict_df_cov(Xs)
    assert calls == [(None, 24, True)]


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, make, match", [
    ("matern12", lambda: gpr.MaternKernel(nu=0.5, input_dims=1), "Matern 1/2.*not differentiable"),
    ("white", lambda: gpr.AddKernel(gpr.SquaredExponentialKernel(input_dims=1), gpr.WhiteKernel(input_dims=1)), "white.*not differentiable"),
    ("gate", lambda: gpr.ChangePointsKernel([5.0], 1.0, gpr.SquaredExponentialKernel(input_dims=1), gpr.MaternKernel(nu=1.5, input_dims=1)), "gate.*yet"),
    ("function", lambda: gpr.AddKernel(gpr.FunctionKernel(lambda x: np.concatenate([x, x * x], axis=1), input_dims=1), gpr.SquaredExponentialKernel(input_dims=1)),
     "FunctionKernel.*yet"),
])
def test_rows_without_a_derivative_are_refused_by_name(name, make, match, monkeypatch):
    monkeypatch.setattr(_lib, "ExactHandle", NoDevice)        # before any device call
    m, Xs = _exact(make())
    for call in (lambda: m.predict_df_cov(Xs), lambda: m.sample_df(Xs)):
        with pytest.raises(NotImplementedError, match=match):
            call()


def test_the_twin_refuses_what_the_library_refuses(monkeypatch):
    dcov_twin.install(monkeypatch, "function")
    for kern in (gpr.MaternKernel(nu=0.5, input_dims=1), gpr.AddKernel(gpr.SquaredExponentialKernel(input_dims=1), gpr.WhiteKernel(input_dims=1))):
        m, Xs = _exact(kern)
        m.predict_f(Xs)
        with pytest.raises(_lib.MogpError) as e:
            m._handle.predict_grad(m._noise_var(), m.jitter, None, m.kernel._kernel_format(Xs), full=True)
        assert e.value.code == _lib.MOGP_EINVAL


def test_a_mean_that_is_not_affine_is_refused_by_name(monkeypatch):
    monkeypatch.setattr(_lib, "ExactHandle", NoDevice)

    class Wave(gpr.Mean):
        def mean(self, X):
            return np.sin(X[:, :1])

    m, Xs = _exact(gpr.SquaredExponentialKernel(input_dims=1), mean=Wave())
    with pytest.raises(NotImplementedError, match="Wave is not affine"):
        m.predict_df_cov(Xs)


def test_sharded_evaluation_is_refused_before_any_device_call(monkeypatch):
    monkeypatch.setattr(_lib, "ExactHandle", NoDevice)
    monkeypatch.setattr(config, "comm", type("Comm", (), dict(world=2, rank=0, force=False, native=True))(), raising=False)
    m = deriv_cases.exact(gpr, "ard")
    with pytest.raises(NotImplementedError, match="use_distributed"):
        m.predict_df_cov(deriv_cases.data("ard")[2])


def test_more_than_8192_stacked_rows_are_refused_before_any_device_call(monkeypatch):
    monkeypatch.setattr(_lib, "ExactHandle", NoDevice)
    m, _ = _exact(gpr.SquaredExponentialKernel(input_dims=1))
    assert gpr.Exact.GRAD_COV_ROWS == 8192
    with pytest.raises(ValueError, match="8192.*8193"):
        m.predict_df_cov(np.linspace(0.0, 10.0, 8193)[:, None])
    # and by the handle past the host
    dcov_twin.install(monkeypatch)
    m, Xs = _exact(gpr.SquaredExponentialKernel(input_dims=1))
    m.predict_f(Xs)
    with pytest.raises(_lib.MogpError) as e:
        m._handle.predict_grad(m._noise_var(), m.jitter, None, m.kernel._kernel_format(np.linspace(0.0, 10.0, 8193)[:, None]), full=True)
    assert e.value.code == _lib.MOGP_EINVAL and "8192" in str(e.value)


# ---- draws ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case, n", [("mosm2", 3), ("trend", None)])
def test_sample_df_is_the_seeded_normal(case, n, monkeypatch):
    import torch
    dcov_twin.install(monkeypatch)
    m, Xs = model(case)
    dmu, dcov = m.predict_df_cov(Xs)
    S, D = dmu.shape
    torch.manual_seed(31)
    got = m.sample_df(Xs, n=n)
    assert got.shape == ((S, D) if n is None else (n, S, D))
    cov = np.array(dcov, dtype=np.float64).reshape(S * D, S * D)
    cov += m.jitter * np.mean(np.diagonal(cov)) * np.eye(S * D)
    torch.manual_seed(31)
    eps = torch.empty((1 if n is None else n, S * D), dtype=torch.float64).normal_().numpy()
    chol = torch.linalg.cholesky(torch.tensor(cov)).numpy()   # torch's own factorisation, as MultivariateNormal takes it: cov is conditioned like 1 / jitter,
    want = (np.reshape(dmu, -1) + eps @ chol.T).reshape(-1, S, D)      # and two LAPACKs' factors may differ by eps * cond; what is left is the product's rounding
    assert err(got.reshape(-1, S, D), want) <= 1e-12


def test_model_sample_derivative_splits_per_channel(monkeypatch):
    import torch
    dcov_twin.install(monkeypatch)
    rng = np.random.default_rng(5)
    xa, xb = np.sort(rng.uniform(0, 10, 40)), np.sort(rng.uniform(0, 10, 30))
    ds = mogptk_amd.DataSet(mogptk_amd.Data(xa, np.sin(xa) + 0.1 * rng.standard_normal(40), name="a"),
                            mogptk_amd.Data(xb, np.cos(xb) + 0.1 * rng.standard_normal(30), name="b"))
    mm = mogptk_amd.Model(ds, gpr.MultiOutputSpectralMixtureKernel(Q=2, output_dims=2, input_dims=1), inference=mogptk_amd.Exact(variance=0.1))
    Xp = [np.linspace(0, 10, 12)[:, None], np.linspace(1, 9, 7)[:, None]]
    torch.manual_seed(9)
    X, draws = mm.sample_derivative(Xp, n=4)
    torch.manual_seed(9)
    flat = mm.gpr.sample_df(mm._to_kernel_format(X), n=4)
    assert [d.shape for d in draws] == [(4, 12, 1), (4, 7, 1)] and flat.shape == (4, 19, 1)
    assert np.array_equal(np.concatenate(draws, axis=1), flat)
    X1, one = mm.sample_derivative(Xp)
    assert [d.shape for d in one] == [(12, 1), (7, 1)]
    mt = mogptk_amd.Model(ds, gpr.MultiOutputSpectralMixtureKernel(Q=2, output_dims=2, input_dims=1), inference=mogptk_amd.Titsias(inducing_points=5))
    with pytest.raises(ValueError, match="exact inference"):
        mt.sample_derivative()


# ---- the coincident limit ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(tdg.TABLES))
def test_coincident_limit_is_the_prior_variance_of_the_derivative(name):
    """H_dd[a][a] of the twin's formulas, every row kind and group of the device tests' tables, is gpr/kernel.py:deriv_diag's kappa"""
    D = tdg.TABLES[name][0]
    X, y, noise, table, kind, shape = tdg.system(name, (40, 25))
    Xk = X[::3]
    H = dcov_twin.hessian_from_table(table, Xk, Xk, kind, shape)
    idx = np.arange(len(Xk))
    got = np.stack([H[idx, d, idx, d] for d in range(D)], axis=1)
    T = table.shape[2]
    want = deriv_diag(table, np.zeros((2, 2, T), dtype=np.int64) if kind is None else kind, np.zeros((2, 2, T)) if shape is None else shape, Xk, D)
    e = err(got, want)
    print(name, "kappa", e)
    assert e <= 1e-12
    flat = H.reshape(len(Xk) * D, len(Xk) * D)
    assert err(flat, flat.T) <= 1e-13                         # H_de[a][b] = H_ed[b][a], cross-channel pairs included
