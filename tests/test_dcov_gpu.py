"""
The joint posterior covariance of df/dx on the device (mogp_exact_predict_grad_cov: csrc/exact.hip, predict_core over D Jacobian row blocks, then
csrc/gram.hip:k_gram_dxdx over the symmetric tile list of the test points less one product V V^T).  First the raw ABI against the numpy twin
(tests/dcov_twin.py) over the sixteen tables of test_deriv_gpu.py, which reach every instantiation of k_gram_dxdx, at the channel sizes and test
sets at which the 64-tiles turn ragged, D S crosses the 128-row GEMM tile and the permutation to caller order changes; a set with coincident
test points (r = 0 OFF the diagonal); the same bits twice; the diagonal against mogp_exact_predict_grad; symmetry and the smallest eigenvalue.
Then both forms of the prediction and the accurate mode, gpr.Exact.predict_df_cov against the reference-side goldens
(tests/golden/dcov.npz), neutrality towards predict_f and the default predict_df, and the ABI's refusals.  Tolerance: test_deriv_cpu.TOL, 1e-9
relative to max(1, max |want|).
"""
import numpy as np
import pytest

from mogptk_amd import gpr, _lib
from kernel_family import err
import deriv_cases
import dcov_twin
import kinds_sweep as ks
from test_deriv_cpu import FX, TOL, model
from test_deriv_gpu import JITTER, TABLES, TESTS, TRAIN, device, draw_tests, flow_predict, system
from helpers import load

pytestmark = pytest.mark.gpu

DX = load("dcov.npz")


def twin(X, y, C, table, kind, shape):
    h = dcov_twin.DcovTableDevice(0, X, y, C)
    h.set_terms(table)
    if kind is not None:
        h.set_kinds(kind, shape)
    return h


def compare(name, h, t, noise, Xs):
    want = t.predict_grad(noise, JITTER, None, Xs, full=True)
    got = h.predict_grad(noise, JITTER, None, Xs, full=True)
    for what, g, w in zip(("dmu", "dcov"), got, want):
        e = err(g, w)
        print(name, what, g.shape, e)
        assert g.shape == w.shape and e <= TOL, (name, what)
    return got


def consistent(name, h, t, noise, Xs, dcov):
    """the diagonal is mogp_exact_predict_grad's dvar (kappa from the twin's coincident H), dcov is symmetric and positive semi-definite"""
    S, D = Xs.shape[0], Xs.shape[1] - 1
    idx = np.arange(S)
    Hs = dcov_twin.hessian_from_table(t.table, Xs, Xs, t.kind, t.shape)
    kappa = np.ascontiguousarray(np.stack([Hs[idx, d, idx, d] for d in range(D)]))
    dvar = h.predict_grad(noise, JITTER, kappa, Xs)[1]
    flat = dcov.reshape(S * D, S * D)
    diag = np.diagonal(flat).reshape(S, D).T
    lam = np.linalg.eigvalsh(0.5 * (flat + flat.T))[0]
    print(name, "diag", err(diag, dvar), "asymmetry", np.max(np.abs(flat - flat.T)), "lambda_min", lam, "max diag", np.max(diag))
    assert err(diag, dvar) <= TOL, name
    assert np.max(np.abs(flat - flat.T)) <= TOL * max(1.0, np.max(np.abs(flat))), name
    # lambda_min >= -TOL max diag wherever the exact answer is positive semi-definite.  These tables are drawn, with cross-channel pairs only scaled
    # until the NOISY training system is positive definite: several are no valid covariance over training and test points together (the twin's own
    # dcov has lambda_min = -0.14 max diag for env_d4), and there the device may fall below the twin's smallest eigenvalue by no more than the same margin
    want = t.predict_grad(noise, JITTER, None, Xs, full=True)[1].reshape(S * D, S * D)
    assert lam >= min(np.linalg.eigvalsh(0.5 * (want + want.T))[0], 0.0) - TOL * np.max(diag), name


@pytest.mark.parametrize("name", list(TABLES))
def test_raw_abi_matches_the_twin(name):
    D = TABLES[name][0]
    for sizes in TRAIN:
        X, y, noise, table, kind, shape = system(name, sizes)
        C = len(sizes)
        h, t = device(X, y, C, table, kind, shape), twin(X, y, C, table, kind, shape)
        rng = np.random.default_rng(7)
        for counts in TESTS:
            Xs, _ = draw_tests(rng, counts, D)
            got = compare("%s %s %s" % (name, sizes, counts), h, t, noise, Xs)
            if sizes == TRAIN[0]:
                consistent("%s %s" % (name, counts), h, t, noise, Xs, got[1])
        if sizes == TRAIN[0]:
            # two test points equal on the same channel, and one input shared by two channels: r = 0 off the diagonal; then the same call twice
            Xs, _ = draw_tests(rng, (5, 5, 5), D)
            ch = Xs[:, 0].astype(int)
            a0, a1 = np.nonzero(ch == 0)[0][:2]
            b0, c0 = np.nonzero(ch == 1)[0][0], np.nonzero(ch == 2)[0][0]
            Xs[a1, 1:] = Xs[a0, 1:]
            Xs[c0, 1:] = Xs[b0, 1:]
            a = compare(name + " coincident", h, t, noise, Xs)
            b = h.predict_grad(noise, JITTER, None, Xs, full=True)
            assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


def test_both_forms_of_the_prediction_and_the_accurate_mode():
    """N = 1100, a product group at D = 1: as tile dataflow, on streams, and on streams in the accurate mode -- each against the twin, the
    dataflow and stream results against each other"""
    sizes = ks.DATAFLOW_SIZES
    X, y, noise, table, kind, shape = system("group4", sizes)
    C = len(sizes)
    h, t = device(X, y, C, table, kind, shape), twin(X, y, C, table, kind, shape)
    Xs, _ = draw_tests(np.random.default_rng(11), (64, 65, 1), 1)
    got = {}
    for form, dataflow in (("8:200", True), ("0", False)):
        with flow_predict(form):
            got[form] = compare("group4 form " + form, h, t, noise, Xs)
            s = h.schedule()
            assert s["dataflow"] == dataflow and not s["dataflow_fell_back"], (form, s)
    assert err(got["8:200"][0], got["0"][0]) <= TOL and err(got["8:200"][1], got["0"][1]) <= TOL
    with flow_predict("0"):
        h.set_accurate(True)
        try:
            compare("group4 accurate", h, t, noise, Xs)
        finally:
            h.set_accurate(False)


@pytest.mark.parametrize("case", list(deriv_cases.CASES))
def test_predict_df_cov_matches_the_reference(case):
    m, Xs = model(case)
    dmu, dcov = m.predict_df_cov(Xs)
    assert isinstance(m._handle, _lib.ExactHandle)
    for name, got, want in (("dmu", dmu, FX[case + "__dmu"]), ("dcov", dcov, DX[case + "__dcov"])):
        e = err(got, want)
        print(case, name, e)
        assert got.shape == want.shape and e <= TOL, name


@pytest.mark.parametrize("case", ["mosm2", "trend", "mohsm", "linmean"])
def test_a_full_call_leaves_nothing_behind(case):
    m, Xs = model(case)
    mu, var = m.predict_f(Xs)
    dmu, dvar = m.predict_df(Xs)
    h = m._handle
    m.predict_df_cov(Xs)
    mu2, var2 = m.predict_f(Xs)
    dmu2, dvar2 = m.predict_df(Xs)
    assert m._handle is h and mu.tobytes() == mu2.tobytes() and var.tobytes() == var2.tobytes()
    assert dmu.tobytes() == dmu2.tobytes() and dvar.tobytes() == dvar2.tobytes()


@pytest.mark.parametrize("kd, word", [(ks.M12, "Matern 1/2"), (ks.WHITE, "white")])
def test_the_library_refuses_rows_without_a_derivative(kd, word):
    """past the host: a table whose row 1 is of kind 2 or 10 is MOGP_EINVAL by name, and the handle goes on working"""
    rng = np.random.default_rng(3)
    X = ks.draw_points(rng, (40,), 1)
    table = np.zeros((1, 1, 2, 5))
    table[0, 0, :, 0], table[0, 0, :, 2] = (0.8, 0.3), (1.0, 0.5)
    kind, shape = np.array([[[0, kd]]], dtype=np.int32), np.zeros((1, 1, 2))
    y = rng.standard_normal(40)
    h = device(X, y, 1, table, kind, shape)
    Xs = ks.draw_points(rng, (6,), 1, duplicate=False)
    noise = np.array([0.3])
    with pytest.raises(_lib.MogpError) as e:
        h.predict_grad(noise, JITTER, None, Xs, full=True)
    assert e.value.code == _lib.MOGP_EINVAL and "row 1 of pair (0, 0)" in str(e.value) and word in str(e.value), str(e.value)
    h.set_kinds(None, None)                                   # the same rows as Gaussian ones: the handle goes on working
    compare("after the refusal", h, twin(X, y, 1, table, None, None), noise, Xs)
