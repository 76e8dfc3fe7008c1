"""
The posterior of df/dx on the device (mogp_exact_predict_grad: csrc/exact.hip, predict_core over D Jacobian row blocks written by
csrc/gram.hip:k_gram_dx behind one factorisation and one substitution).  First the raw ABI against the numpy twin (tests/deriv_twin.py) over
tables that reach every instantiation of k_gram_dx -- Gaussian rows at D = 1 (nine terms: two LDS chunks), 2, 3 and 5 (the generic one), enveloped
rows at D = 1 and 4, every profile kind, a product group of four rows, a dot-product row alone and inside a group -- at the channel sizes and
test sets at which the tile lists, the ragged tiles and the permutation to caller order change.  Then both forms of the prediction and the
accurate mode, gpr.Exact.predict_df against the reference-side goldens (tests/golden/deriv.npz), neutrality towards predict_f, and the
ABI's refusals.  Tolerance: 1e-9 relative to max(1, max |want|) for dmu and dvar (what test_parts_gpu.py holds predict_parts to --
the twin itself meets it against the goldens).
"""
import functools
import os
import numpy as np
import pytest

from mogptk_amd import gpr, _lib
from kernel_family import err
import deriv_cases
import deriv_twin
import kinds_sweep as ks
from test_deriv_cpu import FX, TOL, check_case, model

pytestmark = pytest.mark.gpu

X_ = ks.X_
TABLES = {                                                  # name -> (D, kinds, enveloped)
    "gauss_d1_t9": (1, [0] * 9, False),
    "gauss_d2": (2, [0] * 3, False),
    "gauss_d3": (3, [0] * 3, False),
    "gauss_d5": (5, [0] * 2, False),
    "env_d1": (1, [0] * 3, True),
    "env_d4": (4, [0] * 2, True),
    "rq": (1, [ks.RQ, 0], False),
    "m32": (1, [ks.M32, 0], False),
    "m52": (1, [ks.M52, 0], False),
    "periodic": (1, [ks.PERIODIC, 0], False),
    "sinc": (1, [ks.SINC, 0], False),
    "group4": (1, [ks.M32 | X_, ks.PERIODIC | X_, ks.RQ | X_, 0, ks.M52], False),
    "dot": (1, [ks.DOT, 0], False),
    "dot_group_d3": (3, [ks.DOT | X_, ks.M32, 0 | X_, ks.DOT | X_, ks.RQ], False),
    "profiles_d2": (2, [ks.RQ | X_, 0, ks.M52], False),
    "generic_d5": (5, [ks.M52, ks.RQ | X_, 0, ks.DOT | X_, ks.M32], False),
}
TRAIN = [(71, 129, 33), (65, 1, 63)]
TESTS = [(1, 0, 0), (33, 0, 40), (64, 65, 1)]
JITTER = 1e-8


@functools.lru_cache(maxsize=None)
def system(name, sizes):
    """(X, y, noise, table, kind, shape): a table of the named kinds for channels of `sizes` points, its cross pairs scaled until the TWIN's
    lambda_min(Kj) >= 0.1 (kinds_sweep.make_case's rule: the device is not asked)"""
    D, kinds, env = TABLES[name]
    rng = np.random.default_rng([list(TABLES).index(name)] + list(sizes))
    C, T = len(sizes), len(kinds)
    kind = np.broadcast_to(np.array(kinds, dtype=np.int32), (C, C, T)).copy()
    shape = np.broadcast_to(np.array([0.9 if (k & ks.MASK) == ks.RQ else 3.0 if (k & ks.MASK) == ks.DOT else 0.0 for k in kinds]), (C, C, T)).copy()
    base, kind, shape = ks.draw_table(rng, kinds, D, C, like=(kind, shape))
    if env:                                                 # [.., L_d, c_d]: the envelope on the midpoint, the same seen from either side of a pair
        Lc = np.concatenate([rng.uniform(0.01, 0.06, (C, C, T, D)), rng.uniform(3.0, 7.0, (C, C, T, D))], axis=3)
        Lc = np.where(np.arange(C)[:, None, None, None] >= np.arange(C)[None, :, None, None], Lc, np.swapaxes(Lc, 0, 1))
        base = np.concatenate([base, Lc], axis=3)
    X = ks.draw_points(rng, sizes, D)
    y, noise = rng.standard_normal(len(X)), rng.uniform(0.2, 0.4, C)
    radial = bool(np.any(kind))
    for k in range(14):
        table = ks.scale_cross(base, kind, shape, 0.25 * 2.0 ** -k)
        h = twin(X, y, C, table, kind if radial else None, shape if radial else None)
        if np.linalg.eigvalsh(h._Kj(noise, JITTER, None)[0])[0] >= 0.1:
            break
    else:
        raise AssertionError("no positive definite system for %s" % name)
    return X, y, noise, table, (kind if radial else None), (shape if radial else None)


def twin(X, y, C, table, kind, shape):
    h = deriv_twin.DerivTableDevice(0, X, y, C)
    h.set_terms(table)
    if kind is not None:
        h.set_kinds(kind, shape)
    return h


def device(X, y, C, table, kind, shape):
    h = _lib.ExactHandle(0, X, y, C)
    h.set_terms(table)
    if kind is not None:
        h.set_kinds(kind, shape)
    if table.shape[3] > 2 + 3 * (X.shape[1] - 1):             # enveloped rows: K(x, x) follows the point and enters the relative jitter, as gpr.Exact sets it
        h.set_point_diag(np.diagonal(deriv_twin.tm.gram_from_table(table, X)).copy())
    return h


def draw_tests(rng, counts, D):
    Xs = ks.draw_points(rng, counts, D, duplicate=False, shuffle=True)
    return Xs, rng.uniform(0.5, 2.0, (D, len(Xs)))          # any kappa serves: both sides subtract from the same


class flow_predict:
    """MOGP_FLOW_PREDICT for the calls inside (the library reads it per call); the environment as it was afterwards"""

    def __init__(self, value):
        self.value = value

    def __enter__(self):
        self.old = os.environ.get("MOGP_FLOW_PREDICT")
        os.environ["MOGP_FLOW_PREDICT"] = self.value
        return self

    def __exit__(self, *exc):
        if self.old is None:
            os.environ.pop("MOGP_FLOW_PREDICT", None)
        else:
            os.environ["MOGP_FLOW_PREDICT"] = self.old
        return False


def compare(name, h, t, noise, Xs, kappa):
    want = t.predict_grad(noise, JITTER, kappa, Xs)
    got = h.predict_grad(noise, JITTER, kappa, Xs)
    for what, g, w in zip(("dmu", "dvar"), got, want):
        e = err(g, w)
        print(name, what, g.shape, e)
        assert e <= TOL, (name, what)
    return got


@pytest.mark.parametrize("name", list(TABLES))
def test_raw_abi_matches_the_twin(name):
    D = TABLES[name][0]
    for sizes in TRAIN:
        X, y, noise, table, kind, shape = system(name, sizes)
        C = len(sizes)
        h, t = device(X, y, C, table, kind, shape), twin(X, y, C, table, kind, shape)
        rng = np.random.default_rng(7)
        for counts in TESTS:
            Xs, kappa = draw_tests(rng, counts, D)
            compare("%s %s %s" % (name, sizes, counts), h, t, noise, Xs, kappa)
        if sizes == TRAIN[0]:                                 # a test point ON a training point (r = 0), and the same call twice: the same bits
            Xs, kappa = draw_tests(rng, (5, 5, 5), D)
            Xs[2] = X[7]
            a = compare(name + " coincident", h, t, noise, Xs, kappa)
            b = h.predict_grad(noise, JITTER, kappa, Xs)
            assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


def test_both_forms_of_the_prediction_and_the_accurate_mode():
    """N = 1100 (nine tile rows: the smallest size the dataflow form accepts), a product group at D = 1: as tile dataflow, on streams, and on
    streams in the accurate mode -- each against the twin, the dataflow and stream results against each other"""
    sizes = ks.DATAFLOW_SIZES
    X, y, noise, table, kind, shape = system("group4", sizes)
    C = len(sizes)
    h, t = device(X, y, C, table, kind, shape), twin(X, y, C, table, kind, shape)
    Xs, kappa = draw_tests(np.random.default_rng(11), (64, 65, 1), 1)
    got = {}
    for form, dataflow in (("8:200", True), ("0", False)):
        with flow_predict(form):
            got[form] = compare("group4 form " + form, h, t, noise, Xs, kappa)
            s = h.schedule()
            assert s["dataflow"] == dataflow and not s["dataflow_fell_back"], (form, s)
    assert err(got["8:200"][0], got["0"][0]) <= TOL and err(got["8:200"][1], got["0"][1]) <= TOL
    with flow_predict("0"):
        h.set_accurate(True)
        try:
            compare("group4 accurate", h, t, noise, Xs, kappa)
        finally:
            h.set_accurate(False)


@pytest.mark.parametrize("case", list(deriv_cases.CASES))
def test_predict_df_matches_the_reference(case):
    m, Xs, dmu, dvar = check_case(case)
    assert isinstance(m._handle, _lib.ExactHandle)
    assert np.all(dvar > 0.0)


@pytest.mark.parametrize("case", ["mosm2", "trend", "mohsm", "linmean"])
def test_a_derivative_call_leaves_nothing_behind(case):
    m, Xs = model(case)
    mu, var = m.predict_f(Xs)
    h = m._handle
    m.predict_df(Xs)
    mu2, var2 = m.predict_f(Xs)
    assert m._handle is h and mu.tobytes() == mu2.tobytes() and var.tobytes() == var2.tobytes()


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
        h.predict_grad(noise, JITTER, np.ones((1, 6)), Xs)
    assert e.value.code == _lib.MOGP_EINVAL and "row 1 of pair (0, 0)" in str(e.value) and word in str(e.value), str(e.value)
    h.set_kinds(None, None)                                   # the same rows as Gaussian ones: the handle goes on working
    compare("after the refusal", h, twin(X, y, 1, table, None, None), noise, Xs, np.ones((1, 6)))
