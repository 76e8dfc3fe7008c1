"""
The posterior by kernel part on the device (mogp_exact_predict_parts: csrc/exact.hip, predict_core over P stacked row blocks behind one
factorisation and one substitution) against the reference-side goldens (tests/golden/parts.npz, gen_parts.py) over the cases of
tests/parts_cases.py: mu, var and cov at 1e-9 relative to max(1, max |want|).  Then the N = 2304 case in both substitution forms
(tile dataflow and streams), one part of all rows against predict_f bit for bit in both forms, the count of factorisations, and the ABI's
refusals.
"""
import ctypes
import os
import numpy as np
import pytest

from mogptk_amd import gpr, _lib
from kernel_family import err
import parts_cases
from test_parts_cpu import FX, check_case, model

pytestmark = pytest.mark.gpu


class flow_predict:
    """MOGP_FLOW_PREDICT for the calls inside (the library reads it per call); the environment as it was afterwards"""

    def __enter__(self):
        self.old = os.environ.get("MOGP_FLOW_PREDICT")
        return self

    def set(self, value):
        os.environ["MOGP_FLOW_PREDICT"] = value

    def __exit__(self, *exc):
        if self.old is None:
            os.environ.pop("MOGP_FLOW_PREDICT", None)
        else:
            os.environ["MOGP_FLOW_PREDICT"] = self.old
        return False


@pytest.mark.parametrize("case", parts_cases.SMALL)
def test_every_part_matches_the_reference(case):
    """S = 70 (P x 128 padded rows in several tile rows), S = 1, shuffled channels, the IMO parts that are empty off the diagonal pairs, the
    white part, enveloped rows: mu and var, and cov where the fixture holds it"""
    m, Xs, names, mu, var = check_case(case)
    assert isinstance(m._handle, _lib.ExactHandle)
    if case == "basis":                                       # the white part: nothing in a rectangular Gram, its amplitude on the diagonal
        A = float(m.kernel.kernels[2].magnitude())
        assert names[2] == "2:WhiteKernel" and np.all(mu[2] == 0.0) and np.all(var[2] == A)
        assert np.array_equal(m.predict_parts(Xs, full=True)[2][2], A * np.eye(len(Xs)))
    if case == "imo":                                         # the SE row of channel 1 alone says nothing about channel 0
        only = np.zeros((1, 2, 2, 2), dtype=bool)
        only[0, 1, 1, 0] = True
        mu1, var1 = m.predict_terms(Xs, only)
        ch = Xs[:, 0] == 0
        assert np.all(mu1[0, ch] == 0.0) and np.all(var1[0, ch] == 0.0) and np.any(mu1[0, ~ch] != 0.0)


def test_big_case_in_both_substitution_forms():
    """N = 2304 (18 tile rows), S = 300, P = 3: as tile dataflow and on streams -- each against the golden, against each other, bit-identical
    when repeated, and the marginal likelihood's loss and gradients the same bytes before and after"""
    pre = "big__"
    m, Xs = model("big")
    ps = list(m.parameters())

    def lml_loss():
        loss = float(m.loss())
        return [np.float64(loss).tobytes()] + [p.grad.tobytes() for p in ps]

    got = {}
    with flow_predict() as env:
        env.set("8:200")
        before = lml_loss()
        for form, dataflow in (("8:200", True), ("0", False)):
            env.set(form)
            names, mu, var = m.predict_parts(Xs)
            s = m._handle.schedule()
            assert s["dataflow"] == dataflow and not s["dataflow_fell_back"], (form, s)
            for name, arr in (("mu", mu), ("var", var)):
                e = err(arr[..., 0], FX[pre + name])
                print(pre, form, name, e)
                assert e <= 1e-9, (form, name)
            _, mu2, var2 = m.predict_parts(Xs)
            assert mu.tobytes() == mu2.tobytes() and var.tobytes() == var2.tobytes(), form
            got[form] = (mu, var)
        env.set("8:200")
        assert lml_loss() == before
    assert err(got["8:200"][0], got["0"][0]) <= 1e-9 and err(got["8:200"][1], got["0"][1]) <= 1e-9


def test_one_part_of_all_rows_is_predict_f_bit_for_bit():
    """the same layout with one row block: there is one code path.  Both forms at N = 2304; the small sizes with point rows, an envelope, a
    mean and shuffled channels on streams; the full covariance too"""
    with flow_predict() as env:
        m, Xs = model("big")
        for form in ("8:200", "0"):
            env.set(form)
            mu, var = m.predict_f(Xs)
            mu1, var1 = m.predict_terms(Xs, np.ones((1, 3), dtype=bool))
            assert m._handle.schedule()["dataflow"] == (form != "0")
            assert mu1[0].tobytes() == mu.tobytes() and var1[0].tobytes() == var.tobytes(), form
        for case in ("trend", "mosm", "mohsm", "basis"):
            m, Xs = model(case)
            T = m.parts()[0][1].shape[2]
            for full in (False, True):
                mu, var = m.predict_f(Xs, full=full)
                mu1, var1 = m.predict_terms(Xs, np.ones((1, T), dtype=bool), full=full)
                assert mu1[0].tobytes() == mu.tobytes() and var1[0].tobytes() == var.tobytes(), (case, full)


def test_one_factorisation_for_all_parts():
    """The products of a parts call against those of ONE predict_f on the same test points, on streams at N = 2304, S = 128, P = 3: the
    handle's flop counter over every tile product of the call (mogp_stage_ms; it is reset at the start of an evaluation and counts the
    factorisation's panel and Schur products as well as the substitution's) must stay below twice a prediction's.  From N^3 / 3 + N^2 Srow
    with padded rows -- Srow = 256 against 512 -- the ratio is about 1.25; three separate predictions would be 3."""
    with flow_predict() as env:
        env.set("0")
        m, Xs = model("big")
        Xs = Xs[:128]
        m.predict_f(Xs)
        h = m._handle
        h.set_profiling(True)
        try:
            m.predict_f(Xs)
            one = h.stage_ms()[2]
            m.predict_parts(Xs)
            parts = h.stage_ms()[2]
        finally:
            h.set_profiling(False)
    N = 2304
    print("gemm flops: predict_f %.4g, predict_parts (P = 3) %.4g, ratio %.3f; N^3/3 = %.4g" % (one, parts, parts / one, N ** 3 / 3))
    assert one >= N ** 3 / 3, "the counter does not see the factorisation's products"
    assert one < parts < 2 * one


def test_abi_refusals_leave_the_handle_usable():
    m, Xs = model("sum")
    mu, var = m.predict_f(Xs)
    h = m._handle
    L = _lib.lib()
    dp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    table = np.ascontiguousarray(m.kernel._spectral_terms(1), dtype=np.float64)
    Xk = np.ascontiguousarray(m.kernel._kernel_format(Xs))
    S = Xk.shape[0]
    noise, kss = np.ascontiguousarray(m._noise_var(), dtype=np.float64), np.array([[float(np.sum(table[0, 0, :, 0]))]])
    omu, ovar, info = np.empty(S), np.empty(S), ctypes.c_int64(0)

    def call(P, tabs, mu_out):
        return L.mogp_exact_predict_parts(h._h, dp(noise), None, float(m.jitter), P, dp(tabs), dp(kss), S, dp(Xk), 0,
                                          None if mu_out is None else dp(mu_out), dp(ovar), ctypes.byref(info))

    def valid():
        assert call(1, table[None].copy(), omu) == _lib.MOGP_OK
        assert omu.tobytes() == mu.tobytes() and ovar.tobytes() == var.tobytes()

    valid()
    assert call(0, table[None].copy(), omu) == _lib.MOGP_EINVAL and b"P <= 0" in L.mogp_last_error()
    valid()
    assert call(1, table[None].copy(), None) == _lib.MOGP_EINVAL and b"null" in L.mogp_last_error()
    valid()
    bad = table[None].copy()
    bad[0, 0, 0, 1, 2] *= 1.5                                   # the V column of row 1
    assert call(1, bad, omu) == _lib.MOGP_EINVAL
    msg = L.mogp_last_error().decode()
    assert "pair (0, 0), row 1, column 2" in msg, msg
    valid()
