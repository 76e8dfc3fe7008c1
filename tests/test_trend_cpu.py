"""
Host side of LinearKernel, PolynomialKernel and SincKernel (kinds 6 and 7), without a device: the class surface; the term tables
and kinds they emit alone and under MulKernel, IndependentMultiOutputKernel and LMC (the leading coregionalization row included); the
table form through the numpy twin of the device handle (oracle/table_model.py: dot-product rows and the sinc profile) against closed-form
numpy kernels written here and against the reference's K / K_diag (tests/golden/trend.npz, written by tests/golden/gen_family.py from the
models of tests/trend_cases.py); the chain rule and the per-point diagonal's backward against finite differences of those closed forms and
against the reference's autograd; the refusals; checkpoints.  The bodies shared with the other kernel families are in tests/kernel_family.py.
"""
import os
import numpy as np
import pytest

from mogptk_amd import gpr, _lib
from mogptk_amd.gpr.kernel import KIND_TIMES, KIND_DOT
from mogptk_amd.gpr.singleoutput import KIND_SINC
from mogptk_amd.gpr.model import _gtable_from_moments
import trend_cases as tc
import kernel_family as kf
from family_cases import exact, full_cases
from oracle.table_model import gram_from_table, moments_dense

FAMILY = "trend"
X_ = KIND_TIMES
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the kernels in closed form, straight from their definitions -----------------------------------------------------------------------
def closed_form(k, xa, xb):
    """K(xa, xb) of a single-output kernel object from its constrained parameters (inputs without a channel column)"""
    name = type(k).__name__
    tau = xa[:, None, :] - xb[None, :, :]
    if name in ("LinearKernel", "PolynomialKernel"):
        return (float(k.magnitude()) * (xa @ xb.T) + float(k.bias())) ** (k.degree if name == "PolynomialKernel" else 1)
    if name == "SincKernel":
        return float(k.magnitude()) * np.sinc(tau[..., 0] * k.bandwidth()[0]) * np.cos(2.0 * np.pi * tau[..., 0] * k.frequency()[0])
    if name == "PeriodicKernel":
        return float(k.magnitude()) * np.exp(-2.0 * np.sin(np.pi * tau[..., 0] / k.period()[0]) ** 2 / k.lengthscale()[0] ** 2)
    if name == "SquaredExponentialKernel":
        return float(k.magnitude()) * np.exp(-0.5 * np.sum((tau / k.lengthscale()) ** 2, axis=2))
    if name == "MaternKernel":
        r = np.sqrt(3.0) * np.abs(tau[..., 0]) / k.lengthscale()[0]
        assert k.nu == 1.5
        return float(k.magnitude()) * (1.0 + r) * np.exp(-r)
    if name == "AddKernel":
        return sum(closed_form(s, xa, xb) for s in k.kernels)
    if name == "MulKernel":
        return np.prod([closed_form(s, xa, xb) for s in k.kernels], axis=0)
    raise KeyError(name)


def closed_form_mo(k, Xa, Xb):
    """the same with a channel column, through IndependentMultiOutputKernel and LMC"""
    if k.output_dims is None:
        return closed_form(k, Xa[:, 1:], Xb[:, 1:])
    ca, cb = Xa[:, 0].astype(int), Xb[:, 0].astype(int)
    subs = [closed_form(s, Xa[:, 1:], Xb[:, 1:]) for s in k.kernels]
    if type(k).__name__ == "IndependentMultiOutputKernel":
        return sum((ca[:, None] == c) * (cb[None, :] == c) * s for c, s in enumerate(subs))
    B = np.einsum("iqr,jqr->ijq", k.weight(), k.weight())
    return sum(B[ca][:, cb][..., q] * s for q, s in enumerate(subs))


def kinds_of(case):
    return tc.kernel(gpr, case)._spectral_kinds(tc.CASES[case].get("D", 1))


# ---- tests -----------------------------------------------------------------------------------------------------------------------------
def test_class_surface_matches_the_reference():
    k = gpr.LinearKernel()
    assert [p._name.split(".")[-1] for p in k.parameters()] == ["bias", "magnitude"] and k.bias().shape == () and k.magnitude().shape == ()
    assert float(k.bias.lower) == 0.0 and float(k.magnitude.lower) == gpr.config.positive_minimum
    assert float(k.bias()) == 0.0 and abs(float(k.magnitude()) - 1.0) < 2e-5 and k.name() == "LinearKernel"
    k = gpr.PolynomialKernel(3, 2)                             # degree, input_dims: the reference's order of arguments
    assert (k.degree, k.input_dims) == (3, 2) and not isinstance(k.degree, gpr.Parameter)
    assert [p._name.split(".")[-1] for p in k.parameters()] == ["bias", "magnitude"] and float(k.bias.lower) == 0.0
    with pytest.raises(TypeError):
        gpr.PolynomialKernel()                                 # the degree has no default
    k = gpr.SincKernel()
    assert [p._name.split(".")[-1] for p in k.parameters()] == ["magnitude", "frequency", "bandwidth"]
    assert k.frequency().shape == (1,) and k.bandwidth().shape == (1,) and k.magnitude().shape == ()
    for p in k.parameters():
        assert float(np.asarray(p.lower).reshape(-1)[0]) == gpr.config.positive_minimum and np.all(np.abs(p() - 1.0) < 2e-5)
    assert isinstance(gpr.LinearKernel() * gpr.PeriodicKernel(), gpr.MulKernel) and isinstance(gpr.LinearKernel() + gpr.SincKernel(), gpr.AddKernel)
    x = np.array([[0.5], [2.0], [-1.0]])
    k = gpr.PolynomialKernel(2)
    k.magnitude.assign(0.3); k.bias.assign(0.4)
    assert np.allclose(k.K_diag(x), (float(k.magnitude()) * x[:, 0] ** 2 + float(k.bias())) ** 2, rtol=1e-14)      # the diagonal follows the point
    assert np.allclose(gpr.SincKernel().K_diag(x), gpr.SincKernel().magnitude(), rtol=1e-15)


def test_tables_and_kinds_of_the_three_kernels():
    k = tc.single(gpr, "lin", 1, np.random.default_rng(0))
    assert k._spectral_kinds(1)[0].tolist() == [[[7]]] and k._spectral_kinds(1)[1].tolist() == [[[1.0]]] and k._radial(1) and k._pointwise(1)
    assert np.array_equal(k._spectral_terms(1), [[[[float(k.magnitude()), float(k.bias()), 0.0, 0.0, 0.0]]]])      # the bias in the Psi slot
    k = tc.single(gpr, "poly3", 2, np.random.default_rng(0))
    kd, sh = k._spectral_kinds(2)
    assert kd.tolist() == [[[7]]] and sh.tolist() == [[[3.0]]] and kd.dtype == np.int32 and sh.dtype == np.float64
    assert np.array_equal(k._spectral_terms(2), [[[[float(k.magnitude()), float(k.bias())] + [0.0] * 6]]])
    k = tc.single(gpr, "sinc", 1, np.random.default_rng(0))
    assert k._spectral_kinds(1)[0].tolist() == [[[6]]] and k._radial(1) and not k._pointwise(1)
    assert np.allclose(k._spectral_terms(1), [[[[float(k.magnitude()), 0.0, float(k.bandwidth()[0]) ** 2, float(k.frequency()[0]), 0.0]]]], rtol=1e-15)      # V = bandwidth^2, M = frequency
    assert KIND_SINC == 6 and KIND_DOT == 7

    assert kinds_of("lin_se")[0].tolist() == [[[7, 0]]]
    assert kinds_of("lin_per")[0].tolist() == [[[7 | X_, 5]]]
    kd, sh = kinds_of("poly2_m32")
    assert kd.tolist() == [[[7 | X_, 3]]] and sh.tolist() == [[[2.0, 0.0]]]
    assert kinds_of("sinc_lin")[0].tolist() == [[[6 | X_, 7]]]
    assert kinds_of("straddle")[0].tolist() == [[[0, 3, 6, 0, 3, 5, 6, 7 | X_, 5]]]
    assert kinds_of("big")[0].tolist() == [[[7 | X_, 5, 3]]]
    # IndependentMultiOutputKernel(lin * per, sinc): the groups differ, so each channel gets rows of its own; the other channel's rows are
    # plain rows of zero amplitude there (a dot-product row of zero amplitude would not be zero)
    k = tc.kernel(gpr, "imo")
    kd, _ = k._spectral_kinds(1)
    assert kd.tolist() == [[[7 | X_, 5, 0], [X_, 0, 0]], [[X_, 0, 0], [X_, 0, 6]]]
    A = k._spectral_terms(1)[..., 0]
    assert np.all(A[0, 0, :2] > 0) and A[0, 0, 2] == 0 and np.all(A[1, 1, :2] == 0) and A[1, 1, 2] > 0 and not np.any(A[0, 1]) and not np.any(A[1, 0])
    # LMC over (lin, m32): B_q does not scale a dot-product row through its amplitude, so a plain row of amplitude B_q[i, j] leads its group
    k = tc.kernel(gpr, "lmc")
    kd, sh = k._spectral_kinds(1)
    assert kd.shape == (2, 2, 3) and np.all(kd == np.array([X_, 7, 3])) and np.all(sh == np.array([0.0, 1.0, 0.0]))
    B, t = k._coreg(), k._spectral_terms(1)
    lin, m32 = k.kernels
    assert np.array_equal(t[..., 0, 0], B[..., 0]) and not np.any(t[..., 0, 1:])
    assert np.all(t[..., 1, 0] == lin.magnitude()) and np.all(t[..., 1, 1] == lin.bias()) and not np.any(t[..., 1, 2:])
    assert np.allclose(t[..., 2, 0], B[..., 1] * m32.magnitude(), rtol=1e-15)
    # a dot-product row that does not lead its group leaves the coregionalization factor on the row that does
    k = gpr.LinearModelOfCoregionalizationKernel(gpr.SincKernel() * gpr.LinearKernel(), output_dims=2)
    assert np.all(k._spectral_kinds(1)[0] == np.array([6 | X_, 7])) and k._spectral_terms(1).shape[2] == 2


@pytest.mark.parametrize("case", full_cases(FAMILY))
def test_table_and_kinds_reproduce_the_reference_gram(case):
    k, _, _, _, X, _, want, tol = kf.check_table_and_kinds(FAMILY, case)
    assert np.max(np.abs(closed_form_mo(k, X, X) - want)) <= tol                # the closed forms of this file are the reference's kernels


@pytest.mark.parametrize("case", full_cases(FAMILY))
def test_chain_rule_reproduces_reference_gradients(case, monkeypatch):
    m = kf.check_chain_rule(FAMILY, case, monkeypatch)
    assert m._handle.kind is not None                       # every case of this family carries a kind


def fd_kernels():
    rng = np.random.default_rng(17)
    out = {e: tc.parse(gpr, e, 1, rng) for e in ("lin", "poly3", "sinc", "lin*per", "sinc*poly2", "lin+se", "poly2*m32*per+sinc*lin")}
    out["lin_d2"] = tc.single(gpr, "lin", 2, rng)
    out["poly2_d2"] = tc.single(gpr, "poly2", 2, rng)
    out["imo"] = tc.kernel(gpr, "imo")
    out["lmc"] = tc.kernel(gpr, "lmc")
    out["lmc_mul"] = gpr.LinearModelOfCoregionalizationKernel(tc.parse(gpr, "lin*per", 1, rng), tc.parse(gpr, "sinc*poly2", 1, rng), output_dims=2, Rq=1)
    return out


@pytest.mark.parametrize("name", ["lin", "poly3", "sinc", "lin*per", "sinc*poly2", "lin+se", "poly2*m32*per+sinc*lin", "lin_d2", "poly2_d2", "imo", "lmc", "lmc_mul"])
def test_backward_against_finite_differences_of_the_closed_forms(name):
    """f(raw parameters) = sum_ab G_ab K_ab + sum_a w_a K_aa with K from the CLOSED FORMS of this file (no table inside), G symmetric; its
    gradient from the twin's moments in the device's layout (lower pairs, off-diagonal blocks twice, the odd slots of diagonal
    blocks zeroed), `_gtable_from_moments`, `_point_diag_table_grad` (or the constant diagonal's product rule) and `_spectral_backward`"""
    rng = np.random.default_rng(11)
    k = fd_kernels()[name]
    C, D = k._channels(), k.input_dims
    n = 24
    X = np.concatenate([np.sort(rng.integers(0, C, (n, 1)), axis=0).astype(float), rng.uniform(0, 6, (n, D))], axis=1)
    X[5, 1:] = X[4, 1:]                                       # r = 0 off the diagonal
    G = rng.standard_normal((n, n))
    G = G + G.T
    w = rng.uniform(0.5, 1.5, n)

    def f():
        K = closed_form_mo(k, X, X)
        return float(np.sum(G * K) + np.sum(w * np.diag(K)))

    table = k._spectral_terms(D)
    kind, shape = k._spectral_kinds(D)
    K = gram_from_table(table, X, X, kind, shape)
    assert np.max(np.abs(K - closed_form_mo(k, X, X))) <= 1e-13 * max(1.0, np.max(np.abs(K)))
    mom = moments_dense(table, G, X, X, True, kind, shape)
    assert np.max(np.abs(k._point_diag(table, X, D) - np.diag(K))) <= 1e-13 * max(1.0, np.max(np.abs(K)))
    gt = _gtable_from_moments(table, mom, D, lower=True, kind=kind) + k._point_diag_table_grad(table, X, D, weights=w)
    for p in k.parameters():
        p.grad = None
    k._spectral_backward(gt)
    for p in k.parameters():
        got, raw = np.asarray(p.grad, dtype=np.float64).reshape(-1), p.data.reshape(-1)
        for i in range(raw.size):
            keep, h = raw[i], 1e-6
            raw[i] = keep + h; up = f()
            raw[i] = keep - h; dn = f()
            raw[i] = keep
            fd = (up - dn) / (2 * h)
            assert abs(got[i] - fd) <= 1e-6 * max(1.0, abs(fd)), (name, p._name, got[i], fd)


def test_sinc_series_meets_the_closed_form():
    """the twin's psi switches to its series below s = 1e-8; the device's below pi^2 s = 1 -- both sides of either threshold agree with
    the closed form to rounding where that is well conditioned"""
    s = np.array([0.0, 1e-12, 1e-9, 1e-7, 1e-3, 0.05, 0.1, 0.2, 1.0, 7.3])
    x = np.pi ** 2 * s
    fact = [float(np.prod(np.arange(1, n + 1))) for n in range(20)]
    phi = sum((-x) ** k / fact[2 * k + 1] for k in range(9))
    psi = np.pi ** 2 * sum((-x) ** k * (2 * k + 2) / fact[2 * k + 3] for k in range(8))
    r = np.sqrt(s)
    small = x <= 1.0
    assert np.max(np.abs(phi[small] - np.sinc(r[small]))) <= 4e-16
    mid = small & (s >= 1e-3)
    assert np.max(np.abs(psi[mid] - (np.sinc(r[mid]) - np.cos(np.pi * r[mid])) / s[mid])) <= 1e-12
    assert abs(psi[0] - np.pi ** 2 / 3.0) <= 1e-15 and phi[0] == 1.0


def test_refusals_come_before_any_device_call(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "lib", no_device)
    monkeypatch.setattr(_lib, "ExactHandle", no_device)
    with pytest.raises(NotImplementedError, match="SincKernel with input_dims > 1 is not on the HIP path: the reference measures distance there as"):
        gpr.SincKernel(input_dims=2)
    for cls in (gpr.LinearKernel, gpr.SincKernel, lambda **kw: gpr.PolynomialKernel(2, **kw)):
        with pytest.raises(NotImplementedError, match="active_dims"):
            cls(active_dims=[0])
    for bad in (0, 9, 2.5):
        with pytest.raises(NotImplementedError, match="degree"):
            gpr.PolynomialKernel(bad)
    five = gpr.MulKernel(gpr.LinearKernel(), *[gpr.SincKernel() for _ in range(4)])
    with pytest.raises(NotImplementedError, match="more than 4"):
        five._spectral_terms(1)
    lmc = gpr.LinearModelOfCoregionalizationKernel(gpr.MulKernel(gpr.LinearKernel(), *[gpr.SincKernel() for _ in range(3)]), output_dims=2)
    with pytest.raises(NotImplementedError, match="at most 4 rows"):      # the leading coregionalization row is the fifth
        lmc._spectral_terms(1)
    mo = gpr.IndependentMultiOutputKernel(gpr.LinearKernel(), gpr.SincKernel(), output_dims=2)
    with pytest.raises(NotImplementedError, match="multi-output"):
        (mo * mo)._spectral_terms(1)
    X, y, _ = tc.data("lin")
    Xc, yc, _ = tc.data("imo")
    sparse = dict(Titsias=dict(Z=4), Snelson=dict(Z=4), OpperArchambeau={}, SparseHensman=dict(Z=4), Hensman={})
    for name, kw in sparse.items():
        for build in (lambda: (gpr.LinearKernel(), X, y), lambda: (gpr.PolynomialKernel(2), X, y), lambda: (gpr.SincKernel(), X, y),
                      lambda: (tc.kernel(gpr, "lin_per"), X, y), lambda: (tc.kernel(gpr, "lin_se"), X, y), lambda: (tc.kernel(gpr, "imo"), Xc, yc),
                      lambda: (tc.kernel(gpr, "lmc"), Xc, yc)):
            with pytest.raises(NotImplementedError, match="%s with a non-Gaussian" % name):
                getattr(gpr, name)(*build(), **kw)

    class Comm:                                                 # what use_distributed() leaves in config.comm
        native, world, rank, force = True, 2, 0, False
    saved = getattr(gpr.config, "comm", None)
    gpr.config.comm = Comm()
    try:
        for case in ("lin", "sinc", "poly2_m32"):
            m = exact(FAMILY, gpr, case)
            with pytest.raises(NotImplementedError, match="use_distributed"):
                m.loss()
            assert m._handle is None
    finally:
        gpr.config.comm = saved
    for inner in (gpr.LinearKernel(), gpr.SincKernel(), gpr.PolynomialKernel(2) * gpr.SquaredExponentialKernel()):
        env = gpr.AddKernel(gpr.MultiOutputHarmonizableSpectralKernel(output_dims=1, input_dims=1), gpr.IndependentMultiOutputKernel(inner, output_dims=1))
        with pytest.raises(NotImplementedError, match="enveloped"):
            env(np.zeros((4, 2)))


def test_header_and_bindings_carry_the_kinds():
    src = open(os.path.join(ROOT, "include", "mogp_hip.h")).read()
    assert "#define MOGP_KIND_SINC 6" in src and "#define MOGP_KIND_DOT 7" in src and "#define MOGP_DOT_DEGREE_MAX 8" in src
    assert gpr.singleoutput.DOT_DEGREE_MAX == 8


CHECKPOINTS = ("trend", "lmc")


@pytest.mark.parametrize("tag", CHECKPOINTS)
def test_reference_checkpoint_round_trip(tag, tmp_path):
    pytest.importorskip("torch")
    k = kf.check_checkpoint_loads(FAMILY, tag, tmp_path)
    want = dict(trend={"MulKernel", "LinearKernel", "PeriodicKernel", "PolynomialKernel", "SincKernel"}, lmc={"LinearKernel", "MulKernel", "SincKernel", "PolynomialKernel"})[tag]
    assert want <= set(kf.kernel_names(k))
    degrees = [s.degree for s in _walk(k) if type(s).__name__ == "PolynomialKernel"]
    assert degrees == [dict(trend=2, lmc=3)[tag]]
    kf.check_checkpoint_is_written_as_the_reference_writes_it(FAMILY, tag)


def _walk(k):
    yield k
    for s in getattr(k, "kernels", None) or []:
        yield from _walk(s)
