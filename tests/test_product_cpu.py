"""
Host side of the product kernels and of ConstantKernel, CosineKernel, PeriodicKernel and LocallyPeriodicKernel, without a device:
tables, kinds and group flags of every case of tests/product_cases.py against hand-written expectations; a numpy evaluator of the grouped
table form against the reference's K / K_diag (tests/golden/product.npz, written by tests/golden/gen_product.py); the chain rule through
MulKernel against finite differences of that evaluator and against the reference's autograd; the refusals; checkpoints.
"""
import io
import os
import numpy as np
import pytest

import mogptk_amd
from mogptk_amd import gpr, _lib
from mogptk_amd.gpr.kernel import KIND_TIMES, KIND_MASK, group_slices
from mogptk_amd.gpr.model import _gtable_from_moments
import product_cases as pc
from helpers import load
from test_stationary_cpu import profiles, with_reference_raw, NumpyDevice

X_ = KIND_TIMES
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def golden_K(case):
    for tag in "ab":
        fx = load("product_gram_%s.npz" % tag)
        if case + "__K_tril" in fx:
            tril = fx[case + "__K_tril"]
            n = int(round((np.sqrt(8 * len(tril) + 1) - 1) / 2))
            K = np.zeros((n, n))
            K[np.tril_indices(n)] = tril
            return K + np.tril(K, -1).T
    raise KeyError(case)


def row_parts(row, kind, shape, u):
    """value k (unit amplitude) of one table row at the lags u (na, nb, D), and the integrands of its moments [m0, m4, m1_d, m2_d, m3_d]"""
    D = u.shape[2]
    Psi, V, M = row[1], row[2:2 + D], row[2 + D:2 + 2 * D]
    th = 2.0 * np.pi * (np.sum(M * u, axis=2) + Psi)
    if kind == 5:                                           # E = exp(V (cos - 1)): the phase is the profile's argument
        E = np.exp(V[0] * (np.cos(th) - 1.0))
        return E, [E, E * V[0] * np.sin(th), E * 2.0 * (1.0 - np.cos(th)), 0.0 * E, E * V[0] * u[..., 0] * np.sin(th)]
    phi, psi = profiles(kind, shape, np.sum(V * u * u, axis=2))
    parts = [phi * np.cos(th), phi * np.sin(th)]
    parts += [u[..., d] ** 2 * psi * np.cos(th) for d in range(D)] + [u[..., d] * psi * np.cos(th) for d in range(D)]
    parts += [u[..., d] * phi * np.sin(th) for d in range(D)]
    return phi * np.cos(th), parts


def evaluate(table, kind, shape, Xa, Xb, G=None):
    """K(Xa, Xb) of a term table with kinds and product groups; with an adjoint G also the moments of every ordered channel pair: row f of a
    group sees G weighted by the product of the group's other rows"""
    C, T, D = table.shape[0], table.shape[2], Xa.shape[1] - 1
    ca, cb = Xa[:, 0].astype(int), Xb[:, 0].astype(int)
    K = np.zeros((len(Xa), len(Xb)))
    mom = np.zeros((C, C, T, 2 + 3 * D))
    for i in range(C):
        for j in range(C):
            ia, ib = np.where(ca == i)[0], np.where(cb == j)[0]
            rows = []
            for t in range(T):
                u = Xa[ia, None, 1:] - Xb[None, ib, 1:] + table[i, j, t, 2 + 2 * D:2 + 3 * D]
                rows.append(row_parts(table[i, j, t], int(kind[i, j, t]) & KIND_MASK, shape[i, j, t], u))
            for a, b in group_slices(kind[i, j]):
                vals = [table[i, j, t, 0] * rows[t][0] for t in range(a, b)]
                K[np.ix_(ia, ib)] += np.prod(vals, axis=0)
                if G is not None:
                    for t in range(a, b):
                        w = G[np.ix_(ia, ib)] * np.prod([v for h, v in enumerate(vals) if h != t - a] + [np.ones_like(vals[0])], axis=0)
                        mom[i, j, t] = [np.sum(w * part) for part in rows[t][1]]
    return K, mom


class GroupDevice(NumpyDevice):
    """test_stationary_cpu.NumpyDevice over the grouped evaluator"""

    def eval(self, noise_var, jitter, grad=True, data_var=None):
        import test_stationary_cpu as ts
        saved, ts.evaluate = ts.evaluate, evaluate
        try:
            return super().eval(noise_var, jitter, grad=grad, data_var=data_var)
        finally:
            ts.evaluate = saved


def kinds_of(case):
    return pc.kernel(gpr, case)._spectral_kinds(pc.CASES[case].get("D", 1))


def test_class_surface_matches_the_reference():
    k = gpr.ConstantKernel()
    assert [p._name.split(".")[-1] for p in k.parameters()] == ["magnitude"] and k.magnitude().shape == ()
    k = gpr.CosineKernel(input_dims=3)
    assert [p._name.split(".")[-1] for p in k.parameters()] == ["magnitude", "lengthscale"] and k.lengthscale().shape == (3,)
    for cls in (gpr.PeriodicKernel, gpr.LocallyPeriodicKernel):
        k = cls()
        assert (k.order, k.input_dims) == (0, 1) and k.period().shape == (1,) and k.lengthscale().shape == (1,)
        assert cls(order=-1).lengthscale().shape == ()
        assert [p._name.split(".")[-1] for p in k.parameters()] == ["magnitude", "period", "lengthscale"]
        for p in k.parameters():
            assert float(np.asarray(p.lower).reshape(-1)[0]) == gpr.config.positive_minimum and np.all(np.abs(p() - 1.0) < 2e-5)
    assert isinstance(gpr.SquaredExponentialKernel() * gpr.CosineKernel(), gpr.MulKernel)
    k = gpr.SquaredExponentialKernel() * gpr.CosineKernel() * gpr.ConstantKernel()                # flattened, as the reference's Kernels
    assert len(k.kernels) == 3


def test_tables_kinds_and_flags_of_the_cases():
    assert kinds_of("se_cos")[0].tolist() == [[[X_, 0]]]
    assert kinds_of("m32_cos")[0].tolist() == [[[3 | X_, 0]]]
    assert kinds_of("m12_per")[0].tolist() == [[[2 | X_, 5]]]
    kd, sh = kinds_of("const_rq")
    assert kd.tolist() == [[[X_, 1]]] and sh.tolist() == [[[0.0, 0.7]]]
    assert kinds_of("per")[0].tolist() == [[[5]]]
    assert kinds_of("locper")[0].tolist() == [[[5 | X_, 0]]]
    assert kinds_of("cos")[0].tolist() == [[[0]]] and not pc.kernel(gpr, "cos")._radial(1)
    assert kinds_of("const_se")[0].tolist() == [[[0, 0]]] and not pc.kernel(gpr, "const_se")._radial(1)      # ordinary tables: no kinds travel
    assert kinds_of("dist")[0].tolist() == [[[X_, 0, 4 | X_, 0]]]
    assert kinds_of("three")[0].tolist() == [[[X_, X_, 5]]]
    assert kinds_of("straddle")[0].tolist() == [[[0, 3, 0, 1, 4, 5, 2, X_, 0]]]
    assert kinds_of("lowmag")[0].tolist() == [[[X_, 0, 3]]]
    assert kinds_of("se_cos_d2")[0].tolist() == [[[X_, 0]]]
    assert kinds_of("rq_const_d2")[0].tolist() == [[[1 | X_, 0]]]
    kd, _ = kinds_of("imo")                                  # the same groups in every channel pair, the profiles on the block diagonal
    assert kd.tolist() == [[[X_, 0], [X_, 0]], [[X_, 0], [4 | X_, 5]]]
    kd, _ = kinds_of("lmc")
    assert kd.shape == (2, 2, 3) and np.all(kd == np.array([X_, 0, 3]))
    assert all(kd.dtype == np.int32 for kd in (kinds_of(c)[0] for c in pc.CASES))
    assert all(pc.kernel(gpr, c)._radial(pc.CASES[c].get("D", 1)) for c in pc.PRODUCT_CASES)

    k = pc.kernel(gpr, "se_cos").kernels[0]
    se, cos = k.kernels
    want = np.zeros((1, 1, 2, 5))
    want[0, 0, 0, 0], want[0, 0, 0, 2] = se.magnitude(), 1.0 / se.lengthscale()[0] ** 2
    want[0, 0, 1, 0], want[0, 0, 1, 3] = cos.magnitude(), 1.0 / cos.lengthscale()[0]
    assert np.array_equal(k._spectral_terms(1), want)
    k = pc.kernel(gpr, "locper")
    want = np.zeros((1, 1, 2, 5))
    want[0, 0, 0] = [k.magnitude(), 0.0, 1.0 / k.lengthscale()[0] ** 2, 1.0 / k.period()[0], 0.0]
    want[0, 0, 1] = [1.0, 0.0, 1.0 / k.lengthscale()[0] ** 2, 0.0, 0.0]
    assert np.array_equal(k._spectral_terms(1), want)
    k = pc.kernel(gpr, "dist").kernels[0]                    # (se + m52) * cos: the cosine row twice
    t = k._spectral_terms(1)[0, 0]
    assert np.array_equal(t[1], t[3]) and t[1, 3] == 1.0 / k.kernels[1].lengthscale()[0] and t[0, 0] == k.kernels[0].kernels[0].magnitude()
    k = pc.kernel(gpr, "lmc")                                # the coregionalization factor once per group: on its first row
    B, t = k._coreg(), k._spectral_terms(1)
    assert np.allclose(t[..., 0, 0], B[..., 0] * k.kernels[0].kernels[0].magnitude(), rtol=1e-15)
    assert np.all(t[..., 1, 0] == k.kernels[0].kernels[1].magnitude()) and np.allclose(t[..., 2, 0], B[..., 1] * k.kernels[1].magnitude(), rtol=1e-15)


def test_independent_kernels_with_different_groups_get_rows_of_their_own():
    k = gpr.IndependentMultiOutputKernel(gpr.SquaredExponentialKernel() * gpr.CosineKernel(), gpr.MaternKernel(nu=1.5), output_dims=2)
    kd, _ = k._spectral_kinds(1)
    assert kd.tolist() == [[[X_, 0, 0]] * 2, [[X_, 0, 0], [X_, 0, 3]]]
    A = k._spectral_terms(1)[..., 0]
    assert np.all(A[0, 0, :2] > 0) and A[0, 0, 2] == 0 and np.all(A[1, 1, :2] == 0) and A[1, 1, 2] > 0 and not np.any(A[0, 1]) and not np.any(A[1, 0])
    gt = np.zeros(k._spectral_terms(1).shape)
    gt[1, 1, 2, 0], gt[0, 0, 1, 0] = 2.0, 3.0
    k._spectral_backward(gt)
    assert k.kernels[1].magnitude.grad is not None and k.kernels[0].kernels[1].magnitude.grad is not None


@pytest.mark.parametrize("case", pc.FULL_CASES)
def test_table_and_kinds_reproduce_the_reference_gram(case):
    fx = load("product.npz")
    m = pc.exact(gpr, case)
    with_reference_raw(m, fx, case + "__")
    k = m.kernel
    X, Xs = k._kernel_format(fx[case + "__X"]), k._kernel_format(fx[case + "__Xs"])
    D = X.shape[1] - 1
    table = k._spectral_terms(D)
    kind, shape = k._spectral_kinds(D)
    assert kind.shape == table.shape[:3] == shape.shape and shape.dtype == np.float64
    want = golden_K(case)
    K, _ = evaluate(table, kind, shape, X, X)
    assert np.max(np.abs(K - want)) <= 1e-12 * max(1.0, np.max(np.abs(want)))
    K12, _ = evaluate(table, kind, shape, X, Xs)
    assert np.max(np.abs(K12 - fx[case + "__K12"])) <= 1e-12 * max(1.0, np.max(np.abs(want)))
    kd = k.K_diag(fx[case + "__X"])
    assert np.max(np.abs(kd - fx[case + "__Kdiag"])) <= 1e-12 * max(1.0, np.max(np.abs(want)))
    assert np.max(np.abs(np.diag(K) - kd)) <= 1e-12 * max(1.0, np.max(np.abs(want)))      # what the library's relative jitter takes: sum over groups of prod A


@pytest.mark.parametrize("case", pc.FULL_CASES)
def test_chain_rule_reproduces_reference_gradients(case, monkeypatch):
    """gpr.Exact's own loss path (table push, kinds, moments -> table gradient -> _spectral_backward, the jitter term over groups) over the
    numpy device"""
    fx = load("product.npz")
    monkeypatch.setattr(_lib, "ExactHandle", GroupDevice)
    m = pc.exact(gpr, case)
    ps = with_reference_raw(m, fx, case + "__")
    loss = float(m.loss())
    assert abs(loss - float(fx[case + "__loss"])) <= 1e-9 * max(1.0, abs(float(fx[case + "__loss"])))
    assert (m._handle.kind is not None) == m.kernel._radial(m._handle.D)
    for i, p in enumerate(ps):
        g = fx["%s__p%d_grad" % (case, i)]
        assert np.max(np.abs(p.grad - g)) <= 1e-9 * max(1.0, np.max(np.abs(g))), (p._name, p.grad, g)


@pytest.mark.parametrize("expr", ["(se+m52)*cos", "se*cos*per", "locper*const", "(se+rq)*(cos+per)"])
def test_mulkernel_backward_against_finite_differences(expr):
    """f(raw parameters) = sum_ab G_ab K_ab with K evaluated from the table form in numpy; its gradient through the moments, the host formulas
    and MulKernel._spectral_backward against central differences"""
    rng = np.random.default_rng(11)
    k = pc.parse(gpr, expr, 1, rng)
    X = np.concatenate([np.zeros((25, 1)), rng.uniform(0, 6, (25, 1))], axis=1)
    G = rng.standard_normal((25, 25))

    def f():
        return float(np.sum(G * evaluate(k._spectral_terms(1), *k._spectral_kinds(1), X, X)[0]))

    table = k._spectral_terms(1)
    _, mom = evaluate(table, *k._spectral_kinds(1), X, X, G)
    for p in k.parameters():
        p.grad = None
    k._spectral_backward(_gtable_from_moments(table, mom.reshape(1, -1, 5), 1, lower=True))
    for p in k.parameters():
        got, raw = np.asarray(p.grad, dtype=np.float64).reshape(-1), p.data.reshape(-1)
        for i in range(raw.size):
            keep, h = raw[i], 1e-6
            raw[i] = keep + h; up = f()
            raw[i] = keep - h; dn = f()
            raw[i] = keep
            fd = (up - dn) / (2 * h)
            assert abs(got[i] - fd) <= 1e-6 * max(1.0, abs(fd)), (expr, p._name, got[i], fd)


def test_diagonal_is_the_product_of_the_factors():
    rng = np.random.default_rng(2)
    k = pc.parse(gpr, "(se+m52)*cos*const", 1, rng)
    se, m52 = k.kernels[0].kernels
    want = (float(se.magnitude()) + float(m52.magnitude())) * float(k.kernels[1].magnitude()) * float(k.kernels[2].magnitude())
    assert abs(k._spectral_diag(1)[0] - want) <= 1e-15 * want
    assert abs(gpr.Kernel._spectral_diag(k, 1)[0] - want) <= 4e-16 * want          # the table's own diagonal: sum over groups of prod A
    assert np.allclose(k.K_diag(np.zeros((3, 1))), want, rtol=1e-15)
    for p in k.parameters():
        p.grad = None
    k._spectral_diag_backward(np.array([1.0]), 1)
    link = lambda p: float(np.asarray(p.grad).reshape(-1)[0])
    h = 1e-6
    for p in (se.magnitude, k.kernels[1].magnitude, k.kernels[2].magnitude):
        keep = p.data.copy()
        p.data = keep + h; up = k._spectral_diag(1)[0]
        p.data = keep - h; dn = k._spectral_diag(1)[0]
        p.data = keep
        assert abs(link(p) - (up - dn) / (2 * h)) <= 1e-7
    assert k.kernels[1].lengthscale.grad is None or not np.any(k.kernels[1].lengthscale.grad)


def test_refusals_come_before_any_device_call(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "lib", no_device)
    monkeypatch.setattr(_lib, "ExactHandle", no_device)
    for cls in (gpr.PeriodicKernel, gpr.LocallyPeriodicKernel):
        with pytest.raises(NotImplementedError, match="order > 0"):
            cls(order=1, input_dims=1)
        with pytest.raises(NotImplementedError, match="input_dims > 1"):
            cls(input_dims=2)
    for cls in (gpr.ConstantKernel, gpr.CosineKernel, gpr.PeriodicKernel, gpr.LocallyPeriodicKernel):
        with pytest.raises(NotImplementedError, match="active_dims"):
            cls(active_dims=[0])
    five = gpr.MulKernel(*[gpr.CosineKernel() for _ in range(5)])
    with pytest.raises(NotImplementedError, match="more than 4"):
        five._spectral_terms(1)
    with pytest.raises(NotImplementedError, match="more than 4"):
        (gpr.LocallyPeriodicKernel() * gpr.LocallyPeriodicKernel() * gpr.CosineKernel())._spectral_kinds(1)
    mo = gpr.MultiOutputSpectralMixtureKernel(Q=1, output_dims=2)
    with pytest.raises(NotImplementedError, match="multi-output"):
        (mo * mo)._spectral_terms(1)
    X, y, _ = pc.data("m32_cos")
    Xc, yc, _ = pc.data("imo")
    sparse = dict(Titsias=dict(Z=4), Snelson=dict(Z=4), OpperArchambeau={}, SparseHensman=dict(Z=4), Hensman={})
    for name, kw in sparse.items():
        for build in (lambda: (pc.kernel(gpr, "m32_cos"), X, y), lambda: (gpr.PeriodicKernel(), X, y), lambda: (gpr.LocallyPeriodicKernel(), X, y),
                      lambda: (gpr.ConstantKernel() * gpr.SquaredExponentialKernel(), X, y), lambda: (pc.kernel(gpr, "imo"), Xc, yc),
                      lambda: (pc.kernel(gpr, "lmc"), Xc, yc)):
            with pytest.raises(NotImplementedError, match="%s.*product kernel" % name):
                getattr(gpr, name)(*build(), **kw)
        getattr(gpr, name)(gpr.ConstantKernel() + gpr.CosineKernel(), X, y, **kw)          # ordinary tables: accepted

    class Comm:                                                 # what use_distributed() leaves in config.comm
        native, world, rank, force = True, 2, 0, False
    saved = getattr(gpr.config, "comm", None)
    gpr.config.comm = Comm()
    try:
        m = pc.exact(gpr, "m32_cos")
        with pytest.raises(NotImplementedError, match="product kernels.*use_distributed"):
            m.loss()
        assert m._handle is None
    finally:
        gpr.config.comm = saved
    env = gpr.AddKernel(gpr.MultiOutputHarmonizableSpectralKernel(output_dims=1, input_dims=1),
                        gpr.IndependentMultiOutputKernel(gpr.SquaredExponentialKernel() * gpr.CosineKernel(), output_dims=1))
    with pytest.raises(NotImplementedError, match="enveloped"):
        env(np.zeros((4, 2)))


def test_header_and_bindings_carry_the_flag():
    src = open(os.path.join(ROOT, "include", "mogp_hip.h")).read()
    assert "#define MOGP_KIND_TIMES (1 << 8)" in src and "#define MOGP_KIND_PERIODIC 5" in src
    assert KIND_TIMES == 1 << 8 and gpr.singleoutput.KIND_PERIODIC == 5
    assert hasattr(_lib.lib(), "mogp_model_set_kinds") and hasattr(_lib.lib(), "mogp_gram_kinds")      # no new entry point: these carry the groups


CHECKPOINTS = ("mul", "lmc")


@pytest.mark.parametrize("tag", CHECKPOINTS)
def test_reference_checkpoint_round_trip(tag, tmp_path):
    pytest.importorskip("torch")
    from mogptk_amd import compat
    from test_host_logic import _checkpoint_tree, _tree_differences
    fx = load("product_checkpoints.npz")
    raw = fx[tag + "_file"].tobytes()
    (tmp_path / "ref.npy").write_bytes(raw)
    m = mogptk_amd.LoadModel(str(tmp_path / "ref"))
    ps = list(m.gpr.parameters())
    assert [p._name for p in ps] == [str(n) for n in fx[tag + "_names"]]
    for i, p in enumerate(ps):
        ref = fx["%s_p%d" % (tag, i)]
        assert np.asarray(p()).shape == ref.shape and np.max(np.abs(np.asarray(p()) - ref)) <= 1e-12 * max(1.0, np.max(np.abs(ref))), p._name

    def leaves_of(k):
        return [n for s in k.kernels for n in leaves_of(s)] + [type(k).__name__] if getattr(k, "kernels", None) else [type(k).__name__]
    want = dict(mul={"MulKernel", "CosineKernel", "LocallyPeriodicKernel", "ConstantKernel", "PeriodicKernel"}, lmc={"MulKernel", "CosineKernel", "ConstantKernel"})[tag]
    assert want <= set(leaves_of(m.gpr.kernel))
    if tag == "mul":
        assert m.gpr.kernel.kernels[0].kernels[1].order == -1
    written = compat.dump_reference_model(compat.load_reference_model(raw))
    assert compat.is_reference_checkpoint(written)
    theirs = _checkpoint_tree(compat._Unpickler(io.BytesIO(raw)).load(), {})
    ours = _checkpoint_tree(compat._Unpickler(io.BytesIO(written)).load(), {})
    out = []
    _tree_differences(theirs, ours, tag, out)
    assert not out, out[:5]
