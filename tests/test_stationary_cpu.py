"""
Host side of the stationary kernels (SquaredExponential, RationalQuadratic, Matern, Exponential), without a device: the class
surface against the reference's, the term table and kinds against a numpy evaluator of the radial form and the reference's K / K_diag
(tests/golden/stationary.npz, written by tests/golden/gen_stationary.py from the models of tests/stationary_cases.py), the chain rule
against the reference's autograd with the moments taken from that evaluator, the combinations that are refused, and checkpoints.
"""
import io
import numpy as np
import pytest

import mogptk_amd
from mogptk_amd import gpr, _lib
import stationary_cases as sc
from helpers import load

SQ3, SQ5 = np.sqrt(3.0), np.sqrt(5.0)


def golden_K(case):
    for tag in "ab":
        fx = load("stationary_gram_%s.npz" % tag)
        if case + "__K_tril" in fx:
            tril = fx[case + "__K_tril"]
            n = int(round((np.sqrt(8 * len(tril) + 1) - 1) / 2))
            K = np.zeros((n, n))
            K[np.tril_indices(n)] = tril
            return K + np.tril(K, -1).T
    raise KeyError(case)


def profiles(kind, shape, s):
    """phi(s) and psi(s) = -2 dphi/ds of DESIGN 1b; u psi and u^2 psi are 0 where Matern 1/2 has r = 0, so psi is returned as 0 there"""
    r = np.sqrt(s)
    if kind == 1:
        b = 1.0 + s / (2.0 * shape)
        return b ** -shape, b ** (-shape - 1.0)
    if kind == 2:
        return np.exp(-r), np.where(r > 0, np.exp(-r) / np.where(r > 0, r, 1.0), 0.0)
    if kind == 3:
        return (1.0 + SQ3 * r) * np.exp(-SQ3 * r), 3.0 * np.exp(-SQ3 * r)
    if kind == 4:
        return (1.0 + SQ5 * r + 5.0 * s / 3.0) * np.exp(-SQ5 * r), (5.0 / 3.0) * (1.0 + SQ5 * r) * np.exp(-SQ5 * r)
    return np.exp(-0.5 * s), np.exp(-0.5 * s)


def evaluate(table, kind, shape, Xa, Xb, G=None):
    """K(Xa, Xb) of a term table with kinds (inputs with the channel in column 0); with an adjoint G also the moments
    [m0, m4, m1_d, m2_d, m3_d] of every ordered channel pair, (C, C, T, 2 + 3 D)"""
    C, T, D = table.shape[0], table.shape[2], Xa.shape[1] - 1
    ca, cb = Xa[:, 0].astype(int), Xb[:, 0].astype(int)
    K = np.zeros((len(Xa), len(Xb)))
    mom = np.zeros((C, C, T, 2 + 3 * D))
    for i in range(C):
        for j in range(C):
            ia, ib = np.where(ca == i)[0], np.where(cb == j)[0]
            for t in range(T):
                A, Psi = table[i, j, t, 0], table[i, j, t, 1]
                V, M, Dl = table[i, j, t, 2:2 + D], table[i, j, t, 2 + D:2 + 2 * D], table[i, j, t, 2 + 2 * D:2 + 3 * D]
                u = Xa[ia, None, 1:] - Xb[None, ib, 1:] + Dl
                phi, psi = profiles(kind[i, j, t], shape[i, j, t], np.sum(V * u * u, axis=2))
                ph = 2.0 * np.pi * (np.sum(M * u, axis=2) + Psi)
                K[np.ix_(ia, ib)] += A * phi * np.cos(ph)
                if G is not None:
                    g = G[np.ix_(ia, ib)]
                    mom[i, j, t, 0], mom[i, j, t, 1] = np.sum(g * phi * np.cos(ph)), np.sum(g * phi * np.sin(ph))
                    for d in range(D):
                        mom[i, j, t, 2 + d] = np.sum(g * u[..., d] ** 2 * psi * np.cos(ph))
                        mom[i, j, t, 2 + D + d] = np.sum(g * u[..., d] * psi * np.cos(ph))
                        mom[i, j, t, 2 + 2 * D + d] = np.sum(g * u[..., d] * phi * np.sin(ph))
    return K, mom


class NumpyDevice:
    """what gpr.Exact asks of its device handle for a loss evaluation, answered by the evaluator above (symmetric sums over the full matrix:
    off-diagonal channel blocks count twice, the odd moments of a diagonal block are zero)"""

    def __init__(self, device, X, y, C):
        self.X, self.y, self.C, self.D = np.asarray(X, dtype=np.float64), np.asarray(y, dtype=np.float64).reshape(-1), C, X.shape[1] - 1
        self.kind = None

    def set_terms(self, table):
        self.table, self.T, self.W, self.kind = np.array(table), table.shape[2], table.shape[3], None

    def set_kinds(self, kind, shape):
        self.kind, self.shape = kind, shape

    def eval(self, noise_var, jitter, grad=True, data_var=None):
        C, N = self.C, len(self.y)
        kind = np.zeros(self.table.shape[:3], dtype=int) if self.kind is None else self.kind
        shape = np.zeros(self.table.shape[:3]) if self.kind is None else self.shape
        K, _ = evaluate(self.table, kind, shape, self.X, self.X)
        ch = self.X[:, 0].astype(int)
        jabs = jitter * np.mean(np.diag(K) + noise_var[ch])
        Kj = K + np.diag(noise_var[ch]) + jabs * np.eye(N)
        L = np.linalg.cholesky(Kj)
        alpha = np.linalg.solve(Kj, self.y)
        lml = -0.5 * N * np.log(2.0 * np.pi) - np.sum(np.log(np.diag(L))) - 0.5 * self.y @ alpha
        Gm = 0.5 * (np.outer(alpha, alpha) - np.linalg.inv(Kj))
        _, full = evaluate(self.table, kind, shape, self.X, self.X, Gm)
        D = self.D
        mom = np.zeros((C * (C + 1) // 2, self.T, self.W))
        for i in range(C):
            for j in range(i + 1):
                mom[i * (i + 1) // 2 + j] = full[i, j] if i == j else 2.0 * full[i, j]
                if i == j:
                    mom[i * (i + 1) // 2 + j][:, 1] = 0.0
                    mom[i * (i + 1) // 2 + j][:, 2 + D:2 + 2 * D] = 0.0
        diagG = np.array([np.sum(np.diag(Gm)[ch == c]) for c in range(C)])
        return dict(lml=lml, moments=mom, diagG=diagG, trG=float(np.sum(diagG)), jitter_abs=jabs)


def with_reference_raw(m, fx, pre):
    ps = list(m.parameters())
    assert [p._name for p in ps] == [str(n) for n in fx[pre + "names"]]
    for i, p in enumerate(ps):
        assert p.data.shape == fx["%sp%d_raw" % (pre, i)].shape, p._name
        p.data = np.array(fx["%sp%d_raw" % (pre, i)], dtype=p.data.dtype)
    return ps


def test_class_surface_matches_the_reference():
    k = gpr.SquaredExponentialKernel()
    assert (k.order, k.input_dims) == (0, 1) and k.magnitude().shape == () and k.lengthscale().shape == (1,)
    assert gpr.SquaredExponentialKernel(order=-1, input_dims=3).lengthscale().shape == ()
    assert gpr.SquaredExponentialKernel(input_dims=3).lengthscale().shape == (3,)
    k = gpr.RationalQuadraticKernel(0.7, 0, 2)                 # alpha, order, input_dims: the reference's order of arguments
    assert (k.alpha, k.order, k.input_dims) == (0.7, 0, 2) and k.lengthscale().shape == (2,)
    assert isinstance(k.alpha, float) and not isinstance(k.alpha, gpr.Parameter)
    assert gpr.RationalQuadraticKernel().alpha == 1.0
    k = gpr.MaternKernel(1.5, 1)
    assert k.nu == 1.5 and gpr.MaternKernel().nu == 0.5
    with pytest.raises(ValueError, match="nu parameter must be 0.5, 1.5, or 2.5"):
        gpr.MaternKernel(nu=2.0)
    assert gpr.ExponentialKernel(1).lengthscale().shape == (1,)
    for k in (gpr.SquaredExponentialKernel(), gpr.RationalQuadraticKernel(), gpr.ExponentialKernel()):
        assert float(k.magnitude.lower) == float(k.lengthscale.lower) == gpr.config.positive_minimum
    k = gpr.MaternKernel()
    assert float(k.magnitude.lower) == float(k.lengthscale.lower) == 1e-6
    for k in (gpr.SquaredExponentialKernel(), gpr.RationalQuadraticKernel(), gpr.MaternKernel(), gpr.ExponentialKernel()):
        assert abs(float(k.magnitude()) - 1.0) < 2e-5 and np.all(np.abs(k.lengthscale() - 1.0) < 2e-5)      # (through the softplus link, as in the reference)
        assert [p._name.split(".")[-1] for p in k.parameters()] == ["magnitude", "lengthscale"]


@pytest.mark.parametrize("case", list(sc.CASES))
def test_parameter_order_and_printing_match_the_reference(case, capsys):
    fx = load("stationary.npz")
    m = sc.exact(gpr, case)
    ps = with_reference_raw(m, fx, case + "__")
    for i, p in enumerate(ps):
        ref = fx["%s__p%d_cons" % (case, i)]
        assert np.max(np.abs(np.asarray(p()) - ref)) <= 1e-14 * max(1.0, np.max(np.abs(ref))), p._name
    m.print_parameters()
    lines = capsys.readouterr().out.splitlines()[1:]
    assert [ln.split()[0] for ln in lines] == [str(n) for n in fx[case + "__names"]]


@pytest.mark.parametrize("case", sc.FULL_CASES)
def test_table_and_kinds_reproduce_the_reference_gram(case):
    fx = load("stationary.npz")
    m = sc.exact(gpr, case)
    with_reference_raw(m, fx, case + "__")
    k = m.kernel
    X, Xs = k._kernel_format(fx[case + "__X"]), k._kernel_format(fx[case + "__Xs"])
    D = X.shape[1] - 1
    table = k._spectral_terms(D)
    kind, shape = k._spectral_kinds(D)
    assert kind.shape == table.shape[:3] == shape.shape and kind.dtype == np.int32 and shape.dtype == np.float64
    assert np.all(kind[table[..., 0] == 0.0] == 0)             # padding rows are Gaussian
    want = golden_K(case)
    K, _ = evaluate(table, kind, shape, X, X)
    assert np.max(np.abs(K - want)) <= 1e-12 * max(1.0, np.max(np.abs(want)))
    K12, _ = evaluate(table, kind, shape, X, Xs)
    assert np.max(np.abs(K12 - fx[case + "__K12"])) <= 1e-12 * max(1.0, np.max(np.abs(want)))
    kd = k.K_diag(fx[case + "__X"])
    assert np.max(np.abs(kd - fx[case + "__Kdiag"])) <= 1e-12 * max(1.0, np.max(np.abs(want)))


def test_kinds_of_the_cases():
    kinds = lambda case: sc.kernel(gpr, case)._spectral_kinds(sc.CASES[case].get("D", 1))
    assert not gpr.SquaredExponentialKernel()._radial(1) and not sc.kernel(gpr, "se_d2")._radial(2)
    assert kinds("rq")[0].tolist() == [[[1]]] and kinds("rq")[1].tolist() == [[[0.7]]]
    assert [kinds(c)[0][0, 0, 0] for c in ("m12", "m32", "m52", "exp")] == [2, 3, 4, 2]
    assert kinds("sum")[0][0, 0].tolist() == [0, 3, 0]
    kd, sh = kinds("imo")                                        # different kinds at the same t, nothing off the block diagonal
    assert kd[:, :, 0].tolist() == [[1, 0], [0, 4]] and sh[0, 0, 0] == 0.7
    kd, _ = kinds("lmc")
    assert kd.shape == (2, 2, 2) and np.all(kd[..., 0] == 0) and np.all(kd[..., 1] == 3)
    mix = gpr.MixtureKernel(gpr.MaternKernel(nu=2.5), 3)
    assert mix._spectral_kinds(1)[0][0, 0].tolist() == [4, 4, 4]


@pytest.mark.parametrize("case", sc.FULL_CASES)
def test_chain_rule_reproduces_reference_gradients(case, monkeypatch):
    """gpr.Exact's own loss path (table push, kinds, moments -> table gradient -> _spectral_backward) over the numpy device"""
    fx = load("stationary.npz")
    monkeypatch.setattr(_lib, "ExactHandle", NumpyDevice)
    m = sc.exact(gpr, case)
    ps = with_reference_raw(m, fx, case + "__")
    loss = float(m.loss())
    assert abs(loss - float(fx[case + "__loss"])) <= 1e-9 * max(1.0, abs(float(fx[case + "__loss"])))
    assert (m._handle.kind is not None) == m.kernel._radial(m._handle.D)      # kinds travel only when some kind is non-zero
    for i, p in enumerate(ps):
        g = fx["%s__p%d_grad" % (case, i)]
        assert np.max(np.abs(p.grad - g)) <= 1e-9 * max(1.0, np.max(np.abs(g))), (p._name, p.grad, g)


def test_refusals_come_before_any_device_call(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "lib", no_device)
    monkeypatch.setattr(_lib, "ExactHandle", no_device)
    for cls in (gpr.SquaredExponentialKernel, gpr.RationalQuadraticKernel):
        with pytest.raises(NotImplementedError, match="order > 0"):
            cls(order=1, input_dims=2)
    with pytest.raises(NotImplementedError, match="input_dims > 1"):
        gpr.MaternKernel(nu=1.5, input_dims=2)
    with pytest.raises(NotImplementedError, match="input_dims > 1"):
        gpr.ExponentialKernel(input_dims=2)
    for cls in (gpr.SquaredExponentialKernel, gpr.RationalQuadraticKernel, gpr.MaternKernel, gpr.ExponentialKernel):
        with pytest.raises(NotImplementedError, match="active_dims"):
            cls(active_dims=[0])
    X, y, _ = sc.data("m32")
    Xc, yc, _ = sc.data("imo")
    sparse = dict(Titsias=dict(Z=4), Snelson=dict(Z=4), OpperArchambeau={}, SparseHensman=dict(Z=4), Hensman={})
    for name, kw in sparse.items():
        for build in (lambda: (gpr.MaternKernel(nu=1.5), X, y), lambda: (gpr.RationalQuadraticKernel(), X, y), lambda: (gpr.ExponentialKernel(), X, y),
                      lambda: (gpr.SquaredExponentialKernel() + gpr.MaternKernel(nu=0.5), X, y), lambda: (sc.kernel(gpr, "imo"), Xc, yc),
                      lambda: (sc.kernel(gpr, "lmc"), Xc, yc)):
            with pytest.raises(NotImplementedError, match=name):
                getattr(gpr, name)(*build(), **kw)
        getattr(gpr, name)(gpr.SquaredExponentialKernel(), X, y, **kw)          # kind 0 is an ordinary table: accepted

    class Comm:                                                 # what use_distributed() leaves in config.comm
        native, world, rank, force = True, 2, 0, False
    saved = getattr(gpr.config, "comm", None)
    gpr.config.comm = Comm()
    try:
        m = sc.exact(gpr, "m32")
        with pytest.raises(NotImplementedError, match="use_distributed"):
            m.loss()
        with pytest.raises(NotImplementedError, match="use_distributed"):
            m.predict_f(X[:5])
        assert m._handle is None
    finally:
        gpr.config.comm = saved


CHECKPOINTS = ("add", "imo", "lmc")


@pytest.mark.parametrize("tag", CHECKPOINTS)
def test_reference_checkpoint_loads(tag, tmp_path):
    pytest.importorskip("torch")
    fx = load("stationary_checkpoints.npz")
    (tmp_path / "ref.npy").write_bytes(fx[tag + "_file"].tobytes())
    m = mogptk_amd.LoadModel(str(tmp_path / "ref"))
    ps = list(m.gpr.parameters())
    assert [p._name for p in ps] == [str(n) for n in fx[tag + "_names"]]
    for i, p in enumerate(ps):
        ref = fx["%s_p%d" % (tag, i)]
        assert np.asarray(p()).shape == ref.shape
        assert np.max(np.abs(np.asarray(p()) - ref)) <= 1e-12 * max(1.0, np.max(np.abs(ref))), p._name
    def leaves_of(k):
        return [n for s in k.kernels for n in leaves_of(s)] if getattr(k, "kernels", None) else [type(k).__name__]
    leaves = leaves_of(m.gpr.kernel)
    want = dict(add={"SquaredExponentialKernel", "MaternKernel", "RationalQuadraticKernel", "ExponentialKernel"},
                imo={"RationalQuadraticKernel", "MaternKernel"}, lmc={"SquaredExponentialKernel", "ExponentialKernel", "MaternKernel"})[tag]
    assert want <= set(leaves), leaves
    if tag == "add":
        add = m.gpr.kernel.kernels[0]
        assert add.kernels[0].order == -1 and add.kernels[1].nu == 1.5 and add.kernels[2].alpha == 0.7
    if tag == "imo":
        assert m.gpr.kernel.kernels[0].alpha == 1.3 and m.gpr.kernel.kernels[1].nu == 2.5


@pytest.mark.parametrize("tag", CHECKPOINTS)
def test_reference_checkpoint_is_written_as_the_reference_writes_it(tag):
    pytest.importorskip("torch")
    from mogptk_amd import compat
    from test_host_logic import _checkpoint_tree, _tree_differences
    fx = load("stationary_checkpoints.npz")
    raw = fx[tag + "_file"].tobytes()
    written = compat.dump_reference_model(compat.load_reference_model(raw))
    assert compat.is_reference_checkpoint(written)
    theirs = _checkpoint_tree(compat._Unpickler(io.BytesIO(raw)).load(), {})
    ours = _checkpoint_tree(compat._Unpickler(io.BytesIO(written)).load(), {})
    out = []
    _tree_differences(theirs, ours, tag, out)
    assert not out, out[:5]
    m = compat.load_reference_model(written)
    for i, p in enumerate(m.gpr.parameters()):
        assert np.max(np.abs(np.asarray(p()) - fx["%s_p%d" % (tag, i)])) <= 1e-12 * max(1.0, np.max(np.abs(fx["%s_p%d" % (tag, i)])))
