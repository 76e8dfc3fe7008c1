"""
What the tests of the kernel families share (family_cases.FAMILIES: stationary, product, trend): the goldens of a family, and the bodies of
the tests that every family runs on its own cases -- on the CPU over the numpy twin of the device handle (oracle/table_model.py), on the
device in tests/test_<family>_gpu.py.  A test file names its family and calls these; what only one family asserts stays in its file.
Tolerances: DESIGN 8, relative to max(1, max |want|).
"""
import io
import os
import numpy as np

import mogptk_amd
from mogptk_amd import gpr, _lib
from mogptk_amd.gpr.kernel import KIND_TIMES
from family_cases import cases, exact
from helpers import load
from oracle.table_model import TableDevice, gram_from_table


def golden_K(family, case):
    for tag in "ab":
        fx = load("%s_gram_%s.npz" % (family, tag))
        if case + "__K_tril" in fx:
            tril = fx[case + "__K_tril"]
            n = int(round((np.sqrt(8 * len(tril) + 1) - 1) / 2))
            K = np.zeros((n, n))
            K[np.tril_indices(n)] = tril
            return K + np.tril(K, -1).T
    raise KeyError(case)


def with_reference_raw(m, fx, pre):
    ps = list(m.parameters())
    assert [p._name for p in ps] == [str(n) for n in fx[pre + "names"]]
    for i, p in enumerate(ps):
        assert p.data.shape == fx["%sp%d_raw" % (pre, i)].shape, p._name
        p.data = np.array(fx["%sp%d_raw" % (pre, i)], dtype=p.data.dtype)
    return ps


def reference_model(family, case):
    """(the case's exact model at the reference's raw parameters, its parameters, the family's fixture)"""
    fx = load(family + ".npz")
    m = exact(family, gpr, case)
    return m, with_reference_raw(m, fx, case + "__"), fx


def err(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return np.max(np.abs(a - b)) / max(1.0, np.max(np.abs(b)))


def check_value_and_gradients(m, fx, pre):
    ps = with_reference_raw(m, fx, pre)
    lml = float(m.log_marginal_likelihood())
    e = err(lml, float(fx[pre + "lml"]))
    print(pre, "lml", e)
    assert e <= 1e-9, (lml, float(fx[pre + "lml"]))
    loss = float(m.loss())
    e = err(loss, float(fx[pre + "loss"]))
    print(pre, "loss", e)
    assert e <= 1e-9
    for i, p in enumerate(ps):
        e = err(p.grad, fx["%sp%d_grad" % (pre, i)])
        print(pre, p._name, "grad", e)
        assert e <= 1e-7, (p._name, p.grad, fx["%sp%d_grad" % (pre, i)])


def check_predictions(family, case):
    """predict_f (diagonal and full) and predict_y of whatever device handle the model gets"""
    m, _, fx = reference_model(family, case)
    pre = case + "__"
    Xs = fx[pre + "Xs"]
    mu, var = m.predict_f(Xs)
    mu2, cov = m.predict_f(Xs, full=True)
    ymu, yvar = m.predict_y(Xs)[:2]
    for name, got, want in (("mu", mu, fx[pre + "mu"]), ("var", var, fx[pre + "var"]), ("mu(full)", mu2, fx[pre + "mu"]), ("cov", cov, fx[pre + "cov"]),
                            ("ymu", ymu, fx[pre + "ymu"]), ("yvar", yvar, fx[pre + "yvar"])):
        e = err(np.asarray(got).reshape(np.shape(want)), want)
        print(pre, name, e)
        assert e <= 1e-9, name


# ---- without a device: the numpy twin ---------------------------------------------------------------------------------------------------
def check_table_and_kinds(family, case):
    """the case's table, kinds and shapes through the twin's Gram against the reference's K, K(X, Xs) and K_diag; -> what a family's own
    assertions need: (kernel, table, kind, shape, X with the channel column, the twin's K, the reference's K, the tolerance)"""
    m, _, fx = reference_model(family, case)
    k = m.kernel
    X, Xs = k._kernel_format(fx[case + "__X"]), k._kernel_format(fx[case + "__Xs"])
    D = X.shape[1] - 1
    table = k._spectral_terms(D)
    kind, shape = k._spectral_kinds(D)
    assert kind.shape == table.shape[:3] == shape.shape and shape.dtype == np.float64
    want = golden_K(family, case)
    tol = 1e-12 * max(1.0, np.max(np.abs(want)))
    K = gram_from_table(table, X, kind=kind, shape=shape)
    assert np.max(np.abs(K - want)) <= tol
    assert np.max(np.abs(gram_from_table(table, X, Xs, kind, shape) - fx[case + "__K12"])) <= tol
    kd = k.K_diag(fx[case + "__X"])
    assert np.max(np.abs(kd - fx[case + "__Kdiag"])) <= tol
    assert np.max(np.abs(np.diag(K) - kd)) <= tol           # what the relative jitter takes: per point, the sum over groups of the product of the rows' diagonals
    return k, table, kind, shape, X, K, want, tol


def check_chain_rule(family, case, monkeypatch):
    """gpr.Exact's own loss path (table push, kinds, per-point diagonal, moments -> table gradient -> _spectral_backward, the jitter term)
    over the twin, against the reference's autograd; -> the model"""
    monkeypatch.setattr(_lib, "ExactHandle", TableDevice)
    m, ps, fx = reference_model(family, case)
    loss = float(m.loss())
    assert abs(loss - float(fx[case + "__loss"])) <= 1e-9 * max(1.0, abs(float(fx[case + "__loss"])))
    h = m._handle
    assert (h.kind is not None) == m.kernel._radial(h.D)      # kinds travel only when some kind is non-zero,
    assert (h.point_diag is not None) == m.kernel._pointwise(h.D)      # the per-point diagonal only with a dot-product row
    for i, p in enumerate(ps):
        g = fx["%s__p%d_grad" % (case, i)]
        assert np.max(np.abs(p.grad - g)) <= 1e-9 * max(1.0, np.max(np.abs(g))), (p._name, p.grad, g)
    return m


def kernel_names(k):
    """class names of a kernel and of everything composed under it"""
    return [n for s in getattr(k, "kernels", None) or [] for n in kernel_names(s)] + [type(k).__name__]


def check_checkpoint_loads(family, tag, tmp_path):
    """a file the reference's Model.save() wrote: names and constrained values of the loaded model; -> its kernel"""
    fx = load(family + "_checkpoints.npz")
    (tmp_path / "ref.npy").write_bytes(fx[tag + "_file"].tobytes())
    m = mogptk_amd.LoadModel(str(tmp_path / "ref"))
    ps = list(m.gpr.parameters())
    assert [p._name for p in ps] == [str(n) for n in fx[tag + "_names"]]
    for i, p in enumerate(ps):
        ref = fx["%s_p%d" % (tag, i)]
        assert np.asarray(p()).shape == ref.shape
        assert np.max(np.abs(np.asarray(p()) - ref)) <= 1e-12 * max(1.0, np.max(np.abs(ref))), p._name
    return m.gpr.kernel


def check_checkpoint_is_written_as_the_reference_writes_it(family, tag):
    """load and dump again: the same pickle tree; -> (the bytes written, the fixture)"""
    from mogptk_amd import compat
    from test_host_logic import _checkpoint_tree, _tree_differences
    fx = load(family + "_checkpoints.npz")
    raw = fx[tag + "_file"].tobytes()
    written = compat.dump_reference_model(compat.load_reference_model(raw))
    assert compat.is_reference_checkpoint(written)
    theirs = _checkpoint_tree(compat._Unpickler(io.BytesIO(raw)).load(), {})
    ours = _checkpoint_tree(compat._Unpickler(io.BytesIO(written)).load(), {})
    out = []
    _tree_differences(theirs, ours, tag, out)
    assert not out, out[:5]
    return written, fx


# ---- on the device ----------------------------------------------------------------------------------------------------------------------
def check_gram_matrices(family, case):
    m, _, fx = reference_model(family, case)
    pre = case + "__"
    X, Xs = fx[pre + "X"], fx[pre + "Xs"]
    for name, got, want in (("K", m.kernel(X), golden_K(family, case)), ("K12", m.kernel(X, Xs), fx[pre + "K12"]), ("Kdiag", m.kernel.K_diag(X), fx[pre + "Kdiag"])):
        e = err(got, want)
        print(pre, name, e)
        assert e <= 1e-12, name


def check_both_schedules(family):
    """N = 1100: nine 128-row tiles, the Gram build split into its head and tail launches; MOGP_FLOW is read per evaluation"""
    fx = load(family + ".npz")
    old = {k: os.environ.get(k) for k in ("MOGP_FLOW", "MOGP_FLOW_MIN")}
    try:
        os.environ.pop("MOGP_FLOW", None); os.environ.pop("MOGP_FLOW_MIN", None)
        m = exact(family, gpr, "big")
        check_value_and_gradients(m, fx, "big__")
        assert m._handle.schedule()["dataflow"], m._handle.schedule()
        os.environ["MOGP_FLOW"] = "0"
        m = exact(family, gpr, "big")
        check_value_and_gradients(m, fx, "big__")
        assert not m._handle.schedule()["dataflow"]
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


def check_bit_identical_repeats(family, case):
    m, ps, _ = reference_model(family, case)
    first = None
    for _ in range(30):
        loss = float(m.loss())
        got = [np.float64(loss).tobytes()] + [p.grad.tobytes() for p in ps]
        if first is None:
            first = got
        assert got == first


def check_adam_trace(family):
    fx = load(family + ".npz")
    sc = cases(family)
    X, y, _ = sc.data(sc.ADAM_CASE)
    mm = mogptk_amd.Model(mogptk_amd.DataSet(mogptk_amd.Data(X[:, 0], y, name="a")),
                          gpr.IndependentMultiOutputKernel(sc.kernel(gpr, sc.ADAM_CASE), output_dims=1), inference=mogptk_amd.Exact(variance=sc.NOISE))
    losses, _ = mm.train(method="Adam", iters=sc.ADAM_ITERS, lr=sc.ADAM_LR, verbose=False)
    want = fx["adam__losses"]
    e = err(np.asarray(losses, dtype=np.float64), want)
    print("adam trace", e)
    assert e <= 1e-7
    final = np.concatenate([np.asarray(p.data, dtype=np.float64).reshape(-1) for p in mm.gpr.parameters()])
    assert err(final, fx["adam__final"]) <= 1e-7


def check_models_without_the_new_kinds_are_untouched():
    """Neutrality.  A SpectralMixtureKernel model makes no set_kinds call at all (the Gaussian instantiations are the parent's, instruction
    for instruction: profiles/stationary_kernels.txt) and supplies no per-point diagonal.  The stationary `sum` model of stationary_cases.py
    sends kinds 0 and 3 only, without a flag, every row a group of one that takes the plain radial term: its loss still matches the
    reference, and repeating it gives the same bits."""
    rng = np.random.default_rng(3)
    X = np.sort(rng.uniform(0, 10, (300, 1)), axis=0)
    y = np.sin(X[:, 0]) + 0.1 * rng.standard_normal(300)
    k = gpr.SpectralMixtureKernel(Q=3, input_dims=1)
    k.magnitude.assign([0.9, 0.5, 0.7]); k.mean.assign([[0.1], [0.25], [0.4]]); k.variance.assign([[0.05], [0.02], [0.08]])
    calls, diag_calls = [], []
    real, real_diag = _lib.ExactHandle.set_kinds, _lib.ExactHandle.set_point_diag
    _lib.ExactHandle.set_kinds = lambda self, *a: (calls.append(a), real(self, *a))[1]
    _lib.ExactHandle.set_point_diag = lambda self, *a: (diag_calls.append(a), real_diag(self, *a))[1]
    try:
        m = gpr.Exact(k, X, y, variance=0.1)
        l0 = float(m.loss())
        assert not calls and np.isfinite(l0)                    # all-Gaussian, no product: not one extra call
        m, ps, fx = reference_model("stationary", "sum")
        l1 = float(m.loss())
        g1 = [p.grad.copy() for p in ps]
        assert len(calls) == 1 and not np.any(calls[0][0] & KIND_TIMES) and calls[0][0][0, 0].tolist() == [0, 3, 0]
        assert err(l1, float(fx["sum__loss"])) <= 1e-9
        l2 = float(m.loss())                                    # the same kinds again: the same bits
        assert np.float64(l1).tobytes() == np.float64(l2).tobytes() and all(g.tobytes() == p.grad.tobytes() for g, p in zip(g1, ps))
    finally:
        _lib.ExactHandle.set_kinds, _lib.ExactHandle.set_point_diag = real, real_diag
    assert not diag_calls
