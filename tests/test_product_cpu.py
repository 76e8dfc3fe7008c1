"""
Host side of the product kernels and of ConstantKernel, CosineKernel, PeriodicKernel and LocallyPeriodicKernel, without a device:
tables, kinds and group flags of every case of tests/product_cases.py against hand-written expectations; the grouped table form through
the numpy twin of the device handle (oracle/table_model.py) against the reference's K / K_diag (tests/golden/product.npz, written by
tests/golden/gen_family.py); the chain rule through MulKernel against finite differences of the twin's Gram and against the reference's
autograd; the refusals; checkpoints.  The bodies shared with the other kernel families are in tests/kernel_family.py.
"""
import os
import numpy as np
import pytest

from mogptk_amd import gpr, _lib
from mogptk_amd.gpr.kernel import KIND_TIMES
from mogptk_amd.gpr.model import _gtable_from_moments
import product_cases as pc
import kernel_family as kf
from family_cases import exact, full_cases
from oracle.table_model import gram_from_table, moments_dense

FAMILY = "product"
X_ = KIND_TIMES
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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


@pytest.mark.parametrize("case", full_cases(FAMILY))
def test_table_and_kinds_reproduce_the_reference_gram(case):
    kf.check_table_and_kinds(FAMILY, case)


@pytest.mark.parametrize("case", full_cases(FAMILY))
def test_chain_rule_reproduces_reference_gradients(case, monkeypatch):
    kf.check_chain_rule(FAMILY, case, monkeypatch)


@pytest.mark.parametrize("expr", ["(se+m52)*cos", "se*cos*per", "locper*const", "(se+rq)*(cos+per)"])
def test_mulkernel_backward_against_finite_differences(expr):
    """f(raw parameters) = sum_ab G_ab K_ab with K evaluated from the table form by the twin; its gradient through the moments, the host formulas
    and MulKernel._spectral_backward against central differences"""
    rng = np.random.default_rng(11)
    k = pc.parse(gpr, expr, 1, rng)
    X = np.concatenate([np.zeros((25, 1)), rng.uniform(0, 6, (25, 1))], axis=1)
    G = rng.standard_normal((25, 25))

    def f():
        return float(np.sum(G * gram_from_table(k._spectral_terms(1), X, X, *k._spectral_kinds(1))))

    table = k._spectral_terms(1)
    mom = moments_dense(table, G, X, X, False, *k._spectral_kinds(1))      # one channel: its one ordered pair is its one lower pair
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
        m = exact(FAMILY, gpr, "m32_cos")
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
    k = kf.check_checkpoint_loads(FAMILY, tag, tmp_path)
    want = dict(mul={"MulKernel", "CosineKernel", "LocallyPeriodicKernel", "ConstantKernel", "PeriodicKernel"}, lmc={"MulKernel", "CosineKernel", "ConstantKernel"})[tag]
    assert want <= set(kf.kernel_names(k))
    if tag == "mul":
        assert k.kernels[0].kernels[1].order == -1
    kf.check_checkpoint_is_written_as_the_reference_writes_it(FAMILY, tag)
