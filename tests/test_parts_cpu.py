"""
The posterior by kernel part without a device: gpr.Exact.parts / predict_terms / predict_parts -- the partition rules, the masking
rule, the parts' prior diagonals, chunking, mean and data variance -- over the numpy twin (tests/parts_twin.py) against the reference-side
goldens (tests/golden/parts.npz, gen_parts.py: one reference kernel object per part), and the public surface.  Tolerances: 1e-9 relative to
max(1, max |want|) for mu, var and cov (kernel_family.check_predictions), 1e-12 for Gram matrices (check_table_and_kinds).
"""
import numpy as np
import pytest

import mogptk_amd
import oracle.table_model as tm
from mogptk_amd import gpr
from mogptk_amd.gpr.config import config

import parts_cases
import parts_twin
from helpers import load
from kernel_family import err, with_reference_raw

FX = load("parts.npz")
TWIN = {"change": "changepoint", "basis": "function"}


def model(case):
    m = parts_cases.exact(gpr, case)
    with_reference_raw(m, FX, case + "__")
    return m, parts_cases.data(case)[2]


def masked_tables(m, masks):
    """the masking rule, written out again: the table the model pushed with the amplitudes of the dropped rows, and the bias of dropped
    dot-product rows, set to zero"""
    h = m._handle
    tabs = np.repeat(h.table[None], len(masks), axis=0)
    for p, mask in enumerate(masks):
        tabs[p][~mask, 0] = 0.0
        if h.kind is not None:
            tabs[p][~mask & ((np.asarray(h.kind) & 0xff) == 7), 1] = 0.0
    return tabs


def check_case(case):
    pre = case + "__"
    c = parts_cases.CASES[case]
    m, Xs = model(case)
    names, mu, var = m.predict_parts(Xs)
    P, S = FX[pre + "mu"].shape
    assert len(names) == P and mu.shape == var.shape == (P, S, 1) and mu.dtype == var.dtype == config.dtype
    for name, got in (("mu", mu), ("var", var)):
        e = err(got[..., 0], FX[pre + name])
        print(pre, name, e)
        assert e <= 1e-9, name
    if c.get("full"):
        _, mu_f, cov = m.predict_parts(Xs, full=True)
        e, e_mu = err(cov, FX[pre + "cov"]), err(mu_f[..., 0], FX[pre + "mu"])
        print(pre, "cov", e, e_mu)
        assert cov.shape == (P, S, S) and e <= 1e-9 and e_mu <= 1e-9
    return m, Xs, names, mu, var


@pytest.mark.parametrize("case", list(parts_cases.CASES))
def test_twin_matches_the_reference(case, monkeypatch):
    parts_twin.install(monkeypatch, TWIN.get(case))
    m, Xs, names, mu, var = check_case(case)
    h = m._handle
    assert isinstance(h, parts_twin.PartsTableDevice)
    if parts_cases.CASES[case].get("light"):
        return
    # the masked tables against the reference's own kernel per part, and their sum against the whole table
    masks = [mk for _, mk in m.parts()]
    tabs = masked_tables(m, masks)
    Xk, Xsk = m.kernel._kernel_format(m.X), m.kernel._kernel_format(Xs)[:parts_cases.KROWS]
    grams = [tm.gram_from_table(t, Xsk, Xk, h.kind, h.shape) for t in tabs]
    for p, K in enumerate(grams):
        e = err(K, FX[case + "__Ksx"][p])
        print(case, "Ksx", p, e)
        assert e <= 1e-12, p
    assert err(sum(grams), tm.gram_from_table(h.table, Xsk, Xk, h.kind, h.shape)) <= 1e-12


def test_the_white_part_is_its_amplitude_and_nothing_else(monkeypatch):
    parts_twin.install(monkeypatch, "function")
    m, Xs = model("basis")
    names, mu, var = m.predict_parts(Xs)
    assert names[2] == "2:WhiteKernel"
    A = float(m.kernel.kernels[2].magnitude())
    assert np.all(mu[2] == 0.0) and np.all(var[2] == A)
    _, _, cov = m.predict_parts(Xs, full=True)
    assert np.array_equal(cov[2], A * np.eye(len(Xs)))


# ---- partition rules ---------------------------------------------------------------------------------------------------------------
def test_partition_of_sums_and_mixtures():
    m, _ = model("trend")                                     # Linear + Periodic * SE + Matern 1/2: rows [lin | per, se | m12]
    named = m.parts()
    assert [n for n, _ in named] == ["0:LinearKernel", "1:" + m.kernel.kernels[1].name(), "2:MaternKernel"]
    assert [mk[0, 0].tolist() for _, mk in named] == [[True, False, False, False], [False, True, True, False], [False, False, False, True]]
    m, _ = model("csm")
    named = m.parts()
    assert [n for n, _ in named] == ["0:CrossSpectralKernel", "1:CrossSpectralKernel"]
    assert all(mk.shape == (2, 2, 4) for _, mk in named)
    assert np.all(named[0][1][..., :2]) and not np.any(named[0][1][..., 2:]) and np.array_equal(named[1][1], ~named[0][1])
    m, _ = model("mohsm")
    assert [mk[0, 0].tolist() for _, mk in m.parts()] == [[True, False], [False, True]]


def test_partition_by_component_and_by_base_kernel():
    m, _ = model("mosm")
    named = m.parts()
    assert [n for n, _ in named] == ["0:MultiOutputSpectralMixtureKernel", "1:MultiOutputSpectralMixtureKernel"]
    assert all(mk.shape == (3, 3, 2) for _, mk in named) and np.all(named[0][1][..., 0]) and not np.any(named[0][1][..., 1])
    k = gpr.SpectralMixtureKernel(Q=3, input_dims=2)
    named = k._parts(2)
    assert [mk[0, 0].tolist() for _, mk in named] == [[True] * 2 + [False] * 4, [False] * 2 + [True] * 2 + [False] * 2, [False] * 4 + [True] * 2]
    m, _ = model("smlmc")                                     # two base kernels of two rows each
    named = m.parts()
    assert [n for n, _ in named] == ["0:SpectralMixtureKernel", "1:SpectralMixtureKernel"]
    assert [mk[1, 0].tolist() for _, mk in named] == [[True, True, False, False], [False, False, True, True]]
    # a dot-product row first in its group: the leading coregionalization row belongs to the base kernel's part
    k = gpr.LinearModelOfCoregionalizationKernel(gpr.LinearKernel(input_dims=1), gpr.SquaredExponentialKernel(order=0, input_dims=1), output_dims=2, input_dims=1)
    assert [mk[0, 1].tolist() for _, mk in k._parts(1)] == [[True, True, False], [False, False, True]]


def test_partition_of_independent_channels():
    m, _ = model("imo")                                       # SE + Cosine in both channels: shared rows, pair (c, c) only
    named = m.parts()
    assert [n for n, _ in named] == ["0:SquaredExponentialKernel,SquaredExponentialKernel", "1:CosineKernel,CosineKernel"]
    for i, (_, mk) in enumerate(named):
        assert mk.shape == (2, 2, 2) and not np.any(mk[0, 1]) and not np.any(mk[1, 0])
        assert mk[0, 0].tolist() == mk[1, 1].tolist() == [i == 0, i == 1]
    se = lambda: gpr.SquaredExponentialKernel(order=0, input_dims=1)
    k = gpr.IndependentMultiOutputKernel(gpr.AddKernel(se(), se()), se(), output_dims=2)
    X = np.concatenate([np.repeat([[0.0], [1.0]], 5, axis=0), np.linspace(0, 1, 10)[:, None]], axis=1)
    m = gpr.Exact(k, X, np.zeros(10), variance=0.1)
    with pytest.raises(NotImplementedError, match="predict_terms"):
        m.parts()
    with pytest.raises(NotImplementedError, match="predict_terms"):
        m.predict_parts(X)
    # anything else: one part, the whole kernel
    k = gpr.MulKernel(se(), gpr.CosineKernel(input_dims=1))
    named = k._parts(1)
    assert len(named) == 1 and named[0][0] == k.name() and np.all(named[0][1]) and named[0][1].shape == (1, 1, 2)


def test_a_mask_that_cuts_a_product_group_is_refused(monkeypatch):
    parts_twin.install(monkeypatch)
    m, Xs = model("trend")
    with pytest.raises(ValueError, match="rows 1 .. 2"):
        m.predict_terms(Xs, np.array([[True, True, False, False], [False, False, True, True]]))
    with pytest.raises(ValueError):
        m.predict_terms(Xs, np.ones((1, 3), dtype=bool))       # not the table's T
    with pytest.raises(ValueError):
        m.predict_terms(Xs, np.ones((1, 4)))                   # not boolean


def test_predict_terms_takes_masks_per_channel_pair(monkeypatch):
    parts_twin.install(monkeypatch)
    m, Xs = model("imo")
    names, mu, var = m.predict_parts(Xs)
    masks = np.stack([mk for _, mk in m.parts()])
    assert masks.shape == (2, 2, 2, 2)
    mu2, var2 = m.predict_terms(Xs, masks)
    assert np.array_equal(mu, mu2) and np.array_equal(var, var2)
    # the same rows in every pair, as (P, T): off the diagonal pairs the amplitudes are zero anyway
    mu3, var3 = m.predict_terms(Xs, masks[:, 0, 0])
    assert np.array_equal(mu, mu3) and np.array_equal(var, var3)
    # one channel's SE row alone: the other channel's test points get nothing from it
    only = np.zeros((1, 2, 2, 2), dtype=bool)
    only[0, 1, 1, 0] = True
    mu4, var4 = m.predict_terms(Xs, only)
    ch = Xs[:, 0] == 0
    assert np.all(mu4[0, ch] == 0.0) and np.all(var4[0, ch] == 0.0) and np.array_equal(mu4[0, ~ch], mu[0, ~ch])


@pytest.mark.parametrize("case,which", [("sum", None), ("trend", None), ("mosm", None), ("mohsm", None), ("meanvar", None), ("basis", "function")])
def test_one_part_of_all_rows_is_predict_f(case, which, monkeypatch):
    parts_twin.install(monkeypatch, which)
    m, Xs = model(case)
    T = m.parts()[0][1].shape[2]
    for full in (False, True):
        mu, var = m.predict_f(Xs, full=full)
        mu1, var1 = m.predict_terms(Xs, np.ones((1, T), dtype=bool), full=full)
        want = mu if m.mean is None else mu - np.asarray(m.mean(Xs)).reshape(-1, 1)
        assert np.array_equal(var1[0], var)
        assert np.array_equal(mu1[0], want) if m.mean is None else err(mu1[0], want) <= 1e-15


@pytest.mark.parametrize("case", ["sum", "meanvar", "mosm", "trend"])
def test_the_parts_sum_to_the_prediction(case, monkeypatch):
    """|sum_p mu_p + mean - mu| <= (P + 1) 1e-9 max(1, max |mu_p|): each side holds its golden at 1e-9"""
    parts_twin.install(monkeypatch)
    m, Xs = model(case)
    if parts_cases.CASES[case]["S"] == 1:
        Xs = np.concatenate([Xs, np.linspace(0.0, 10.0, 40)[:, None]])
    _, mu_p, _ = m.predict_parts(Xs)
    mu, _ = m.predict_f(Xs)
    total = np.sum(mu_p, axis=0) + (0.0 if m.mean is None else np.asarray(m.mean(Xs)).reshape(-1, 1))
    P = mu_p.shape[0]
    assert (m.mean is not None) == (case == "meanvar")
    assert np.max(np.abs(total - mu)) <= (P + 1) * 1e-9 * max(1.0, np.max(np.abs(mu_p)))


def test_test_points_are_taken_in_chunks(monkeypatch):
    parts_twin.install(monkeypatch)
    m, Xs = model("sum")
    names, mu, var = m.predict_parts(Xs)
    calls = []
    real = parts_twin.PartsTableDevice.predict_parts
    monkeypatch.setattr(parts_twin.PartsTableDevice, "predict_parts", lambda self, nv, j, tabs, kss, X, **kw: (calls.append((tabs.shape[0], X.shape[0])), real(self, nv, j, tabs, kss, X, **kw))[1])
    monkeypatch.setattr(gpr.Exact, "PART_ROWS", 64)            # 3 parts: 21 points per call
    _, mu2, var2 = m.predict_parts(Xs)
    assert calls == [(3, 21), (3, 21), (3, 21), (3, 7)] and all(P * S <= 64 for P, S in calls)
    assert mu2.shape == mu.shape and err(mu2, mu) <= 1e-13 and err(var2, var) <= 1e-13


def test_the_default_chunk_is_65536_stacked_rows():
    assert gpr.Exact.PART_ROWS == 65536


def test_loss_and_gradients_are_unchanged_by_a_parts_call(monkeypatch):
    parts_twin.install(monkeypatch)
    m, Xs = model("meanvar")
    ps = list(m.parameters())

    def lml_loss():
        loss = float(m.loss())
        return [np.float64(loss).tobytes()] + [p.grad.tobytes() for p in ps if p.grad is not None]

    before = lml_loss()
    m.predict_parts(Xs); m.predict_parts(Xs, full=True); m.predict_terms(Xs, np.ones((1, 3), dtype=bool))
    assert lml_loss() == before and len(before) > 1


# ---- refusals and the public surface -----------------------------------------------------------------------------------------------------
def test_sharded_evaluation_is_refused_before_any_device_call(monkeypatch):
    class NoDevice:
        def __init__(self, *a, **k):
            raise AssertionError("a device handle was created")

    from mogptk_amd import _lib
    monkeypatch.setattr(_lib, "ExactHandle", NoDevice)
    monkeypatch.setattr(config, "comm", type("Comm", (), dict(world=2, rank=0, force=False, native=True))(), raising=False)
    m = parts_cases.exact(gpr, "sum")
    Xs = parts_cases.data("sum")[2]
    with pytest.raises(NotImplementedError, match="use_distributed"):
        m.predict_parts(Xs)
    with pytest.raises(NotImplementedError, match="use_distributed"):
        m.predict_terms(Xs, np.ones((1, 3), dtype=bool))


def test_other_models_have_no_parts():
    import stationary_cases as sc
    X, y, _ = sc.data("se0")
    k = lambda: sc.kernel(gpr, "se0")
    for m in (gpr.Titsias(k(), X, y, Z=5), gpr.Snelson(k(), X, y, Z=5), gpr.OpperArchambeau(k(), X, y), gpr.Hensman(k(), X, y),
              gpr.SparseHensman(k(), X, y, Z=5)):
        for name in ("predict_parts", "predict_terms", "parts"):
            assert not hasattr(m, name), (m.name(), name)
    mm = mogptk_amd.Model(mogptk_amd.DataSet(mogptk_amd.Data(X[:, 0], y, name="a")), gpr.IndependentMultiOutputKernel(k(), output_dims=1),
                          inference=mogptk_amd.Titsias(inducing_points=5))
    with pytest.raises(ValueError, match="exact inference"):
        mm.predict_parts()


def test_model_predict_parts_on_two_channels(monkeypatch):
    parts_twin.install(monkeypatch)
    rng = np.random.default_rng(5)
    xa, xb = np.sort(rng.uniform(0, 10, 40)), np.sort(rng.uniform(0, 10, 30))
    ds = mogptk_amd.DataSet(mogptk_amd.Data(xa, np.sin(xa) + 0.1 * rng.standard_normal(40), name="a"),
                            mogptk_amd.Data(xb, np.cos(xb) + 0.1 * rng.standard_normal(30), name="b"))
    mm = mogptk_amd.Model(ds, gpr.MultiOutputSpectralMixtureKernel(Q=2, output_dims=2, input_dims=1), inference=mogptk_amd.Exact(variance=0.1))
    Xp = [np.linspace(0, 10, 12)[:, None], np.linspace(1, 9, 7)[:, None]]
    X, names, mu, lower, upper = mm.predict_parts(Xp, sigma=3)
    assert names == ["0:MultiOutputSpectralMixtureKernel", "1:MultiOutputSpectralMixtureKernel"]
    assert len(X) == 2 and len(mu) == len(lower) == len(upper) == 2
    _, mu_g, var_g = mm.gpr.predict_parts(mm._to_kernel_format(X))
    for p in range(2):
        assert [v.shape for v in mu[p]] == [(12,), (7,)] == [v.shape for v in lower[p]] == [v.shape for v in upper[p]]
        flat, sd = mu_g[p].reshape(-1), 3 * np.sqrt(var_g[p].reshape(-1))
        assert np.array_equal(np.concatenate(mu[p]), flat)
        assert np.array_equal(np.concatenate(lower[p]), flat - sd) and np.array_equal(np.concatenate(upper[p]), flat + sd)
    # the sum over the parts is the latent mean in transformed space (no mean function here)
    mu_f, _ = mm.gpr.predict_f(mm._to_kernel_format(X))
    assert np.max(np.abs(np.concatenate(mu[0]) + np.concatenate(mu[1]) - mu_f.reshape(-1))) <= 3e-9 * max(1.0, np.max(np.abs(mu_g)))
    X2, names2, mu2, _, _ = mm.predict_parts()               # the data set's own prediction inputs
    assert names2 == names and [len(v) for v in mu2[0]] == [len(x) for x in X2]
