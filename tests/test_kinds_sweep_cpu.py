"""
The kinds sweep without a device (tests/kinds_sweep.py, tests/kinds_twin.py): the conditions every generated case has to meet before the
device is compared with the twin on it; the composed twin against the two family twins it is composed from; and the twin's moments --
among them the odd moments m2_d, m3_d, m4 of non-Gaussian profiles on off-diagonal channel pairs with a delay, a phase and a frequency,
which no golden contains -- against central differences of the twin's own LML through the host's `_gtable_from_moments`.
"""
import numpy as np
import pytest

import oracle.table_model as tm
from mogptk_amd.gpr.model import _gtable_from_moments
import kernel_family as kf
import kinds_sweep as ks
import kinds_twin
import changepoint_twin
import function_twin
import loo_twin


@pytest.mark.parametrize("program,sizes", ks.SWEEP, ids=ks.case_id)
def test_every_case_is_well_conditioned_and_its_cross_pairs_matter(program, sizes):
    """conditions on the inputs, not measurements: lambda_min and cond are the bound the generators of this project assert (accurate mode
    never engages), k <= 5 keeps the cross pairs from being scaled away, and so does the ratio"""
    c = ks.case(program, sizes)
    print(program, sizes, "k", c.k, "lambda_min", c.lambda_min, "cond", c.cond, "largest cross entry / largest diagonal entry", c.cross_ratio)
    assert c.k <= 5
    assert c.lambda_min >= 0.1 and c.cond < 1e5
    if c.C > 1:
        assert c.cross_ratio >= 5e-3
    # the programs respect what check_kinds asks for: the same flags in every pair, the last row unflagged, groups of at most four rows
    assert np.all((c.kind & ks.X_) == (c.kind[0, 0] & ks.X_)) and not (c.kind[0, 0, -1] & ks.X_)
    run = 0
    for k in c.kind[0, 0]:
        run = run + 1 if k & ks.X_ else 0
        assert run < 4
    assert np.all(c.table[np.arange(c.C), np.arange(c.C)][..., 1][(c.kind[np.arange(c.C), np.arange(c.C)] & 0xff) != ks.DOT] == 0.0)
    assert not np.any(c.table[np.arange(c.C), np.arange(c.C)][..., 2 + 2 * c.D:])      # Psi = Delta = 0 on diagonal pairs: table_diag relies on it
    assert np.array_equal(c.kind, np.transpose(c.kind, (1, 0, 2)))


@pytest.mark.parametrize("family,case,install", [("changepoint", "two", changepoint_twin.install), ("function", "white_f", function_twin.install)])
def test_the_composed_twin_reproduces_the_family_twins(family, case, install):
    """the Gram matrix and the leave-one-out figures of one case of each family, under the family's own twin and under the composed one"""
    m, _, fx = kf.reference_model(family, case)
    k = m.kernel
    X = k._kernel_format(fx[case + "__X"])
    table, kind, shape, _ = k._device_terms(X.shape[1] - 1)
    assert np.any(np.isin(kind & 0xff, (8, 9, 10)))
    noise = m._noise_var()
    got = []
    for put, cls in ((install, loo_twin.LooTableDevice), (kinds_twin.install, kinds_twin.KindsTableDevice)):
        with pytest.MonkeyPatch.context() as mp:
            put(mp)
            K = tm.gram_from_table(table, X, kind=kind, shape=shape)
            h = cls(0, X, m.y, k._channels())
            h.set_terms(table)
            h.set_kinds(kind, shape)
            got.append((K, h.loo(noise, m.jitter, grad=True)))
    (K0, l0), (K1, l1) = got
    assert kf.err(K1, K0) <= 1e-12 and kf.err(K1, kf.golden_K(family, case)) <= 1e-12
    for name in ("loo", "mu", "var", "moments", "diagG", "trG", "jitter_abs"):
        e = kf.err(l1[name], l0[name])
        print(family, case, name, e)
        assert e <= 1e-12, name
    assert tm.row_parts.__module__ == tm.__name__ and tm.moments_dense.__module__ == tm.__name__      # nothing is left behind


def parameter_slots(kd, D, cross):
    """the table columns that are parameters of a row of kind `kd` and that the host's chain rule differentiates; cross: an off-diagonal
    pair (Psi and Delta are zero by construction on the diagonal pairs and are not parameters there)"""
    V, M, Dl = list(range(2, 2 + D)), list(range(2 + D, 2 + 2 * D)), list(range(2 + 2 * D, 2 + 3 * D))
    if kd == ks.DOT:
        return [0, 1]
    if kd == ks.GATE:
        return [0, 2, 3]
    if kd == ks.WDOT:
        return [0] + V
    if kd == ks.WHITE:
        return [0]
    if kd == ks.PERIODIC:                                    # reads V_0 and the phase; of the frequencies the device differentiates M_0
        return [0, 2, 2 + D] + ([1] + Dl if cross else [])
    return [0] + V + M + ([1] + Dl if cross else [])


@pytest.mark.parametrize("program", list(ks.PROGRAMS))
def test_twin_moments_are_the_derivatives_of_the_twins_own_lml(program):
    """central differences of the twin's LML (jitter 0, step 1e-6 max(1, |theta|)) against `_gtable_from_moments` of the twin's moments, for
    every table entry that is a parameter of its row, at the project's own finite-difference bound 1e-5 max(1, |g|)"""
    c = ks.case(program, (21, 0, 13))
    worst = 0.0
    with ks.installed():
        h = ks.twin_device(c)
        res = h.eval(c.noise, 0.0, grad=True)
        g = _gtable_from_moments(c.table, res["moments"], c.D, lower=True, kind=c.kind)

        def lml(table):
            h.set_terms(table)
            h.set_kinds(c.kind, c.shape)
            return h.eval(c.noise, 0.0, grad=False)["lml"]

        odd = 0.0
        for i in range(c.C):
            for j in range(i + 1):
                if c.sizes[i] == 0 or c.sizes[j] == 0:
                    assert not np.any(res["moments"][i * (i + 1) // 2 + j])
                    continue
                for t in range(c.T):
                    kd = int(c.kind[i, j, t]) & 0xff
                    for col in parameter_slots(kd, c.D, i != j):
                        step = 1e-6 * max(1.0, abs(c.table[i, j, t, col]))
                        up, dn = c.table.copy(), c.table.copy()
                        up[i, j, t, col] += step
                        dn[i, j, t, col] -= step
                        fd = (lml(up) - lml(dn)) / (2.0 * step)
                        e = abs(g[i, j, t, col] - fd) / max(1.0, abs(fd))
                        worst = max(worst, e)
                        assert e <= 1e-5, (program, (i, j), t, kd, col, g[i, j, t, col], fd)
                    if i != j and kd in (1, 2, 3, 4, 5, 6):
                        odd = max(odd, float(np.max(np.abs(res["moments"][i * (i + 1) // 2 + j, t, [1] + list(range(2 + c.D, 2 + 3 * c.D))]))))
    print(program, "largest finite-difference error", worst, "largest odd moment of a non-Gaussian cross-pair row", odd)
    if any((k & 0xff) in (1, 2, 3, 4, 5, 6) for k in ks.PROGRAMS[program][1]):
        assert odd > 0.0                                    # the odd moments this pins are not zero
