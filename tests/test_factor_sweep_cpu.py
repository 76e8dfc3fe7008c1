"""
The factorisation sweep without a device (tests/factor_sweep.py): what every case has to be before a schedule of the exact path is compared
with the reference on it, measured from the reference alone.

Shape: the tile-row count and the outer blocks the table of cases claims.  Conditioning: cond(Kj) inside the envelope of DESIGN 7, and not
so small that an error in a panel would hide.  The reference's own error: it is used at 1e-9 (kernel_family.err) and has to be a
hundredth of that, 1e-11 -- against two Newton steps in np.longdouble up to N = 640 (a product above that takes a minute), and at every
size the Cholesky-built inverse against numpy's LU-built one and the spectral norm of Kj X - I.  The banded cases: a numpy restatement of
the library's e^-50 rule says the planned inverse is taken (fraction below 0.85, the library's own threshold).
"""
import numpy as np
import pytest

import factor_sweep as fs
from kernel_family import err

COND_LO, COND_HI = 1e2, 1e5
REF_TOL = 1e-11
PLAN_MAX = 0.85


@pytest.mark.parametrize("name", fs.ALL)
def test_case_has_the_shape_the_table_claims(name):
    c = fs.case(name)
    assert c.X.shape == (c.N, 2) and c.y.shape == (c.N,) and sum(c.sizes) == c.N
    assert np.array_equal(np.bincount(c.X[:, 0].astype(np.int64), minlength=c.C), c.sizes)
    assert fs.tile_rows(c.N) == c.nb and fs.outer_blocks(c.nb) == c.blocks and sum(c.blocks) == c.nb
    assert c.table.shape == (c.C, c.C, fs.Q, 5)
    if c.banded:
        assert np.all(np.diff(c.X[:, 1]) >= 0) and len(set(c.X[:, 0])) == 2          # interleaved in x order
    else:
        assert np.any(np.diff(c.X[:, 0]) < 0)                  # the caller's rows are shuffled: not grouped by channel


def test_the_sweep_holds_the_edges_it_is_meant_to():
    nbs = {fs.case(n).nb for n in fs.CASES}
    assert {1, 2, 3, 4, 5, 7, 8, 9, 10, 11, 13} == nbs
    assert {nb % 4 for nb in nbs if nb > 4} == {0, 1, 2, 3}                            # every shape of a last outer block behind a full one
    one_row = [n for n in fs.CASES if fs.case(n).N % fs.TILE == 1]
    assert sorted(fs.case(n).N for n in one_row) == [513, 1025, 1537]                   # one valid row next to 127 of identity padding
    assert {512, 1024} <= {fs.case(n).N for n in fs.CASES}                              # no padding at all
    assert fs.case("n256").sizes == (128, 128, 0) and 1 in fs.case("n300").sizes
    assert [fs.case(n).blocks[-1] for n in fs.BANDED] == [3, 1] and fs.case("b700x837").N % fs.TILE == 1
    for S, sizes in fs.TEST_SETS.items():
        assert sum(sizes) == S
    assert sorted(-(-S // fs.TILE) + 1 for S in fs.TEST_SETS) == [2, 2, 3, 4]           # tile rows of [K_sf ; y^T]
    assert any(0 in s for S, s in fs.TEST_SETS.items() if S > 1)
    assert sorted(fs.case(n).nb for n in fs.PREDICT_CASES) == [5, 8, 9, 13]


@pytest.mark.parametrize("name", fs.ALL)
def test_conditioning_and_the_references_own_error(name):
    c, ref = fs.case(name), fs.reference(name)
    Kj, X = ref["Kj"], ref["Kinv"]
    ev = np.linalg.eigvalsh(Kj)
    cond = float(ev[-1] / ev[0])
    print("factor sweep |", name, "| cond(Kj) |", cond)
    assert COND_LO <= cond <= COND_HI
    assert (ref["lmax"] / ref["lmin"]) ** 2 <= cond * (1 + 1e-9)                       # the pivot range is a LOWER estimate of it
    e_lu = err(X, np.linalg.inv(Kj))
    resid = float(np.linalg.norm(Kj @ X - np.eye(c.N), 2))
    print("factor sweep |", name, "| Cholesky-built against LU-built inverse |", e_lu, "| norm2(Kj X - I) |", resid)
    assert e_lu <= REF_TOL and resid <= REF_TOL
    # the pieces hang together: W is the inverse factor in the sorted order, alpha and the LML follow from it
    o = c.order
    W = ref["W"]
    assert np.array_equal(W, np.tril(W))
    assert err(W @ Kj[np.ix_(o, o)] @ W.T, np.eye(c.N)) <= REF_TOL
    assert err(Kj @ ref["alpha"], c.y) <= REF_TOL
    lml = -0.5 * c.N * np.log(2.0 * np.pi) - 0.5 * ref["logdet"] - 0.5 * float(c.y @ ref["alpha"])
    assert abs(lml - ref["lml"]) <= 1e-12 * abs(ref["lml"])
    G = 0.5 * (np.outer(ref["alpha"], ref["alpha"]) - X)
    assert abs(np.trace(G) - ref["trG"]) <= REF_TOL * max(1.0, abs(ref["trG"]))
    if c.N <= fs.NEWTON_MAX_N:
        e_newton = err(X, fs.newton_inverse(Kj, X).astype(np.float64))
        print("factor sweep |", name, "| against two Newton steps in longdouble |", e_newton)
        assert e_newton <= REF_TOL


@pytest.mark.parametrize("name", list(fs.BANDED))
def test_banded_cases_take_the_planned_inverse(name):
    frac = fs.planned_fraction(fs.case(name))
    print("factor sweep |", name, "| planned fraction of the lower tiles (numpy restatement) |", frac)
    assert 0.0 < frac < PLAN_MAX


@pytest.mark.parametrize("name", ["n513", "n800", "n1024"])
def test_what_the_single_sweep_inversion_loses_by_itself(name):
    """The sweep schedule (csrc/sweep.hip) inverts pivot block after pivot block in place, and every later block corrects the inverse of the
    earlier ones by a subtraction.  Its numpy restatement in float64 (oracle/table_model.py: the sharded stages on one rank) is 1e-13 from
    the reference while there is one pivot block of valid rows (N = 513) and 1e-11 from two on -- the figures the device shows on the same
    cases, so they are the algorithm's and not a kernel's.  Held to a tenth of the 1e-9 the device is held to."""
    c, ref = fs.case(name), fs.reference(name)
    h = fs.twin(c)
    _, nblocks = h.shard_begin(0, 1, c.noise, c.jitter)
    assert nblocks == len(c.blocks)
    for kb in range(nblocks):
        h.shard_block(kb)
    alpha, _ = h.shard_alpha()
    o = c.order
    Kinv = -(np.tril(h.A) + np.tril(h.A, -1).T)[:c.N, :c.N]
    e_K, e_a = err(Kinv, ref["Kinv"][np.ix_(o, o)]), err(alpha[:c.N], ref["alpha"][o])
    print("factor sweep |", name, "| numpy restatement of the single sweep | Kinv |", e_K, "| alpha |", e_a)
    assert e_K <= 1e-10 and e_a <= 1e-10


def test_the_other_cases_form_every_tile():
    """shuffled rows have no band: the restated rule plans every tile, so the default schedules of these cases are the dense ones"""
    for name in fs.CASES:
        assert fs.planned_fraction(fs.case(name)) > PLAN_MAX, name
