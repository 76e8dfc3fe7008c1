"""
The radial instantiations of k_gram and k_moments (csrc/gram.hip: DT in {1, 2, 3, generic}, GATE in {0, 1, 2}) swept over row kinds, input
dimensions and shapes through the raw C ABI, against the composed numpy twin (tests/kinds_twin.py) on identical inputs
(tests/kinds_sweep.py): every kind 0 - 10 alone and in groups; off-diagonal channel pairs with a delay, a phase and a frequency under
non-Gaussian profiles, so that the odd moments m2_d, m3_d, m4 are non-zero there (the twin's are pinned by finite differences in
tests/test_kinds_sweep_cpu.py); one to four channels in shuffled caller order, one-point and empty channels, N around 64, 128 and 512,
full tiles at an odd column offset, and N = 1100 on the dataflow schedule.  Evaluation (LML, jitter, moments, diagG, trG, Kj^-1, alpha,
data_var, the per-point diagonal formed by the library and given by the caller), mogp_gram_kinds square and rectangular, predictions,
leave-one-out and leave-fold-out, and one handle taking several tables in turn.  Errors are kernel_family.err, relative to
max(1, max |want|), printed per case; the bounds are DESIGN 8's.  Last, what the sweep found in k_moments' reduction (moment rows wider than
16 doubles), on the Gaussian instantiations that share it.
"""
import functools
import types
import numpy as np
import pytest

from mogptk_amd import gpr, _lib
import kernel_family as kf
import kinds_sweep as ks
import kinds_twin

pytestmark = pytest.mark.gpu

TOL_GRAM, TOL_VALUE, TOL_JITTER, TOL_MOMENT, TOL_SOLVE = 1e-12, 1e-9, 1e-14, 1e-7, 1e-9
SQUARE = [(65, 1, 63), (71, 129, 33)]
TRAIN = (71, 129, 33)


class Report:
    """prints every figure of a case, fails at the end with all that missed their bound"""

    def __init__(self, *tag):
        self.tag, self.bad = " ".join(ks.case_id(t) for t in tag), []

    def add(self, name, e, tol):
        print("kinds sweep |", self.tag, "|", name, "|", e)
        if not e <= tol:
            self.bad.append((name, e, tol))

    def err(self, name, got, want, tol):
        self.add(name, kf.err(got, want), tol)

    def done(self):
        assert not self.bad, (self.tag, self.bad)


def device(c, table=True):
    h = _lib.ExactHandle(gpr.config.device, c.X, c.y, c.C)
    if table:
        h.set_terms(c.table)
        h.set_kinds(c.kind, c.shape)
    return h


def compare_gradient_outputs(r, got, want, value):
    r.err(value, got[value], want[value], TOL_VALUE)
    r.add("jitter_abs", abs(got["jitter_abs"] - want["jitter_abs"]) / want["jitter_abs"], TOL_JITTER)
    for name in ("moments", "diagG", "trG"):
        r.err(name, got[name], want[name], TOL_MOMENT)


@pytest.mark.parametrize("program,sizes", ks.SWEEP, ids=ks.case_id)
def test_evaluation(program, sizes, monkeypatch):
    """mogp_exact_eval with the library forming the per-point diagonal itself; with a data_var; with the diagonal given by the caller"""
    monkeypatch.delenv("MOGP_FLOW", raising=False)
    monkeypatch.delenv("MOGP_FLOW_MIN", raising=False)
    c = ks.case(program, sizes)
    rng = np.random.default_rng(c.N)
    dvar = rng.uniform(0.0, 0.1, c.N)
    with ks.installed():
        ref = ks.twin_device(c)
        want = ref.eval(c.noise, c.jitter, grad=True)
        Kinv, alpha = ref.fetch(1), ref.fetch(2)
        Kdiag = np.diagonal(ref._gram(c.X)).copy()
        want2 = ref.eval(c.noise, c.jitter, grad=False, data_var=dvar)
    r = Report("eval", program, sizes)
    dev = device(c)
    got = dev.eval(c.noise, c.jitter, grad=True)
    if sizes == ks.DATAFLOW_SIZES:
        print("kinds sweep |", r.tag, "| schedule |", dev.schedule())
        assert dev.schedule()["dataflow"], dev.schedule()
    compare_gradient_outputs(r, got, want, "lml")
    r.err("Kinv", dev.fetch(1), Kinv, TOL_SOLVE)
    r.err("alpha", dev.fetch(2), alpha, TOL_SOLVE)
    got2 = dev.eval(c.noise, c.jitter, grad=False, data_var=dvar)
    r.err("lml(data_var)", got2["lml"], want2["lml"], TOL_VALUE)
    r.add("jitter_abs(data_var)", abs(got2["jitter_abs"] - want2["jitter_abs"]) / want2["jitter_abs"], TOL_JITTER)
    if c.point_rows:
        dev.set_point_diag(Kdiag)
        got3 = dev.eval(c.noise, c.jitter, grad=True)
        r.add("jitter_abs(point_diag)", abs(got3["jitter_abs"] - got["jitter_abs"]) / got["jitter_abs"], TOL_JITTER)
        r.err("lml(point_diag)", got3["lml"], got["lml"], 1e-12)
    r.done()


def white_groups(c):
    """the rows of the groups that hold a white row"""
    rows, start = [], 0
    for t in range(c.T):
        if not (c.kind[0, 0, t] & ks.X_):
            if np.any((c.kind[0, 0, start:t + 1] & 0xff) == ks.WHITE):
                rows += list(range(start, t + 1))
            start = t + 1
    return rows


@pytest.mark.parametrize("program", list(ks.PROGRAMS))
def test_gram(program):
    """mogp_gram_kinds: square, and rectangular against shuffled second sets with an empty and a one-point channel"""
    D = ks.PROGRAMS[program][0]
    r = Report("gram", program)
    for sizes in SQUARE:
        c = ks.case(program, sizes)
        rng = np.random.default_rng(c.N + 1)
        seconds = [("copy", c.X.copy())] + [(ks.case_id(s), ks.draw_points(rng, s, D)) for s in [(0, 64, 1), (33, 65, 130)]]
        with ks.installed():
            want = kinds_twin.gram_from_table(c.table, c.X, None, c.kind, c.shape)
            wants = [kinds_twin.gram_from_table(c.table, c.X, X2, c.kind, c.shape) for _, X2 in seconds]
        K = _lib.gram(gpr.config.device, c.C, D, c.table, c.X, None, c.kind, c.shape)
        r.err("%s square" % ks.case_id(sizes), K, want, TOL_GRAM)
        assert np.array_equal(K, K.T)
        rows = white_groups(c)
        for (name, X2), w in zip(seconds, wants):
            K = _lib.gram(gpr.config.device, c.C, D, c.table, c.X, X2, c.kind, c.shape)
            r.err("%s against %s" % (ks.case_id(sizes), name), K, w, TOL_GRAM)
            if rows:                                        # a white row is zero in every rectangular call, to the bit
                K = _lib.gram(gpr.config.device, c.C, D, c.table[:, :, rows], c.X, X2, c.kind[:, :, rows], c.shape[:, :, rows])
                assert not np.any(K), (program, sizes, name)
    r.done()


@pytest.mark.parametrize("program", list(ks.PROGRAMS))
def test_predictions(program):
    """mogp_exact_predict, diagonal and full: one test point, a set with an empty channel, a shuffled set that crosses a 64-tile in two channels"""
    c = ks.case(program, TRAIN)
    rng = np.random.default_rng(c.T)
    tests = [("1", ks.draw_points(rng, (0, 1, 0), c.D)), ("33x0x40", ks.draw_points(rng, (33, 0, 40), c.D, shuffle=False)),
             ("64x65x1 shuffled", ks.draw_points(rng, (64, 65, 1), c.D))]
    r = Report("predict", program)
    dev = device(c)
    for name, Xs in tests:
        with ks.installed():
            ref = ks.twin_device(c)
            kss = ks.kss_diag(c, Xs)
            assert kss.shape == ((len(Xs),) if c.point_rows else (c.C,))
            mu, var = ref.predict(c.noise, c.jitter, kss, Xs)
            mu2, cov = ref.predict(c.noise, c.jitter, kss, Xs, full=True)
        got_mu, got_var = dev.predict(c.noise, c.jitter, kss, Xs)
        r.err(name + " mu", got_mu, mu, TOL_SOLVE)
        r.err(name + " var", got_var, var, TOL_SOLVE)
        got_mu, got_cov = dev.predict(c.noise, c.jitter, kss, Xs, full=True)
        r.err(name + " mu(full)", got_mu, mu2, TOL_SOLVE)
        r.err(name + " cov", got_cov, cov, TOL_SOLVE)
    r.done()


def fold_labels(c):
    """folds in the device's channel-sorted order, handed over in the caller's: one that crosses row 64 and a channel boundary, one that
    crosses row 128 (of 128 points, over a channel boundary, where N allows), two of one point each, and points in no fold"""
    order = np.argsort(c.X[:, 0], kind="stable")
    blocks = [range(100, 228), range(60, 76)] if c.N >= 233 else [range(100, c.N - 1), range(60, 70)]
    blocks += [[0], [c.N - 1]]
    lab = np.full(c.N, -1, dtype=np.int32)
    for f, b in enumerate(blocks):
        lab[order[list(b)]] = f
    return lab, len(blocks)


@pytest.mark.parametrize("sizes", SQUARE, ids=ks.case_id)
@pytest.mark.parametrize("program", list(ks.PROGRAMS))
def test_leave_one_out_and_cross_validation(program, sizes):
    c = ks.case(program, sizes)
    lab, nfolds = fold_labels(c)
    assert np.any(lab < 0) and max(np.bincount(lab[lab >= 0])) == (128 if c.N >= 233 else c.N - 101)
    with ks.installed():
        ref = ks.twin_device(c)
        want_loo = ref.loo(c.noise, c.jitter, grad=True)
        want_cv = ref.cv(c.noise, c.jitter, lab, nfolds, grad=True)
    r = Report("loo/cv", program, sizes)
    dev = device(c)
    for value, got, want in (("loo", dev.loo(c.noise, c.jitter, grad=True), want_loo), ("cv", dev.cv(c.noise, c.jitter, lab, nfolds, grad=True), want_cv)):
        compare_gradient_outputs(r, got, want, value)
        held = ~np.isnan(want["mu"])
        assert np.array_equal(np.isnan(got["mu"]), ~held) and np.array_equal(np.isnan(got["var"]), ~held)
        assert np.array_equal(held, lab >= 0) or value == "loo"
        r.err(value + " mu", got["mu"][held], want["mu"][held], TOL_SOLVE)
        r.err(value + " var", got["var"][held], want["var"][held], TOL_SOLVE)
    r.done()


OTHER_D1 = [3 | ks.X_, 8, 1, 7 | ks.X_, 2, 6 | ks.X_, 4]      # T = 7 like profiles_d1, other kinds; a gate row and no white row: GATE = 1


@functools.lru_cache(maxsize=None)
def handle_sequence():
    first = ks.case("profiles_d1", (65, 1, 63))
    other = ks.make_case("other_d1", 1, OTHER_D1, first.sizes, 101, points=first)
    again = ks.make_case("other_d1 new values", 1, OTHER_D1, first.sizes, 102, points=first, like=other)
    no_kinds = types.SimpleNamespace(kind=np.zeros((first.C, first.C, 3), dtype=np.int32), shape=np.zeros((first.C, first.C, 3)))
    gauss = ks.make_case("gaussian", 1, [0, 0, 0], first.sizes, 103, points=first, like=no_kinds)      # Gaussian on the cross pairs too
    gates = ks.make_case("gates_d1", 1, ks.PROGRAMS["gates_d1"][1], first.sizes, 104, points=first)
    return first, other, again, gauss, gates


def test_one_handle_takes_several_tables_in_turn():
    """kinds, other kinds of the same T, new values under the kinds that persist, a Gaussian table of another T (the kinds are dropped),
    gate rows, and the first table again: bit for bit what it gave the first time"""
    first, other, again, gauss, gates = handle_sequence()
    assert np.array_equal(again.kind, other.kind) and np.array_equal(again.shape, other.shape) and not np.array_equal(again.table, other.table)
    assert not np.any(gauss.kind) and gauss.T == 3
    r = Report("one handle")
    dev = device(first, table=False)
    bits = []
    for step, c, kinds in ((1, first, True), (2, other, True), (3, again, False), (4, gauss, False), (5, gates, True), (6, first, True)):
        assert c.k <= 5 and c.lambda_min >= 0.1 and c.cond < 1e5      # the conditions of tests/test_kinds_sweep_cpu.py, for the tables made here
        with ks.installed():
            ref = ks.twin_device(c)
            if step == 4:
                ref.set_kinds(None, None)                   # the twin without kinds
            want = ref.eval(c.noise, c.jitter, grad=True)
        dev.set_terms(c.table)
        if kinds:
            dev.set_kinds(c.kind, c.shape)
        got = dev.eval(c.noise, c.jitter, grad=True)
        rr = Report("one handle", "step %d %s" % (step, c.program))
        compare_gradient_outputs(rr, got, want, "lml")
        r.bad += rr.bad
        if step in (1, 6):
            bits.append([np.float64(got[k]).tobytes() for k in ("lml", "trG", "jitter_abs")] + [got["moments"].tobytes(), got["diagG"].tobytes()])
    r.done()
    assert bits[0] == bits[1]


def gaussian_case(D, sizes, envelope=False):
    """Gaussian rows without kinds through the same generator; envelope: rows of width 2 + 5 D, with L_d <= V_d so that every row stays positive
    semi-definite on the diagonal pairs (exp((V - L / 4) a b) is, for V >= L / 4)"""
    C = len(sizes)
    none = types.SimpleNamespace(kind=np.zeros((C, C, 3), dtype=np.int32), shape=np.zeros((C, C, 3)))
    c = ks.make_case("gaussian_d%d" % D, D, [0, 0, 0], sizes, [D] + list(sizes), like=none)
    if envelope:
        rng = np.random.default_rng(D)
        wide = np.zeros(c.table.shape[:3] + (2 + 5 * D,))
        wide[..., :2 + 3 * D] = c.table
        for i in range(C):
            for j in range(i + 1):
                wide[i, j, :, 2 + 3 * D:2 + 4 * D] = c.table[i, i, :, 2:2 + D] * rng.uniform(0.2, 1.0, (3, D))
                wide[i, j, :, 2 + 4 * D:] = rng.uniform(-1.0, 1.0, (3, D)) * np.where(np.arange(D) == 0, 5.0, 1.0) + np.where(np.arange(D) == 0, 5.0, 0.0)
                wide[j, i, :, 2 + 3 * D:] = wide[i, j, :, 2 + 3 * D:]
        c.table = wide
    return c


@pytest.mark.parametrize("D,sizes,envelope", [(5, TRAIN, False), (8, TRAIN, False), (3, (65, 1, 63), True)], ids=["d5", "d8", "d3-envelope"])
def test_moment_rows_wider_than_sixteen(D, sizes, envelope):
    """what the sweep found, where it also applied: k_moments reduces 16 moments per pass, and the Gaussian instantiations share the reduction --
    rows of 2 + 3 D with D = 5 and 8 (the generic form) and of 2 + 5 D with D = 3 (the envelope), against the oracle's twin"""
    from oracle.table_model import TableDevice
    c = gaussian_case(D, sizes, envelope)
    assert c.table.shape[3] > 16
    ref, dev = TableDevice(0, c.X, c.y, c.C), _lib.ExactHandle(gpr.config.device, c.X, c.y, c.C)
    ref.set_terms(c.table)
    dev.set_terms(c.table)
    Kj, _ = ref._Kj(c.noise, c.jitter, None)
    ev = np.linalg.eigvalsh(Kj)
    print("lambda_min", ev[0], "cond", ev[-1] / ev[0])
    assert ev[0] >= 0.1 and ev[-1] / ev[0] < 1e5
    if envelope:
        kdiag = np.diagonal(ref._gram(c.X)).copy()
        ref.set_point_diag(kdiag)
        dev.set_point_diag(kdiag)
    want, got = ref.eval(c.noise, c.jitter, grad=True), dev.eval(c.noise, c.jitter, grad=True)
    r = Report("wide rows", "D = %d" % D, "envelope" if envelope else "plain")
    compare_gradient_outputs(r, got, want, "lml")
    r.err("moments 16 and up", got["moments"][..., 16:], want["moments"][..., 16:], TOL_MOMENT)
    assert np.any(want["moments"][..., 16:])
    r.done()
