"""
The three software pipelines of the headline path -- k_gram_strip2 (runs of up to 8 tiles: double-buffered factors, scalars mod 3, the wave
pairs' turns for odd T, the diagonal store on a run's last tile), the persistent k_gram<DT, RAD, GATE> and k_moments_x<3|4> (csrc/gram.hip) --
at sizes where a second tile follows a first.  The launches are planned on one or three CUs (mogp_ctx_plan_cus) so that a list of a few dozen
tiles is cut into long runs and walked by two workgroups; the chunks cases reach chunks of three tiles at the device's own count.  Cases and
their conditions: tests/spectral_sweep.py, tests/test_spectral_sweep_cpu.py.

Kj is read back as the model path wrote it (mogp_model_gram) and compared with the longdouble restatement of the term formula
(tests/spectral_ref.py); evaluations go against oracle.table_model.TableDevice.  Errors are relative to max(1, max |want|) (kernel_family.err)
unless said otherwise, printed per case; the bounds are DESIGN 8's as the kinds sweep uses them (Gram 1e-12, value 1e-9, solves 1e-9, the
jitter 1e-14) and the 1e-9 of test_device_raw_outputs_against_numpy_model, relative to the largest moment, for the spectral moments.
"""
import contextlib
import functools
import numpy as np
import pytest

from mogptk_amd import gpr, _lib
from oracle.table_model import TableDevice
import kernel_family as kf
import kinds_sweep as ks
import sparse_sweep as ss
import spectral_ref as ref
import spectral_sweep as sw

pytestmark = pytest.mark.gpu

TOL_GRAM, TOL_VALUE, TOL_JITTER, TOL_MOMENT, TOL_SOLVE = 1e-12, 1e-9, 1e-14, 1e-9, 1e-9
SIZES = (71, 129, 33)
BASELINE = {}                                                # what a handle gave before the module's first plan_cus call


class Report:
    """prints every figure of a case, fails at the end with all that missed their bound"""

    def __init__(self, *tag):
        self.tag, self.bad = " ".join(sw.case_id(t) for t in tag), []

    def add(self, name, e, tol):
        print("spectral sweep |", self.tag, "|", name, "|", e, "| bound", tol)
        if not e <= tol:
            self.bad.append((name, e, tol))

    def err(self, name, got, want, tol):
        self.add(name, kf.err(got, want), tol)

    def done(self):
        assert not self.bad, (self.tag, self.bad)


def device(c):
    h = _lib.ExactHandle(gpr.config.device, c.X, c.y, c.C)
    h.set_terms(c.table)
    return h


@contextlib.contextmanager
def planned_on(ncu):
    """`with planned_on(ncu):` -- the launches of the block planned on ncu CUs, the device's own count afterwards whatever the block raised"""
    _lib.plan_cus(ncu)
    try:
        yield
    finally:
        _lib.plan_cus(0)


def eval_bits(got):
    return [np.float64(got[k]).tobytes() for k in ("lml", "trG", "jitter_abs")] + [got["moments"].tobytes(), got["diagG"].tobytes()]


@pytest.fixture(scope="module", autouse=True)
def planned_cus():
    """the first thing the module does on the device, before any mogp_ctx_plan_cus: a probe and an evaluation on a fresh handle (the bits
    plan_cus(0) must give back); the device's count restored whatever happens"""
    try:
        c = sw.runs_case((704,), 3)
        h = device(c)
        BASELINE["probe"] = h.gram_probe(c.noise, c.jitter, c.dvar)
        BASELINE["eval"] = eval_bits(h.eval(c.noise, c.jitter, grad=True))
        BASELINE["handle"] = h
        yield
    finally:
        _lib.plan_cus(0)
        BASELINE.clear()


@functools.lru_cache(maxsize=None)
def reference_kj(name):
    """(longdouble Kj in channel-sorted order, the float64 twin's) with noise, jitter and data_var on the diagonal"""
    c = dict(sw.gram_cases())[name]()
    order = ref.sorted_order(c.X)
    K, _ = ref.kj(c.table, c.X, c.noise, c.jitter, c.dvar)
    twin = TableDevice(0, c.X, c.y, c.C)
    twin.set_terms(c.table)
    Kt, _ = twin._Kj(c.noise, c.jitter, c.dvar)
    return K[np.ix_(order, order)], Kt[np.ix_(order, order)]


def lower_err(got, want):
    """kernel_family.err over the lower triangle, the difference taken in longdouble"""
    low = np.tril_indices(len(want))
    return float(np.max(np.abs(got[low] - want[low])) / max(1.0, float(np.max(np.abs(want[low])))))


@pytest.mark.parametrize("name", [n for n, _ in sw.gram_cases()])
def test_probe_against_reference_and_bits_across_cuts(name):
    """Kj as the model path writes it, planned on the device's CUs (single tiles), on one (runs of up to 8, two workgroups walking the rest) and on
    three: each against the longdouble Kj, and the same bits from all three -- a tile's arithmetic depends neither on its place in a run nor on
    the workgroup.  The far case's bound carries the rounding of the per-point phases the device forms from absolute inputs: half an ulp per
    fma, two points, slope 2 pi, a margin of 2"""
    c = dict(sw.gram_cases())[name]()
    want, twin = reference_kj(name)
    bound = TOL_GRAM
    r = Report("probe", name)
    if name == "far":
        P = ref.phase_magnitude(c.table, c.X)
        bound = TOL_GRAM + 4.0 * np.pi * c.D * 2.0 ** -52 * P
        print("spectral sweep |", r.tag, "| phase magnitude P |", P, "| bound", bound)
    r.add("float64 twin", lower_err(twin, want), bound)
    dev = device(c)
    probes = {}
    for ncu in (0, 1, 3):
        with planned_on(ncu):
            K = probes[ncu] = dev.gram_probe(c.noise, c.jitter, c.dvar)
            cut = dev.strip_runs(0)
        assert np.all(np.isfinite(K)) and not np.any(np.triu(K, 1))
        # the handle's own list is the host plan's for that count (tests/test_spectral_sweep_cpu.py holds the plan to its invariants): single
        # tiles at the device's count, the plan's runs below it
        plan = _lib.strip_plan(c.sizes, ncu or cut["ncu"])
        assert (cut["runs"], cut["rest"], cut["longest"]) == (int(np.sum(plan[:, 0] == 1)), int(np.sum(plan[:, 0] == 0)), int(np.max(plan[plan[:, 0] == 1, 3]))), (ncu, cut)
        assert cut["longest"] == 1 if ncu == 0 else cut["ncu"] == ncu
        r.add("device, planned on %d CUs" % ncu, lower_err(K, want), bound)
    r.done()
    assert np.array_equal(probes[1], probes[0]) and np.array_equal(probes[3], probes[0])


def spectral_table(D, envelope):
    """the sparse sweep's kernels (MOSM; MOHSM for the enveloped rows) with the kinds sweep's points"""
    rng = np.random.default_rng([7, D, int(envelope)])
    table = np.array(ss.draw_kernel(rng, D, 2 if D == 5 else 3, envelope)._spectral_terms(D))
    return table, ks.draw_points(rng, SIZES, D), ks.draw_points(rng, (33, 65, 130), D)


@pytest.mark.parametrize("envelope", [False, True], ids=["plain", "envelope"])
@pytest.mark.parametrize("D", [2, 3, 5])
def test_stateless_gram_bits_across_grids(D, envelope):
    """mogp_gram_ex, square and rectangular: with one CU planned two workgroups walk all tiles (the persistent path of k_gram<2>, <3> and the
    generic form, with and without the envelope), and the bits are those of one tile per workgroup; each also against the longdouble reference"""
    table, X, X2 = spectral_table(D, envelope)
    assert table.shape[3] == (2 + 5 * D if envelope else 2 + 3 * D)
    r = Report("gram_ex", "D = %d" % D, "envelope" if envelope else "plain")
    for name, second in (("square", None), ("rectangular", X2)):
        got = {}
        for ncu in (0, 1, 3):
            with planned_on(ncu):
                got[ncu] = _lib.gram(gpr.config.device, len(SIZES), D, table, X, second)
        want = ref.gram(table, X, second)
        r.add(name, float(np.max(np.abs(got[0] - want)) / max(1.0, float(np.max(np.abs(want))))), TOL_GRAM)
        assert np.array_equal(got[1], got[0]) and np.array_equal(got[3], got[0]), name
    r.done()


@pytest.mark.parametrize("program", list(ks.PROGRAMS))
def test_kinds_gram_bits_across_grids(program):
    """mogp_gram_kinds on every program of the kinds sweep: the persistent path of every radial instantiation of k_gram"""
    D = ks.PROGRAMS[program][0]
    c = ks.case(program, SIZES)
    X2 = ks.draw_points(np.random.default_rng(c.N + 1), (33, 65, 130), D)
    for name, second in (("square", None), ("rectangular", X2)):
        got = {}
        for ncu in (0, 1, 3):
            with planned_on(ncu):
                got[ncu] = _lib.gram(gpr.config.device, c.C, D, c.table, c.X, second, c.kind, c.shape)
        assert np.array_equal(got[1], got[0]) and np.array_equal(got[3], got[0]), (program, name)
        assert np.all(np.isfinite(got[0])) and np.any(got[0])


@functools.lru_cache(maxsize=None)
def twin_eval(name):
    c = dict(sw.all_cases())[name]()
    t = TableDevice(0, c.X, c.y, c.C)
    t.set_terms(c.table)
    want = t.eval(c.noise, c.jitter, grad=True)
    return want, t.fetch(1), t.fetch(2)


def compare_eval(r, dev, got, want, Kinv, alpha):
    r.err("lml", got["lml"], want["lml"], TOL_VALUE)
    r.add("jitter_abs", abs(got["jitter_abs"] - want["jitter_abs"]) / want["jitter_abs"], TOL_JITTER)
    for k in ("moments", "diagG"):
        r.add(k, np.max(np.abs(got[k] - want[k])) / np.max(np.abs(want[k])), TOL_MOMENT)
    r.add("trG", abs(got["trG"] - want["trG"]) / abs(want["trG"]), TOL_MOMENT)
    r.err("Kinv", dev.fetch(1), Kinv, TOL_SOLVE)
    r.err("alpha", dev.fetch(2), alpha, TOL_SOLVE)


EVAL = ([("runs-%s-T%d" % (sw.case_id(s), T), (0, 3)) for s, T in sw.RUNS if T <= 5]
        + [("chunks-%s-T%d" % (sw.case_id(s), T), (0,)) for s, T in sw.CHUNKS])


@pytest.mark.parametrize("name,ncus", EVAL, ids=[n for n, _ in EVAL])
def test_evaluation_on_long_runs_and_chunks(name, ncus, monkeypatch):
    """mogp_exact_eval with gradients against TableDevice: the runs cases planned on the device's CUs and on three (the moment kernel then walks
    chunks of up to 19 tiles that cross every pair boundary of the three-channel lists), the chunks cases at the device's own count (528 tiles:
    chunks of 3; 32 channels: every tile a pair of its own, and a table too large for the Gram kernel's LDS copy).

    The moments at 3 and at 0 planned CUs are printed as equal or not and NOT asserted equal: k_moments_x adds a chunk's tiles of one pair up in
    each thread's registers before its one reduction per run, so the order in which a pair's entries are added follows the chunking
    (k_moment_reduce itself adds the slots in list order, whatever wrote them).  LML, Kj^-1 and alpha do not pass through it and ARE equal"""
    monkeypatch.delenv("MOGP_FLOW", raising=False)
    monkeypatch.delenv("MOGP_FLOW_MIN", raising=False)
    c = dict(sw.all_cases())[name]()
    want, Kinv, alpha = twin_eval(name)
    r = Report("eval", name)
    dev = device(c)
    got, mats = {}, {}
    for ncu in ncus:
        with planned_on(ncu):
            got[ncu] = dev.eval(c.noise, c.jitter, grad=True)
            rr = Report("eval", name, "planned on %d CUs" % ncu)
            compare_eval(rr, dev, got[ncu], want, Kinv, alpha)
            mats[ncu] = (dev.fetch(1), dev.fetch(2))
        r.bad += rr.bad
    if len(ncus) > 1:
        a, b = got[ncus[0]], got[ncus[1]]
        print("spectral sweep |", r.tag, "| moments bit-identical across chunkings |", np.array_equal(a["moments"], b["moments"]),
              "| largest difference / largest moment |", np.max(np.abs(a["moments"] - b["moments"])) / np.max(np.abs(a["moments"])))
        assert a["lml"] == b["lml"] and a["jitter_abs"] == b["jitter_abs"]
        assert np.array_equal(mats[ncus[0]][0], mats[ncus[1]][0]) and np.array_equal(mats[ncus[0]][1], mats[ncus[1]][1])
    r.done()


@pytest.mark.parametrize("sizes", sw.DATAFLOW_SIZES, ids=sw.case_id)
def test_dataflow_schedule_on_one_planned_cu(sizes, monkeypatch):
    """1100 points in three channels, T = 3, on the dataflow schedule with its two Gram launches' lists cut for one CU.  367 + 400 + 333: the head
    launch (columns below 512) holds runs of several tiles, the tail launch no strip tile at all (channels 1 and 2 start at odd offsets) and
    runs on the general kernel alone.  368 + 400 + 332: even offsets, runs of several tiles in both launches"""
    monkeypatch.delenv("MOGP_FLOW", raising=False)
    monkeypatch.delenv("MOGP_FLOW_MIN", raising=False)
    c = sw.dataflow_case(sizes)
    want, Kinv, alpha = twin_eval("dataflow-%s" % sw.case_id(sizes))
    dev = device(c)
    r = Report("eval", "dataflow", c.name)
    for ncu in (1, 0):
        with planned_on(ncu):
            got = dev.eval(c.noise, c.jitter, grad=True)
            head, tail = dev.strip_runs(1), dev.strip_runs(2)
            print("spectral sweep |", r.tag, "| planned on %d CUs | schedule |" % ncu, dev.schedule(), "| head list |", head, "| tail list |", tail)
            assert dev.schedule()["dataflow"], dev.schedule()
            assert head["runs"] > 0 and (head["longest"] > 1) == (ncu == 1), head
            if sizes[0] % 2 == 0:
                assert tail["runs"] > 0 and (tail["longest"] > 1) == (ncu == 1), tail
            else:
                assert tail["runs"] == 0 and tail["rest"] > 0, tail
            rr = Report("eval", "dataflow", c.name, "planned on %d CUs" % ncu)
            compare_eval(rr, dev, got, want, Kinv, alpha)
        r.bad += rr.bad
    r.done()


def test_sparse_kuf_runs_on_the_strip_kernel_across_cuts():
    """a Titsias case the strip kernel takes (sparse_sweep's generator; T = 3, rows of 5; 3 full row blocks of Z against 10 full column tiles
    of X): with one CU planned the (Z, X) list holds runs of 8 tiles -- read back from the handle (mogp_model_strip_runs), on a new handle and on
    a live one whose list is cut again -- and ELBO, mom_uf and gZ are the bits of the device's own count, where every run is one tile; the
    ELBO and the moments also against the twin at the sparse sweep's bounds"""
    c = sw.sparse_case()
    want = ss.twin(c).titsias_eval(c.Z, c.sigma, c.jitter, c.kff, grad=True)
    r = Report("titsias", "640 against 192")

    def run(dev, ncu, tag):
        with planned_on(ncu):
            got = dev.titsias_eval(c.Z, c.sigma, c.jitter, c.kff, grad=True)
            cut = dev.strip_runs(4)
        print("spectral sweep |", r.tag, "|", tag, "| (Z, X) list |", cut)
        assert cut["runs"] > 0 and cut["rest"] == 0, cut       # all 30 tiles are full and at even offsets: none for the general kernel
        assert cut["longest"] == (8 if ncu == 1 else 1), cut
        r.err(tag + " elbo", got["elbo"], want["elbo"], 1e-9)
        for k in ("mom_uu", "mom_uf"):
            r.err(tag + " " + k, got[k], want[k], 1e-7)
        return got

    live = device(c)
    own = run(live, 0, "device's count")
    recut = run(live, 1, "live handle, one CU")
    fresh = run(device(c), 1, "new handle, one CU")
    back = run(live, 0, "live handle, back")
    r.done()
    for other in (recut, fresh, back):
        assert other["elbo"] == own["elbo"]
        assert np.array_equal(other["mom_uf"], own["mom_uf"]) and np.array_equal(other["gZ"], own["gZ"])
    assert np.any(own["mom_uf"]) and np.any(own["gZ"])


def test_plan_cus_zero_gives_back_the_bits_of_an_untouched_handle():
    """a probe and an evaluation under plan_cus(0) -- on the handle that was created before the module's first plan_cus call, after it has been
    through another count, and on a new one -- are bit for bit what that handle gave then"""
    c = sw.runs_case((704,), 3)
    h = BASELINE["handle"]
    with planned_on(3):
        moved = h.gram_probe(c.noise, c.jitter, c.dvar)
        h.eval(c.noise, c.jitter, grad=True)
        assert h.strip_runs(0)["longest"] == 8
    assert np.array_equal(moved, BASELINE["probe"])
    for dev in (h, device(c)):
        assert np.array_equal(dev.gram_probe(c.noise, c.jitter, c.dvar), BASELINE["probe"])
        assert dev.strip_runs(0)["longest"] == 1
        assert eval_bits(dev.eval(c.noise, c.jitter, grad=True)) == BASELINE["eval"]
    with pytest.raises(_lib.MogpError):
        _lib.plan_cus(-1)
    with pytest.raises(_lib.MogpError, match="no evaluation has completed"):      # the probe ends what the last evaluation left, like any evaluation
        h.gram_probe(c.noise, c.jitter)
        h.fetch(2)
