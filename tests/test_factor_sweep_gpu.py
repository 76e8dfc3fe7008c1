"""
Every schedule under which the exact path factorises and inverts Kj -- fused as tile dataflow (csrc/flow.hip), fused as streams
(csrc/potri.hip) on the persistent chain kernel and on the launch-per-step chain, phases (POTRF, TRTRI, LAUUM), sweep (csrc/sweep.hip), the
accurate mode -- with the planned inverse and both forms of the prediction's forward substitution on top, held to an INDEPENDENT inverse:
numpy / scipy in float64 on the same inputs (tests/factor_sweep.py; its own error is pinned at a hundredth of the bounds used here by
tests/test_factor_sweep_cpu.py).  The sizes are the ones at which the launches change: 1 to 13 tile rows with every shape of the last
outer block, one valid row in the last tile (N = 513, 1025, 1537), no padding at all (512, 1024), an empty channel and a one-point channel.

MOGP_GRAD_PATH, MOGP_CHAIN and MOGP_FULL_INVERSE are read once per process: one fresh child per configuration
(tests/factor_sweep_child.py), one after the other, each with a time limit; a child that fails ends there and nothing is tried again.  The
child writes what the device said, this module compares.  Every figure is printed, all misses of a test fail together.

Bounds, errors as kernel_family.err unless said: LML 1e-9 and jitter_abs 1e-14 relative; moments, diagG, trG 1e-7;
W = L^-1 (mogp_model_fetch 0), Kj^-1 (1), alpha (2) 1e-9; the pivot range against diag(L) 1e-9 relative; predictions 1e-9.  W is held
wherever the handle keeps it; the sweep (which inverts in place) and the accurate mode (which keeps L) refuse mogp_model_fetch(0) in words,
asserted.  Equal bits are asserted where the design claims them: a second evaluation on the same handle, dataflow against streams on W and
Kj^-1 at every size, the default schedule from 8 tile rows on against the forced dataflow form, a handle back from the accurate mode against
a fresh one, the planned inverse against MOGP_FULL_INVERSE=1 on LML, moments, diagG and trG, a gradient evaluation before and after the
predictions.  Whether the chain kernel and the launch-per-step chain agree to the bit is printed, not asserted.
"""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import factor_sweep as fs
from kernel_family import err

pytestmark = pytest.mark.gpu

TOL_LML, TOL_JITTER, TOL_GRAD, TOL_MATRIX, TOL_PIVOT, TOL_PREDICT = 1e-9, 1e-14, 1e-7, 1e-9, 1e-9, 1e-9
PLAN_MAX = 0.85
# a child is one process start (a second or two with the library) and, per case, a dozen evaluations of at most 1537 points with their N x N
# copies home: seconds.  Forty times that, so that a loaded machine does not decide a test
CHILD_TIMEOUT = 240
HERE = os.path.dirname(os.path.abspath(__file__))
ONCE_PER_PROCESS = ("MOGP_GRAD_PATH", "MOGP_CHAIN", "MOGP_FULL_INVERSE")
PER_CALL = ("MOGP_FLOW", "MOGP_FLOW_MIN", "MOGP_FLOW_PREDICT")          # the child sets these itself
ENV = {
    "default": {}, "predict": {},
    "phases": {"MOGP_GRAD_PATH": "phases"}, "sweep": {"MOGP_GRAD_PATH": "sweep"}, "chain0": {"MOGP_CHAIN": "0"},
    "banded_fused": {"MOGP_GRAD_PATH": "fused"}, "banded_phases": {"MOGP_GRAD_PATH": "phases"},
    "full_fused": {"MOGP_GRAD_PATH": "fused", "MOGP_FULL_INVERSE": "1"}, "full_phases": {"MOGP_GRAD_PATH": "phases", "MOGP_FULL_INVERSE": "1"},
}
REFUSAL = "%d: mogp_model_fetch: no evaluation has completed yet" % -1          # MOGP_EINVAL and the words of csrc/mogp_api.hip


CHILDREN = {}


def run_child(config):
    env = {k: v for k, v in os.environ.items() if k not in ONCE_PER_PROCESS + PER_CALL}
    env.update(ENV[config])
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, config + ".npz")
        run = subprocess.run([sys.executable, os.path.join(HERE, "factor_sweep_child.py"), config, path], capture_output=True, text=True,
                             timeout=CHILD_TIMEOUT, env=env)
        assert run.returncode == 0 and "FACTOR_SWEEP_CHILD_OK" in run.stdout, (config, run.returncode, run.stdout[-1500:], run.stderr[-3000:])
        if run.stderr.strip():
            print("factor sweep | child", config, "| stderr |", run.stderr[-1500:])
        with np.load(path) as f:
            return {k: f[k] for k in f.files}


def child(config):
    """what one configuration's process wrote, as a dict.  Run ONCE however many tests read it: a configuration that failed (or ran into its
    time limit) is not started again, the next reader gets the same failure"""
    if config not in CHILDREN:
        try:
            CHILDREN[config] = run_child(config)
        except (AssertionError, subprocess.TimeoutExpired) as e:
            CHILDREN[config] = e
    if isinstance(CHILDREN[config], BaseException):
        raise CHILDREN[config]
    return CHILDREN[config]


class Report:
    """prints every figure of a case, fails at the end with all that missed their bound"""

    def __init__(self, test):
        self.test, self.bad, self.worst = test, [], {}

    def add(self, case, mode, name, e, tol):
        print("factor sweep |", case, "|", mode, "|", name, "|", e)
        key = (mode, name)
        self.worst[key] = max(self.worst.get(key, 0.0), float(e))
        if not e <= tol:
            self.bad.append((case, mode, name, e, tol))

    def relative(self, case, mode, name, got, want, tol):
        self.add(case, mode, name, abs(float(got) - float(want)) / abs(float(want)), tol)

    def tensor(self, case, mode, name, got, want, tol):
        self.add(case, mode, name, err(got, want), tol)

    def true(self, case, mode, name, ok, detail=None):
        print("factor sweep |", case, "|", mode, "|", name, "|", bool(ok), "" if detail is None else detail)
        if not ok:
            self.bad.append((case, mode, name, detail))

    def bits(self, case, mode, name, pair):
        """pair: (equal to the bit, largest difference) as the child measured it"""
        self.true(case, mode, name + " (equal bits)", pair[0] == 1.0, "largest difference %g" % pair[1])

    def done(self):
        for m in sorted({m for m, _ in self.worst}):
            print("factor sweep worst |", m, "|", ", ".join("%s %.1e" % (n, e) for (mm, n), e in sorted(self.worst.items()) if mm == m))
        assert not self.bad, (self.test, self.bad)


def lower(packed, N):
    M = np.zeros((N, N))
    M[np.tril_indices(N)] = packed
    return M


def symmetric(packed, N):
    M = lower(packed, N)
    return M + np.tril(M, -1).T


def sched(v):
    return dict(dataflow=bool(v[0]), chain_kernel=bool(v[1]), dataflow_fell_back=bool(v[2]), chain_fell_back=bool(v[3]), dataflow_timeouts=int(v[4]))


def check_schedule(rep, case, mode, v, dataflow, chain_kernel=True):
    s = sched(v)
    ok = s["dataflow"] == dataflow and s["chain_kernel"] == chain_kernel and not s["dataflow_fell_back"] and not s["chain_fell_back"] and s["dataflow_timeouts"] == 0
    rep.true(case, mode, "schedule as asked (dataflow %s, chain kernel %s)" % (dataflow, chain_kernel), ok, s)


def check_outputs(rep, out, name, mode, holds_W=True, pivots=True, matrices_from=None):
    """the outputs of one gradient evaluation against the reference; matrices_from: the mode whose copy of W and Kj^-1 stands for this one's
    (equal bits, asserted by the caller)"""
    c, ref = fs.case(name), fs.reference(name)
    g = lambda k, m=mode: out["%s/%s/%s" % (name, m, k)]
    rep.relative(name, mode, "lml", g("lml"), ref["lml"], TOL_LML)
    rep.relative(name, mode, "jitter_abs", g("jitter_abs"), ref["jitter_abs"], TOL_JITTER)
    rep.tensor(name, mode, "moments", g("moments"), ref["moments"], TOL_GRAD)
    rep.tensor(name, mode, "diagG", g("diagG"), ref["diagG"], TOL_GRAD)
    rep.tensor(name, mode, "trG", g("trG"), ref["trG"], TOL_GRAD)
    mm = matrices_from or mode
    refusal = str(g("W_refused"))
    if holds_W:
        rep.true(name, mode, "fetch(0) is answered", refusal == "" and bool(g("W_upper_zero")), refusal)
        if refusal == "":
            rep.tensor(name, mode, "W", lower(g("W", mm), c.N), ref["W"], TOL_MATRIX)
    else:
        rep.true(name, mode, "fetch(0) is refused in the documented words", refusal == REFUSAL, refusal)
    rep.true(name, mode, "fetch(1) is symmetric", bool(g("Kinv_symmetric")))
    rep.tensor(name, mode, "Kinv", symmetric(g("Kinv", mm), c.N), ref["Kinv"], TOL_MATRIX)
    rep.tensor(name, mode, "alpha", g("alpha"), ref["alpha"], TOL_MATRIX)
    check_pivots(rep, name, mode, g("pivots"), pivots)


def check_pivots(rep, name, mode, got, reported=True):
    ref = fs.reference(name)
    if reported:
        rep.relative(name, mode, "pivot min", got[0], ref["lmin"], TOL_PIVOT)
        rep.relative(name, mode, "pivot max", got[1], ref["lmax"], TOL_PIVOT)
    else:
        rep.true(name, mode, "pivot range reported as 0, 0", got[0] == 0.0 and got[1] == 0.0, got)


def check_lml_only(rep, out, name, mode, holds_W=True):
    """the evaluation without gradients (POTRF and TRTRI, or the refined factor alone) and the W it leaves"""
    c, ref = fs.case(name), fs.reference(name)
    g = lambda k: out["%s/%s/%s" % (name, mode, k)]
    rep.relative(name, mode, "lml", g("lml"), ref["lml"], TOL_LML)
    rep.relative(name, mode, "jitter_abs", g("jitter_abs"), ref["jitter_abs"], TOL_JITTER)
    check_pivots(rep, name, mode, g("pivots"))
    refusal = str(g("W_refused"))
    if holds_W:
        rep.true(name, mode, "fetch(0) is answered", refusal == "", refusal)
        if refusal == "":
            rep.tensor(name, mode, "W", lower(g("W"), c.N), ref["W"], TOL_MATRIX)
    else:
        rep.true(name, mode, "fetch(0) is refused in the documented words", refusal == REFUSAL, refusal)


def test_fused_schedules_and_the_accurate_mode():
    """the default process: streams (MOGP_FLOW=0), dataflow forced from two tile rows on (MOGP_FLOW=1, MOGP_FLOW_MIN=2), nothing set from 8
    tile rows on, the LML-only call, the accurate mode and the way back from it"""
    out, rep = child("default"), Report("default")
    for name in fs.CASES:
        c = fs.case(name)
        check_schedule(rep, name, "stream", out[name + "/stream/sched"], dataflow=False)
        check_outputs(rep, out, name, "stream")
        rep.true(name, "stream", "every tile of the inverse formed", out[name + "/stream/frac"] == 1.0, out[name + "/stream/frac"])
        rep.bits(name, "stream", "second evaluation on the handle", out[name + "/stream/repeat"])
        check_lml_only(rep, out, name, "stream_lml_only")
        if c.nb >= 2:
            check_schedule(rep, name, "flow", out[name + "/flow/sched"], dataflow=True)          # a silent detour to streams fails here
            eq = out[name + "/flow/equals_stream"]
            rep.bits(name, "flow", "W and Kinv against the stream form", eq)
            check_outputs(rep, out, name, "flow", matrices_from="stream" if eq[0] == 1.0 else None)
            rep.bits(name, "flow", "second evaluation on the handle", out[name + "/flow/repeat"])
        if c.nb >= 8:
            check_schedule(rep, name, "auto", out[name + "/auto/sched"], dataflow=True)
            rep.bits(name, "auto", "nothing set against dataflow forced", out[name + "/auto/equals_flow"])
        check_schedule(rep, name, "accurate", out[name + "/accurate/sched"], dataflow=False)
        check_outputs(rep, out, name, "accurate", holds_W=False)
        rep.bits(name, "accurate", "second evaluation on the handle", out[name + "/accurate/repeat"])
        check_lml_only(rep, out, name, "accurate_lml_only", holds_W=False)
        check_schedule(rep, name, "after_accurate", out[name + "/after_accurate/sched"], dataflow=c.nb >= 8)
        rep.bits(name, "after_accurate", "back from the accurate mode against a fresh handle", out[name + "/after_accurate/equals_fresh"])
    rep.done()


@pytest.mark.parametrize("config", ["phases", "sweep", "chain0"])
def test_schedule_of_its_own_process(config):
    """MOGP_GRAD_PATH=phases, MOGP_GRAD_PATH=sweep, MOGP_CHAIN=0 (fused streams on the launch-per-step chain)"""
    out, rep = child(config), Report(config)
    for name in fs.CASES:
        check_schedule(rep, name, config, out["%s/%s/sched" % (name, config)], dataflow=False, chain_kernel=config != "chain0")
        check_outputs(rep, out, name, config, holds_W=config != "sweep", pivots=config != "sweep")
        rep.true(name, config, "every tile of the inverse formed", out["%s/%s/frac" % (name, config)] == 1.0)
        rep.bits(name, config, "second evaluation on the handle", out["%s/%s/repeat" % (name, config)])
        check_lml_only(rep, out, name, config + "_lml_only")         # POTRF and TRTRI whatever the gradient's schedule: W is there, under sweep too
    if config == "chain0":
        base = child("default")
        for name in fs.CASES:
            eq = {k: np.array_equal(out["%s/chain0/%s" % (name, k)], base["%s/stream/%s" % (name, k)]) for k in ("W", "Kinv", "alpha", "lml", "moments")}
            print("factor sweep |", name, "| chain0 | launch-per-step chain against the chain kernel, equal bits (not asserted) |", eq)
    rep.done()


@pytest.mark.parametrize("path", ["fused", "phases"])
def test_planned_inverse_with_a_partial_last_block(path):
    """the banded cases: 11 tile rows (last outer block of 3) and 13 (of one tile with one valid row).  The evaluation takes the plan by the
    library's own rule (fraction below 0.85), matches the reference, mogp_model_fetch(1) completes the inverse on demand, and LML, moments,
    diagG and trG are those of the same schedule with every tile formed (MOGP_FULL_INVERSE=1), to the bit"""
    mode, full_mode = "banded_" + path, "full_" + path
    out, full, rep = child(mode), child(full_mode), Report(mode)
    for name in fs.BANDED:
        frac = float(out["%s/%s/frac" % (name, mode)])
        rep.true(name, mode, "the plan is taken (inverse_fraction below %g)" % PLAN_MAX, 0.0 < frac < PLAN_MAX, frac)
        rep.true(name, mode, "and again behind the completed inverse", float(out["%s/%s/frac_again" % (name, mode)]) == frac)
        rep.true(name, full_mode, "every tile formed", float(full["%s/%s/frac" % (name, full_mode)]) == 1.0)
        check_schedule(rep, name, mode, out["%s/%s/sched" % (name, mode)], dataflow=False)          # a planned inverse takes the stream form
        check_schedule(rep, name, full_mode, full["%s/%s/sched" % (name, full_mode)], dataflow=False)
        check_outputs(rep, out, name, mode)                                                      # fetch(1): completed on demand
        check_outputs(rep, full, name, full_mode)
        rep.bits(name, mode, "second evaluation on the handle", out["%s/%s/repeat" % (name, mode)])
        for k in ("lml", "moments", "diagG", "trG"):
            a, b = out["%s/%s/%s" % (name, mode, k)], full["%s/%s/%s" % (name, full_mode, k)]
            rep.true(name, mode, k + " equal to the bits of MOGP_FULL_INVERSE=1", np.array_equal(a, b), "largest difference %g" % float(np.max(np.abs(a - b))))
    rep.done()


def test_prediction_in_both_forms():
    """5, 8, 9 and 13 tile rows against test sets of 1, 128, 129 and 300 points (2, 2, 3 and 4 tile rows of [K_sf ; y^T]) in shuffled order:
    factorisation and forward substitution as one dataflow schedule (MOGP_FLOW_PREDICT=2:200, asserted through mogp_model_schedule) and as
    streams, each against TableDevice.predict and against the other; the full covariance at S = 129; the accurate mode once; a gradient
    evaluation (dataflow: the two plans share the handle's counters) before and after, equal bits"""
    out, rep = child("predict"), Report("predict")
    for name in fs.PREDICT_CASES:
        want = fs.reference_predictions(name)
        ref = fs.reference(name)
        check_schedule(rep, name, "predict", out[name + "/predict/grad_sched"], dataflow=True)
        rep.relative(name, "predict", "lml of the gradient evaluation", out[name + "/predict_grad/lml"], ref["lml"], TOL_LML)
        rep.tensor(name, "predict", "moments of the gradient evaluation", out[name + "/predict_grad/moments"], ref["moments"], TOL_GRAD)
        rep.bits(name, "predict", "gradient evaluation before and after the predictions", out[name + "/predict/grad_equal"])
        for S in fs.TEST_SETS:
            got = {}
            for form in ("flow", "stream"):
                key, mode = "%s/predict_%s_%d/" % (name, form, S), "predict %s S=%d" % (form, S)
                check_schedule(rep, name, mode, out[key + "sched"], dataflow=form == "flow")
                got[form] = (out[key + "mu"], out[key + "var"])
                rep.tensor(name, "predict " + form, "mu", got[form][0], want[S][0], TOL_PREDICT)
                rep.tensor(name, "predict " + form, "var", got[form][1], want[S][1], TOL_PREDICT)
                rep.bits(name, mode, "the same prediction again", out[key + "repeat"])
                if S == fs.FULL_COV_S:
                    check_schedule(rep, name, mode + " full", out[key + "sched_full"], dataflow=form == "flow")
                    rep.tensor(name, "predict " + form, "mu (full)", out[key + "mu_full"], want[S][0], TOL_PREDICT)
                    rep.tensor(name, "predict " + form, "cov", out[key + "cov"], want["cov"], TOL_PREDICT)
                    got[form] += (out[key + "cov"],)
            for i, k in enumerate(("mu", "var", "cov")[:len(got["flow"])]):
                rep.tensor(name, "predict flow against stream", k, got["flow"][i], got["stream"][i], TOL_PREDICT)
            if (name, S) == fs.ACCURATE_PREDICT:
                key = "%s/predict_accurate_%d/" % (name, S)
                check_schedule(rep, name, "predict accurate", out[key + "sched"], dataflow=False)
                rep.tensor(name, "predict accurate", "mu", out[key + "mu"], want[S][0], TOL_PREDICT)
                rep.tensor(name, "predict accurate", "var", out[key + "var"], want[S][1], TOL_PREDICT)
    rep.done()
