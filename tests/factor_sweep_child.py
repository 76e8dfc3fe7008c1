"""
The device side of the factorisation sweep (tests/test_factor_sweep_gpu.py): ONE configuration of the exact path's schedules per process,
because MOGP_GRAD_PATH, MOGP_CHAIN and MOGP_FULL_INVERSE are read once per process -- the parent sets them in this process's environment,

    python tests/factor_sweep_child.py <configuration> <out.npz>

and this module loops over the cases of tests/factor_sweep.py through the raw ABI (mogptk_amd._lib.ExactHandle), asks the device and writes
what it said: the outputs the parent holds to the reference, how every evaluation was scheduled, and -- device against device, where the
claim is equal bits -- whether two results were equal and how far apart if not.  Nothing is compared with the reference here and nothing is
asserted about numbers; an error of the library ends the process (no retry) and the parent reports it.  W and Kj^-1 travel as their lower
triangles: mogp_model_fetch fills the rest by construction, which is recorded as checked.

Configurations: default (MOGP_FLOW toggled per call: dataflow forced from two tile rows on, streams, nothing set from 8 tile rows on; the
LML-only call; the accurate mode and back), phases, sweep, chain0 (one loop over the cases each), banded_fused / banded_phases and
full_fused / full_phases (the banded cases), predict.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

from mogptk_amd import _lib            # noqa: E402
import factor_sweep as fs              # noqa: E402

FLOW_KEYS = ("MOGP_FLOW", "MOGP_FLOW_MIN", "MOGP_FLOW_PREDICT")
SCHED_BITS = ("dataflow", "chain_kernel", "dataflow_fell_back", "chain_fell_back")


def set_flow(**kw):
    """the switches flow.hip and exact.hip read per call: those given, the others unset"""
    for k in FLOW_KEYS:
        os.environ.pop(k, None)
    for k, v in kw.items():
        os.environ["MOGP_" + k] = v


def handle(c):
    h = _lib.ExactHandle(0, c.X, c.y, c.C)
    h.set_terms(c.table)
    return h


def pivots(h):
    lo, hi = np.zeros(1), np.zeros(1)
    _lib.check(_lib.lib().mogp_model_pivot_range(h._h, _lib._dp(lo), _lib._dp(hi)))
    return np.array([lo[0], hi[0]])


def schedule(h):
    s = h.schedule()
    return np.array([int(s[k]) for k in SCHED_BITS] + [s["dataflow_timeouts"]])


def packed(M):
    return M[np.tril_indices(M.shape[0])]


def fetch_W(h):
    """(W or None, the refusal's text or "")"""
    try:
        return h.fetch(0), ""
    except _lib.MogpError as e:
        return None, "%d: %s" % (e.code, e)


def same(a, b):
    """(equal to the bit, largest difference) of two dicts of arrays over the keys of the first"""
    worst, eq = 0.0, True
    for k in a:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        if not np.array_equal(x, y):
            eq = False
            worst = max(worst, float(np.max(np.abs(x - y))) if x.shape == y.shape else np.inf)
    return np.array([float(eq), worst])


def grad_outputs(h, c, matrices=True):
    """a gradient evaluation and everything the handle says about it -> dict of arrays"""
    a = h.eval(c.noise, c.jitter, grad=True)
    r = dict(lml=np.float64(a["lml"]), jitter_abs=np.float64(a["jitter_abs"]), moments=a["moments"], diagG=a["diagG"], trG=np.float64(a["trG"]),
             sched=schedule(h), frac=np.float64(h.inverse_fraction()), pivots=pivots(h))
    if matrices:
        W, refusal = fetch_W(h)
        r["W_refused"] = np.array(refusal)
        if W is not None:
            r["W_upper_zero"] = np.array(not np.any(np.triu(W, 1)))
            r["W"] = packed(W)
        K = h.fetch(1)
        r["Kinv_symmetric"] = np.array(np.array_equal(K, K.T))
        r["Kinv"] = packed(K)
        r["alpha"] = h.fetch(2)
    return r


NUMBERS = ("lml", "jitter_abs", "moments", "diagG", "trG", "pivots")
BITS = NUMBERS + ("W", "Kinv", "alpha")


def bits_of(r):
    return {k: r[k] for k in BITS if k in r}


def lml_only(h, c):
    b = h.eval(c.noise, c.jitter, grad=False)
    r = dict(lml=np.float64(b["lml"]), jitter_abs=np.float64(b["jitter_abs"]), pivots=pivots(h))
    W, refusal = fetch_W(h)
    r["W_refused"] = np.array(refusal)
    if W is not None:
        r["W"] = packed(W)
    return r


def put(out, case, mode, r, drop=()):
    for k, v in r.items():
        if k not in drop:
            out["%s/%s/%s" % (case, mode, k)] = v


def one_schedule(out, c, mode, h=None):
    """evaluation, the same again on the same handle, the LML-only call: what every configuration records of a case"""
    h = h or handle(c)
    first = grad_outputs(h, c)
    put(out, c.name, mode, first)
    again = grad_outputs(h, c)
    out["%s/%s/repeat" % (c.name, mode)] = same(bits_of(first), bits_of(again))
    put(out, c.name, mode + "_lml_only", lml_only(h, c))
    return h, first


def run_default(out):
    for name in fs.CASES:
        c = fs.case(name)
        set_flow(FLOW="0")
        h, stream = one_schedule(out, c, "stream")
        if c.nb >= 2:
            set_flow(FLOW="1", FLOW_MIN="2")
            flow = grad_outputs(h, c)
            again = grad_outputs(h, c)
            out["%s/flow/repeat" % name] = same(bits_of(flow), bits_of(again))
            eq = same({k: flow[k] for k in ("W", "Kinv")}, stream)
            out["%s/flow/equals_stream" % name] = eq
            put(out, name, "flow", flow, drop=("W", "Kinv") if eq[0] else ())      # equal bits: the stream form's copy stands for both
        if c.nb >= 8:
            set_flow()
            auto = grad_outputs(h, c)
            out["%s/auto/sched" % name] = auto["sched"]
            out["%s/auto/equals_flow" % name] = same(bits_of(auto), bits_of(flow))
        set_flow()
        h.set_accurate(1)
        acc = grad_outputs(h, c)
        put(out, name, "accurate", acc)
        out["%s/accurate/repeat" % name] = same(bits_of(acc), bits_of(grad_outputs(h, c)))
        put(out, name, "accurate_lml_only", lml_only(h, c))
        h.set_accurate(0)
        back = grad_outputs(h, c)
        h.close()
        h2 = handle(c)
        out["%s/after_accurate/equals_fresh" % name] = same(bits_of(back), bits_of(grad_outputs(h2, c)))
        out["%s/after_accurate/sched" % name] = back["sched"]
        h2.close()


def run_one_path(out, mode, names):
    set_flow()
    for name in names:
        h, _ = one_schedule(out, fs.case(name), mode)
        h.close()


def run_chain0(out):
    set_flow(FLOW="0")          # (without the chain kernel there is no dataflow form: said anyway, so that the configuration names its schedule)
    for name in fs.CASES:
        h, _ = one_schedule(out, fs.case(name), "chain0")
        h.close()


def run_banded(out, mode, full):
    """the planned inverse (or, full: every tile, MOGP_FULL_INVERSE=1 in the environment, the stream form of the same schedule): the outputs,
    Kj^-1 completed on demand behind them, and the evaluation once more"""
    set_flow(FLOW="0") if full else set_flow()
    for name in fs.BANDED:
        c = fs.case(name)
        h = handle(c)
        first = grad_outputs(h, c)
        put(out, name, mode, first)
        again = grad_outputs(h, c, matrices=False)            # ... behind a fetch that completed the inverse in place
        out["%s/%s/repeat" % (name, mode)] = same({k: first[k] for k in NUMBERS}, again)
        out["%s/%s/frac_again" % (name, mode)] = again["frac"]
        h.close()


def run_predict(out):
    for name in fs.PREDICT_CASES:
        c = fs.case(name)
        h = handle(c)
        set_flow(FLOW_MIN="2")
        before = grad_outputs(h, c, matrices=False)
        out["%s/predict/grad_sched" % name] = before["sched"]
        for S in fs.TEST_SETS:
            Xs = fs.test_points(name, S)
            for form, env in (("flow", dict(FLOW_MIN="2", FLOW_PREDICT="2:200")), ("stream", dict(FLOW_MIN="2", FLOW_PREDICT="0"))):
                set_flow(**env)
                mu, var = h.predict(c.noise, c.jitter, c.kss, Xs)
                key = "%s/predict_%s_%d/" % (name, form, S)
                out[key + "mu"], out[key + "var"], out[key + "sched"] = mu, var, schedule(h)
                mu2, var2 = h.predict(c.noise, c.jitter, c.kss, Xs)
                out[key + "repeat"] = same(dict(mu=mu, var=var), dict(mu=mu2, var=var2))
                if S == fs.FULL_COV_S:
                    mu, cov = h.predict(c.noise, c.jitter, c.kss, Xs, full=True)
                    out[key + "mu_full"], out[key + "cov"], out[key + "sched_full"] = mu, cov, schedule(h)
            if (name, S) == fs.ACCURATE_PREDICT:
                set_flow(FLOW_MIN="2", FLOW_PREDICT="2:200")    # the accurate prediction is the stream form whatever this says
                h.set_accurate(1)
                mu, var = h.predict(c.noise, c.jitter, c.kss, Xs)
                key = "%s/predict_accurate_%d/" % (name, S)
                out[key + "mu"], out[key + "var"], out[key + "sched"] = mu, var, schedule(h)
                h.set_accurate(0)
        set_flow(FLOW_MIN="2")
        after = grad_outputs(h, c, matrices=False)
        out["%s/predict/grad_equal" % name] = same({k: before[k] for k in NUMBERS}, after)
        put(out, name, "predict_grad", {k: before[k] for k in ("lml", "moments")})
        h.close()


CONFIGS = {
    "default": run_default,
    "phases": lambda out: run_one_path(out, "phases", fs.CASES),
    "sweep": lambda out: run_one_path(out, "sweep", fs.CASES),
    "chain0": run_chain0,
    "banded_fused": lambda out: run_banded(out, "banded_fused", False),
    "banded_phases": lambda out: run_banded(out, "banded_phases", False),
    "full_fused": lambda out: run_banded(out, "full_fused", True),
    "full_phases": lambda out: run_banded(out, "full_phases", True),
    "predict": run_predict,
}


def main(config, path):
    out = {}
    CONFIGS[config](out)
    out["env"] = np.array(" ".join("%s=%s" % (k, os.environ[k]) for k in ("MOGP_GRAD_PATH", "MOGP_CHAIN", "MOGP_FULL_INVERSE") if k in os.environ))
    np.savez(path, **out)
    print("FACTOR_SWEEP_CHILD_OK", config, len(out))


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
