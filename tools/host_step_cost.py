"""The host's share of one training step of a plain MOSM model with the device taken out: the model of bench.build_mosm(N, 4, 3) over a stub handle
whose set_terms, eval and -- for the native step -- device part return a cached result at once (one evaluation of the numpy twin, made before
anything is timed).  Prints the median wall-clock cost of loss() + _Adam.step() with gpr.config.host_fast off and on, in the same run, and the
largest distance between the native transforms (csrc/hoststep.hip) and gpr/parameter.py on a grid of raw values.  Needs no GPU.
usage: python tools/host_step_cost.py [steps = 400] [N = 256]"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import bench
from mogptk_amd import _lib, gpr
from mogptk_amd.gpr.parameter import Softplus, Sigmoid
from mogptk_amd.model import _Adam
from oracle.table_model import TableDevice

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 400
N = int(sys.argv[2]) if len(sys.argv) > 2 else 256


class Stub:
    """the methods gpr.Exact.loss() calls on a device handle, with nothing behind them"""
    res = None

    def __init__(self, device, X, y, C):
        self.N, self.D, self.C = X.shape[0], X.shape[1] - 1, C

    def set_terms(self, table):
        self.T, self.W = table.shape[2], table.shape[3]

    def eval(self, noise_var, jitter, grad=True, data_var=None):
        return Stub.res

    def step(self, plan, jitter, data_var=None):            # mogp_exact_step without its device part: two native calls where the library makes one
        plan.forward()
        if getattr(plan, "filled", None) is not Stub.res:
            plan.moments[...], plan.diagG[...], plan.filled = Stub.res["moments"], Stub.res["diagG"], Stub.res
            plan.out[:] = (Stub.res["lml"], Stub.res["trG"], Stub.res["jitter_abs"], 0.0, 0.0)
        plan.backward(Stub.res["trG"], jitter)


def cost(on):
    gpr.config.host_fast = on
    m = bench.build_mosm(N, 4, 3, None)
    m.loss()
    opt = _Adam(list(m.parameters()), lr=1e-6)
    loss, adam = [], []
    for i in range(steps + 20):
        t0 = time.perf_counter(); m.loss(); t1 = time.perf_counter(); opt.step(); t2 = time.perf_counter()
        if i >= 20:
            loss.append(t1 - t0); adam.append(t2 - t1)
    return 1e6 * float(np.median(loss)), 1e6 * float(np.median(adam)), [p.data.copy() for p in m.parameters()]


def ulps(a, b):
    return int(np.max(np.abs(np.ascontiguousarray(a).view(np.int64) - np.ascontiguousarray(b).view(np.int64))))


def grid():
    x = np.linspace(-400.0, 400.0, 160001)
    n = x.size
    out = []
    for name, tr in (("softplus beta 0.1", Softplus(lower=1e-8)), ("softplus beta -0.1", Softplus(lower=3.0, beta=-0.1)), ("sigmoid", Sigmoid(lower=0.01, upper=0.5))):
        d = (1 if isinstance(tr, Softplus) else 2, tr.lower, getattr(tr, "upper", None), getattr(tr, "beta", None), getattr(tr, "threshold", None))
        plan = _lib.StepPlan(1, n, 1, 1, [d] * 6, 1.0, 1.0, np.ones(1), n, [1] * 6)
        plan.raw[:] = 0.0
        plan.raw[:n] = x
        plan.transcendentals()
        plan.forward()
        with np.errstate(over="ignore"):
            out.append("%s: value %d ulp, derivative %d ulp" % (name, ulps(plan.cons[:n], tr.forward(x)), ulps(plan.dcons[:n], tr.dforward(x))))
    return "; ".join(out)


m = bench.build_mosm(N, 4, 3, None)
twin = TableDevice(0, m.kernel._kernel_format(m.X), m.y, 4)
twin.set_terms(m.kernel._spectral_terms(1))
Stub.res = twin.eval(m._noise_var(), m.jitter, grad=True)
_lib.ExactHandle = Stub
off = cost(False)
on = cost(True)
drift = max(float(np.max(np.abs(a - b))) for a, b in zip(off[2], on[2]))
print("host cost of one training step, device stubbed, N = %d, median of %d steps (us):" % (N, steps))
print("  host_fast off: loss() %.1f + Adam %.1f = %.1f" % (off[0], off[1], off[0] + off[1]))
print("  host_fast on:  loss() %.1f + Adam %.1f = %.1f   (%.2f of off; the bound is 0.20)" % (on[0], on[1], on[0] + on[1], (on[0] + on[1]) / (off[0] + off[1])))
print("  largest difference of a raw parameter after the %d steps of both: %.3g" % (steps + 21, drift))
print("native transforms against gpr/parameter.py, 160001 raw values in [-400, 400]: " + grid())
