"""The host side of one training step of the headline configuration, by the wall clock (no profiler in the loop).  With the numpy form of the host algebra
(MOGP_HOST_FAST=0): Python in front of the native evaluation (raw -> constrained parameters -> term table -> mogp_model_set_terms), the native call, Python
behind it (moments -> chain rule -> raw gradients), the Adam update.  With the native step (the default): Python in front of mogp_exact_step, the call -- which
now holds the table and the chain rule as well as the evaluation --, Python behind it, the Adam update.
usage: python tools/host_profile.py [steps]"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import bench
steps = int(sys.argv[1]) if len(sys.argv) > 1 else 300
m, run_step, _ = bench.build_model("cfg2", 0)
step = bench.training_step(m, run_step, "exact")
for _ in range(10):
    step()
h = m._handle
T = dict(set_terms0=[], set_terms1=[], eval0=[], eval1=[], step0=[], step1=[])
o_eval, o_set, o_step = h.eval, h.set_terms, getattr(h, "step", None)
def eval_(*a, **k):
    T["eval0"].append(time.perf_counter()); r = o_eval(*a, **k); T["eval1"].append(time.perf_counter()); return r
def set_(*a, **k):
    T["set_terms0"].append(time.perf_counter()); r = o_set(*a, **k); T["set_terms1"].append(time.perf_counter()); return r
def step_(*a, **k):
    T["step0"].append(time.perf_counter()); r = o_step(*a, **k); T["step1"].append(time.perf_counter()); return r
h.eval, h.set_terms = eval_, set_
if o_step is not None:
    h.step = step_
from mogptk_amd.model import _Adam
opt = _Adam(list(m.parameters()), lr=1e-6)
marks, A = [], []
for _ in range(steps):                      # every evaluation sees new parameters, as in training (an unchanged parameter set hits the term-table memo)
    t0 = time.perf_counter(); run_step(); t1 = time.perf_counter(); opt.step(); t2 = time.perf_counter()
    marks.append((t0, t1)); A.append(t2 - t0)
n = steps
us = lambda v: 1e6 * float(np.median(v))
loss_only = [b - a for a, b in marks]
if len(T["step0"]) == n:                    # the native step
    pre = [T["step0"][i] - marks[i][0] for i in range(n)]
    nat = [T["step1"][i] - T["step0"][i] for i in range(n)]
    post = [marks[i][1] - T["step1"][i] for i in range(n)]
    print("loss() alone (native step): %.1f us = python before the native call %.1f + mogp_exact_step (table, evaluation, chain rule) %.1f + python behind it %.1f" %
          (us(loss_only), us(pre), us(nat), us(post)))
else:
    pre = [T["set_terms0"][i] - marks[i][0] for i in range(n)]
    st = [T["set_terms1"][i] - T["set_terms0"][i] for i in range(n)]
    mid = [T["eval0"][i] - T["set_terms1"][i] for i in range(n)]
    nat = [T["eval1"][i] - T["eval0"][i] for i in range(n)]
    post = [marks[i][1] - T["eval1"][i] for i in range(n)]
    print("loss() alone: %.1f us = python before set_terms %.1f + set_terms %.1f + python up to the native call %.1f + native evaluation %.1f + python behind it %.1f" %
          (us(loss_only), us(pre), us(st), us(mid), us(nat), us(post)))
print("loss() + Adam step: %.1f us  (the optimiser's share: %.1f us)" % (us(A), us(A) - us(loss_only)))
