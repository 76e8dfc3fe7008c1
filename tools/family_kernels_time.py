"""The two tile kernels of the exact path under a kernel-family model (tests/<family>_cases.py): Gram build and gradient-moment pass, HIP events
around the kernel inside gradient evaluations (as tools/tile_kernels_time.py times them for the MOSM model), median of `reps` after three
warm-up evaluations.  `what` is a case of the family (its own data, unless N is given) or, for a family with `parse`, a kernel expression
such as "f2+se"; with N the inputs are N sorted points over [0, N / 100] (one channel; a two-channel case splits them 3 : 2; further input
dimensions uniform over [0, 1]).
usage: python tools/family_kernels_time.py <family> <what> [N] [reps]"""
import json, os, sys
import numpy as np
os.environ.setdefault("MOGP_GRAD_PATH", "phases")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import family_cases
from mogptk_amd import gpr, _lib

family, what = sys.argv[1], sys.argv[2]
N = int(sys.argv[3]) if len(sys.argv) > 3 else 0
reps = int(sys.argv[4]) if len(sys.argv) > 4 else 30
mod = family_cases.cases(family)
if what in mod.CASES:
    k = mod.kernel(gpr, what)
    X, y, _ = mod.data(what)
else:
    k = family_cases.top(gpr, mod.parse(gpr, what, 1, np.random.default_rng(1)))
    X, y, _ = mod.data(next(iter(mod.CASES)))
if N:
    rng = np.random.default_rng(2)
    x = np.sort(rng.uniform(0.0, N / 100.0, N))
    y = np.sin(x) + 0.1 * rng.standard_normal(N)
    X = x[:, None] if k.output_dims is None else np.stack([(np.arange(N) >= 3 * N // 5).astype(np.float64), x], 1)
    if (k.input_dims or 1) > 1:                               # further input dimensions: uniform over [0, 1]
        X = np.concatenate([X, rng.uniform(0.0, 1.0, (N, k.input_dims - 1))], axis=1)
m = gpr.Exact(k, X, y, variance=mod.NOISE)
for _ in range(3):
    loss = float(m.loss())
h = m._handle
h.set_profiling(True)
g, mo = [], []
for _ in range(reps):
    m.loss()
    ms, _, _ = h.stage_ms()
    g.append(ms[_lib.ST_GRAM_KERNEL]); mo.append(ms[_lib.ST_MOMENT_KERNEL])
print(json.dumps(dict(family=family, what=what, N=len(y), loss=loss, gram_us=1e3 * float(np.median(g)), gram_min_us=1e3 * min(g),
                      moments_us=1e3 * float(np.median(mo)), moments_min_us=1e3 * min(mo))))
