"""Leave-fold-out cross-validation beside leave-one-out on the benchmark model (MOSM, C = 4, Q = 3, N = 8192): wall time of loo_loss() and of
cv_loss() over blocks of `block` consecutive points per channel (what Model.block_folds makes), median of `reps`, and inside the CV call the
two kernels of csrc/lfo.hip by HIP events (mogp_model_fetch 4: k_cv_folds; the zero fill of S with k_cv_cols) as shares of the call.  One
process, one pass, its own time limit (SIGALRM): a run that does not finish is reported as such, not repeated.
usage: python tools/cv_time.py [N] [C] [Q] [block] [reps] [limit_s]"""
import json, os, signal, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench
from mogptk_amd import _lib

N = int(sys.argv[1]) if len(sys.argv) > 1 else 8192
C = int(sys.argv[2]) if len(sys.argv) > 2 else 4
Q = int(sys.argv[3]) if len(sys.argv) > 3 else 3
block = int(sys.argv[4]) if len(sys.argv) > 4 else 64
reps = int(sys.argv[5]) if len(sys.argv) > 5 else 15
limit = int(sys.argv[6]) if len(sys.argv) > 6 else 240


def out_of_time(*_):
    print(json.dumps(dict(N=N, error="time limit of %d s reached" % limit)), flush=True)
    os._exit(3)


signal.signal(signal.SIGALRM, out_of_time)
signal.alarm(limit)

m = bench.build_mosm(N, C, Q, 0)
X = np.asarray(m.X, dtype=np.float64)
folds = np.empty(X.shape[0], dtype=np.int32)
first = 0
for c in np.unique(X[:, 0]):
    rows = np.flatnonzero(X[:, 0] == c)
    rows = rows[np.argsort(X[rows, 1], kind="stable")]
    folds[rows] = first + np.arange(rows.size) // block
    first += -(-rows.size // block)


def wall(fn):
    fn(); fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); t.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(t)), float(min(t))


lml_ms, lml_min = wall(m.loss)
loo_ms, loo_min = wall(m.loo_loss)
cv_ms, cv_min = wall(lambda: m.cv_loss(folds))
h = m._handle
h.set_profiling(True)
kf, kc, tot = [], [], []
for _ in range(reps):
    m.cv_loss(folds)
    a, b = h.fetch(4)
    kf.append(a); kc.append(b); tot.append(h.stage_ms()[0][_lib.ST_TOTAL])          # the device's own span of the call
h.set_profiling(False)
kf, kc, tot = float(np.median(kf)), float(np.median(kc)), float(np.median(tot))
print(json.dumps(dict(N=N, C=C, Q=Q, block=block, folds=int(first), reps=reps, lml_loss_ms=lml_ms, lml_loss_min_ms=lml_min, loo_loss_ms=loo_ms, loo_loss_min_ms=loo_min,
                      cv_loss_ms=cv_ms, cv_loss_min_ms=cv_min, cv_over_loo=cv_ms / loo_ms, cv_device_ms=tot, k_cv_folds_ms=kf, k_cv_cols_with_fill_ms=kc,
                      k_cv_folds_share=kf / tot, k_cv_cols_share=kc / tot, loo_bytes=h.loo_bytes())))
