"""The posterior by kernel part beside one prediction: predict_f against predict_terms with P = 1, 2, 4 masks on the same test points, on
(i) the benchmark model (MOSM, C = 4, Q = 3, N = 8192; S = 2048) and (ii) SE + Matern 3/2 + RQ at N = 8192, each with the substitution as tile
dataflow (MOGP_FLOW_PREDICT=8:200) and on streams (=0).  Per line: the device's span of the call by HIP events (set_profiling: MOGP_ST_TOTAL, from the
training Gram to the last reduction) and the wall time of the Python call, medians of `reps`; the products' flop count of the call.  P = 1 is all rows
(predict_f's own arithmetic), P = 2 is {row 0}, {the rest}, P = 4 is the three rows and all rows again.  One process, one pass, its own time limit.
usage: python tools/predict_parts_time.py [N] [S] [reps] [limit_s]"""
import json, os, signal, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench
from mogptk_amd import _lib, gpr, synth

N = int(sys.argv[1]) if len(sys.argv) > 1 else 8192
S = int(sys.argv[2]) if len(sys.argv) > 2 else 2048
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 7
limit = int(sys.argv[4]) if len(sys.argv) > 4 else 400


def out_of_time(*_):
    print(json.dumps(dict(N=N, error="time limit of %d s reached" % limit)), flush=True)
    os._exit(3)


signal.signal(signal.SIGALRM, out_of_time)
signal.alarm(limit)


def sum_model():
    rng = np.random.default_rng(3)
    X = np.sort(rng.uniform(0, 500.0, (N, 1)), axis=0)
    y = np.sin(X[:, 0]) + 0.3 * np.cos(3.1 * X[:, 0]) + 0.1 * rng.standard_normal(N)
    k = gpr.AddKernel(gpr.SquaredExponentialKernel(order=0, input_dims=1), gpr.MaternKernel(nu=1.5, input_dims=1),
                      gpr.RationalQuadraticKernel(alpha=0.7, order=0, input_dims=1))
    for s, l in zip(k.kernels, (0.8, 0.5, 1.0)):
        s.lengthscale.assign(np.array([l]))
    return gpr.Exact(k, X, y, variance=0.1), np.linspace(0.0, 500.0, S)[:, None]


def measure(m, calls):
    """the calls in turn, `reps` rounds (alternating: a drift of the clocks or a neighbour's load meets all of them alike)
    -> per call (device ms median, min, max; wall ms median; flop of the call; dataflow)"""
    h = m._handle
    for call in calls:
        call(); call()
    dev, wall, meta = [[] for _ in calls], [[] for _ in calls], [None] * len(calls)
    for _ in range(reps):
        for i, call in enumerate(calls):
            t0 = time.perf_counter(); call(); wall[i].append(1e3 * (time.perf_counter() - t0))
            ms, _, flops = h.stage_ms()
            dev[i].append(ms[_lib.ST_TOTAL])
            meta[i] = (flops, h.schedule()["dataflow"])
    return [(float(np.median(d)), float(min(d)), float(max(d)), float(np.median(w))) + mt for d, w, mt in zip(dev, wall, meta)]


for name, (m, Xs) in (("mosm_c4q3", (bench.build_mosm(N, 4, 3, 0), synth.test_inputs(S, 4))), ("se+m32+rq", sum_model())):
    T = 3
    rows = np.eye(T, dtype=bool)
    masks = {1: np.ones((1, T), dtype=bool), 2: np.stack([rows[0], ~rows[0]]), 4: np.concatenate([rows, np.ones((1, T), dtype=bool)])}
    for form in ("8:200", "0"):
        os.environ["MOGP_FLOW_PREDICT"] = form
        m.predict_f(Xs)
        m._handle.set_profiling(True)
        res = measure(m, [lambda: m.predict_f(Xs)] + [(lambda P: (lambda: m.predict_terms(Xs, masks[P])))(P) for P in (1, 2, 4)])
        m._handle.set_profiling(False)
        for label, r in zip(("predict_f", "P=1", "P=2", "P=4"), res):
            print(json.dumps(dict(model=name, N=N, S=S, form=form, call=label, device_ms=round(r[0], 3), device_min=round(r[1], 3), device_max=round(r[2], 3),
                                  wall_ms=round(r[3], 3), gflop=round(r[4] / 1e9, 1), dataflow=r[5], device_over_predict_f=round(r[0] / res[0][0], 3))), flush=True)
