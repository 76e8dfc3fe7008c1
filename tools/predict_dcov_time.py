"""The joint covariance of df/dx beside a prediction with its full covariance: predict_df_cov against predict_f(full=True) at the same
number of stacked test rows, on one handle each for the benchmark model (MOSM, C = 4, Q = 3, D = 1, N = 8192; S = 2048) and for SE + RQ + Matern 3/2
at D = 1 (S = 2048) and SE + RQ with one lengthscale per dimension at D = 2 (S = 1024 points: 2048 stacked rows, predict_f at S = 2048; the Matern
kernels are D = 1 on this path).  The two calls do the
same N^3/3 + N^2 rows + rows^2 N flops and differ by one Gram-type kernel, so predict_f is the yardstick and the ratio is what is recorded.  Per line:
the device's span of the call by HIP events (set_profiling: MOGP_ST_TOTAL) and the wall time of the Python call, medians of `reps` alternating calls
after two warm-up calls each.  The duration of k_gram_dxdx itself is a kernel trace's to give (one more run of this tool under the profiler).
One process, one pass, its own time limit.
usage: python tools/predict_dcov_time.py [N] [rows] [reps] [limit_s]"""
import json, os, signal, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench
from mogptk_amd import _lib, gpr, synth

N = int(sys.argv[1]) if len(sys.argv) > 1 else 8192
rows = int(sys.argv[2]) if len(sys.argv) > 2 else 2048
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
limit = int(sys.argv[4]) if len(sys.argv) > 4 else 400


def out_of_time(*_):
    print(json.dumps(dict(N=N, error="time limit of %d s reached" % limit)), flush=True)
    os._exit(3)


signal.signal(signal.SIGALRM, out_of_time)
signal.alarm(limit)


def stationary(D):
    rng = np.random.default_rng(5)
    X = rng.uniform(0.0, 100.0 if D == 1 else 10.0, (N, D))
    y = np.sin(0.3 * X[:, 0]) + 0.3 * np.cos(X[:, -1]) + 0.1 * rng.standard_normal(N)
    ks = [gpr.SquaredExponentialKernel(order=0, input_dims=D), gpr.RationalQuadraticKernel(alpha=0.7, order=0, input_dims=D)]
    if D == 1:                                              # (the Matern kernels are D = 1 on this path)
        ks.append(gpr.MaternKernel(nu=1.5, input_dims=D))
    for k, ls in zip(ks, (3.0, 6.0, 1.5)):
        k.lengthscale.assign(np.full(tuple(k.lengthscale().shape), ls) * (1.0 + 0.2 * np.arange(k.lengthscale().size).reshape(tuple(k.lengthscale().shape))))
    lo, hi = X.min(axis=0), X.max(axis=0)
    return gpr.Exact(gpr.AddKernel(*ks), X, y, variance=0.1), lambda S: lo + (hi - lo) * np.random.default_rng(6).uniform(0.02, 0.98, (S, D))


def measure(name, m, D, Xf, Xd):
    calls = [("predict_f_full", lambda: m.predict_f(Xf, full=True)), ("predict_df_cov", lambda: m.predict_df_cov(Xd))]
    for _, call in calls:
        call(); call()
    h = m._handle
    h.set_profiling(True)
    dev, wall, flow = {n: [] for n, _ in calls}, {n: [] for n, _ in calls}, {}
    for _ in range(reps):                                   # alternating: a drift of the clocks or a neighbour's load meets both alike
        for n, call in calls:
            t0 = time.perf_counter(); call(); wall[n].append(1e3 * (time.perf_counter() - t0))
            dev[n].append(h.stage_ms()[0][_lib.ST_TOTAL])
            flow[n] = h.schedule()["dataflow"]
    h.set_profiling(False)
    base = float(np.median(dev["predict_f_full"]))
    for n, _ in calls:
        d = dev[n]
        print(json.dumps(dict(model=name, N=N, D=D, S=len(Xd) if n == "predict_df_cov" else len(Xf), rows=rows, call=n, device_ms=round(float(np.median(d)), 3),
                              device_min=round(min(d), 3), device_max=round(max(d), 3), wall_ms=round(float(np.median(wall[n])), 3), dataflow=flow[n],
                              device_over_predict_f=round(float(np.median(d)) / base, 3))), flush=True)


Xs = synth.test_inputs(rows, 4)
measure("mosm_c4q3", bench.build_mosm(N, 4, 3, 0), 1, Xs, Xs)
for D in (1, 2):
    m, draw = stationary(D)
    measure("se_rq_m32" if D == 1 else "se_rq_ard", m, D, draw(rows), draw(rows // D))
