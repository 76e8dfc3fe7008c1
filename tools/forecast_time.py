"""The rolling-origin forecast beside what it stands next to: an LML-only evaluation, a prediction at S test points and the forecast for H
horizons on the same handle, on the benchmark model (MOSM, C = 4, Q = 3, D = 1, N = 8192; S = 2048, H = 4).  Per line: the device's span of the call
by HIP events (set_profiling: MOGP_ST_TOTAL, from the training Gram to the call's last kernel) and the wall time of the Python call, medians of `reps`
after two warm-up calls each.  One process, one pass, its own time limit.  The two kernels' own times come from a kernel trace of this script.
usage: python tools/forecast_time.py [N] [S] [H] [reps] [limit_s]"""
import json, os, signal, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench
from mogptk_amd import _lib, synth

N = int(sys.argv[1]) if len(sys.argv) > 1 else 8192
S = int(sys.argv[2]) if len(sys.argv) > 2 else 2048
H = int(sys.argv[3]) if len(sys.argv) > 3 else 4
reps = int(sys.argv[4]) if len(sys.argv) > 4 else 7
limit = int(sys.argv[5]) if len(sys.argv) > 5 else 300


def out_of_time(*_):
    print(json.dumps(dict(N=N, error="time limit of %d s reached" % limit)), flush=True)
    os._exit(3)


signal.signal(signal.SIGALRM, out_of_time)
signal.alarm(limit)

m, Xs = bench.build_mosm(N, 4, 3, 0), synth.test_inputs(S, 4)
x = np.asarray(m.X, dtype=np.float64)[:, -1]
order = np.argsort(x, kind="stable")
xs = x[order]
span = xs[-1] - xs[0]
cut = np.stack([np.searchsorted(xs, xs - f * span + 1e-9 * span, side="right") for f in np.linspace(0.002, 0.1, H)]).astype(np.int64)      # H horizons, 0.2 % .. 10 % of the range
calls = [("lml", lambda: m.log_marginal_likelihood()), ("predict_f", lambda: m.predict_f(Xs)), ("forecast", lambda: m.forecast_log_likelihood(order, cut))]
for _, call in calls:
    call(); call()
h = m._handle
h.set_profiling(True)
dev, wall, flow = {n: [] for n, _ in calls}, {n: [] for n, _ in calls}, {}
for _ in range(reps):                                       # alternating: a drift of the clocks or a neighbour's load meets all alike
    for name, call in calls:
        t0 = time.perf_counter(); call(); wall[name].append(1e3 * (time.perf_counter() - t0))
        dev[name].append(h.stage_ms()[0][_lib.ST_TOTAL])
        flow[name] = h.schedule()["dataflow"]
h.set_profiling(False)
base = float(np.median(dev["lml"]))
for name, _ in calls:
    d = dev[name]
    print(json.dumps(dict(model="mosm_c4q3", N=N, S=S, H=H, call=name, device_ms=round(float(np.median(d)), 3), device_min=round(min(d), 3), device_max=round(max(d), 3),
                          wall_ms=round(float(np.median(wall[name])), 3), dataflow=flow[name], device_over_lml=round(float(np.median(d)) / base, 3))), flush=True)
