"""The posterior of df/dx beside one prediction: predict_f against predict_df on the same handle and test points, on the benchmark model
(MOSM, C = 4, Q = 3, D = 1, N = 8192; S = 2048), in the default form of the prediction.  Per line: the device's span of the call by HIP events
(set_profiling: MOGP_ST_TOTAL, from the training Gram to the last reduction) and the wall time of the Python call, medians of `reps` after two
warm-up calls each; the products' flop count of the call.  One process, one pass, its own time limit.
usage: python tools/predict_df_time.py [N] [S] [reps] [limit_s]"""
import json, os, signal, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench
from mogptk_amd import _lib, synth

N = int(sys.argv[1]) if len(sys.argv) > 1 else 8192
S = int(sys.argv[2]) if len(sys.argv) > 2 else 2048
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 7
limit = int(sys.argv[4]) if len(sys.argv) > 4 else 300


def out_of_time(*_):
    print(json.dumps(dict(N=N, error="time limit of %d s reached" % limit)), flush=True)
    os._exit(3)


signal.signal(signal.SIGALRM, out_of_time)
signal.alarm(limit)

m, Xs = bench.build_mosm(N, 4, 3, 0), synth.test_inputs(S, 4)
calls = [("predict_f", lambda: m.predict_f(Xs)), ("predict_df", lambda: m.predict_df(Xs))]
for _, call in calls:
    call(); call()
h = m._handle
h.set_profiling(True)
dev, wall, meta = {n: [] for n, _ in calls}, {n: [] for n, _ in calls}, {}
for _ in range(reps):                                       # alternating: a drift of the clocks or a neighbour's load meets both alike
    for name, call in calls:
        t0 = time.perf_counter(); call(); wall[name].append(1e3 * (time.perf_counter() - t0))
        ms, _, flops = h.stage_ms()
        dev[name].append(ms[_lib.ST_TOTAL])
        meta[name] = (flops, h.schedule()["dataflow"])
h.set_profiling(False)
base = float(np.median(dev["predict_f"]))
for name, _ in calls:
    d = dev[name]
    print(json.dumps(dict(model="mosm_c4q3", N=N, S=S, D=1, call=name, device_ms=round(float(np.median(d)), 3), device_min=round(min(d), 3), device_max=round(max(d), 3),
                          wall_ms=round(float(np.median(wall[name])), 3), gflop=round(meta[name][0] / 1e9, 1), dataflow=meta[name][1],
                          device_over_predict_f=round(float(np.median(d)) / base, 3))), flush=True)
