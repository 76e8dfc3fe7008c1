"""
The native training step (mogp_exact_step, mogp_adam_step) on the device against the numpy form of the same host algebra: loss() and an Adam
run with gpr.config.host_fast on and off, from the same raw values.  The device work is the same call (mogp_exact_eval) either way and
the host arithmetic is the numpy form's bit for bit (exp and log1p are numpy's on both paths), so the same table goes in; what can still
separate two evaluations is the device's own run-to-run variation, if any.  Asserted: the LML to 1e-12 relative, every gradient tensor to
1e-8 of its max-abs -- a thousand times inside the suite's own 1e-9 / 1e-5 for these quantities.
N = 300: three tile rows, the last ragged; N = 1100: nine tile rows, the smallest size on the dataflow schedule.
"""
import numpy as np
import pytest

from mogptk_amd import gpr, synth
from mogptk_amd.gpr.config import config
from mogptk_amd.model import _Adam

pytestmark = pytest.mark.gpu

C, Q = 2, 2


def build(N):
    X, y = synth.make_data(N, C)
    h = synth.mosm_hypers(C, Q)
    k = gpr.MultiOutputSpectralMixtureKernel(Q=Q, output_dims=C)
    for name in ("weight", "mean", "variance", "delay", "phase"):
        getattr(k, name).assign(h[name])
    m = gpr.Exact(k, X, y, variance=h["scale"] ** 2)
    m.likelihood.scale.assign(h["scale"])
    return m


def evaluate(m, on, monkeypatch):
    monkeypatch.setattr(config, "host_fast", on)
    loss = m.loss()
    return loss, [None if p.grad is None else p.grad.copy() for p in m.parameters()]


@pytest.mark.parametrize("N", [300, 1100])
def test_loss_and_gradients_on_and_off(N, monkeypatch):
    m = build(N)
    raw = [p.data.copy() for p in m.parameters()]
    off, g_off = evaluate(m, False, monkeypatch)
    assert getattr(m._handle, "_step_plan", None) is None            # the numpy form made no plan
    for p, r in zip(m.parameters(), raw):
        assert np.array_equal(p.data, r)
    on, g_on = evaluate(m, True, monkeypatch)
    assert m._handle._step_plan is not None                          # the native step ran
    print("N", N, "loss off", float(off), "on", float(on), "rel", abs(on - off) / abs(off))
    assert type(on) is type(off) and abs(on - off) <= 1e-12 * abs(off)
    for p, a, b in zip(m.parameters(), g_on, g_off):
        assert (a is None) == (b is None)
        print(p._name, "max-abs", float(np.max(np.abs(b))), "difference", float(np.max(np.abs(a - b))))
        assert a.shape == b.shape == p.data.shape and a.dtype == b.dtype
        assert np.max(np.abs(a - b)) <= 1e-8 * np.max(np.abs(b))
    if N >= 1100:
        assert m._handle.schedule()["dataflow"]


def test_adam_trace_on_and_off(monkeypatch):
    traces = []
    for on in (False, True):
        monkeypatch.setattr(config, "host_fast", on)
        m = build(300)
        opt = _Adam(list(m.parameters()), lr=1e-3)
        trace = []
        for _ in range(20):
            trace.append(float(m.loss()))
            opt.step()
        traces.append(np.array(trace))
    print("largest relative difference of the loss trace:", float(np.max(np.abs(traces[1] - traces[0]) / np.abs(traces[0]))))
    assert np.all(np.diff(traces[0]) != 0.0)                          # the parameters moved
    assert np.all(np.abs(traces[1] - traces[0]) <= 1e-10 * np.abs(traces[0]))
