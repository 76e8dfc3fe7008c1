"""
The native host side of a plain MOSM training step (csrc/hoststep.hip: mogp_mosm_step_forward, mogp_mosm_step_backward, mogp_adam_step) against
the numpy form it stands in for, without a GPU: the device between forward and backward is the numpy twin.

Bounds.  The backward and Adam are element-wise arithmetic in the numpy form's operation order (+, -, *, /, sqrt: correctly rounded on both
sides), so from identical inputs they must agree bit for bit.  The forward needs exp and log1p, where libm and numpy's own vector loops round
differently (2 ulp in the values, 4 in the derivatives, measured on two hosts: profiles/host_fast_step.txt) -- enough to break the suite's
bitwise comparisons between models on the two paths -- so the plan takes them from numpy and hands them to the native code.  The distance
between the two forms is then 0 (measured on a grid of 160 001 raw values in [-400, 400] for every transform), four times that is 0, and
every comparison below is bit for bit.
"""
import copy

import numpy as np
import pytest

from mogptk_amd import _lib, gpr, synth
from mogptk_amd.gpr.config import config
from mogptk_amd.gpr.parameter import Parameter, Softplus, Sigmoid
from mogptk_amd.model import _Adam

import loo_twin

SHAPES = [(1, 1, 1), (2, 2, 1), (4, 3, 1), (3, 2, 2)]
N = 40


class StepDevice(loo_twin.LooTableDevice):
    """the numpy twin with the native step's entry: host algebra in native code, the evaluation between its halves by the twin; counts calls"""

    def __init__(self, *a):
        super().__init__(*a)
        self.steps, self.evals, self.last = 0, 0, None

    def eval(self, *a, **k):
        self.evals += 1
        self.last = super().eval(*a, **k)
        return self.last

    def loo(self, *a, **k):
        self.evals += 1
        return super().loo(*a, **k)

    def step(self, plan, jitter, data_var=None):
        self.steps += 1
        plan.forward()
        self.set_terms(plan.table.copy())
        res = loo_twin.LooTableDevice.eval(self, plan.noise_var.copy(), jitter, grad=True, data_var=data_var)
        plan.moments[...], plan.diagG[...] = res["moments"], res["diagG"]
        plan.out[:] = (res["lml"], res["trG"], res["jitter_abs"], 0.0, 0.0)
        plan.backward(res["trG"], jitter)


@pytest.fixture
def device(monkeypatch):
    monkeypatch.setattr(_lib, "ExactHandle", StepDevice)
    monkeypatch.setattr(config, "host_fast", True)
    return StepDevice


def build(C, Q, D, per_channel=True, sigmoid=True, **kw):
    """a MOSM model at N = 40 with: weights raw beyond the softplus threshold in places, the mean between two bounds (sigmoid), the variance not trained"""
    X, y = synth.make_data(N, C, D)
    h = synth.mosm_hypers(C, Q, D)
    k = gpr.MultiOutputSpectralMixtureKernel(Q=Q, output_dims=C, input_dims=D)
    k.weight.assign(h["weight"])
    k.weight.data = k.weight.data + np.where(np.arange(C * Q).reshape(C, Q) % 2 == 0, 250.0, 0.0)       # beta x = 25 > threshold = 20: the linear branch
    k.mean.assign(h["mean"], lower=0.01, upper=0.5 if sigmoid else None)
    k.variance.assign(h["variance"], train=False)
    k.delay.assign(h["delay"])
    k.phase.assign(h["phase"])
    m = gpr.Exact(k, X, y, variance=(h["scale"] ** 2 if per_channel else 0.04), **kw)
    return m


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def generic_forward(m):
    params = m.kernel._step_blocks()[0] + (m.likelihood.scale,)
    cons = [np.asarray(p(), dtype=np.float64) for p in params]
    dcons = [np.asarray(p.dconstrained(), dtype=np.float64) for p in params]
    return params, cons, dcons, m.kernel._spectral_terms(m._D), m._noise_var()


def test_transforms_are_bit_identical_on_a_grid():
    """the native forward against gpr/parameter.py on 160 001 raw values in [-400, 400], both branches of every transform"""
    x = np.linspace(-400.0, 400.0, 160001)
    n = x.size
    for tr in (Softplus(lower=1e-8), Softplus(lower=3.0, beta=-0.1), Sigmoid(lower=0.01, upper=0.5)):
        kind = 1 if isinstance(tr, Softplus) else 2
        plan = _lib.StepPlan(1, n, 1, 1, [(kind, tr.lower, getattr(tr, "upper", None), getattr(tr, "beta", None), getattr(tr, "threshold", None))] * 6,
                             1.0, 1.0, np.ones(1), n, [1] * 6)             # one channel, n mixtures: the weight block is the grid
        plan.raw[:n] = x
        plan.raw[n:] = 0.0
        plan.transcendentals()
        plan.forward()
        with np.errstate(over="ignore"):
            assert same_bits(plan.cons[:n], tr.forward(x)) and same_bits(plan.dcons[:n], tr.dforward(x)), vars(tr)


@pytest.mark.parametrize("C,Q,D", SHAPES)
@pytest.mark.parametrize("per_channel", [True, False])
def test_forward_matches_the_generic_path(device, C, Q, D, per_channel):
    m = build(C, Q, D, per_channel)
    params, cons, dcons, table, noise = generic_forward(m)
    plan = m._step_plan("lml")
    assert plan is not None and plan.nscale == (C if per_channel else 1)
    plan.gather([p.data for p in params])
    plan.forward()
    for i, p in enumerate(params):
        assert same_bits(plan.block(plan.cons, i, p.data.shape), cons[i]) and same_bits(plan.block(plan.dcons, i, p.data.shape), dcons[i]), p._name
    big = m.kernel.weight.data * 0.1 > 20.0
    assert np.any(big) and same_bits(plan.block(plan.cons, 0, (C, Q))[big], (1e-8 + m.kernel.weight.data)[big])       # the linear branch: lower + x
    assert same_bits(plan.table, table) and same_bits(plan.noise_var, noise)


@pytest.mark.parametrize("C,Q,D", SHAPES)
def test_table_is_bit_identical_from_identical_constrained_values(device, C, Q, D):
    """every softplus block beyond its threshold (constrained = lower + raw exactly on both sides), the others untransformed: the constrained
    values cannot differ, so neither may the table or the noise"""
    m = build(C, Q, D, sigmoid=False)
    k = m.kernel
    for p in (k.weight, k.mean, k.variance, m.likelihood.scale):
        assert type(p.transform) is Softplus
        p.data = 201.0 + np.arange(p.data.size, dtype=np.float64).reshape(p.data.shape) / 7.0
    k.mean.data = k.mean.data / 1e3 + 200.5
    params, cons, dcons, table, noise = generic_forward(m)
    plan = m._step_plan("lml")
    plan.gather([p.data for p in params])
    plan.forward()
    for i, p in enumerate(params):
        assert same_bits(plan.block(plan.cons, i, p.data.shape), cons[i]) and same_bits(plan.block(plan.dcons, i, p.data.shape), dcons[i])
    assert same_bits(plan.table, table) and same_bits(plan.noise_var, noise)


@pytest.mark.parametrize("C,Q,D", SHAPES)
@pytest.mark.parametrize("per_channel", [True, False])
def test_backward_is_bit_identical_from_identical_constrained_inputs(device, monkeypatch, C, Q, D, per_channel):
    m = build(C, Q, D, per_channel)
    monkeypatch.setattr(config, "host_fast", False)
    m.loss()
    h = m._handle
    assert h.steps == 0 and h.evals == 1
    want = [None if p.grad is None else p.grad.copy() for p in m.parameters()]
    params, cons, dcons, table, noise = generic_forward(m)
    monkeypatch.setattr(config, "host_fast", True)
    plan = m._step_plan("lml")
    for i in range(6):
        plan.cons[plan.starts[i]:plan.ends[i]] = cons[i].reshape(-1)
        plan.dcons[plan.starts[i]:plan.ends[i]] = dcons[i].reshape(-1)
    plan.table[...], plan.moments[...], plan.diagG[...] = table, h.last["moments"], h.last["diagG"]
    plan.graw[:] = np.nan
    plan.backward(h.last["trG"], m.jitter)
    assert [p is q for p, q in zip(m.parameters(), params)] == [True] * 6
    for i, (p, g) in enumerate(zip(params, want)):
        assert (g is None) == (not plan.trained[i]), p._name
        got = plan.block(plan.graw, i, p.data.shape)
        if g is None:
            assert np.all(np.isnan(got))                  # left unset
        else:
            assert g.dtype == np.float64 and same_bits(got, g), (p._name, got, g)
    assert (want[3] is None) == (C == 1) and (want[4] is None) == (C == 1)


@pytest.mark.parametrize("C,Q,D", SHAPES)
def test_loss_on_and_off_agree(device, monkeypatch, C, Q, D):
    m = build(C, Q, D)
    monkeypatch.setattr(config, "host_fast", False)
    off = m.loss()
    want = [None if p.grad is None else p.grad.copy() for p in m.parameters()]
    monkeypatch.setattr(config, "host_fast", True)
    on = m.loss()
    assert m._handle.steps == 1 and m._handle.evals == 1
    assert type(on) is type(off) and on == off
    for p, g in zip(m.parameters(), want):
        assert (p.grad is None) == (g is None)
        if g is not None:
            assert p.grad.shape == p.data.shape and p.grad.dtype == p.data.dtype and same_bits(p.grad, g)
    first = [p.grad for p in m.parameters()]
    m.loss()
    assert all(a is not b for a, b in zip(first, (p.grad for p in m.parameters())) if a is not None)        # fresh arrays every step


def test_plan_follows_the_structure(device):
    m = build(2, 2, 1)
    m.loss()
    plan = m._handle._step_plan
    m.loss()
    assert m._handle._step_plan is plan
    m.kernel.weight.assign(lower=1e-3)                    # a new bound: a new transform, a new plan
    m.loss()
    assert m._handle._step_plan is not plan and m._handle.steps == 3
    assert float(m._handle._step_plan.lower[0]) == 1e-3
    twin = copy.deepcopy(m)                                 # the plan stays with the handle, which a copy does not share
    assert twin._handle is None or twin._handle is not m._handle
    import pickle
    pickle.loads(pickle.dumps(m)).kernel.weight()


@pytest.mark.parametrize("what", ["pegged", "prior", "dtype"])
def test_a_plan_that_no_longer_fits_is_left(device, what):
    """a model that took the native step and THEN stops being eligible: the kept plan is checked again on every call"""
    m = build(2, 2, 1)
    m.loss()
    h = m._handle
    assert (h.steps, h.evals) == (1, 0)
    if what == "pegged":
        _pegged(m)
    elif what == "prior":
        _prior(m)
    else:
        m.kernel.mean.data = m.kernel.mean.data.astype(np.float32)
    if what == "prior":
        with pytest.raises(NotImplementedError):
            m.loss()
    else:
        m.loss()
    assert m._handle is h and (h.steps, h.evals) == (1, 1)
    if what == "dtype":
        m.kernel.mean.data = m.kernel.mean.data.astype(np.float64)
        m.loss()
        assert (h.steps, h.evals) == (2, 1)                  # eligible again: the native step again


@pytest.mark.parametrize("C", [7, 8, 9, 20, 128, 129, 130, 300])
def test_shared_scale_gradient_sums_as_numpy(C):
    """the shared noise scale's gradient is -2 sigma np.sum(gvar) dsigma: the native sum follows np.add.reduce's association (in order below 8
    elements, eight partial sums per block up to 128, blocks pairwise beyond), every branch of which this walks"""
    rng = np.random.default_rng(C)
    plan = _lib.StepPlan(C, 1, 1, 1, [(0, None, None, None, None)] * 6, 1.0, 1.0, rng.integers(1, 9, C).astype(np.float64), 40, [1] * 6)
    plan.cons[:] = rng.uniform(0.5, 1.5, plan.cons.size)
    plan.dcons[:] = rng.uniform(0.5, 1.5, plan.cons.size)
    plan.table[...] = rng.uniform(0.5, 1.5, plan.table.shape)
    plan.moments[...] = rng.standard_normal(plan.moments.shape)
    plan.diagG[:] = rng.standard_normal(C) * 10.0 ** rng.integers(-3, 3, C)
    trG, jitter = 0.37, 1e-3
    plan.backward(trG, jitter)
    gvar = plan.diagG + (jitter * trG / 40) * plan.counts
    want = -(2.0 * plan.cons[-1] * np.sum(gvar)) * plan.dcons[-1]
    assert same_bits(plan.graw[-1], want)


def _adam_params(rng):
    ps = [Parameter(rng.standard_normal(s)) for s in ((3, 2), (3, 2, 1), (4,), ())]
    for p in ps:
        p.data = rng.standard_normal(p.data.shape)
    return ps


@pytest.mark.parametrize("amsgrad", [False, True])
@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_adam_native_is_bit_identical(monkeypatch, amsgrad, wd):
    rng = np.random.default_rng(5)
    a = _adam_params(rng)
    b = [copy.deepcopy(p) for p in a]
    oa, ob = _Adam(a, lr=1e-2, weight_decay=wd, amsgrad=amsgrad), _Adam(b, lr=1e-2, weight_decay=wd, amsgrad=amsgrad)
    for step in range(50):
        for i, (p, q) in enumerate(zip(a, b)):
            g = rng.standard_normal(p.data.shape) * 10.0 ** rng.integers(-6, 3)
            p.grad = q.grad = None
            if i != 2 or step >= 10:                       # the third tensor gains its gradient at step 10
                p.grad, q.grad = g.copy(), g.copy()
        monkeypatch.setattr(config, "host_fast", True)
        oa.step()
        monkeypatch.setattr(config, "host_fast", False)
        ob.step()
        for p, q in zip(a, b):
            assert p.data.shape == q.data.shape and same_bits(p.data, q.data), step
    oa._unflatten(); ob._unflatten()
    for p, q in zip(a, b):
        for key in ("m", "v", "vmax"):
            assert same_bits(oa.state[id(p)][key], ob.state[id(q)][key])
        assert oa.state[id(p)]["t"] == ob.state[id(q)]["t"]


def _pegged(m):
    m.kernel.phase.peg(m.kernel.delay, lambda v: v[..., 0])


def _prior(m):
    m.kernel.weight.prior = object()


@pytest.mark.parametrize("what", ["pegged", "prior", "mean", "mosk", "float32", "loo", "switch"])
def test_everything_else_takes_the_generic_path(device, monkeypatch, what):
    C, Q = 2, 2
    kw, call, raises = {}, "loss", None
    if what == "float32":
        monkeypatch.setattr(config, "dtype", np.float32)
    if what == "mean":
        kw["mean"] = gpr.ConstantMean()
    m = build(C, Q, 1, **kw)
    if what == "mosk":
        X, y = synth.make_data(N, C)
        m = gpr.Exact(gpr.MixtureKernel(gpr.MultiOutputSpectralKernel(output_dims=C), Q), X, y, variance=[0.04] * C)
    if what == "pegged":
        _pegged(m)
    if what == "prior":
        _prior(m)
        raises = NotImplementedError                      # priors are not on this path at all: log_prior says so, behind the evaluation
    if what == "loo":
        call = "loo_loss"
    if what == "switch":
        monkeypatch.setattr(config, "host_fast", False)
    if raises:
        with pytest.raises(raises):
            getattr(m, call)()
    else:
        getattr(m, call)()
    h = m._handle
    assert isinstance(h, StepDevice) and h.steps == 0 and h.evals == 1


def test_the_plain_model_takes_the_native_path(device):
    m = build(2, 2, 1)
    m.loss()
    assert m._handle.steps == 1 and m._handle.evals == 0


def test_a_bad_plan_says_which_call_failed():
    plan = _lib.StepPlan(1, 1, 1, 1, [(0, None, None, None, None)] * 6, 1.0, 1.0, np.ones(1), 40, [1] * 6)
    plan.tkind[0] = 7                                       # no such transform
    with pytest.raises(_lib.MogpError, match="mogp_mosm_step_forward"):
        plan.forward()
