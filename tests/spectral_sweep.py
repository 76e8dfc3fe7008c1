"""
The generator of the spectral sweep (tests/test_spectral_sweep_cpu.py, tests/test_spectral_sweep_gpu.py): cases for the three software pipelines
of the headline path -- k_gram_strip2 (runs of up to 8 tiles), the persistent k_gram<1> and k_moments_x<3|4> (csrc/gram.hip) -- at the smallest
sizes at which a second tile follows a first once the launches are planned on one or three CUs (mogp_ctx_plan_cus), and for the per-tile
mode choice (Taylor degree 4 .. 12 / 14, GT_SKIP, GT_GENERAL).  Seeded numpy only; a case is a function of (group, name, T), built once.

The tables come from the project's own kernels (MultiOutputSpectralMixtureKernel; MOHSM for the enveloped rows of the stateless Gram), so
Kj is positive definite without tuning.  One input column; a channel's points sit near the integers 0, 1, 2, ... (a full tile spans 63, so
zmax = |V| hr hc of a full tile is |V| * 31.5^2 within a few percent), and the cases choose V from the zmax they want.
"""
import functools
import types
import numpy as np

from mogptk_amd import gpr, _lib

GT = 64
HH = 31.5 * 31.5                                            # hr * hc of two full tiles of unit-spaced points
JITTER = 1e-8
LAMBDA_MIN = 0.1
SKIP, GENERAL = -1, 0
DEGREE_EDGES = [(1.19e-3, 4), (4.93e-3, 5), (0.0139, 6), (0.0308, 7), (0.0578, 8), (0.0968, 9), (0.149, 10), (0.2147, 11), (0.294, 12)]
DEGREES = (4, 5, 6, 7, 8, 9, 10, 11, 12, 14)

RUN_SIZES = [(640,), (704,), (128, 256, 192), (129, 256), (65, 640), (66, 576)]
RUNS = [(s, T) for s in RUN_SIZES for T in (3, 4)] + [((640,), T) for T in (1, 2, 5, 8, 9)]
# zmax of the four terms, three cases: every degree and GT_GENERAL between them
BAND_Z = {"bands_a": (6e-4, 9e-3, 0.044, 0.12), "bands_b": (3e-3, 0.022, 0.077, 0.18), "bands_c": (0.25, 0.37, 0.6, 1.0)}
BANDS = list(BAND_Z) + ["skip", "zero_amp", "shuffled", "gap", "equal"]
CHUNKS = [((2048,), 3), ((2048,), 4), ((40,) * 32, 3)]
FAR = ((300,), 2)
# the dataflow schedule's two Gram launches: the kinds sweep's sizes, where channels 1 and 2 start at odd offsets (no strip tile beyond column 512),
# and the same N with even offsets, where the tail launch holds runs too
DATAFLOW_SIZES = [(367, 400, 333), (368, 400, 332)]
PLAN_SIZES = RUN_SIZES + [s for s, _ in CHUNKS] + [FAR[0]] + DATAFLOW_SIZES


def case_id(v):
    if isinstance(v, tuple):
        return "%dx%d" % (len(v), v[0]) if len(v) > 4 and len(set(v)) == 1 else "x".join(str(s) for s in v)
    return str(v)


def draw_kernel(rng, C, Q, z=None, freq=(0.004, 0.05), delay=2.0):
    """MOSM with drawn parameters; z: (Q,) the zmax the terms' V aim at (None: drawn log-uniformly over the polynomial bands)"""
    k = gpr.MultiOutputSpectralMixtureKernel(Q=Q, output_dims=C, input_dims=1)
    zq = np.exp(rng.uniform(np.log(0.004), np.log(0.25), (C, Q))) if z is None else np.tile(np.asarray(z, dtype=float), (C, 1))
    k.variance.assign((zq / HH)[..., None])
    k.mean.assign(rng.uniform(freq[0], freq[1], (C, Q, 1)))
    k.delay.assign(rng.normal(0.0, delay, (C, Q, 1)) if C > 1 else np.zeros((C, Q, 1)))
    k.phase.assign(rng.normal(0.0, 0.3, (C, Q)) if C > 1 else np.zeros((C, Q)))
    k.weight.assign(np.ones((C, Q)))
    A = k._spectral_terms(1)[np.arange(C), np.arange(C), :, 0]
    k.weight.assign(np.sqrt(rng.uniform(0.5, 1.5, (C, Q)) * (2.0 / (1 + Q)) / A))
    return k


def draw_inputs(rng, sizes, first=None):
    """X (N, 2): channel c's points in ascending order near 0, 1, 2, ... (or `first[c]`, as given), the channels interleaved in caller order --
    the stable sort by channel keeps each channel's order"""
    chan = np.repeat(np.arange(len(sizes)), sizes)
    chan = chan[rng.permutation(len(chan))]
    X = np.zeros((len(chan), 2))
    X[:, 0] = chan
    for c, n in enumerate(sizes):
        X[chan == c, 1] = (np.arange(n) + 0.3 * rng.uniform(0.0, 1.0, n)) if first is None else first[c]
    return X


def finish(c, rng, kernel):
    c.table = np.array(kernel._spectral_terms(1))
    c.C, c.N, c.D, c.T, c.jitter = len(c.sizes), int(sum(c.sizes)), 1, c.table.shape[2], JITTER
    c.y = rng.standard_normal(c.N)
    c.noise = rng.uniform(0.2, 0.4, c.C)
    c.dvar = rng.uniform(0.0, 0.1, c.N)
    return c


@functools.lru_cache(maxsize=None)
def runs_case(sizes, T):
    rng = np.random.default_rng([1, T] + list(sizes))
    c = types.SimpleNamespace(group="runs", name=case_id(sizes), sizes=sizes)
    c.X = draw_inputs(rng, sizes)
    return finish(c, rng, draw_kernel(rng, len(sizes), T))


@functools.lru_cache(maxsize=None)
def bands_case(name):
    sizes = (640,)
    rng = np.random.default_rng([2, BANDS.index(name)])
    c = types.SimpleNamespace(group="bands", name=name, sizes=sizes)
    x = np.arange(640) + 0.3 * rng.uniform(0.0, 1.0, 640)
    z = BAND_Z.get(name, BAND_Z["bands_a" if name in ("zero_amp", "gap") else "bands_b"])
    if name == "skip":
        # three groups of 4, 4 and 2 tiles, 400 and 2000 apart: V gap^2 = 16, 160, 1600, 48 between the first two (terms 1 and 2 are skipped in
        # those tiles, the others are not) and 400 at the least towards the third (every term is)
        z = tuple(v * HH for v in (1e-4, 1e-3, 1e-2, 3e-4))
        x = x + 400.0 * (np.arange(640) >= 256) + 2000.0 * (np.arange(640) >= 512)
    if name == "gap":
        x = x + 1e3 * (np.arange(640) >= 100)                # one gap of 1e3 inside the second tile
    if name == "equal":
        x[128:192] = x[128]                                  # every input of the third tile the same: hr = hc = 0 on its diagonal tile
    if name == "shuffled":
        x = x[rng.permutation(640)]                          # one channel in caller order: every tile spans the whole range
    c.X = draw_inputs(rng, sizes, first=[x])
    finish(c, rng, draw_kernel(rng, 1, 4, z=z))
    if name == "zero_amp":
        c.table[:, :, 1, 0] = 0.0
    return c


@functools.lru_cache(maxsize=None)
def chunks_case(sizes, T):
    rng = np.random.default_rng([3, T, len(sizes), sizes[0]])
    c = types.SimpleNamespace(group="chunks", name=case_id(sizes), sizes=sizes)
    c.X = draw_inputs(rng, sizes)
    return finish(c, rng, draw_kernel(rng, len(sizes), T))


@functools.lru_cache(maxsize=None)
def far_case():
    """year-valued inputs: 300 points on [2000, 2003], frequencies up to 12 a year"""
    sizes, T = FAR
    rng = np.random.default_rng([4])
    c = types.SimpleNamespace(group="far", name="far", sizes=sizes)
    x = 2000.0 + (np.arange(300) + 0.3 * rng.uniform(0.0, 1.0, 300)) / 100.0
    c.X = draw_inputs(rng, sizes, first=[x])
    k = draw_kernel(rng, 1, T, z=(0.05 * 1e4, 0.2 * 1e4), freq=(6.0, 12.0))      # (the spacing is 1 / 100: V on that scale)
    k.mean.assign(np.array([[[12.0], [7.3]]]))
    return finish(c, rng, k)


@functools.lru_cache(maxsize=None)
def dataflow_case(sizes):
    T = 3
    rng = np.random.default_rng([5] + list(sizes))
    c = types.SimpleNamespace(group="dataflow", name=case_id(sizes), sizes=sizes)
    c.X = draw_inputs(rng, sizes)
    return finish(c, rng, draw_kernel(rng, len(sizes), T))


SPARSE = ((640,), (192,), 3)                                 # training sizes, inducing sizes, T: ten full column tiles against three full row blocks


@functools.lru_cache(maxsize=None)
def sparse_case():
    """a Titsias case from the sparse sweep's own generator (its MOSM kernel for one input column, its inducing inputs) with rows of width 5 and
    T = 3, which the strip kernel takes: 640 training and 192 inducing points of channel 0, the first column stretched to [0, 30] so that
    192 inducing points keep the spacing the sparse sweep's 64 have on [0, 10]"""
    import kinds_sweep as ks
    import sparse_sweep as ss
    train, induce, T = SPARSE
    rng = np.random.default_rng([6])
    c = types.SimpleNamespace(group="sparse", name="titsias", D=1, C=ss.C, envelope=False, sigma=ss.SIGMA, jitter=ss.JITTER,
                              train=ss.pad(train), induce=ss.pad(induce))
    c.kernel = ss.draw_kernel(rng, 1, T, False)
    c.table = np.array(c.kernel._spectral_terms(1))
    c.X = ks.draw_points(rng, c.train, 1)
    c.X[:, 1] *= 3.0
    c.N, c.T = len(c.X), T
    c.y = rng.standard_normal(c.N)
    c.Z = ss.draw_inducing(rng, c.induce, 1, c.X)
    c.kff = ss.diag(c, c.X)
    return c


def gram_cases():
    """every case whose Kj goes against the reference: (id, thunk)"""
    out = [("runs-%s-T%d" % (case_id(s), T), functools.partial(runs_case, s, T)) for s, T in RUNS]
    out += [("bands-%s" % n, functools.partial(bands_case, n)) for n in BANDS]
    out.append(("far", far_case))
    return out


def all_cases():
    return gram_cases() + [("chunks-%s-T%d" % (case_id(s), T), functools.partial(chunks_case, s, T)) for s, T in CHUNKS] + [("dataflow-%s" % case_id(s), functools.partial(dataflow_case, s)) for s in DATAFLOW_SIZES]


# ---- accounting: the per-tile mode choice of the strip kernel's `scalars` (csrc/gram.hip), restated ------------------------------------------
def degree(zmax):
    for edge, deg in DEGREE_EDGES:
        if zmax <= edge:
            return deg
    return 14


def tile_modes(c):
    """[(r0, c0, pair, [mode per term])] of every full tile at an even column offset (the strip kernel's tiles: the runs of mogp_strip_plan,
    expanded); modes are SKIP, GENERAL or the Taylor degree"""
    order = np.argsort(c.X[:, 0], kind="stable")
    xs = c.X[order, 1]
    off = np.concatenate([[0], np.cumsum(c.sizes)])

    def block(p0):                                          # centre and half span of the 64-point block that starts at p0
        ch = int(np.searchsorted(off, p0, side="right") - 1)
        v = xs[p0:min(p0 + GT, off[ch + 1])]
        return 0.5 * (v.min() + v.max()), 0.5 * (v.max() - v.min())

    out = []
    for row in _lib.strip_plan(c.sizes, 1):
        if row[0] != 1:
            continue
        r0, c0, n, pair = (int(v) for v in row[1:5])
        tab = c.table[pair // c.C, pair % c.C]
        cr, hr = block(r0)
        for u in range(n):
            cc, hc = block(c0 + u * GT)
            modes = []
            for A, _, V, _, dl in tab[:, :5]:
                s = (cr - cc) + dl
                zmax, es = abs(V) * hr * hc, V * s * s
                mu = max(0.0, abs(s) - hr - hc)
                emin, efac = V * mu * mu, abs(V) * (hr * hr + hc * hc + 2.0 * (hr + hc) * abs(s))
                if A == 0.0 or 0.5 * emin > 50.0:
                    modes.append(SKIP)
                elif not zmax <= 0.45 or not 0.5 * es < 600.0 or not 0.5 * efac < 600.0:
                    modes.append(GENERAL)
                else:
                    modes.append(degree(zmax))
            out.append((r0, c0 + u * GT, pair, modes))
    return out
