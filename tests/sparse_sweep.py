"""
The generator of the sparse sweep (tests/test_sparse_sweep_cpu.py, tests/test_sparse_sweep_gpu.py): term tables that reach every
instantiation of k_moments with a dense adjoint (csrc/gram.hip: DT in {1, 2, 3, generic}, ZG on / off, ENV on / off), with training and
inducing sets of the channel sizes at which the inducing blocks (64 points, `blk_z`), the padded size (128, `Mpad`) and the place where
Titsias' beta rides (N a multiple of 128 or not) change.  Seeded numpy only; a case is a function of (program, training sizes, inducing
sizes) and is built once, and so is what the numpy twin (oracle/table_model.py) makes of it.

K_uu carries no noise, so the tables are valid covariances by construction: plain rows are a MultiOutputSpectralMixtureKernel's with
drawn weight, mean, variance, delay and phase; enveloped rows (width 2 + 5 D) a MixtureKernel's of MultiOutputHarmonizableSpectralKernel
with a shared spectrum, one lengthscale and neither delay nor phase.  The weights are set so that every diagonal amplitude is the drawn
one, whatever (2 pi)^(D / 2) sqrt(prod V) makes of it at D = 8.  Every table has three channels; sizes of fewer channels leave the others
empty.  tests/test_sparse_sweep_cpu.py asserts the conditions every case has to meet; ranges, draws and the pairing of training with
inducing sizes were set until the twin alone met them, and the device was not asked.
"""
import functools
import types
import numpy as np

from mogptk_amd import gpr
from oracle.table_model import TableDevice, gram_from_table, _jr_block, _jc_block
import kinds_sweep as ks

C = 3
JITTER = 1e-6                                               # the raw tests' value (tests/test_gpu_parity.py)
JITTER_DENSE = 1e-4
SIGMA = 0.3

PROGRAMS = {                                                # name -> (D, Q, envelope)
    "d1_t9": (1, 9, False),                                 # more terms than one LDS chunk (MOGP_TC = 8)
    "d2": (2, 3, False),
    "d3": (3, 3, False),
    "d5": (5, 2, False),                                    # the generic form, rows of 17
    "d8": (8, 2, False),                                    # rows of 26
    "d1_env": (1, 3, True),
    "d2_env": (2, 2, True),
    "d3_env": (3, 2, True),                                 # rows of 17
    "d4_env": (4, 2, True),                                 # the generic form with an envelope, rows of 22
}
TRAIN = [(100, 156, 0), (71, 129, 33), (193, 5, 187), (384,)]      # N = 256, 233, 385, 384: a multiple of 128 twice
INDUCE = [(1,), (64,), (65,), (128,), (129,), (63, 0, 66), (1, 130, 61), (64, 64, 128), (0, 65, 0)]
EVERY_SHAPE = ("d1_t9", "d3")                               # the programs every inducing shape runs with
WITH = {(1,): (384,), (64,): (100, 156, 0), (65,): (71, 129, 33), (128,): (193, 5, 187), (129,): (384,), (63, 0, 66): (71, 129, 33),
        (1, 130, 61): (193, 5, 187), (64, 64, 128): (100, 156, 0), (0, 65, 0): (100, 156, 0)}
TWO_SHAPES = [(1, 130, 61), (64, 64, 128)]                   # what every other program runs with: several blocks in a channel
# (with one input column, three channels of one spectrum and an envelope that leaves a third of the range, 130 points in a channel, or
# twice 65, put cond(K_uu) above the bound of the CPU module at every lengthscale that still leaves the u^2 moments visible: 65 do not)
OWN_SHAPES = {"d1_env": [((71, 129, 33), (65,)), ((100, 156, 0), (0, 65, 0))]}
M_ABOVE_N = ("d3", (71, 129, 33), (64, 64, 128))             # M = 256 > N = 233; channel 1 of (63, 0, 66) above has data and no inducing point
HANDLE_STEPS = ("d3", (193, 5, 187), [(1, 130, 61), (1,), (64, 64, 128), (1, 130, 61)])      # one handle, these inducing sets in turn
SWEEP = ([(p, WITH[m], m) for p in EVERY_SHAPE for m in INDUCE] + [M_ABOVE_N] + [HANDLE_STEPS[:2] + (m,) for m in HANDLE_STEPS[2][1:3]]
         + [(p,) + tm for p in PROGRAMS if p not in EVERY_SHAPE for tm in OWN_SHAPES.get(p, [(WITH[m], m) for m in TWO_SHAPES])])
TINY = ((21, 0, 13), (4, 3, 2))                              # the finite-difference size
DENSE_TRAIN = (65, 1, 63)
DENSE_PROGRAMS = ("d2", "d3", "d5", "d1_env", "d2_env", "d3_env", "d4_env")
OA_PROGRAMS = ("d2", "d3", "d5", "d1_t9")
TEST_SETS = [("1", (0, 1, 0), False), ("33x0x40", (33, 0, 40), False), ("64x65x1 shuffled", (64, 65, 1), True)]

DRAW = {"d1_env": 2, "d2_env": 4, "d3_env": 1}              # program -> which draw of its table: the first that meets the CPU module's conditions

case_id = ks.case_id


def pad(sizes):
    return tuple(sizes) + (0,) * (C - len(sizes))


def draw_kernel(rng, D, Q, envelope):
    """the project's own kernel with drawn parameters: V on the scale of the inputs (first column on [0, 10], the others on [-1, 1])"""
    wide = np.where(np.arange(D) == 0, 1.0, 0.0)            # 1 on the first input column
    # up to 130 inducing points of a channel share the first column's [0, 10]: where it is the only column (and, less so, one of two) the
    # lengthscale 1 / sqrt(V) has to come down towards their spacing, or K_uu is the jitter's and not the kernel's and d/dZ the residue of a
    # cancellation; not further, or the u^2 moments (of the order of the lengthscale squared) hide under m0.  The ranges below are where the
    # twin alone meets all three conditions of tests/test_sparse_sweep_cpu.py; Snelson's noise variance (0.7 to 1) is set by the same.
    v0 = {1: 6.0 if envelope else 10.0, 2: 6.0}.get(D, 2.0)
    v_lo, v_hi = np.where(wide > 0, v0, 0.5), np.where(wide > 0, 4.0 * v0, 3.0)
    per = np.sqrt(0.5 * (v_lo + v_hi))                       # frequencies and delays on the scale of the lengthscale
    m_lo, m_hi, delay = 0.05 * per, 0.3 * per, 0.6 / per
    target = rng.uniform(0.5, 1.5, (C, Q))                   # the diagonal amplitudes
    if not envelope:
        k = gpr.MultiOutputSpectralMixtureKernel(Q=Q, output_dims=C, input_dims=D)
        k.mean.assign(rng.uniform(m_lo, m_hi, (C, Q, D)))
        k.variance.assign(rng.uniform(v_lo, v_hi, (C, Q, D)))
        k.delay.assign(rng.normal(0.0, 1.0, (C, Q, D)) * delay)
        k.phase.assign(rng.normal(0.0, 0.3, (C, Q)))
        k.weight.assign(np.ones((C, Q)))
        A = k._spectral_terms(D)[np.arange(C), np.arange(C), :, 0]
        k.weight.assign(np.sqrt(target / A))
        return k
    k = gpr.MixtureKernel(gpr.MultiOutputHarmonizableSpectralKernel(output_dims=C, input_dims=D), Q)
    for q in range(Q):
        k[q].mean.assign(np.tile(rng.uniform(m_lo, m_hi, (1, D)), (C, 1)))
        k[q].variance.assign(np.tile(rng.uniform(v_lo, v_hi, (1, D)), (C, 1)))
        k[q].lengthscale.assign(np.full(C, rng.uniform(0.8, 1.1) if D == 1 else rng.uniform(0.6, 0.9)))
        k[q].center.assign(np.where(wide > 0, 5.0, 0.0) + rng.uniform(-1.0, 1.0, D) * np.where(wide > 0, 1.0, 0.3))
        k[q].delay.assign(np.zeros((C, D)))
        k[q].phase.assign(np.zeros(C))
        k[q].weight.assign(np.ones(C))
        A = k[q]._spectral_terms(D)[np.arange(C), np.arange(C), 0, 0]
        k[q].weight.assign(np.sqrt(target[:, q] / A))
    return k


def draw_inducing(rng, sizes, D, X, shuffle=True):
    """inducing inputs inside the range of the data (of all channels: a channel may have five training points, or none, and 130 inducing
    ones): the first column one point per stratum of the range, between a quarter and three quarters of it, which keeps them half a
    stratum apart; the others uniform"""
    lo, hi = np.min(X[:, 1:], axis=0), np.max(X[:, 1:], axis=0)
    rows = []
    for ch, m in enumerate(sizes):
        if m == 0:
            continue
        z = rng.uniform(lo, hi, (m, D))
        z[:, 0] = lo[0] + (np.arange(m) + rng.uniform(0.25, 0.75, m)) * (hi[0] - lo[0]) / m
        rows.append(np.concatenate([np.full((m, 1), float(ch)), z], axis=1))
    Z = np.concatenate(rows)
    return Z[rng.permutation(len(Z))] if shuffle else Z


def diag(c, Xk):
    """K_diag as the sparse entry points take it: per channel for plain rows, per point for enveloped ones"""
    if c.envelope:
        return c.kernel._point_diag(c.table, Xk, c.D)
    return c.kernel._spectral_diag(c.D)


def make_case(program, train, induce, grouped=False):
    """grouped: the dense Hensman model's inputs, grouped by channel, which are its inducing inputs too (`induce` None)"""
    D, Q, envelope = PROGRAMS[program]
    train = pad(train)
    seed = [list(PROGRAMS).index(program), 3 * int(grouped)] + list(train)      # (3: the first stream whose grouped cases meet the CPU module's conditions)
    rng = np.random.default_rng(seed)                         # the data: a function of the program and the training sizes alone
    c = types.SimpleNamespace(program=program, train=train, D=D, C=C, envelope=envelope, N=int(sum(train)), jitter=JITTER, sigma=SIGMA)
    c.kernel = draw_kernel(np.random.default_rng([list(PROGRAMS).index(program), DRAW.get(program, 0)]), D, Q, envelope)      # one table per program
    c.table = np.array(c.kernel._spectral_terms(D))
    c.T, c.W = c.table.shape[2], c.table.shape[3]
    c.X = ks.draw_points(rng, train, D, duplicate=not grouped, shuffle=not grouped)      # (a duplicate would be a duplicate inducing point)
    c.y = rng.standard_normal(c.N)
    c.noise = rng.uniform(0.7, 1.0, C)
    if grouped:
        c.induce, c.Z, c.jitter = train, c.X.copy(), JITTER_DENSE
    else:
        c.induce = pad(induce)
        rng = np.random.default_rng(seed + [1000] + list(c.induce))      # the inducing set and q(u): of the inducing sizes too
        c.Z = draw_inducing(rng, c.induce, D, c.X)
    c.M = len(c.Z)
    c.Zg = c.Z[np.argsort(c.Z[:, 0], kind="stable")]         # grouped by channel: what the Hensman models take (q(u) follows the order)
    c.kff = diag(c, c.X)
    c.q_mu = rng.normal(0.0, 0.5, c.M)                       # the Hensman models' q(u), as the raw tests draw it
    c.q_sqrt = np.tril(rng.normal(0.0, 0.05, (c.M, c.M))) + np.diag(rng.uniform(0.5, 1.2, c.M)) + np.triu(rng.normal(0.0, 1.0, (c.M, c.M)), 1)
    c.e, c.f = rng.standard_normal(c.N), -rng.uniform(0.5, 2.0, c.N)
    c.nu, c.lam = rng.normal(0.0, 0.5, c.N), rng.uniform(0.5, 3.0, c.N)      # Opper-Archambeau's q(f)
    return c


@functools.lru_cache(maxsize=None)
def case(program, train, induce):
    return make_case(program, train, induce)


@functools.lru_cache(maxsize=None)
def dense_case(program):
    return make_case(program, DENSE_TRAIN, None, grouped=True)


@functools.lru_cache(maxsize=None)
def oa_case(program, train):
    return make_case(program, train, (1,))                   # the inducing set is not used


def twin(c):
    h = TableDevice(0, c.X, c.y, c.C)
    h.set_terms(c.table)
    return h


def cond_kuu(table, Z, jitter):
    """cond(K_uu + jitter_abs I), jitter_abs relative to the mean diagonal as every sparse entry point has it"""
    K = gram_from_table(table, Z)
    ev = np.linalg.eigvalsh(K + jitter * np.mean(np.diagonal(K)) * np.eye(len(Z)))
    return float(ev[-1] / ev[0])


@functools.lru_cache(maxsize=None)
def test_sets(program):
    D = PROGRAMS[program][0]
    rng = np.random.default_rng([77, list(PROGRAMS).index(program)])
    return [(name, ks.draw_points(rng, sizes, D, duplicate=False, shuffle=shuffle)) for name, sizes, shuffle in TEST_SETS]


def gz_cancellation(c, h, Z, gZ):
    """[largest sum over b of |G_ab dK_ab / dz_a|, through K_uf and K_uu together] / [largest entry of gZ], from the adjoints the twin's last
    evaluation kept: by how much d/dZ is the residue of a cancellation.  Where the inducing points of a channel are dense in plenty of data
    the bound no longer depends on where they are, and the two halves of d/dZ cancel"""
    GA, GB = h._adjoints
    if not np.any(gZ):
        return 0.0
    cz, cx = Z[:, 0].astype(np.int64), c.X[:, 0].astype(np.int64)
    total = np.zeros(gZ.shape)
    for i in range(C):
        ri = np.nonzero(cz == i)[0]
        for j in range(C):
            rj, zj = np.nonzero(cx == j)[0], np.nonzero(cz == j)[0]
            if len(ri) and len(rj):
                total[ri] += np.sum(np.abs(GB[np.ix_(ri, rj)][..., None] * _jr_block(c.table[i, j], Z[ri, 1:], c.X[rj, 1:])), axis=1)
            if len(ri) and len(zj):
                J = _jr_block(c.table[i, j], Z[ri, 1:], Z[zj, 1:]) if i >= j else np.transpose(_jc_block(c.table[j, i], Z[zj, 1:], Z[ri, 1:]), (1, 0, 2))
                total[ri] += 2.0 * np.sum(np.abs(GA[np.ix_(ri, zj)][..., None] * J), axis=1)
    return float(np.max(total) / np.max(np.abs(gZ)))


# what the twin makes of a case, once for the conditions of the CPU module and for every comparison of the GPU module; treat as read-only
@functools.lru_cache(maxsize=None)
def twin_titsias(program, train, induce):
    c = case(program, train, induce)
    h = twin(c)
    res = h.titsias_eval(c.Z, c.sigma, c.jitter, c.kff, grad=True)
    res["gz_cancellation"] = gz_cancellation(c, h, c.Z, res["gZ"])
    return res


@functools.lru_cache(maxsize=None)
def twin_snelson(program, train, induce):
    c = case(program, train, induce)
    h = twin(c)
    res = h.snelson_eval(c.Z, c.noise, c.jitter, c.kff, grad=True)
    res["gz_cancellation"] = gz_cancellation(c, h, c.Z, res["gZ"])
    return res


def svgp_pair(c, dense=False):
    h = twin(c)
    fwd = h.svgp_forward(c.Zg, c.q_mu, c.q_sqrt, c.jitter, c.kff, dense=dense)
    bwd = h.svgp_backward(c.e, c.f)
    bwd["gz_cancellation"] = gz_cancellation(c, h, c.Zg, bwd["gZ"])
    tests = [h.svgp_forward(c.Zg, c.q_mu, c.q_sqrt, c.jitter, c.kff, Xs=Xs, kss_diag=diag(c, Xs), dense=dense) for _, Xs in test_sets(c.program)]
    return fwd, bwd, tests


@functools.lru_cache(maxsize=None)
def twin_svgp(program, train, induce):
    return svgp_pair(case(program, train, induce))


@functools.lru_cache(maxsize=None)
def twin_svgp_dense(program):
    return svgp_pair(dense_case(program), dense=True)


@functools.lru_cache(maxsize=None)
def twin_oa(program, train):
    """(forward, backward, [(mu, var, cov) per test set]) of the Opper-Archambeau entries"""
    c = oa_case(program, train)
    h = twin(c)
    fwd = h.oa_forward(c.nu, c.lam)
    bwd = h.oa_backward(c.e, c.f)
    tests = []
    for _, Xs in test_sets(program):
        mu, var = h.oa_predict(c.nu, c.lam, diag(c, Xs), Xs)
        tests.append((mu, var, h.oa_predict(c.nu, c.lam, diag(c, Xs), Xs, full=True)[1]))
    return fwd, bwd, tests


def parameter_mask(c, Zc, Xc, lower):
    """(pairs, W) boolean: the moment slots that bear a parameter and are not zero by construction -- pairs with points on both sides; of
    those the even slots everywhere (m0 -> A, m1_d -> V_d, m3_d -> M_d, the envelope's two), the odd ones (m4 -> Psi, m2_d -> Delta_d) on
    off-diagonal channel pairs alone.  Zc, Xc: points per channel on the row and the column side; lower: mom_uu's pair index"""
    D = c.D
    pairs = [(i, j) for i in range(C) for j in range(i + 1)] if lower else [(i, j) for i in range(C) for j in range(C)]
    mask = np.zeros((len(pairs), c.W), dtype=bool)
    odd = [1] + list(range(2 + D, 2 + 2 * D))
    for p, (i, j) in enumerate(pairs):
        if Zc[i] == 0 or Xc[j] == 0:
            continue
        mask[p] = True
        if i == j:
            mask[p, odd] = False
            if lower and Zc[i] == 1:                         # one point against itself: u = 0, and only m0 and the envelope's slots are left
                mask[p, 2:2 + 3 * D] = False
    return mask


def slot_ratios(c, res, names=("mom_uu", "mom_uf", "gZ")):
    """per tensor the smallest [largest entry of a slot] / [largest entry of the tensor] over the slots that bear a parameter"""
    out = {}
    for name in names:
        a = np.abs(res[name])
        if name == "gZ":
            out[name] = float(np.min(np.max(a, axis=0)) / np.max(a))
            continue
        if not np.any(a):
            continue
        if name == "mom":                                    # Opper-Archambeau: the training points against themselves
            mask = parameter_mask(c, c.train, c.train, True)
        else:
            mask = parameter_mask(c, c.induce, c.induce if name == "mom_uu" else c.train, name == "mom_uu")
        per_slot = np.max(np.where(mask[:, None, :], a, 0.0), axis=(0, 1))
        out[name] = float(np.min(per_slot[np.any(mask, axis=0)]) / np.max(a))
    return out
