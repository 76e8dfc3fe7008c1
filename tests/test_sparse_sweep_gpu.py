"""
The sparse and variational entry points (Titsias, Snelson, the Hensman models, Opper-Archambeau) swept over input dimensions, term counts
and tile edges through the raw C ABI, against the numpy twin (oracle/table_model.py) on identical inputs (tests/sparse_sweep.py; the twin
is pinned at these D by tests/test_sparse_sweep_cpu.py).  Every figure is printed per case; the bounds are those of the raw tests of
tests/test_gpu_parity.py.  Matrices are measured against the largest entry of the twin's tensor; every moment slot and every column of gZ
is held to the same bound on its own scale as well, error / max(largest of the slot, 1e-3 largest of the tensor).

launch_moments (csrc/gram.hip) sends a dense adjoint to k_moments<DT, DENSE = true, ZG, ENV>.  A case that reaches each of the sixteen,
with M spanning at least two 64-point blocks in some channel (sizes are training points and inducing points per channel):

    DT       ZG   ENV   case
    1        on   off   test_titsias / test_snelson / test_svgp  d1_t9   193x5x187  1x130x61   (T = 9: two LDS chunks)
    2        on   off   test_titsias / test_snelson / test_svgp  d2      193x5x187  1x130x61
    3        on   off   test_titsias / test_snelson / test_svgp  d3      100x156x0  64x64x128
    generic  on   off   test_titsias / test_snelson / test_svgp  d5, d8  193x5x187  1x130x61   (rows of 17 and 26)
    1        on   on    test_titsias / test_snelson / test_svgp  d1_env  71x129x33  65         (65 points: two blocks)
    2        on   on    test_titsias / test_snelson / test_svgp  d2_env  193x5x187  1x130x61
    3        on   on    test_titsias / test_snelson / test_svgp  d3_env  100x156x0  64x64x128  (rows of 17)
    generic  on   on    test_titsias / test_snelson / test_svgp  d4_env  193x5x187  1x130x61   (rows of 22)
    1        off  off   test_oa  d1_t9  193x5x187
    2        off  off   test_oa  d2     193x5x187;   test_svgp_dense  d2  65x1x63
    3        off  off   test_oa  d3     193x5x187;   test_svgp_dense  d3  65x1x63
    generic  off  off   test_oa  d5     193x5x187;   test_svgp_dense  d5  65x1x63
    1        off  on    test_svgp_dense  d1_env  65x1x63
    2        off  on    test_svgp_dense  d2_env  65x1x63
    3        off  on    test_svgp_dense  d3_env  65x1x63
    generic  off  on    test_svgp_dense  d4_env  65x1x63

Opper-Archambeau takes no envelope: mogp_oa_forward refuses one by name, which test_oa_refuses_an_envelope_by_name asserts.

What the sweep found.  sparse_workspace (csrc/sparse.hip) cleared the padding rows of the K_uf panel and of its working copy only when Mpad
changed; Snelson and the Hensman models clear the panel themselves, Titsias writes both with one Gram kernel and relied on the padding.  One
handle that evaluated 256 inducing points and then 192 -- the same Mpad -- kept 64 rows of the earlier K_uf in v v^T: ELBO 0.9 % off, mom_uf
0.7 and gZ 55 times the largest entry of the twin's.  test_one_handle_takes_several_inducing_sets_in_turn is that case; the rows from M up to
the previous M are now cleared.  And a property of the inputs, not a fault: with 129 inducing points of one channel on [0, 10] d/dZ is the
residue of sums 3.4e5 times larger, and the device's gZ lay 4.4e-7 of the largest entry from the twin's while its moments lay 2e-14 from
them.  The twin's own fp64 sums are 3.5e-11 from np.longdouble sums of the same terms, so four times that would not have been a bound the
device meets; the distance is the accuracy of a Gram entry (1e-12) times the cancellation.  The generator's first-column V was
raised until that ratio stays below 1e5 (tests/test_sparse_sweep_cpu.py: GZ_CANCELLATION, asserted per case on the twin alone), and at
the ratio 8e4 that is left the device's gZ is 4.5e-8 from the twin's: the bound 1e-7 stands as it is.
"""
import numpy as np
import pytest

from mogptk_amd import gpr, _lib
import sparse_sweep as ss

pytestmark = pytest.mark.gpu

TOL_VALUE, TOL_JITTER, TOL_DSIGMA, TOL_PREDICT = 1e-9, 1e-14, 1e-8, 1e-8
TOL_MOMENT = {"titsias": 1e-7, "oa": 1e-7, "snelson": 1e-6, "svgp": 1e-6}
SLOT_FLOOR = 1e-3


class Report:
    """prints every figure of a case, fails at the end with all that missed their bound"""

    def __init__(self, *tag):
        self.tag, self.bad = " ".join(ss.case_id(t) for t in tag), []

    def add(self, name, e, tol):
        print("sparse sweep |", self.tag, "|", name, "|", e)
        if not e <= tol:
            self.bad.append((name, e, tol))

    def scalar(self, name, got, want, tol):
        self.add(name, abs(got - want) / abs(want), tol)

    def tensor(self, name, got, want, tol):
        """against the largest entry of the twin's tensor; a tensor that is zero in the twin is zero on the device, to the bit"""
        scale = np.max(np.abs(want))
        if scale == 0.0:
            self.add(name + " (zero)", float(np.max(np.abs(got))), 0.0)
        else:
            self.add(name, float(np.max(np.abs(np.asarray(got) - want)) / scale), tol)

    def slots(self, name, got, want, tol):
        """every slot (last axis) on its own scale"""
        scale = np.max(np.abs(want))
        if scale == 0.0:
            return
        axes = tuple(range(want.ndim - 1))
        e = np.max(np.abs(got - want), axis=axes) / np.maximum(np.max(np.abs(want), axis=axes), SLOT_FLOOR * scale)
        self.add(name + " worst slot (%d)" % int(np.argmax(e)), float(np.max(e)), tol)

    def absolute(self, name, got, want, tol):
        self.add(name, float(np.max(np.abs(np.asarray(got) - want)) / max(1.0, np.max(np.abs(want)))), tol)

    def done(self):
        assert not self.bad, (self.tag, self.bad)


def device(c):
    h = _lib.ExactHandle(gpr.config.device, c.X, c.y, c.C)
    h.set_terms(c.table)
    return h


def compare_inducing_outputs(r, got, want, tol):
    for name in ("mom_uu", "mom_uf", "gZ"):
        r.tensor(name, got[name], want[name], tol)
        r.slots(name, got[name], want[name], tol)
    r.scalar("trGA", got["trGA"], want["trGA"], tol)


def compare_titsias(r, c, got, want):
    r.scalar("elbo", got["elbo"], want["elbo"], TOL_VALUE)
    r.scalar("jitter_abs", got["jitter_abs"], want["jitter_abs"], TOL_JITTER)
    compare_inducing_outputs(r, got, want, TOL_MOMENT["titsias"])
    r.scalar("dsigma", got["dsigma"], want["dsigma"], TOL_DSIGMA)


@pytest.mark.parametrize("program,train,induce", ss.SWEEP, ids=ss.case_id)
def test_titsias(program, train, induce):
    c = ss.case(program, train, induce)
    want = ss.twin_titsias(program, train, induce)
    ref, dev = ss.twin(c), device(c)
    r = Report("titsias", program, train, induce)
    compare_titsias(r, c, dev.titsias_eval(c.Z, c.sigma, c.jitter, c.kff, grad=True), want)
    for name, Xs in ss.test_sets(program):
        kss = ss.diag(c, Xs)
        assert kss.shape == ((len(Xs),) if c.envelope else (c.C,))
        mu, var = ref.titsias_predict(c.Z, c.sigma, c.jitter, Xs, kss)
        got_mu, got_var = dev.titsias_predict(c.Z, c.sigma, c.jitter, Xs, kss)
        r.tensor(name + " mu", got_mu, mu, TOL_PREDICT)
        r.add(name + " var", float(np.max(np.abs(got_var - var))), TOL_PREDICT)
    r.absolute(name + " cov", dev.sparse_predict_cov(len(Xs)), ref.sparse_predict_cov(len(Xs)), TOL_PREDICT)
    r.done()


@pytest.mark.parametrize("program,train,induce", ss.SWEEP, ids=ss.case_id)
def test_snelson(program, train, induce):
    c = ss.case(program, train, induce)
    want = ss.twin_snelson(program, train, induce)
    ref, dev = ss.twin(c), device(c)
    r = Report("snelson", program, train, induce)
    got = dev.snelson_eval(c.Z, c.noise, c.jitter, c.kff, grad=True)
    r.scalar("lml", got["lml"], want["lml"], TOL_VALUE)
    r.scalar("jitter_abs", got["jitter_abs"], want["jitter_abs"], TOL_JITTER)
    compare_inducing_outputs(r, got, want, TOL_MOMENT["snelson"])
    assert want["hsum"].shape == ((c.N,) if c.envelope else (c.C,))
    r.tensor("hsum", got["hsum"], want["hsum"], TOL_MOMENT["snelson"])
    for name, Xs in ss.test_sets(program):
        kss = ss.diag(c, Xs)
        mu, var = ref.snelson_predict(c.Z, c.noise, c.jitter, Xs, c.kff, kss)
        got_mu, got_var = dev.snelson_predict(c.Z, c.noise, c.jitter, Xs, c.kff, kss)
        r.tensor(name + " mu", got_mu, mu, TOL_PREDICT)
        r.add(name + " var", float(np.max(np.abs(got_var - var))), TOL_PREDICT)
    r.done()


def compare_svgp(r, c, dev, want, dense):
    fwd, bwd, tests = want
    got = dev.svgp_forward(c.Zg, c.q_mu, c.q_sqrt, c.jitter, c.kff, dense=dense)
    r.scalar("jitter_abs", got["jitter_abs"], fwd["jitter_abs"], TOL_JITTER)
    r.tensor("mu", got["mu"], fwd["mu"], TOL_PREDICT)
    r.tensor("var", got["var"], fwd["var"], TOL_PREDICT)
    got = dev.svgp_backward(c.e, c.f)
    compare_inducing_outputs(r, got, bwd, TOL_MOMENT["svgp"])
    r.tensor("g_qmu", got["g_qmu"], bwd["g_qmu"], TOL_MOMENT["svgp"])
    r.tensor("g_qsqrt", np.tril(got["g_qsqrt"]), bwd["g_qsqrt"], TOL_MOMENT["svgp"])
    for (name, Xs), w in zip(ss.test_sets(c.program), tests):
        got = dev.svgp_forward(c.Zg, c.q_mu, c.q_sqrt, c.jitter, c.kff, Xs=Xs, kss_diag=ss.diag(c, Xs), dense=dense)
        r.tensor(name + " mu", got["mu"], w["mu"], TOL_PREDICT)
        r.add(name + " var", float(np.max(np.abs(got["var"] - w["var"]))), TOL_PREDICT)


@pytest.mark.parametrize("program,train,induce", ss.SWEEP, ids=ss.case_id)
def test_svgp(program, train, induce):
    """mogp_svgp_forward / _backward, sparse, with arbitrary dE/dmu and dE/dvar (the likelihood is the caller's); the forward pass at test inputs"""
    c = ss.case(program, train, induce)
    r = Report("svgp", program, train, induce)
    compare_svgp(r, c, device(c), ss.twin_svgp(program, train, induce), False)
    r.done()


@pytest.mark.parametrize("program", ss.DENSE_PROGRAMS)
def test_svgp_dense(program):
    """the dense Hensman model, Z = X grouped by channel at jitter 1e-4: the dense adjoint without input gradients (ZG off), mom_uf and gZ
    exactly zero where the twin's are"""
    c = ss.dense_case(program)
    want = ss.twin_svgp_dense(program)
    assert not np.any(want[1]["mom_uf"]) and not np.any(want[1]["gZ"])
    r = Report("svgp dense", program, c.train)
    compare_svgp(r, c, device(c), want, True)
    r.done()


@pytest.mark.parametrize("train", ss.TRAIN, ids=ss.case_id)
@pytest.mark.parametrize("program", ss.OA_PROGRAMS)
def test_oa(program, train):
    """mogp_oa_forward / _backward / _predict (diagonal and full): the dense symmetric adjoint of the training points themselves"""
    c = ss.oa_case(program, train)
    fwd, bwd, tests = ss.twin_oa(program, train)
    dev = device(c)
    r = Report("oa", program, train)
    got = dev.oa_forward(c.nu, c.lam)
    r.scalar("kl", got["kl"], fwd["kl"], TOL_VALUE)
    r.tensor("mu", got["mu"], fwd["mu"], TOL_PREDICT)
    r.tensor("var", got["var"], fwd["var"], TOL_PREDICT)
    got = dev.oa_backward(c.e, c.f)
    r.tensor("mom", got["mom"], bwd["mom"], TOL_MOMENT["oa"])
    r.slots("mom", got["mom"], bwd["mom"], TOL_MOMENT["oa"])
    r.tensor("g_nu", got["g_nu"], bwd["g_nu"], TOL_MOMENT["oa"])
    r.tensor("g_lambda", got["g_lambda"], bwd["g_lambda"], TOL_MOMENT["oa"])
    for (name, Xs), (mu, var, cov) in zip(ss.test_sets(program), tests):
        kss = ss.diag(c, Xs)
        got_mu, got_var = dev.oa_predict(c.nu, c.lam, kss, Xs)
        r.tensor(name + " mu", got_mu, mu, TOL_PREDICT)
        r.add(name + " var", float(np.max(np.abs(got_var - var))), TOL_PREDICT)
        got_mu, got_cov = dev.oa_predict(c.nu, c.lam, kss, Xs, full=True)
        r.tensor(name + " mu(full)", got_mu, mu, TOL_PREDICT)
        r.absolute(name + " cov", got_cov, cov, TOL_PREDICT)
    r.done()


def test_oa_refuses_an_envelope_by_name():
    c = ss.oa_case("d3_env", ss.DENSE_TRAIN)
    with pytest.raises(_lib.MogpError, match="does not take terms with an envelope"):
        device(c).oa_forward(c.nu, c.lam)


def test_one_handle_takes_several_inducing_sets_in_turn():
    """one handle, inducing sets of 192, 1, 256 and 192 points again: the scratch of the input-gradient pass, the panels and the adjoints are
    reused across sizes; every step against the twin, and the last bit for bit what the first gave (k_gz_reduce adds in a fixed order and
    the scratch is cleared per launch)"""
    program, train, steps = ss.HANDLE_STEPS
    dev = device(ss.case(program, train, steps[0]))
    r = Report("one handle", program, train)
    bits = []
    for step, induce in enumerate(steps):
        c = ss.case(program, train, induce)
        got = dev.titsias_eval(c.Z, c.sigma, c.jitter, c.kff, grad=True)
        rr = Report("one handle", program, train, "step %d" % (step + 1), induce)
        compare_titsias(rr, c, got, ss.twin_titsias(program, train, induce))
        r.bad += rr.bad
        bits.append([np.float64(got[k]).tobytes() for k in ("elbo", "trGA", "dsigma", "jitter_abs")] + [got[k].tobytes() for k in ("mom_uu", "mom_uf", "gZ")])
    r.done()
    assert bits[0] == bits[-1]


@pytest.mark.parametrize("program", ["d5", "d8", "d3_env"])
def test_wide_rows_in_dense_mode(program):
    """moment rows wider than 16 doubles with a dense adjoint -- the reduction that was wrong in exact mode (tests/test_kinds_sweep_gpu.py):
    the slots 16 and up of mom_uu and mom_uf on their own, which are not zero"""
    train, induce = ss.WITH[(64, 64, 128)], (64, 64, 128)
    c = ss.case(program, train, induce)
    assert c.W > 16
    want = ss.twin_titsias(program, train, induce)
    got = device(c).titsias_eval(c.Z, c.sigma, c.jitter, c.kff, grad=True)
    r = Report("wide rows", program, train, induce)
    for name in ("mom_uu", "mom_uf"):
        assert np.all(np.max(np.abs(want[name][..., 16:]), axis=(0, 1)) > 0.0)
        r.tensor(name + " 16 and up", got[name][..., 16:], want[name][..., 16:], TOL_MOMENT["titsias"])
        r.slots(name + " 16 and up", got[name][..., 16:], want[name][..., 16:], TOL_MOMENT["titsias"])
    r.done()
