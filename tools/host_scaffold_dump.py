"""What the six gpr models hand back -- loss(), every parameter's .grad, log_marginal_likelihood(), predict_f() -- written to one .npz, to compare two
versions of mogptk_amd/gpr/model.py bit for bit (numpy.array_equal): the host layer regroups no arithmetic between them or the dump says where.
  python tools/host_scaffold_dump.py --out new.npz                              this tree's gpr/model.py through the library (needs a GPU)
  python tools/host_scaffold_dump.py --out old.npz --model-file OLD_MODEL.py    another version of that file (git show REV:mogptk_amd/gpr/model.py > OLD_MODEL.py)
  python tools/host_scaffold_dump.py --twin ...                                 on the numpy twin of the device (oracle/table_model.py), no GPU
  python tools/host_scaffold_dump.py --compare old.npz new.npz                  exit status 1 unless both hold the same names and equal arrays
Models: Exact, Titsias, Snelson, OpperArchambeau, SparseHensman, Hensman, each single-output (SM), two-channel (MOSM) and enveloped (MOHSM); Exact, Titsias and
Snelson with a ConstantMean and a LinearMean; Exact with per-channel noise and data_variance; Exact with a Matern kernel; Exact and Snelson under
use_single_precision().  N = 300 (170 / 130 over two channels), 2 x 16 inducing points, 37 test points.
  --n N --m M         N training points in the same 17 : 13 split and at the same density, 2 x M inducing points (two builds of the library, selected through MOGP_LIB_PATH: --n 1100
                      --m 160 is 9 tile rows, the smallest size that reaches the 128 x 128 GEMMs, the stream-K solves and the dataflow schedule)
  --skip A,B          leave out the cases whose tag holds one of these words (OpperArchambeau, Hensman, f32, ...)
The twin has no gradient of the sparse bounds with respect to the mean, so --twin leaves out the loss() of Titsias / Snelson with a mean; it also leaves out
the Matern model, which the twin carries by now (kinds and product groups, exact evaluations only), so that dumps stay comparable with older ones; it adds the ill-conditioned Exact model of tests/test_host_logic.py and records the file:line its RuntimeWarning is attributed to."""
import argparse, importlib.util, os, sys, warnings
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np


def compare(a, b):
    A, B = np.load(a), np.load(b)
    bad = sorted(set(A.files) ^ set(B.files)) + [k for k in A.files if k in B.files and not np.array_equal(A[k], B[k])]
    for k in bad:
        print("  DIFFERENT", k)
    print("VERDICT: %d arrays in %s, %d in %s: %s" % (len(A.files), a, len(B.files), b, "all bit-identical" if not bad else "%d differ" % len(bad)))
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--twin", action="store_true")
    ap.add_argument("--model-file")
    ap.add_argument("--compare", nargs=2)
    ap.add_argument("--n", type=int, default=300)
    ap.add_argument("--m", type=int, default=16)
    ap.add_argument("--skip", default="")
    args = ap.parse_args()
    if args.compare:
        return compare(*args.compare)

    from mogptk_amd import gpr, _lib
    M = gpr
    if args.model_file:                       # the model classes of another version of gpr/model.py, inside this package (its relative imports resolve here)
        spec = importlib.util.spec_from_file_location("mogptk_amd.gpr.model_other", args.model_file)
        M = importlib.util.module_from_spec(spec)
        sys.modules[spec.name] = M
        spec.loader.exec_module(M)
    if args.twin:
        from oracle.table_model import TableDevice

        class Twin(TableDevice):
            """the numpy twin plus the affine mean table of the device handle (exact evaluations only: d loss / d m = dp/dr = -alpha)"""

            def __init__(self, device, X, y, C):
                super().__init__(device, X, y, C)
                self.y0 = self.y

            def set_mean(self, coef):
                c = self.X[:, 0].astype(np.int64)
                self.y = self.y0 - (coef[c, 0] + np.sum(coef[c, 1:] * self.X[:, 1:], axis=1)).reshape(-1, 1)

            def mean_grad(self):
                c, a = self.X[:, 0].astype(np.int64), -self._last[1].reshape(-1)
                return np.array([np.r_[np.sum(a[c == k]), a[c == k] @ self.X[c == k, 1:]] for k in range(self.C)])

        _lib.ExactHandle = Twin

    np.random.seed(7)
    rng = np.random.default_rng(7)
    n0, S = (17 * args.n + 15) // 30, 37
    n1 = args.n - n0
    span = 10.0 * args.n / 300                  # the inputs keep their density: the Gram matrices stay as well conditioned as at N = 300
    x = np.r_[np.sort(rng.uniform(0, span, n0)), np.sort(rng.uniform(0, span, n1))]
    X2 = np.c_[np.r_[np.zeros(n0), np.ones(n1)], x]
    y = np.sin(x) + 0.3 * X2[:, 0] * np.cos(2 * x) + 0.1 * rng.standard_normal(n0 + n1)
    xs = rng.uniform(-1, span + 1, S)
    Xs2 = np.c_[np.r_[np.zeros(19), np.ones(18)], xs]
    perm = rng.permutation(n0 + n1)             # the channels interleaved, as data comes
    X2, y = X2[perm], y[perm]
    X1, Xs1 = X2[:, 1:], Xs2[:, 1:]
    dvar = 0.01 * rng.uniform(0.5, 1.5, n0 + n1)

    kernels = {
        "so": (lambda: gpr.SpectralMixtureKernel(Q=2, input_dims=1), X1, Xs1, 2 * args.m),
        "mosm": (lambda: gpr.MultiOutputSpectralMixtureKernel(Q=2, output_dims=2, input_dims=1), X2, Xs2, args.m),
        "mohsm": (lambda: gpr.MixtureKernel(gpr.MultiOutputHarmonizableSpectralKernel(output_dims=2, input_dims=1), 2), X2, Xs2, args.m),
        "matern": (lambda: gpr.MaternKernel(1.5, 1), X1, Xs1, 2 * args.m),
    }
    build = {
        "Exact": lambda k, X, Z, **kw: M.Exact(k, X, y, variance=kw.pop("variance", 0.04), **kw),
        "Titsias": lambda k, X, Z, **kw: M.Titsias(k, X, y, Z=Z, variance=0.04, **kw),
        "Snelson": lambda k, X, Z, **kw: M.Snelson(k, X, y, Z=Z, variance=kw.pop("variance", 0.04), **kw),
        "OpperArchambeau": lambda k, X, Z, **kw: M.OpperArchambeau(k, X, y, **kw),
        "SparseHensman": lambda k, X, Z, **kw: M.SparseHensman(k, X, y, Z=Z, **kw),
        "Hensman": lambda k, X, Z, **kw: M.Hensman(k, X, y, **kw),
    }
    cases = [(c, kn, {}) for c in build for kn in ("so", "mosm", "mohsm")]
    cases += [(c, "mosm", dict(mean=mk)) for c in ("Exact", "Titsias", "Snelson") for mk in ("cmean", "lmean")]
    cases += [("Exact", "mosm", dict(variance=[0.04, 0.09], data_variance=dvar)), ("Exact", "matern", {})]
    cases += [("Exact", "mosm", dict(variance=[0.04, 0.09], f32=True)), ("Snelson", "mosm", dict(variance=[0.04, 0.09], f32=True)), ("Snelson", "mosm", dict(f32=True))]

    out = {}
    for cls, kn, kw in cases:
        kw = dict(kw)
        tag = ".".join([cls, kn] + ["%s" % (v if isinstance(v, str) else k) for k, v in sorted(kw.items())])
        if args.twin and kn == "matern":
            continue
        if any(w and w in tag.split(".") for w in args.skip.split(",")):
            continue
        f32, mean = kw.pop("f32", False), kw.pop("mean", None)
        if f32:
            gpr.use_single_precision()
        try:
            mk, X, Xs, Z = kernels[kn]
            if mean is not None:
                kw["mean"] = gpr.ConstantMean() if mean == "cmean" else gpr.LinearMean(input_dims=X.shape[1])
            m = build[cls](mk(), X, Z, **kw)
            for p in m.parameters():                       # away from the initial values, in the parameter's own dtype
                name, d = str(p._name).split(".")[-1], p.data
                if name == "induction_points":
                    d = d.copy()
                    d[:, X.shape[1] - 1:] += 0.05 * rng.standard_normal((d.shape[0], 1))
                elif name == "q_sqrt":
                    d = d + 0.05 * np.tril(rng.standard_normal(d.shape))
                else:
                    d = d + 0.1 * rng.standard_normal(d.shape)
                p.data = np.asarray(d, dtype=p.data.dtype)
            if not (args.twin and mean is not None and cls != "Exact"):
                out[tag + ".loss"] = np.asarray(m.loss())
                for i, p in enumerate(m.parameters()):
                    out["%s.grad_%02d" % (tag, i)] = np.zeros(0) if p.grad is None else np.asarray(p.grad)
            out[tag + ".lml"] = np.asarray(m.log_marginal_likelihood())
            for full, names in ((False, (".mu", ".var")), (True, (".full_mu", ".full_cov"))):
                try:
                    out[tag + names[0]], out[tag + names[1]] = [np.asarray(a) for a in m.predict_f(Xs, full=full)]
                except NotImplementedError:                # Snelson has no full covariance, OpperArchambeau predicts with a constant kernel diagonal only
                    pass
        except Exception as e:                                 # a combination the library refuses (OpperArchambeau with enveloped terms, the dense Hensman model with
            if type(e).__name__ not in ("MogpError", "CholeskyException"):      # interleaved channels) or a matrix it finds indefinite (the perturbed MOHSM model at N = 1100):
                raise                                          # the message, leading-minor order included, is part of the dump; what was evaluated before it stays
            out[tag + ".refused"] = np.array(str(e))
            print(tag, "refused:", e, flush=True)
            continue
        finally:
            gpr.use_double_precision()
        print(tag, "loss", out.get(tag + ".loss"), "lml", out[tag + ".lml"], flush=True)

    if args.twin:                                          # the warning of an ill-conditioned Exact model names its caller's line
        class Reporting(_lib.ExactHandle):
            condition_estimate = lambda self: 3e6
            set_accurate = lambda self, on: None

        _lib.ExactHandle = Reporting
        for what in ("loss", "predict_f"):
            m = M.Exact(kernels["mosm"][0](), X2, y, variance=0.04)
            with warnings.catch_warnings(record=True) as w:
                warnings.simplefilter("always")
                m.loss() if what == "loss" else m.predict_f(Xs2)
            assert len(w) == 1, [str(v.message) for v in w]
            out["illcond.%s.warned_at" % what] = np.array("%s:%d" % (os.path.basename(w[0].filename), w[0].lineno))
            print("illcond", what, "->", out["illcond.%s.warned_at" % what])
    np.savez(args.out, **out)
    print("wrote %d arrays to %s" % (len(out), args.out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
