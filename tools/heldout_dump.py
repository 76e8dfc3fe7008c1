"""What the held-out entry points of the exact path hand back -- mogp_exact_loo, mogp_exact_cv, and mogp_exact_eval around them on the same handle --
written to one .npz, to compare two builds of the library bit for bit (numpy.array_equal, NaN positions included).
  MOGP_LIB_PATH=OLD.so python tools/heldout_dump.py --out old.npz        one process per library (needs a GPU)
  python tools/heldout_dump.py --out new.npz
  python tools/heldout_dump.py --compare old.npz new.npz                 exit status 1 unless both hold the same names and equal arrays
Raw outputs through the C ABI (_lib.ExactHandle): C = 3 ragged channels, Q = 2, D = 1, inputs shuffled, fixed seeds; N = 699 (stream schedules) and
N = 1100 (the dataflow schedule, asserted through mogp_model_schedule after every gradient call).  On ONE handle per size, in this order:
  c01 eval LML only, c02 eval grad, c03 loo, c04 loo grad, c05 eval grad, c06 cv, c07 cv grad, c07b the same call again (the cached fold upload),
  c08 cv grad with other folds (re-upload), c09 loo grad, c10 eval grad.  Folds hold 1, 7, 128 and then 64 points each; a tenth of the points is in no fold.
Every call records its outputs, mogp_model_pivot_range, mogp_model_loo_bytes, the schedule bit and whether mogp_model_fetch(0) is refused (W is gone).
N = 699 only, fresh handles: mean.* (a mean table: mogp_model_mean_grad and fetch 3 after loo and cv), kinds.* (one Matern-3/2 row per pair), env.* (rows of
width 2 + 5 D with a point diagonal), dvar.* (data_var), acc.* (mogp_model_set_accurate(1): loo and cv with gradients, then accurate off and eval),
prof.* (profiling on: fetch 4 gives two finite positive times after a cv gradient call -- not compared -- and its refusal after a call without gradients),
refuse.* (code | message of: a fold of 129 points, nfolds = 0, a label out of range, null mu to mogp_exact_loo, null gradient outputs with MOGP_EVAL_GRAD
to all three entry points; none reaches the device), and phases.*: a child process with MOGP_GRAD_PATH=phases for c02, c04 and c07."""
import argparse, ctypes, os, subprocess, sys, zlib
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np


def compare(a, b):
    A, B = np.load(a), np.load(b)
    bad = sorted(set(A.files) ^ set(B.files))
    for k in sorted(set(A.files) & set(B.files)):
        x, y = A[k], B[k]
        same = x.shape == y.shape and (np.array_equal(x, y, equal_nan=True) if x.dtype.kind == "f" else np.array_equal(x, y))
        print("  %-34s %-12s crc32 %08x  %s" % (k, x.shape, zlib.crc32(np.ascontiguousarray(x).tobytes()), "EQUAL" if same else "DIFFERENT"))
        if not same:
            bad.append(k)
    for k in bad:
        print("  DIFFERENT", k)
    print("  VERDICT: %d arrays in %s, %d in %s: %s" % (len(A.files), a, len(B.files), b, "all bit-identical" if not bad else "%d differ" % len(bad)))
    return 1 if bad else 0


def make_folds(rng, N, head):
    """labels in the caller's row order: folds of the sizes in `head`, then of 64 points, a tenth of the points in no fold"""
    rows = rng.permutation(N)
    lab = np.full(N, -1, dtype=np.int32)
    at, f = 0, 0
    for size in list(head) + [64] * N:
        if at + size > N - N // 10:
            break
        lab[rows[at:at + size]] = f
        at += size; f += 1
    return lab, f


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--compare", nargs=2)
    ap.add_argument("--phases-child", action="store_true")
    args = ap.parse_args()
    if args.compare:
        return compare(*args.compare)

    from mogptk_amd import gpr, _lib
    from mogptk_amd.gpr.singleoutput import KIND_MATERN32
    L, G = _lib.lib(), _lib.MOGP_EVAL_GRAD
    out = {}

    def refusal(call):
        try:
            call()
        except _lib.MogpError as e:
            return np.array("%d | %s" % (e.code, e))
        return np.array("accepted")

    def record(tag, h, res, dataflow=None):
        for key, v in res.items():
            if v is not None:
                out[tag + "." + key] = np.asarray(v)
        lo, hi = np.zeros(1), np.zeros(1)
        _lib.check(L.mogp_model_pivot_range(h._h, _lib._dp(lo), _lib._dp(hi)))
        s = h.schedule()
        if dataflow:
            assert s["dataflow"] and not s["dataflow_fell_back"], (tag, s)
        out[tag + ".pivots"], out[tag + ".loo_bytes"], out[tag + ".dataflow"] = np.r_[lo, hi], np.array(h.loo_bytes()), np.array(s["dataflow"])
        out[tag + ".w_refused"] = refusal(lambda: h.fetch(0))
        print(tag, {k: float(v) for k, v in res.items() if k in ("lml", "loo", "cv")}, "dataflow", s["dataflow"], flush=True)

    def inputs(N, C=3, Q=2):
        rng = np.random.default_rng(N)
        sizes = rng.multinomial(N - C, np.ones(C) / C) + 1
        X = np.concatenate([np.stack([np.full(s, float(c)), rng.uniform(0, 10, s)], axis=1) for c, s in enumerate(sizes)])[rng.permutation(N)]
        y = rng.standard_normal(N)
        k = gpr.MultiOutputSpectralMixtureKernel(Q=Q, output_dims=C)
        k.weight.assign(rng.uniform(0.5, 1.5, (C, Q))); k.mean.assign(rng.uniform(0.02, 0.4, (C, Q, 1)))
        k.variance.assign(rng.uniform(0.05, 0.5, (C, Q, 1))); k.delay.assign(rng.normal(0, 0.3, (C, Q, 1))); k.phase.assign(rng.normal(0, 0.3, (C, Q)))
        return rng, X, y, k._spectral_terms(1), rng.uniform(0.05, 0.2, C)

    def handle(X, y, table, C=3):
        h = _lib.ExactHandle(0, X, y, C)
        h.set_terms(table)
        return h

    J = 1e-8
    for N in (699, 1100):
        rng, X, y, table, noise = inputs(N)
        lab, nf = make_folds(rng, N, (1, 7, 128))
        lab2, nf2 = make_folds(rng, N, (3, 40, 128, 5))
        flow = N == 1100
        cases = [("c01.eval", lambda h: h.eval(noise, J, grad=False), False), ("c02.eval_grad", lambda h: h.eval(noise, J), flow),
                 ("c03.loo", lambda h: h.loo(noise, J, grad=False), False), ("c04.loo_grad", lambda h: h.loo(noise, J), flow),
                 ("c05.eval_grad", lambda h: h.eval(noise, J), flow), ("c06.cv", lambda h: h.cv(noise, J, lab, nf, grad=False), False),
                 ("c07.cv_grad", lambda h: h.cv(noise, J, lab, nf), flow), ("c07b.cv_grad_again", lambda h: h.cv(noise, J, lab, nf), flow),
                 ("c08.cv_grad_other_folds", lambda h: h.cv(noise, J, lab2, nf2), flow), ("c09.loo_grad", lambda h: h.loo(noise, J), flow),
                 ("c10.eval_grad", lambda h: h.eval(noise, J), flow)]
        if args.phases_child:
            assert os.environ.get("MOGP_GRAD_PATH") == "phases"
            cases = [c for c in cases if c[0][:3] in ("c02", "c04", "c07") and c[0] != "c07b.cv_grad_again"]
        h = handle(X, y, table)
        for name, call, dataflow in cases:
            record("n%d.%s" % (N, name), h, call(h), dataflow and not args.phases_child)
        h.close()
        if args.phases_child or N != 699:
            continue

        def held_out(tag, h, **kw):
            for name, call in (("loo_grad", lambda: h.loo(noise, J, **kw)), ("cv_grad", lambda: h.cv(noise, J, lab, nf, **kw))):
                record("n699.%s.%s" % (tag, name), h, call())
                if tag == "mean":
                    out["n699.mean.%s.g" % name], out["n699.mean.%s.dpdr" % name] = h.mean_grad(), h.fetch(3)

        h = handle(X, y, table)
        h.set_mean(np.array([[0.3, 0.01], [-0.2, 0.02], [0.1, -0.03]]))
        held_out("mean", h)
        h.close()

        k1 = gpr.MultiOutputSpectralMixtureKernel(Q=1, output_dims=3)         # rank-one coregionalisation of ONE profile: positive definite under any kind
        k1.weight.assign(rng.uniform(0.5, 1.5, (3, 1))); k1.mean.assign(np.zeros((3, 1, 1))); k1.variance.assign(np.full((3, 1, 1), 0.3))
        k1.delay.assign(np.zeros((3, 1, 1))); k1.phase.assign(np.zeros((3, 1)))
        t1 = k1._spectral_terms(1)
        h = handle(X, y, t1)
        h.set_kinds(np.full(t1.shape[:3], KIND_MATERN32, dtype=np.int32), np.zeros(t1.shape[:3]))
        held_out("kinds", h)
        h.close()

        ke = gpr.MixtureKernel(gpr.MultiOutputHarmonizableSpectralKernel(output_dims=3, input_dims=1), 2)
        for p in ke.parameters():
            p.data = np.asarray(p.data + 0.1 * rng.standard_normal(p.data.shape), dtype=p.data.dtype)
        te = ke._device_terms(1)[0]
        assert te.shape[3] == 2 + 5
        h = handle(X, y, te)
        h.set_point_diag(ke._point_diag(te, ke._kernel_format(X), 1))
        held_out("env", h)
        h.close()

        h = handle(X, y, table)
        held_out("dvar", h, data_var=rng.uniform(0.0, 0.1, N))
        h.close()

        h = handle(X, y, table)
        h.set_accurate(1)
        held_out("acc", h)
        h.set_accurate(0)
        record("n699.acc_off.eval_grad", h, h.eval(noise, J))
        h.close()

        h = handle(X, y, table)
        h.set_profiling(True)
        h.cv(noise, J, lab, nf)
        t = h.fetch(4)
        assert np.all(np.isfinite(t)) and np.all(t > 0), t
        out["n699.prof.cv_grad.two_finite_positive_times"] = np.array(True)
        h.cv(noise, J, lab, nf, grad=False)
        out["n699.prof.cv.fetch4"] = refusal(lambda: h.fetch(4))
        h.close()

        h = handle(X, y, table)
        dp, i32p = _lib._dp, lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
        d, i64 = [ctypes.c_double() for _ in range(3)], ctypes.c_int64(0)
        mu, var, mom, dg = np.empty(N), np.empty(N), np.zeros((6, 2, 5)), np.zeros(3)
        tail = (ctypes.byref(d[1]), ctypes.byref(d[2]), ctypes.byref(i64))
        refusals = {
            "fold_of_129": lambda: h.cv(noise, J, np.where(np.arange(N) < 129, 0, -1), 1, grad=False),
            "nfolds_0": lambda: h.cv(noise, J, lab, 0, grad=False),
            "label_out_of_range": lambda: h.cv(noise, J, np.where(np.arange(N) < 5, 3, -1), 2, grad=False),
            "loo_null_mu": lambda: _lib.check(L.mogp_exact_loo(h._h, dp(noise), None, J, 0, ctypes.byref(d[0]), None, dp(var), None, None, *tail)),
            "eval_null_grad": lambda: _lib.check(L.mogp_exact_eval(h._h, dp(noise), None, J, G, ctypes.byref(d[0]), None, dp(dg), *tail)),
            "loo_null_grad": lambda: _lib.check(L.mogp_exact_loo(h._h, dp(noise), None, J, G, ctypes.byref(d[0]), dp(mu), dp(var), dp(mom), None, *tail)),
            "cv_null_grad": lambda: _lib.check(L.mogp_exact_cv(h._h, dp(noise), None, J, G, i32p(lab), nf, ctypes.byref(d[0]), dp(mu), dp(var), dp(mom), dp(dg),
                                                               None, ctypes.byref(d[2]), ctypes.byref(i64))),
        }
        for name, call in refusals.items():
            out["n699.refuse." + name] = refusal(call)
            assert str(out["n699.refuse." + name]) != "accepted", name
            print("refuse", name, "->", out["n699.refuse." + name])
        h.close()

    if not args.phases_child:                                  # MOGP_GRAD_PATH is read once per process: a child of its own, under its own time limit
        child = args.out + ".phases.npz"
        subprocess.run([sys.executable, os.path.abspath(__file__), "--phases-child", "--out", child], env=dict(os.environ, MOGP_GRAD_PATH="phases"),
                       check=True, timeout=120)
        with np.load(child) as ph:
            out.update({"phases." + k: ph[k] for k in ph.files})
        os.remove(child)
    np.savez(args.out, **out)
    print("wrote %d arrays to %s" % (len(out), args.out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
