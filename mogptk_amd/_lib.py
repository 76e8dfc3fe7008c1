"""
ctypes binding of libmogp_hip.so (include/mogp_hip.h).  This is the only place the package touches the
native library.  There is NO fallback: if the library is missing, or no gfx950 device is visible when a
compute entry point is called, the call fails loudly.
"""
import atexit
import ctypes
import os
import threading
import weakref
import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MOGP_LIB_PATH") or os.path.join(_HERE, "csrc", "libmogp_hip.so")      # (MOGP_LIB_PATH: another build of the same library, for A/B runs)

MOGP_OK, MOGP_EINVAL, MOGP_EHIP, MOGP_ENOTPD, MOGP_ENONFINITE, MOGP_ENODEVICE = 0, -1, -2, -3, -4, -5
MOGP_EVAL_GRAD = 1
COMM_ID_BYTES = 128
ALLGATHER_CB = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64)
ALLREDUCE_CB = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64)
ST_GRAM, ST_POTRF, ST_TRTRI, ST_LAUUM, ST_SOLVE, ST_MOMENTS, ST_TOTAL, ST_GEMM_KERNEL, ST_GRAM_KERNEL, ST_MOMENT_KERNEL, ST_COUNT = range(11)

_lib = None
_lock = threading.RLock()
_ctx = {}
_live = weakref.WeakSet()             # open ExactHandles (shutdown() closes them before their contexts go)

c_dp = ctypes.POINTER(ctypes.c_double)
c_i64p = ctypes.POINTER(ctypes.c_int64)
c_ip = ctypes.POINTER(ctypes.c_int)

# name -> (restype, argtypes); mirrors include/mogp_hip.h one to one (tests check every symbol is exported)
SIGNATURES = {
    "mogp_version": (ctypes.c_char_p, []),
    "mogp_last_error": (ctypes.c_char_p, []),
    "mogp_device_count": (ctypes.c_int, []),
    "mogp_ctx_create": (ctypes.c_int, [ctypes.c_int, ctypes.POINTER(ctypes.c_void_p)]),
    "mogp_ctx_destroy": (ctypes.c_int, [ctypes.c_void_p]),
    "mogp_ctx_device_name": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int]),
    "mogp_model_create": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_int, c_dp, c_dp,
                                         ctypes.POINTER(ctypes.c_void_p)]),
    "mogp_model_destroy": (ctypes.c_int, [ctypes.c_void_p]),
    "mogp_model_set_y": (ctypes.c_int, [ctypes.c_void_p, c_dp]),
    "mogp_model_set_mean": (ctypes.c_int, [ctypes.c_void_p, c_dp]),
    "mogp_model_mean_grad": (ctypes.c_int, [ctypes.c_void_p, c_dp]),
    "mogp_model_set_terms": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, c_dp]),
    "mogp_model_set_terms_ex": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, c_dp]),
    "mogp_model_set_point_diag": (ctypes.c_int, [ctypes.c_void_p, c_dp]),
    "mogp_gram_ex": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_dp,
                                    ctypes.c_int64, c_dp, ctypes.c_int64, c_dp, c_dp]),
    "mogp_gram": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_dp,
                                 ctypes.c_int64, c_dp, ctypes.c_int64, c_dp, c_dp]),
    "mogp_model_set_kinds": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, c_ip, c_dp]),
    "mogp_gram_kinds": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_dp, c_ip, c_dp,
                                       ctypes.c_int64, c_dp, ctypes.c_int64, c_dp, c_dp]),
    "mogp_exact_eval": (ctypes.c_int, [ctypes.c_void_p, c_dp, c_dp, ctypes.c_double, ctypes.c_int,
                                       c_dp, c_dp, c_dp, c_dp, c_dp, c_i64p]),
    "mogp_exact_loo": (ctypes.c_int, [ctypes.c_void_p, c_dp, c_dp, ctypes.c_double, ctypes.c_int,
                                      c_dp, c_dp, c_dp, c_dp, c_dp, c_dp, c_dp, c_i64p]),
    "mogp_exact_cv": (ctypes.c_int, [ctypes.c_void_p, c_dp, c_dp, ctypes.c_double, ctypes.c_int, ctypes.POINTER(ctypes.c_int32), ctypes.c_int64,
                                     c_dp, c_dp, c_dp, c_dp, c_dp, c_dp, c_dp, c_i64p]),
    "mogp_model_loo_bytes": (ctypes.c_int, [ctypes.c_void_p, c_i64p]),
    "mogp_exact_forecast": (ctypes.c_int, [ctypes.c_void_p, c_dp, c_dp, ctypes.c_double, c_i64p, ctypes.c_int, c_i64p,
                                           c_dp, c_dp, c_dp, c_dp, c_i64p]),
    "mogp_exact_predict": (ctypes.c_int, [ctypes.c_void_p, c_dp, c_dp, ctypes.c_double, c_dp, ctypes.c_int64, c_dp,
                                          ctypes.c_int, c_dp, c_dp, c_i64p]),
    "mogp_exact_predict_parts": (ctypes.c_int, [ctypes.c_void_p, c_dp, c_dp, ctypes.c_double, ctypes.c_int, c_dp, c_dp, ctypes.c_int64, c_dp,
                                                ctypes.c_int, c_dp, c_dp, c_i64p]),
    "mogp_exact_predict_grad": (ctypes.c_int, [ctypes.c_void_p, c_dp, c_dp, ctypes.c_double, c_dp, ctypes.c_int64, c_dp, c_dp, c_dp, c_i64p]),
    "mogp_exact_predict_grad_cov": (ctypes.c_int, [ctypes.c_void_p, c_dp, c_dp, ctypes.c_double, ctypes.c_int64, c_dp, c_dp, c_dp, c_i64p]),
    "mogp_titsias_eval": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, c_dp, ctypes.c_double, ctypes.c_double, c_dp, ctypes.c_int,
                                         c_dp, c_dp, c_dp, c_dp, c_dp, c_dp, c_dp, c_i64p]),
    "mogp_titsias_fetch": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, c_dp]),
    "mogp_titsias_predict": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, c_dp, ctypes.c_double, ctypes.c_double, c_dp,
                                            ctypes.c_int64, c_dp, c_dp, c_dp, c_i64p]),
    "mogp_titsias_eval_sharded": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, c_dp, ctypes.c_double, ctypes.c_double, c_dp, ctypes.c_int,
                                                 c_dp, c_dp, c_dp, c_dp, c_dp, c_dp, c_dp, c_i64p]),
    "mogp_titsias_predict_sharded": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, c_dp, ctypes.c_double, ctypes.c_double, c_dp,
                                                    ctypes.c_int64, c_dp, c_dp, c_dp, c_i64p]),
    "mogp_comm_unique_id": (ctypes.c_int, [ctypes.c_void_p]),
    "mogp_comm_init_rccl": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int]),
    "mogp_comm_init_external": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "mogp_comm_destroy": (ctypes.c_int, [ctypes.c_void_p]),
    "mogp_comm_info": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]),
    "mogp_comm_selftest": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]),
    "mogp_shard_stage_ms": (ctypes.c_int, [ctypes.c_void_p, c_dp]),
    "mogp_model_inverse_fraction": (ctypes.c_int, [ctypes.c_void_p, c_dp]),
    "mogp_model_pivot_range": (ctypes.c_int, [ctypes.c_void_p, c_dp, c_dp]),
    "mogp_model_set_accurate": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    "mogp_exact_eval_sharded": (ctypes.c_int, [ctypes.c_void_p, c_dp, c_dp, ctypes.c_double, c_dp, c_dp, c_dp, c_dp, c_dp, c_i64p]),
    "mogp_exact_predict_sharded": (ctypes.c_int, [ctypes.c_void_p, c_dp, c_dp, ctypes.c_double, c_dp, ctypes.c_int64, c_dp, c_dp, c_dp, c_i64p]),
    "mogp_shard_config": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int]),
    "mogp_model_work_bytes": (ctypes.c_int, [ctypes.c_void_p, c_i64p, c_i64p]),
    "mogp_shard_begin": (ctypes.c_int, [ctypes.c_void_p, c_dp, c_dp, ctypes.c_double, c_dp, ctypes.POINTER(ctypes.c_int)]),
    "mogp_shard_pack": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_void_p), c_i64p]),
    "mogp_shard_unpack": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    "mogp_shard_block": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    "mogp_shard_alpha": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p), c_i64p]),
    "mogp_shard_finish": (ctypes.c_int, [ctypes.c_void_p, c_dp, c_dp, c_dp, c_i64p]),
    "mogp_dev_copy": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int]),
    "mogp_set_profiling": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    "mogp_stage_ms": (ctypes.c_int, [ctypes.c_void_p, c_dp, c_i64p, c_dp]),
    "mogp_model_fetch": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, c_dp]),
    "mogp_model_schedule": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int)]),
    "mogp_model_flow_replay": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    "mogp_ctx_plan_cus": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    "mogp_strip_plan": (ctypes.c_int, [ctypes.c_int, c_i64p, ctypes.c_int, c_i64p, ctypes.c_int64, c_i64p]),
    "mogp_model_strip_runs": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, c_i64p]),
    "mogp_model_gram": (ctypes.c_int, [ctypes.c_void_p, c_dp, c_dp, ctypes.c_double, c_dp]),
    "mogp_model_flow_diag": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint)]),
    "mogp_flow_plan": (ctypes.c_int, [ctypes.c_int, c_i64p, ctypes.c_int64, c_i64p]),
    "mogp_flow_plan_rhs": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, c_i64p, ctypes.c_int64, ctypes.POINTER(ctypes.c_int64)]),
    "mogp_flow_trace": (ctypes.c_int, [ctypes.c_void_p, c_i64p, ctypes.c_int64, c_i64p]),
    "mogp_snelson_eval": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, c_dp, c_dp, ctypes.c_double, c_dp, ctypes.c_int,
                                         ctypes.POINTER(ctypes.c_double), c_dp, c_dp, c_dp, ctypes.POINTER(ctypes.c_double), c_dp,
                                         ctypes.POINTER(ctypes.c_double), c_i64p]),
    "mogp_snelson_predict": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, c_dp, c_dp, ctypes.c_double, c_dp, c_dp, ctypes.c_int64, c_dp,
                                            c_dp, c_dp, c_i64p]),
    "mogp_snelson_eval_sharded": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, c_dp, c_dp, ctypes.c_double, c_dp, ctypes.c_int,
                                         ctypes.POINTER(ctypes.c_double), c_dp, c_dp, c_dp, ctypes.POINTER(ctypes.c_double), c_dp,
                                         ctypes.POINTER(ctypes.c_double), c_i64p]),
    "mogp_snelson_predict_sharded": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, c_dp, c_dp, ctypes.c_double, c_dp, c_dp, ctypes.c_int64, c_dp,
                                            c_dp, c_dp, c_i64p]),
    "mogp_svgp_forward": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, c_dp, c_dp, c_dp, ctypes.c_double, c_dp, ctypes.c_int, ctypes.c_int64,
                                         c_dp, c_dp, c_dp, c_dp, ctypes.POINTER(ctypes.c_double), c_i64p]),
    "mogp_svgp_backward": (ctypes.c_int, [ctypes.c_void_p, c_dp, c_dp, c_dp, c_dp, c_dp, ctypes.POINTER(ctypes.c_double), c_dp, c_dp]),
    "mogp_svgp_backward_sharded": (ctypes.c_int, [ctypes.c_void_p, c_dp, c_dp, c_dp, c_dp, c_dp, ctypes.POINTER(ctypes.c_double), c_dp, c_dp]),
    "mogp_oa_forward": (ctypes.c_int, [ctypes.c_void_p, c_dp, c_dp, c_dp, c_dp, ctypes.POINTER(ctypes.c_double), c_i64p]),
    "mogp_oa_backward": (ctypes.c_int, [ctypes.c_void_p, c_dp, c_dp, c_dp, c_dp, c_dp]),
    "mogp_oa_predict": (ctypes.c_int, [ctypes.c_void_p, c_dp, c_dp, c_dp, ctypes.c_int64, c_dp, ctypes.c_int, c_dp, c_dp, c_i64p]),
    "mogp_sparse_predict_cov": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, c_dp]),
    "mogp_mosm_terms": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, c_dp, c_dp, c_dp, c_dp, c_dp, ctypes.c_double, ctypes.c_double, c_dp]),
    "mogp_mosm_terms_backward": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, c_dp, c_dp, c_dp, c_dp, c_dp, ctypes.c_double,
                                                ctypes.c_double, c_dp, c_dp, c_dp, c_dp, c_dp, c_dp]),
    "mogp_mosm_step_forward": (ctypes.c_int, [ctypes.c_int] * 4 + [c_dp, c_ip, c_dp, c_dp, c_dp, c_dp, c_dp, c_dp, ctypes.c_double, ctypes.c_double,
                                              c_dp, c_dp, c_dp, c_dp]),
    "mogp_mosm_step_backward": (ctypes.c_int, [ctypes.c_int] * 4 + [c_dp] * 5 + [ctypes.c_double, ctypes.c_double, c_dp, ctypes.c_int64,
                                                                               ctypes.c_double, ctypes.c_double, c_ip, c_dp]),
    "mogp_exact_step": (ctypes.c_int, [ctypes.c_void_p] + [ctypes.c_int] * 4 + [c_dp, c_ip, c_dp, c_dp, c_dp, c_dp, c_dp, c_dp, ctypes.c_double, ctypes.c_double,
                                                                               c_dp, ctypes.c_double, c_dp, c_ip] + [c_dp] * 8 + [c_i64p]),
    "mogp_adam_step": (ctypes.c_int, [ctypes.c_int, c_i64p] + [c_dp] * 5 + [ctypes.c_double] * 5 + [ctypes.c_int, c_dp, c_dp]),
}


class MogpError(RuntimeError):
    def __init__(self, code, message, info=0):
        super().__init__(message)
        self.code = code
        self.info = info


def lib():
    """Load libmogp_hip.so (built in-tree by __graft_entry__.build()).  Raises if it is absent."""
    global _lib
    with _lock:
        if _lib is None:
            if not os.path.exists(LIB_PATH):
                raise ImportError(
                    "libmogp_hip.so not found at %s: build it with `python __graft_entry__.py` "
                    "(hipcc --offload-arch=gfx950).  mogptk_amd has no CPU fallback." % LIB_PATH)
            l = ctypes.CDLL(LIB_PATH)
            for name, (res, args) in SIGNATURES.items():
                fn = getattr(l, name)
                fn.restype = res
                fn.argtypes = args
            _lib = l
    return _lib


def _dp(a):
    return None if a is None else a.ctypes.data_as(c_dp)


def _f64(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.float64)


def check(code, info=0):
    if code != MOGP_OK:
        msg = lib().mogp_last_error()
        raise MogpError(code, (msg.decode() if msg else "mogp error %d" % code), info)


def context(device=0):
    """One C-ABI context per device ordinal, created on first use."""
    l = lib()
    with _lock:
        if device not in _ctx:
            h = ctypes.c_void_p()
            check(l.mogp_ctx_create(int(device), ctypes.byref(h)))
            _ctx[device] = h
        return _ctx[device]


def comm_selftest(device=0):
    """-> (ranks_seen, rank_sum) of one library-issued all-reduce over the context's communicator (mogp_comm_selftest)"""
    seen, rsum = ctypes.c_int(0), ctypes.c_int(0)
    check(lib().mogp_comm_selftest(context(device), ctypes.byref(seen), ctypes.byref(rsum)))
    return seen.value, rsum.value


def device_name(device=0):
    buf = ctypes.create_string_buffer(256)
    check(lib().mogp_ctx_device_name(context(device), buf, 256))
    return buf.value.decode()


def _ip(a):
    return None if a is None else a.ctypes.data_as(c_ip)


def plan_cus(ncu, device=0):
    """measurement / test switch (mogp_ctx_plan_cus): the CU count the Gram and moment launches of the device's context plan their strip runs and
    persistent grids with; 0 restores the device's own count"""
    check(lib().mogp_ctx_plan_cus(context(device), int(ncu)))


def strip_plan(sizes, ncu):
    """-> int64 array [rows, 8] of the strip plan of a symmetric training Gram over channels of `sizes` points on `ncu` CUs (mogp_strip_plan, host
    only): runs [1, r0, c0, n, pair, diag, 64, 64] first, then the rest tiles [0, r0, c0, 1, pair, diag, rows, columns]"""
    sizes = np.ascontiguousarray(sizes, dtype=np.int64)
    cnt = ctypes.c_int64(0)
    check(lib().mogp_strip_plan(int(sizes.size), sizes.ctypes.data_as(c_i64p), int(ncu), None, 0, ctypes.byref(cnt)))
    out = np.zeros((cnt.value, 8), dtype=np.int64)
    check(lib().mogp_strip_plan(int(sizes.size), sizes.ctypes.data_as(c_i64p), int(ncu), out.ctypes.data_as(c_i64p), out.size, ctypes.byref(cnt)))
    return out


def gram(device, C, D, table, X1, X2=None, kind=None, shape=None):
    """K(X1[,X2]) through mogp_gram; with radial kinds (gpr/kernel.py: _spectral_kinds) through mogp_gram_kinds."""
    table = _f64(table)
    X1 = _f64(X1)
    X2 = _f64(X2)
    T = table.shape[2]
    M1 = X1.shape[0]
    M2 = M1 if X2 is None else X2.shape[0]
    out = np.empty((M1, M2), dtype=np.float64)
    if kind is not None:
        kind = np.ascontiguousarray(kind, dtype=np.int32)
        shape = _f64(shape)
        assert kind.shape == table.shape[:3] and shape.shape == table.shape[:3]
        check(lib().mogp_gram_kinds(context(device), C, D, T, int(table.shape[3]), _dp(table), _ip(kind), _dp(shape), M1, _dp(X1),
                                    0 if X2 is None else M2, _dp(X2), _dp(out)))
        return out
    check(lib().mogp_gram_ex(context(device), C, D, T, int(table.shape[3]), _dp(table), M1, _dp(X1),
                             0 if X2 is None else M2, _dp(X2), _dp(out)))
    return out


def shutdown():
    """Release every model and context of this process while the HIP runtime is still up.  Registered with atexit: left to the interpreter's
    own teardown, the handles' destructors ran after the runtime's (harmless on its own, a crash inside rocprofv3's exit hooks under the
    profiler).  Calling it earlier is allowed; the next use of the library makes a new context."""
    with _lock:
        for h in list(_live):
            try:
                h.close()
            except Exception:
                pass
        if _lib is not None:
            for c in list(_ctx.values()):
                try:
                    _lib.mogp_ctx_destroy(c)
                except Exception:
                    pass
        _ctx.clear()


atexit.register(shutdown)


TRANSFORM_IDENTITY, TRANSFORM_SOFTPLUS, TRANSFORM_SIGMOID = 0, 1, 2


def _check_host(code, name):
    """the host-only entry points (csrc/hoststep.hip, csrc/hostalg.hip) return a code and leave mogp_last_error alone: the message is made here"""
    if code != MOGP_OK:
        raise MogpError(code, "%s failed (%d): a bad argument -- shape, transform kind or null pointer" % (name, code))


class StepPlan:
    """Buffers and ready-made arguments of the native MOSM training step (csrc/hoststep.hip, csrc/step.hip) for one model structure.  Everything
    is flat over [weight C Q | mean C Q D | variance C Q D | delay C Q D | phase C Q | noise scale nscale].  `transforms`: one
    (kind, lower, upper, beta, threshold) per block, lower / upper scalars or arrays of the block's shape; `trained`: one flag per block.
    The plan holds ctypes pointers into its own arrays, so it lives on a device handle (or in a test), never on a model, kernel or
    parameter: those are pickled and deep-copied."""

    def __init__(self, C, Q, D, nscale, transforms, twopi, phase_scale, counts, N, trained):
        self.C, self.Q, self.D, self.nscale, self.N = int(C), int(Q), int(D), int(nscale), int(N)
        sizes = [C * Q, C * Q * D, C * Q * D, C * Q * D, C * Q, nscale]
        self.ends = np.cumsum(sizes)
        self.starts = self.ends - sizes
        self._cuts = [0] + [int(e) for e in self.ends]
        self._trained = [bool(t) for t in trained]
        self.params = ()
        n = int(self.ends[-1])
        W = 2 + 3 * D
        self.tkind = np.zeros(n, dtype=np.int32)
        self.lower, self.upper, self.beta, self.threshold = np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(n)
        for (kind, lo, up, beta, thr), a, b in zip(transforms, self.starts, self.ends):
            self.tkind[a:b] = kind
            for dst, val in ((self.lower, lo), (self.upper, up), (self.beta, beta), (self.threshold, thr)):
                dst[a:b] = 0.0 if val is None else np.asarray(val, dtype=np.float64).reshape(-1)       # one value, or one per element
        self.trained = np.ascontiguousarray(trained, dtype=np.int32)
        self.counts = _f64(counts)
        assert self.trained.shape == (6,) and self.counts.shape == (C,)
        self.raw, self.cons, self.dcons, self.graw = np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(n)
        # exp and log1p stay numpy's, so that the constrained values are the numpy form's to the last bit: z = beta x (x itself under a sigmoid),
        # en = exp(-z), lp = log1p(exp(z)) with z capped at the softplus threshold (beyond it the native code takes the linear branch and reads neither)
        self._scale = np.where(self.tkind == TRANSFORM_SOFTPLUS, self.beta, np.where(self.tkind == TRANSFORM_SIGMOID, 1.0, 0.0))
        self._cap = np.where(self.tkind == TRANSFORM_SOFTPLUS, self.threshold, np.inf)
        self._z, self.lp, self.en = np.zeros(n), np.zeros(n), np.zeros(n)
        self.table = np.zeros((C, C, Q, W))
        self.noise_var = np.zeros(C)
        self.moments = np.zeros((C * (C + 1) // 2, Q, W))
        self.diagG = np.zeros(C)
        self.out = np.zeros(5)                      # LML, trG, jitter_abs, smallest and largest pivot
        self.info = ctypes.c_int64(0)
        self.twopi, self.phase_scale = float(twopi), float(phase_scale)
        shape = (self.C, self.Q, self.D, self.nscale)
        self._fwd = shape + (_dp(self.raw), _ip(self.tkind), _dp(self.lower), _dp(self.upper), _dp(self.beta), _dp(self.threshold), _dp(self.lp), _dp(self.en),
                             self.twopi, self.phase_scale, _dp(self.cons), _dp(self.dcons), _dp(self.table), _dp(self.noise_var))
        self._bwd_head = shape + (_dp(self.cons), _dp(self.dcons), _dp(self.table), _dp(self.moments), _dp(self.diagG))
        self._bwd_tail = (_dp(self.counts), self.N, self.twopi, self.phase_scale, _ip(self.trained), _dp(self.graw))
        self._step_args = None

    def gather(self, tensors):
        """the raw tensors (one per block) into the flat buffer"""
        np.concatenate([t.reshape(-1) for t in tensors], out=self.raw)
        self.transcendentals()

    def transcendentals(self):
        """lp and en of the raw values in the buffer, by numpy"""
        z, lp, en = self._z, self.lp, self.en
        with np.errstate(over="ignore", invalid="ignore"):
            np.multiply(self._scale, self.raw, out=z)
            np.negative(z, out=en)
            np.exp(en, out=en)
            np.minimum(z, self._cap, out=z)
            np.exp(z, out=lp)
            np.log1p(lp, out=lp)

    def block(self, flat, i, shape):
        return flat[self._cuts[i]:self._cuts[i + 1]].reshape(shape)

    def scatter_grad(self):
        """`.grad` of the plan's parameters (`params`, set by the owner) from a fresh copy of graw: arrays of every parameter's own shape,
        None for a block that is not trained.  The arrays are disjoint views of that ONE fresh vector (they share `.base`), not arrays that
        each own their memory as the numpy form's do"""
        g = self.graw.copy()
        cuts = self._cuts
        for i, p in enumerate(self.params):
            p.grad = g[cuts[i]:cuts[i + 1]].reshape(p.data.shape) if self._trained[i] else None

    def forward(self):
        """raw -> cons, dcons, table, noise_var (mogp_mosm_step_forward)"""
        _check_host(lib().mogp_mosm_step_forward(*self._fwd), "mogp_mosm_step_forward")

    def backward(self, trG, jitter):
        """cons, dcons, table, moments, diagG -> graw (mogp_mosm_step_backward)"""
        _check_host(lib().mogp_mosm_step_backward(*self._bwd_head, float(trG), float(jitter), *self._bwd_tail), "mogp_mosm_step_backward")

    def step_args(self, jitter, data_var):
        """what mogp_exact_step takes behind the model handle (kept until the jitter or the data variance array changes)"""
        c = self._step_args
        if c is None or c[0] != jitter or c[1] is not data_var:
            dv = _f64(data_var)
            c = self._step_args = (jitter, data_var, dv, self._fwd[:14] + (_dp(dv), float(jitter), _dp(self.counts), _ip(self.trained)) + self._fwd[14:] +
                                   (_dp(self.moments), _dp(self.diagG), _dp(self.out), _dp(self.graw), ctypes.byref(self.info)))
        return c[3]

    def condition_estimate(self):
        """as ExactHandle.condition_estimate, from the pivots the last step returned"""
        lo, hi = self.out[3], self.out[4]
        return float((hi / lo) ** 2) if lo > 0.0 else float("nan")


class AdamPlan:
    """Buffers and ready-made arguments of mogp_adam_step for one flat group of tensors (ends[s]: one past tensor s).  m, v, vmax are the
    optimiser's flat state and are updated in place; the caller gathers the raw values into x and the gradients into g, sets the bias
    corrections bc1 / bc2 (one per tensor) and reads the new values from x."""

    def __init__(self, ends, m, v, vmax):
        self.ends = np.ascontiguousarray(ends, dtype=np.int64)
        n, k = int(self.ends[-1]), self.ends.shape[0]
        for a in (m, v, vmax):
            assert a.dtype == np.float64 and a.flags.c_contiguous and a.shape == (n,)
        self.m, self.v, self.vmax = m, v, vmax
        self.x, self.g, self.bc1, self.bc2 = np.empty(n), np.empty(n), np.empty(k), np.empty(k)
        self._head = (k, self.ends.ctypes.data_as(c_i64p), _dp(self.x), _dp(self.g), _dp(m), _dp(v), _dp(vmax))
        self._tail = (_dp(self.bc1), _dp(self.bc2))

    def step(self, lr, beta1, beta2, eps, weight_decay, amsgrad):
        _check_host(lib().mogp_adam_step(*self._head, lr, beta1, beta2, eps, weight_decay, 1 if amsgrad else 0, *self._tail), "mogp_adam_step")


class ExactHandle:
    """Owner of one mogp_model (device workspaces for a fixed training set)."""

    def __init__(self, device, X, y, C):
        X = _f64(X)
        y = _f64(np.asarray(y).reshape(-1))
        self.N = X.shape[0]
        self.D = X.shape[1] - 1
        self.C = C
        self.device = device
        h = ctypes.c_void_p()
        self._h = ctypes.c_void_p()             # stays null if creation fails: close() / __del__ then have nothing to destroy
        check(lib().mogp_model_create(context(device), self.N, self.D, C, _dp(X), _dp(y), ctypes.byref(h)))
        self._h = h
        _live.add(self)

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value is not None:
            lib().mogp_model_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_y(self, y):
        y = _f64(np.asarray(y).reshape(-1))
        check(lib().mogp_model_set_y(self._h, _dp(y)))

    def set_mean(self, coef):
        """the affine mean table (C x (1 + D)), or None for no mean; the device recomputes the residual only when the table changed"""
        if coef is None:
            check(lib().mogp_model_set_mean(self._h, None))
            return
        coef = _f64(coef)
        assert coef.shape == (self.C, 1 + self.D)
        check(lib().mogp_model_set_mean(self._h, _dp(coef)))

    def mean_grad(self):
        """g = d loss / d table of the last gradient evaluation, (C, 1 + D)"""
        g = np.empty((self.C, 1 + self.D))
        check(lib().mogp_model_mean_grad(self._h, _dp(g)))
        return g

    def set_terms(self, table):
        table = _f64(table)
        assert table.shape[0] == self.C and table.shape[1] == self.C and table.shape[3] in (2 + 3 * self.D, 2 + 5 * self.D)
        self.T = table.shape[2]
        self.W = int(table.shape[3])                 # 2 + 3 D, or 2 + 5 D for terms with an envelope (MOHSM)
        check(lib().mogp_model_set_terms_ex(self._h, self.T, self.W, _dp(table)))

    def set_kinds(self, kind, shape):
        """radial profile and shape of every (pair, term) of the table just set (mogp_model_set_kinds); None: all Gaussian"""
        if kind is None:
            check(lib().mogp_model_set_kinds(self._h, self.T, None, None))
            return
        kind = np.ascontiguousarray(kind, dtype=np.int32)
        shape = _f64(shape)
        assert kind.shape == (self.C, self.C, self.T) and shape.shape == kind.shape
        check(lib().mogp_model_set_kinds(self._h, self.T, _ip(kind), _dp(shape)))

    def set_point_diag(self, kdiag):
        """K_diag per training point for kernels whose diagonal is not constant per channel (None: back to the table's constant)"""
        check(lib().mogp_model_set_point_diag(self._h, _dp(_f64(kdiag))))

    def eval(self, noise_var, jitter, grad=True, data_var=None):
        """-> dict(lml, moments[P,T,W], diagG[C], trG, jitter_abs)"""
        noise_var = _f64(noise_var)
        data_var = _f64(data_var)
        from .gpr.config import config as _cfg
        comm = getattr(_cfg, "comm", None)
        if grad and comm is not None and (comm.world > 1 or comm.force):
            if getattr(comm, "native", False):
                return self.eval_sharded(noise_var, jitter, data_var)
            from . import dist as _dist
            return _dist.sharded_eval(self, comm, noise_var, jitter, data_var)
        lml, trG, jit, info = ctypes.c_double(), ctypes.c_double(), ctypes.c_double(), ctypes.c_int64(0)
        moments, diagG = self._grad_outputs(grad)
        code = lib().mogp_exact_eval(self._h, _dp(noise_var), _dp(data_var), float(jitter),
                                     MOGP_EVAL_GRAD if grad else 0, ctypes.byref(lml), _dp(moments), _dp(diagG),
                                     ctypes.byref(trG), ctypes.byref(jit), ctypes.byref(info))
        check(code, info.value)
        return dict(lml=lml.value, moments=moments, diagG=diagG, trG=trG.value, jitter_abs=jit.value)

    def step(self, plan, jitter, data_var=None):
        """one training step's evaluation of a plain MOSM model in one native call (mogp_exact_step): plan.raw -> plan.out (LML, trG,
        jitter_abs, pivots) and plan.graw; the table, moments and diagG of the step stay in the plan's buffers"""
        assert plan.C == self.C and plan.D == self.D and plan.N == self.N
        self.T, self.W = plan.Q, 2 + 3 * plan.D
        code = lib().mogp_exact_step(self._h, *plan.step_args(jitter, data_var))
        check(code, plan.info.value)

    def _grad_outputs(self, grad=True):
        """(moments[P,T,W], diagG[C]) for an entry point to fill; (None, None) without gradients"""
        C = self.C
        return (np.zeros((C * (C + 1) // 2, self.T, self.W)), np.zeros(C)) if grad else (None, None)

    def _held_out(self, key, entry, noise_var, jitter, grad, data_var, *score_args):
        """a held-out score (mogp_exact_loo / mogp_exact_cv; score_args: what the entry point takes in front of its outputs) -> the result dict under `key`"""
        noise_var = _f64(noise_var)
        data_var = _f64(data_var)
        score, trG, jit, info = ctypes.c_double(), ctypes.c_double(), ctypes.c_double(), ctypes.c_int64(0)
        mu, var = np.empty(self.N), np.empty(self.N)
        moments, diagG = self._grad_outputs(grad)
        code = entry(self._h, _dp(noise_var), _dp(data_var), float(jitter), MOGP_EVAL_GRAD if grad else 0, *score_args, ctypes.byref(score),
                     _dp(mu), _dp(var), _dp(moments), _dp(diagG), ctypes.byref(trG), ctypes.byref(jit), ctypes.byref(info))
        check(code, info.value)
        return {key: score.value, "mu": mu, "var": var, "moments": moments, "diagG": diagG, "trG": trG.value, "jitter_abs": jit.value}

    def loo(self, noise_var, jitter, grad=True, data_var=None):
        """leave-one-out predictive log-likelihood (mogp_exact_loo) -> dict(loo, mu[N], var[N], moments[P,T,W], diagG[C], trG, jitter_abs): the
        gradient outputs are those of dL/dKj in the layout of `eval`; never sharded (gpr.Exact refuses before it gets here)"""
        return self._held_out("loo", lib().mogp_exact_loo, noise_var, jitter, grad, data_var)

    def cv(self, noise_var, jitter, fold, nfolds, grad=True, data_var=None):
        """leave-fold-out cross-validation (mogp_exact_cv) -> dict(cv, mu[N], var[N], moments[P,T,W], diagG[C], trG, jitter_abs).  fold: N labels in
        the model's row order, -1 or 0 .. nfolds - 1; mu and var are NaN where the label is -1.  The gradient outputs are those of dL/dKj in the
        layout of `eval`; never sharded (gpr.Exact refuses before it gets here)"""
        fold = np.ascontiguousarray(fold, dtype=np.int32)
        if fold.shape != (self.N,):
            raise ValueError("fold must hold one label per training point")
        return self._held_out("cv", lib().mogp_exact_cv, noise_var, jitter, grad, data_var, fold.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), int(nfolds))

    def forecast(self, noise_var, jitter, order, cut, data_var=None):
        """the rolling-origin forecast (mogp_exact_forecast): order (N,) the model's row at every time position, cut (H, N) per horizon and time
        position the number of leading points the prediction may use (-1: skipped) -> dict(score[H], mu[H, N], var[H, N], jitter_abs), mu and
        var in the model's row order and NaN where skipped; never sharded (gpr.Exact refuses before it gets here)"""
        noise_var = _f64(noise_var)
        data_var = _f64(data_var)
        order = np.ascontiguousarray(order, dtype=np.int64)
        cut = np.ascontiguousarray(cut, dtype=np.int64)
        if order.shape != (self.N,) or cut.ndim != 2 or cut.shape[1] != self.N:
            raise ValueError("order must hold one row per time position and cut one row of N cuts per horizon")
        H = cut.shape[0]
        score, mu, var = np.empty(H), np.empty((H, self.N)), np.empty((H, self.N))
        jit, info = ctypes.c_double(), ctypes.c_int64(0)
        code = lib().mogp_exact_forecast(self._h, _dp(noise_var), _dp(data_var), float(jitter), order.ctypes.data_as(c_i64p), H,
                                         cut.ctypes.data_as(c_i64p), _dp(score), _dp(mu), _dp(var), ctypes.byref(jit), ctypes.byref(info))
        check(code, info.value)
        return dict(score=score, mu=mu, var=var, jitter_abs=jit.value)

    def loo_bytes(self):
        """device memory held for `loo` and `cv` alone (mogp_model_loo_bytes): 0 on a handle that never called either"""
        b = ctypes.c_int64(0)
        check(lib().mogp_model_loo_bytes(self._h, ctypes.byref(b)))
        return int(b.value)

    def eval_sharded(self, noise_var, jitter, data_var=None):
        """mogp_exact_eval_sharded: the evaluation spread over the ranks of the context's communicator (collectives inside the library)"""
        lml, trG, jit, info = ctypes.c_double(), ctypes.c_double(), ctypes.c_double(), ctypes.c_int64(0)
        moments, diagG = self._grad_outputs()
        code = lib().mogp_exact_eval_sharded(self._h, _dp(_f64(noise_var)), _dp(_f64(data_var)), float(jitter), ctypes.byref(lml), _dp(moments),
                                             _dp(diagG), ctypes.byref(trG), ctypes.byref(jit), ctypes.byref(info))
        check(code, info.value)
        return dict(lml=lml.value, moments=moments, diagG=diagG, trG=trG.value, jitter_abs=jit.value)

    def predict(self, noise_var, jitter, kss_diag, Xs, full=False, data_var=None):
        noise_var = _f64(noise_var)
        kss_diag = _f64(kss_diag)
        data_var = _f64(data_var)
        Xs = _f64(Xs)
        S = Xs.shape[0]
        from .gpr.config import config as _cfg
        comm = getattr(_cfg, "comm", None)
        if not full and comm is not None and getattr(comm, "native", False) and (comm.world > 1 or comm.force):
            mu, var, info = np.empty(S), np.empty(S), ctypes.c_int64(0)
            code = lib().mogp_exact_predict_sharded(self._h, _dp(noise_var), _dp(data_var), float(jitter), _dp(kss_diag), S, _dp(Xs),
                                                    _dp(mu), _dp(var), ctypes.byref(info))
            check(code, info.value)
            return mu.reshape(-1, 1), var.reshape(-1, 1)
        mu = np.empty(S)
        var = np.empty((S, S) if full else S)
        info = ctypes.c_int64(0)
        code = lib().mogp_exact_predict(self._h, _dp(noise_var), _dp(data_var), float(jitter), _dp(kss_diag), S, _dp(Xs),
                                        1 if full else 0, _dp(mu), _dp(var), ctypes.byref(info))
        check(code, info.value)
        return mu.reshape(-1, 1), (var if full else var.reshape(-1, 1))

    def predict_parts(self, noise_var, jitter, part_tables, kss_diag, Xs, full=False, data_var=None):
        """the posterior of every addend of the covariance behind one factorisation (mogp_exact_predict_parts): part_tables (P, C, C, T, W) are the
        table last set with other amplitudes (and biases of dot-product rows), kss_diag (P, C) or (P, S) each part's prior diagonal
        -> mu (P, S, 1), var (P, S, 1) or (P, S, S) with full; no noise, no mean.  Never sharded (gpr.Exact refuses before it gets here)"""
        noise_var = _f64(noise_var)
        data_var = _f64(data_var)
        part_tables = _f64(part_tables)
        kss_diag = _f64(kss_diag)
        Xs = _f64(Xs)
        S = Xs.shape[0]
        if part_tables.ndim != 5 or part_tables.shape[1:] != (self.C, self.C, self.T, self.W):
            raise ValueError("part_tables must be (P, C, C, T, W) with the shape of the table last set")
        P = part_tables.shape[0]
        if kss_diag.ndim != 2 or kss_diag.shape[0] != P or kss_diag.shape[1] not in (self.C, S):
            raise ValueError("kss_diag must hold one row per part, per channel or per test point")
        mu = np.empty((P, S))
        var = np.empty((P, S, S) if full else (P, S))
        info = ctypes.c_int64(0)
        code = lib().mogp_exact_predict_parts(self._h, _dp(noise_var), _dp(data_var), float(jitter), P, _dp(part_tables), _dp(kss_diag), S, _dp(Xs),
                                              1 if full else 0, _dp(mu), _dp(var), ctypes.byref(info))
        check(code, info.value)
        return mu.reshape(P, S, 1), (var if full else var.reshape(P, S, 1))

    def predict_grad(self, noise_var, jitter, dkss_diag, Xs, data_var=None, full=False):
        """the posterior of df/dx_d at the test points behind one factorisation (mogp_exact_predict_grad): dkss_diag (D, S) the prior variance
        kappa_d of the derivative per input dimension and test point -> dmu (D, S), dvar (D, S); no noise, no mean.  Never sharded, and no row
        of kind 2, 8, 9 or 10 (gpr.Exact refuses before it gets here; the library refuses again).
        full (mogp_exact_predict_grad_cov): the joint covariance of all derivatives -> dmu (D, S), dcov (S, D, S, D); dkss_diag is None (the
        diagonal is the device's own second-derivative Gram), D * S <= GRAD_COV_ROWS"""
        noise_var = _f64(noise_var)
        data_var = _f64(data_var)
        Xs = _f64(Xs)
        S = Xs.shape[0]
        if full:
            if dkss_diag is not None:
                raise ValueError("the joint covariance takes no dkss_diag: its diagonal comes from the device")
            dmu = np.empty((self.D, S))
            dcov = np.empty((S, self.D, S, self.D))
            info = ctypes.c_int64(0)
            code = lib().mogp_exact_predict_grad_cov(self._h, _dp(noise_var), _dp(data_var), float(jitter), S, _dp(Xs), _dp(dmu), _dp(dcov),
                                                     ctypes.byref(info))
            check(code, info.value)
            return dmu, dcov
        dkss_diag = _f64(dkss_diag)
        if dkss_diag.shape != (self.D, S):
            raise ValueError("dkss_diag must be (D, S): one row per input dimension, one value per test point")
        dmu = np.empty((self.D, S))
        dvar = np.empty((self.D, S))
        info = ctypes.c_int64(0)
        code = lib().mogp_exact_predict_grad(self._h, _dp(noise_var), _dp(data_var), float(jitter), _dp(dkss_diag), S, _dp(Xs), _dp(dmu), _dp(dvar),
                                             ctypes.byref(info))
        check(code, info.value)
        return dmu, dvar

    # -- sharded evaluation stages (mogp_shard_*): buffers are raw device pointers, counts are in doubles ------------------
    def shard_begin(self, rank, world, noise_var, jitter, data_var=None):
        check(lib().mogp_shard_config(self._h, int(rank), int(world)))
        jit, nblocks = ctypes.c_double(), ctypes.c_int()
        check(lib().mogp_shard_begin(self._h, _dp(_f64(noise_var)), _dp(_f64(data_var)), float(jitter), ctypes.byref(jit), ctypes.byref(nblocks)))
        return jit.value, nblocks.value

    def shard_pack(self, kb):
        send, recv, count = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_int64()
        check(lib().mogp_shard_pack(self._h, kb, ctypes.byref(send), ctypes.byref(recv), ctypes.byref(count)))
        return send.value, recv.value, count.value

    def shard_unpack(self, kb):
        check(lib().mogp_shard_unpack(self._h, kb))

    def shard_block(self, kb):
        check(lib().mogp_shard_block(self._h, kb))

    def shard_alpha(self):
        buf, count = ctypes.c_void_p(), ctypes.c_int64()
        check(lib().mogp_shard_alpha(self._h, ctypes.byref(buf), ctypes.byref(count)))
        return buf.value, count.value

    def shard_finish(self):
        lml, info = ctypes.c_double(), ctypes.c_int64(0)
        moments, diagG = self._grad_outputs()
        check(lib().mogp_shard_finish(self._h, ctypes.byref(lml), _dp(moments), _dp(diagG), ctypes.byref(info)), info.value)
        return lml.value, moments, diagG

    def mem_get(self, ptr, count):
        h = np.empty(int(count), dtype=np.float64)
        check(lib().mogp_dev_copy(h.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(ptr), 8 * int(count), 0))
        return h

    def mem_put(self, ptr, arr):
        arr = np.ascontiguousarray(arr, dtype=np.float64)
        check(lib().mogp_dev_copy(ctypes.c_void_p(ptr), arr.ctypes.data_as(ctypes.c_void_p), 8 * arr.size, 1))

    def titsias_fetch(self, which, M):
        """intermediates of the last Titsias gradient evaluation in the device's channel-sorted order (mogp_titsias_fetch): 0 dELBO/dKuu (M x M),
        1 dELBO/dKuf without its rank-one part (M x N), 2 beta (M), 3 r (N), 4 v = L^-1 Kuf (M x N), 5 L (M x M), 6 Qs, 7 Pq = Qs^-1, 8 t1 = Pq v y"""
        shape = {0: (M, M), 1: (M, self.N), 2: (M,), 3: (self.N,), 4: (M, self.N), 5: (M, M), 6: (M, M), 7: (M, M), 8: (M,)}[which]
        out = np.empty(shape)
        check(lib().mogp_titsias_fetch(self._h, int(which), int(M), _dp(out)))
        return out

    def titsias_eval(self, Z, sigma, jitter, kff_diag, grad=True, sharded=False):
        """Titsias bound (+ gradient outputs) through mogp_titsias_eval, or -- this handle holding one shard of the data -- through
        mogp_titsias_eval_sharded (the same result on every rank: the full model's)"""
        Z = _f64(Z)
        kff_diag = _f64(kff_diag)
        M = Z.shape[0]
        C, T, W, D = self.C, self.T, self.W, self.D      # rows of the width set_terms took (2 + 3 D, or 2 + 5 D with an envelope)
        self._check_diag("kff_diag", kff_diag, self.N)
        elbo, trGA, dsig, jit = ctypes.c_double(), ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
        info = ctypes.c_int64(0)
        mom_uu = np.zeros((C * (C + 1) // 2, T, W)) if grad else None
        mom_uf = np.zeros((C * C, T, W)) if grad else None
        gZ = np.zeros((M, D)) if grad else None
        fn = lib().mogp_titsias_eval_sharded if sharded else lib().mogp_titsias_eval
        code = fn(self._h, M, _dp(Z), float(sigma), float(jitter), _dp(kff_diag),
                  MOGP_EVAL_GRAD if grad else 0, ctypes.byref(elbo), _dp(mom_uu), _dp(mom_uf), _dp(gZ),
                  ctypes.byref(trGA), ctypes.byref(dsig), ctypes.byref(jit), ctypes.byref(info))
        check(code, info.value)
        return dict(elbo=elbo.value, mom_uu=mom_uu, mom_uf=mom_uf, gZ=gZ, trGA=trGA.value, dsigma=dsig.value,
                    jitter_abs=jit.value)

    def titsias_predict(self, Z, sigma, jitter, Xs, kss_diag, sharded=False):
        Z, Xs, kss_diag = _f64(Z), _f64(Xs), _f64(kss_diag)
        S = Xs.shape[0]
        self._check_diag("kss_diag", kss_diag, S)
        mu, var = np.empty(S), np.empty(S)
        info = ctypes.c_int64(0)
        fn = lib().mogp_titsias_predict_sharded if sharded else lib().mogp_titsias_predict
        code = fn(self._h, Z.shape[0], _dp(Z), float(sigma), float(jitter), _dp(kss_diag), S, _dp(Xs), _dp(mu), _dp(var), ctypes.byref(info))
        check(code, info.value)
        return mu.reshape(-1, 1), var.reshape(-1, 1)

    def _check_diag(self, name, diag, npoints):
        """K_diag arrays of the sparse / variational entry points: one value per CHANNEL, or -- with enveloped terms (rows of width 2 + 5 D),
        whose diagonal follows the points -- one per point; the C side indexes them accordingly, so the length is checked here"""
        want = npoints if self.W > 2 + 3 * self.D else self.C
        if diag is None or diag.size != want:
            raise ValueError("%s must have %d entries (%s), got %s" % (name, want, "per point: the terms carry an envelope" if want != self.C else "per channel",
                                                                       None if diag is None else diag.size))

    def snelson_eval(self, Z, noise_var, jitter, kff_diag, grad=True, sharded=False):
        """Snelson (FITC) marginal likelihood (+ gradient outputs) through mogp_snelson_eval"""
        Z, noise_var, kff_diag = _f64(Z), _f64(noise_var), _f64(kff_diag)
        M = Z.shape[0]
        C, T, W, D = self.C, self.T, self.W, self.D       # W = 2 + 5 D with enveloped terms: kff_diag per point in, dp/dKff per point out
        env = W > 2 + 3 * D
        if kff_diag.size != (self.N if env else C):
            raise ValueError("kff_diag must have %d entries" % (self.N if env else C))
        lml, trGA, jit = ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
        info = ctypes.c_int64(0)
        mom_uu = np.zeros((C * (C + 1) // 2, T, W)) if grad else None
        mom_uf = np.zeros((C * C, T, W)) if grad else None
        gZ = np.zeros((M, D)) if grad else None
        hsum = np.zeros(self.N if env else C) if grad else None
        fn = lib().mogp_snelson_eval_sharded if sharded else lib().mogp_snelson_eval
        code = fn(self._h, M, _dp(Z), _dp(noise_var), float(jitter), _dp(kff_diag), MOGP_EVAL_GRAD if grad else 0,
                  ctypes.byref(lml), _dp(mom_uu), _dp(mom_uf), _dp(gZ), ctypes.byref(trGA), _dp(hsum), ctypes.byref(jit), ctypes.byref(info))
        check(code, info.value)
        return dict(lml=lml.value, mom_uu=mom_uu, mom_uf=mom_uf, gZ=gZ, trGA=trGA.value, hsum=hsum, jitter_abs=jit.value)

    def snelson_predict(self, Z, noise_var, jitter, Xs, kff_diag, kss_diag, sharded=False):
        Z, Xs, noise_var, kff_diag, kss_diag = _f64(Z), _f64(Xs), _f64(noise_var), _f64(kff_diag), _f64(kss_diag)
        S = Xs.shape[0]
        self._check_diag("kff_diag", kff_diag, self.N)
        self._check_diag("kss_diag", kss_diag, S)
        mu, var = np.empty(S), np.empty(S)
        info = ctypes.c_int64(0)
        fn = lib().mogp_snelson_predict_sharded if sharded else lib().mogp_snelson_predict
        code = fn(self._h, Z.shape[0], _dp(Z), _dp(noise_var), float(jitter), _dp(kff_diag), _dp(kss_diag), S, _dp(Xs),
                  _dp(mu), _dp(var), ctypes.byref(info))
        check(code, info.value)
        return mu.reshape(-1, 1), var.reshape(-1, 1)

    def svgp_forward(self, Z, q_mu, q_sqrt, jitter, kff_diag, Xs=None, kss_diag=None, dense=False):
        """mean / variance of q(f) of the Hensman models at the training inputs (Xs None) or at Xs, through mogp_svgp_forward"""
        Z, q_mu, q_sqrt, kff_diag = _f64(Z), _f64(np.reshape(q_mu, -1)), _f64(q_sqrt), _f64(kff_diag)
        M = Z.shape[0]
        S = 0 if Xs is None else int(np.shape(Xs)[0])
        Xs = None if Xs is None else _f64(Xs)
        kss = None if kss_diag is None else _f64(kss_diag)
        n = self.N if Xs is None else S
        if Xs is None:
            self._check_diag("kff_diag", kff_diag, self.N)
        else:
            self._check_diag("kss_diag", kss, S)
        mu, var = np.empty(n), np.empty(n)
        jit = ctypes.c_double()
        info = ctypes.c_int64(0)
        code = lib().mogp_svgp_forward(self._h, M, _dp(Z), _dp(q_mu), _dp(q_sqrt), float(jitter), _dp(kff_diag), 1 if dense else 0, S,
                                       _dp(Xs), _dp(kss), _dp(mu), _dp(var), ctypes.byref(jit), ctypes.byref(info))
        check(code, info.value)
        self._svgp_M = M
        return dict(mu=mu, var=var, jitter_abs=jit.value)

    def svgp_backward(self, e, f, sharded=False):
        e, f = _f64(np.reshape(e, -1)), _f64(np.reshape(f, -1))
        C, T, W, D, M = self.C, self.T, self.W, self.D, self._svgp_M       # W = 2 + 5 D with enveloped terms
        mom_uu, mom_uf = np.zeros((C * (C + 1) // 2, T, W)), np.zeros((C * C, T, W))
        gZ, g_qmu, g_S = np.zeros((M, D)), np.zeros(M), np.zeros((M, M))
        trGA = ctypes.c_double()
        fn = lib().mogp_svgp_backward_sharded if sharded else lib().mogp_svgp_backward
        check(fn(self._h, _dp(e), _dp(f), _dp(mom_uu), _dp(mom_uf), _dp(gZ), ctypes.byref(trGA), _dp(g_qmu), _dp(g_S)))
        return dict(mom_uu=mom_uu, mom_uf=mom_uf, gZ=gZ, trGA=trGA.value, g_qmu=g_qmu, g_qsqrt=g_S)

    def oa_forward(self, q_nu, q_lambda):
        """mean / variance of q(f) of the Opper-Archambeau model at the training inputs and its `kl` term, through mogp_oa_forward"""
        q_nu, q_lambda = _f64(np.reshape(q_nu, -1)), _f64(np.reshape(q_lambda, -1))
        mu, var = np.empty(self.N), np.empty(self.N)
        kl = ctypes.c_double()
        info = ctypes.c_int64(0)
        check(lib().mogp_oa_forward(self._h, _dp(q_nu), _dp(q_lambda), _dp(mu), _dp(var), ctypes.byref(kl), ctypes.byref(info)), info.value)
        return dict(mu=mu, var=var, kl=kl.value)

    def oa_backward(self, e, f):
        e, f = _f64(np.reshape(e, -1)), _f64(np.reshape(f, -1))
        mom = np.zeros((self.C * (self.C + 1) // 2, self.T, 2 + 3 * self.D))
        g_nu, g_lambda = np.zeros(self.N), np.zeros(self.N)
        check(lib().mogp_oa_backward(self._h, _dp(e), _dp(f), _dp(mom), _dp(g_nu), _dp(g_lambda)))
        return dict(mom=mom, g_nu=g_nu, g_lambda=g_lambda)

    def oa_predict(self, q_nu, q_lambda, kss_diag, Xs, full=False):
        q_nu, q_lambda, kss_diag, Xs = _f64(np.reshape(q_nu, -1)), _f64(np.reshape(q_lambda, -1)), _f64(kss_diag), _f64(Xs)
        S = Xs.shape[0]
        mu, var = np.empty(S), np.empty((S, S) if full else S)
        info = ctypes.c_int64(0)
        check(lib().mogp_oa_predict(self._h, _dp(q_nu), _dp(q_lambda), _dp(kss_diag), S, _dp(Xs), 1 if full else 0, _dp(mu), _dp(var),
                                    ctypes.byref(info)), info.value)
        return mu.reshape(-1, 1), (var if full else var.reshape(-1, 1))

    def sparse_predict_cov(self, S):
        """full S x S covariance of the last sparse prediction on this handle (Titsias / Hensman), through mogp_sparse_predict_cov"""
        cov = np.empty((int(S), int(S)))
        check(lib().mogp_sparse_predict_cov(self._h, int(S), _dp(cov)))
        return cov

    def set_profiling(self, on=True):
        check(lib().mogp_set_profiling(self._h, 1 if on else 0))

    def stage_ms(self):
        ms = np.zeros(ST_COUNT)
        n = ctypes.c_int64(0)
        fl = ctypes.c_double(0)
        check(lib().mogp_stage_ms(self._h, _dp(ms), ctypes.byref(n), ctypes.byref(fl)))
        return ms, n.value, fl.value

    def shard_stage_ms(self):
        """(exchange on the critical stream, serial, next_cols, bulk, exchange on the communication stream, the critical stream's wait for it) ms of the
        last profiled sharded evaluation"""
        ms = np.zeros(6)
        check(lib().mogp_shard_stage_ms(self._h, _dp(ms)))
        return ms

    def schedule(self):
        """-> dict(dataflow, chain_kernel, dataflow_fell_back, chain_fell_back, dataflow_timeouts): how the last gradient evaluation was scheduled (mogp_model_schedule)"""
        f = ctypes.c_int(0)
        check(lib().mogp_model_schedule(self._h, ctypes.byref(f)))
        return dict(dataflow=bool(f.value & 1), chain_kernel=bool(f.value & 2), dataflow_fell_back=bool(f.value & 4), chain_fell_back=bool(f.value & 8),
                    dataflow_timeouts=(f.value >> 8) & 0xffff)

    def flow_diag(self):
        """-> dict of the dataflow schedule's deep-look counters over this model's life (mogp_model_flow_diag)"""
        out = (ctypes.c_uint * 8)()
        check(lib().mogp_model_flow_diag(self._h, out))
        return dict(deep_looks=out[0], stale_heads=out[1], stale_counters=out[2], deep_polls=out[3], stale_polls=out[4], last=(out[5], out[6], out[7] & 0xffff, out[7] >> 16))

    def flow_replay(self, on):
        """measurement mode (mogp_model_flow_replay): the next gradient evaluations run the dataflow kernel alone on the replay plan"""
        check(lib().mogp_model_flow_replay(self._h, 1 if on else 0))

    accurate_mode = False          # what the last set_accurate asked for (a NEW handle starts in the fast mode, as the device object does)

    def set_accurate(self, on):
        """gradient evaluations in the backward-stable form (mogp_model_set_accurate): slower, for ill-conditioned Kj"""
        check(lib().mogp_model_set_accurate(self._h, 1 if on else 0))
        self.accurate_mode = bool(on)

    def condition_estimate(self):
        """(largest / smallest diagonal entry of L)^2 of the last factorisation: a lower estimate of cond(Kj); nan when it was not reported"""
        lo, hi = np.zeros(1), np.zeros(1)
        check(lib().mogp_model_pivot_range(self._h, _dp(lo), _dp(hi)))
        return float((hi[0] / lo[0]) ** 2) if lo[0] > 0.0 else float("nan")

    def work_bytes(self):
        """(bytes of the N x N work matrix this handle has physical memory for, bytes of the whole matrix): a rank of a sharded evaluation holds its own
        tile rows only (mogp_model_work_bytes)"""
        b, w = ctypes.c_int64(0), ctypes.c_int64(0)
        check(lib().mogp_model_work_bytes(self._h, ctypes.byref(b), ctypes.byref(w)))
        return int(b.value), int(w.value)

    def inverse_fraction(self):
        """fraction of the lower tiles of Kj^-1 the last gradient evaluation formed (1.0 = all; see include/mogp_hip.h)"""
        f = np.zeros(1)
        check(lib().mogp_model_inverse_fraction(self._h, _dp(f)))
        return float(f[0])

    def strip_runs(self, which=0):
        """-> dict(ncu, runs, rest, longest) of one of the handle's strip lists as it stands (mogp_model_strip_runs): which 0 the training Gram's,
        1 / 2 its head / tail lists, 3 the owned list, 4 the sparse models' (Z, X) list; ncu -1: never built"""
        out = np.zeros(4, dtype=np.int64)
        check(lib().mogp_model_strip_runs(self._h, int(which), out.ctypes.data_as(c_i64p)))
        return dict(ncu=int(out[0]), runs=int(out[1]), rest=int(out[2]), longest=int(out[3]))

    def gram_probe(self, noise_var, jitter, data_var=None):
        """Kj as the exact path writes it before factoring it (mogp_model_gram): N x N in channel-sorted order, lower triangle, zeros above"""
        out = np.empty((self.N, self.N))
        check(lib().mogp_model_gram(self._h, _dp(_f64(noise_var)), _dp(_f64(data_var)), float(jitter), _dp(out)))
        return out

    def fetch(self, which):
        out = np.empty(2 if which == 4 else self.N if which in (2, 3) else (self.N, self.N))
        check(lib().mogp_model_fetch(self._h, which, _dp(out)))
        return out
