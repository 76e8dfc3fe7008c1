"""
Kernel base classes for the HIP path -- host-side mirror of mogptk/gpr/kernel.py.

A kernel on this path does two things on the host (O(C^2 Q) scalars) and nothing else:
  * `_spectral_terms(D)`   : constrained parameters -> unified spectral term table
                              [C, C, T, 2+3D] = [A, Psi, V_d.., M_d.., Delta_d..]   
  * `_spectral_kinds(D)`   : the radial profile of every (pair, term) -- all Gaussian unless a stationary kernel of gpr/singleoutput.py is inside
  * `_spectral_backward(g)`: d loss / d table  ->  `.grad` on every raw parameter (the chain rule the
                              reference gets from autograd through gpr/multioutput.py:182-199 etc.)
All O(N^2) / O(N^3) work (Gram build, Cholesky, solves, gradient moments) runs in the HIP library
behind the C ABI (include/mogp_hip.h).  There is no CPU fallback.
"""
import copy
import numpy as np

from .config import config
from .parameter import Parameter, ParameterHolder


def term_width(D):
    return 2 + 3 * D


def env_width(D):
    """rows with a Gaussian envelope on the input midpoint: [A, Psi, V_d, M_d, Delta_d, L_d, c_d]"""
    return 2 + 5 * D


def pad_width(table, width):
    """a table of the narrow row width as one of the wide width (no envelope: L = 0)"""
    if table.shape[3] == width:
        return table
    out = np.zeros(table.shape[:3] + (width,))
    out[..., :table.shape[3]] = table
    return out


# Product groups: a row whose kind carries KIND_TIMES multiplies with the next row; a maximal run of flagged rows plus the row that
# ends it is a group of at most GROUP_MAX rows, and the kernel is the sum over groups of the product of their rows.  The low bits stay the profile.
KIND_TIMES, KIND_MASK, GROUP_MAX = 1 << 8, 0xff, 4
# The dot-product row (A <x_a, x_b> + c)^n of LinearKernel / PolynomialKernel: A in the amplitude slot, the bias c in the Psi slot, n the shape.
# It is the one row whose diagonal value follows the point, (A |x|^2 + c)^n, instead of being its amplitude.
KIND_DOT = 7
# The gate row A h(x_a) h(x_b), h(x) = sigmoid(beta (x - l)), of ChangePointsKernel: the signed steepness beta in the V slot, the location l in
# the M slot, A = 1 (one input dimension).  Its diagonal value A h(x)^2 follows the point too: both are "point rows".
KIND_GATE = 8
# The weighted-dot row A sum_d V_d x_a,d x_b,d of FunctionKernel: the basis functions' values are input columns of their own behind the
# model's inputs, V holds the weights on those columns; its diagonal A sum_d V_d x_d^2 follows the point.  The white row of WhiteKernel: A
# where row and column are the same point of the same set, 0 elsewhere; its diagonal is A, like a profile's.
KIND_WDOT, KIND_WHITE = 9, 10
POINT_KINDS = (KIND_DOT, KIND_GATE, KIND_WDOT)
MAXD = 8                                                    # input columns of the device (MOGP_MAXD), feature columns included


def _sigmoid(z):
    """1 / (1 + exp(-z)) without overflow for any finite z; the complement 1 - sigmoid(z) is _sigmoid(-z)"""
    e = np.exp(-np.abs(z))
    return np.where(z >= 0, 1.0, e) / (1.0 + e)


def group_slices(kind_row):
    """[(first, last + 1)] of the groups of one (channel pair)'s kind row"""
    out, t0 = [], 0
    for t, k in enumerate(kind_row):
        if not (int(k) & KIND_TIMES) or t == len(kind_row) - 1:
            out.append((t0, t + 1))
            t0 = t + 1
    return out


def group_diag(A, kind_row):
    """sum over groups of the product of the rows' amplitudes: the diagonal K(x, x) of a pair whose profiles are 1 at zero distance"""
    return float(sum(np.prod(A[a:b]) for a, b in group_slices(kind_row)))


def group_diag_grad(A, kind_row):
    """d group_diag / d A_t: the product of the OTHER rows of t's group (1 for a group of one)"""
    g = np.ones(len(A))
    for a, b in group_slices(kind_row):
        for t in range(a, b):
            g[t] = np.prod(np.delete(A[a:b], t - a))
    return g


PROFILE_PSI0 = {0: 1.0, 1: 1.0, 3: 3.0, 4: 5.0 / 3.0, 6: np.pi ** 2 / 3.0}      # psi(0) = -2 dphi/ds at s = 0: Gaussian, RQ, Matern 3/2, Matern 5/2, sinc
KIND_NAMES = {2: "Matern 1/2 (exponential)", KIND_GATE: "gate (change-point)", KIND_WDOT: "weighted-dot (FunctionKernel)", KIND_WHITE: "white"}


def deriv_diag(table, kind, shape, Xk, D):
    """kappa (S, D): the prior variance of df/dx_d at every point of Xk (channel column first), kappa_d(x) = d^2 K(x, x')/dx_d dx'_d at x = x'
    (DESIGN 1f), from the diagonal pair (c, c) of the point's channel.  Each row brings its quadruple (k, d_a k, d_b k, d_a d_b k) at coincident
    inputs and a product group multiplies them by the product rule -- the cross terms d_a k_h d_b k_g, which vanish unless two point rows share
    a group, included.  The diagonal pairs carry no delay and no phase (u = 0, theta = 0 at coincident inputs)."""
    table, Xk = np.asarray(table, dtype=np.float64), np.asarray(Xk, dtype=np.float64)
    S, env = Xk.shape[0], table.shape[3] > 2 + 3 * D
    x, ch = Xk[:, 1:1 + D], Xk[:, 0].astype(np.int64)
    out = np.zeros((S, D))
    for c in np.unique(ch):
        rows = np.nonzero(ch == c)[0]
        xc, tab, kd = x[rows], table[c, c], np.asarray(kind[c, c])
        if np.any(tab[:, 1][(kd & KIND_MASK) != KIND_DOT] != 0.0) or np.any(tab[:, 2 + 2 * D:2 + 3 * D] != 0.0):
            raise NotImplementedError("the derivative's prior variance is written for diagonal channel pairs without a delay or a phase")
        for a, b in group_slices(kd):
            quad = None
            for t in range(a, b):
                r, k = tab[t], int(kd[t]) & KIND_MASK
                A, V, M = r[0], r[2:2 + D], r[2 + D:2 + 2 * D]
                if k == KIND_DOT:
                    n = int(shape[c, c, t])
                    bb = A * np.sum(xc * xc, axis=1, keepdims=True) + r[1]
                    p1 = n * bb ** (n - 1) if n > 1 else np.ones_like(bb)
                    p2 = n * (n - 1) * bb ** (n - 2) if n > 1 else np.zeros_like(bb)
                    q = (np.broadcast_to(bb ** n, xc.shape), p1 * A * xc, p1 * A * xc, p2 * A * A * xc * xc + p1 * A)
                elif k == 5:                                # periodic: exp(V_0 (cos theta - 1))
                    one = np.ones_like(xc)
                    q = (A * one, 0.0 * one, 0.0 * one, A * V[0] * (2.0 * np.pi * M) ** 2 * one)
                elif k in PROFILE_PSI0:
                    kv = A * np.ones((len(rows), 1))
                    d1, d2 = np.zeros_like(xc), V * PROFILE_PSI0[k] + (2.0 * np.pi * M) ** 2
                    if env:                                 # the envelope sits on the midpoint: a = x - c at coincident inputs
                        Lv, mid = r[2 + 3 * D:2 + 4 * D], xc - r[2 + 4 * D:2 + 5 * D]
                        kv = kv * np.exp(-0.5 * np.sum(Lv * mid * mid, axis=1, keepdims=True))
                        d1 = -0.5 * Lv * mid * kv
                        d2 = d2 + 0.25 * (Lv * Lv * mid * mid - Lv)
                    q = (np.broadcast_to(kv, xc.shape), d1, d1, kv * d2)
                else:
                    raise NotImplementedError("a %s row has no derivative on this path" % KIND_NAMES.get(k, "kind-%d" % k))
                quad = q if quad is None else (quad[0] * q[0], quad[1] * q[0] + quad[0] * q[1], quad[2] * q[0] + quad[0] * q[2],
                                               quad[3] * q[0] + quad[1] * q[2] + quad[2] * q[1] + quad[0] * q[3])
            out[rows] += quad[3]
    return out


# One evaluation asks every kernel of a composition for its term table several times (push to the device, then again at each level
# of the chain rule -- AddKernel even asks only to learn T) while no parameter can change.  A model evaluation opens this cache.
_TERMS_CACHE = None


class terms_cache:
    """context: memoise `_spectral_terms` per kernel object for the duration of ONE model evaluation (tables are shared: read-only)"""

    def __enter__(self):
        global _TERMS_CACHE
        self._prev = _TERMS_CACHE
        _TERMS_CACHE = {}
        return self

    def __exit__(self, *exc):
        global _TERMS_CACHE
        _TERMS_CACHE = self._prev
        return False


def cached_terms(fn):
    name = fn.__name__

    def wrapper(self, D):
        cache = _TERMS_CACHE
        if cache is None:
            return fn(self, D)
        key = (id(self), D, name)
        if key not in cache:
            cache[key] = fn(self, D)
        return cache[key]
    wrapper.__doc__ = fn.__doc__
    return wrapper


class Kernel(ParameterHolder):
    """Base kernel (reference gpr/kernel.py:5-191)."""

    def __init__(self, input_dims=None, active_dims=None):
        if active_dims is not None:
            raise NotImplementedError("active_dims is not on the HIP path")
        self.input_dims = input_dims
        self.active_dims = None
        self.output_dims = None

    def name(self):
        return self.__class__.__name__

    def __setattr__(self, name, val):
        if name == "train":
            for p in self.parameters():
                p.train = val
            return
        super().__setattr__(name, val)

    def __call__(self, X1, X2=None):
        """validate + K, reference gpr/kernel.py:23-35"""
        X1, X2 = self._check_input(X1, X2)
        return self.K(X1, X2)

    def _check_input(self, X1, X2=None):
        """reference gpr/kernel.py:60-80"""
        X1 = np.asarray(X1.detach().cpu().numpy() if hasattr(X1, "detach") else X1, dtype=np.float64)
        if X1.ndim != 2:
            raise ValueError("X should have two dimensions (data_points,input_dims)")
        if X1.shape[0] == 0 or X1.shape[1] == 0:
            raise ValueError("X must not be empty")
        if X2 is not None:
            X2 = np.asarray(X2.detach().cpu().numpy() if hasattr(X2, "detach") else X2, dtype=np.float64)
            if X2.ndim != 2:
                raise ValueError("X should have two dimensions (data_points,input_dims)")
            if X2.shape[0] == 0:
                raise ValueError("X must not be empty")
            if X1.shape[1] != X2.shape[1]:
                raise ValueError("input dimensions for X1 and X2 must match")
        return X1, X2

    def _check_kernels(self, kernels, length=None):
        """Normalise what a combinator was given -- one kernel, several, or one list (reference gpr/kernel.py:82-110, same messages) -- into a
        list of `length` kernels that agree on input and output dimensions; a single kernel is cloned up to `length`."""
        if isinstance(kernels, tuple):
            items = list(kernels[0]) if (len(kernels) == 1 and isinstance(kernels[0], list)) else list(kernels)
        else:
            items = kernels if isinstance(kernels, list) else [kernels]
        if not items:
            raise ValueError("must pass at least one kernel")
        if length is not None and len(items) != length:
            if len(items) > 1:
                raise ValueError("must pass %d kernels" % length)
            items = items + [items[0].clone() for _ in range(length - 1)]
        if not all(isinstance(k, Kernel) for k in items):
            raise ValueError("must pass kernels")
        if len({k.input_dims for k in items}) > 1:
            raise ValueError("kernels must have same input dimensions")
        if len({k.output_dims for k in items if k.output_dims is not None}) > 1:
            raise ValueError("multi-output kernels must have same output dimensions")
        return items

    def clone(self):
        return copy.deepcopy(self)

    def iterkernels(self):
        yield self

    # -- the HIP seam ------------------------------------------------------------------------
    def _channels(self):
        """number of channels the device sees (single-output kernels run as one implicit channel)"""
        return 1 if self.output_dims is None else self.output_dims

    def _kernel_format(self, X):
        """single-output kernels have no channel column: prepend channel 0.  Behind the inputs: the feature columns phi_k(x) of every
        distinct FunctionKernel leaf, in leaf order (none: the array as it was)"""
        if self.output_dims is None:
            X = np.concatenate([np.zeros((X.shape[0], 1)), X], axis=1)
        leaves = self._feature_leaves()
        if not leaves:
            return X
        x = X[:, 1:]
        return np.concatenate([X] + [k._phi_values(x) for k in leaves], axis=1)

    # -- feature columns (FunctionKernel): the composition's table, kinds and gradient keep the kernels' own D; the device sees D + F
    def _feature_leaves(self):
        """the distinct FunctionKernel leaves of the composition in leaf order; each learns the offset of its columns among the feature columns"""
        out = []

        def walk(k):
            if hasattr(k, "_phi_values") and not any(k is o for o in out):
                out.append(k)
            for s in getattr(k, "kernels", None) or []:
                walk(s)
        walk(self)
        off = 0
        for k in out:
            k._feature_offset = off
            off += k._features()
        return out

    def _device_terms(self, Dd):
        """(table, kind, shape, D) for inputs of Dd device columns: the composition's own D = Dd - F, its kinds and shapes, and its table re-laid
        to Dd columns -- V, M, Delta widened with zeros, and the magnitude of its leaf in the V slots of every weighted-dot row.  Without a
        FunctionKernel: the kernel's own arrays.  What the device cannot carry is refused here, before any device call."""
        leaves = self._feature_leaves()
        F = sum(k._features() for k in leaves)
        D = Dd - F
        if leaves and Dd > MAXD:
            raise NotImplementedError("the basis functions of a FunctionKernel travel as input columns: %d input dimension%s and %d features make %d "
                                      "columns, the device takes %d; use fewer basis functions (sum features that share a weight inside phi)"
                                      % (D, "" if D == 1 else "s", F, Dd, MAXD))
        table = self._spectral_terms(D)
        kind, shape = self._spectral_kinds(D)
        if not leaves:
            return table, kind, shape, D
        kd = kind & KIND_MASK
        if np.any(kd == KIND_DOT):
            raise NotImplementedError("LinearKernel / PolynomialKernel beside a FunctionKernel is not on the MI355X spectral path: the dot-product "
                                      "row sums over every input column of the device, the feature columns included; put x among the features "
                                      "instead (phi = [x, ...] is the linear kernel)")
        if np.any(kd == KIND_GATE):
            raise NotImplementedError("ChangePointsKernel in a model that holds a FunctionKernel is not on the MI355X spectral path: gate rows take "
                                      "one input column on the device; weigh the basis functions by the sigmoid inside phi instead")
        if table.shape[3] > term_width(D):
            raise NotImplementedError("a sum of enveloped (harmonizable) terms and a FunctionKernel is not on the HIP path")
        wide = np.zeros(table.shape[:3] + (term_width(Dd),))
        wide[..., :2] = table[..., :2]
        for b in range(3):
            wide[..., 2 + b * Dd:2 + b * Dd + D] = table[..., 2 + b * D:2 + (b + 1) * D]
        for k in leaves:
            rows = (kd == KIND_WDOT) & (shape == k._feature_offset)
            c0 = 2 + D + k._feature_offset
            wide[rows, c0:c0 + k._features()] = np.reshape(k.magnitude(), -1)
        return wide, kind, shape, D

    def _table_backward(self, gtable):
        """d loss / d (the table `_device_terms` returned) -> `.grad`: a weighted-dot row's V columns on its leaf's feature columns are
        d / d magnitude (every copy of the row accumulates), the rest narrows back to the kernels' own columns for `_spectral_backward`"""
        leaves = self._feature_leaves()
        if not leaves:
            return self._spectral_backward(gtable)
        F = sum(k._features() for k in leaves)
        Dd = (gtable.shape[3] - 2) // 3
        D = Dd - F
        kind, shape = self._spectral_kinds(D)
        kd = kind & KIND_MASK
        for k in leaves:
            rows = (kd == KIND_WDOT) & (shape == k._feature_offset)
            c0 = 2 + D + k._feature_offset
            k.magnitude.accumulate_grad(np.reshape(np.sum(gtable[rows][:, c0:c0 + k._features()], axis=0), k.magnitude.data.shape))
        own = np.zeros(gtable.shape[:3] + (term_width(D),))
        own[..., :2] = gtable[..., :2]
        for b in range(3):
            own[..., 2 + b * D:2 + (b + 1) * D] = gtable[..., 2 + b * Dd:2 + b * Dd + D]
        self._spectral_backward(own)

    def _spectral_terms(self, D):
        raise NotImplementedError("%s is not on the MI355X spectral path (MOSM / SM / CSM are)" % self.name())

    def _spectral_backward(self, gtable):
        raise NotImplementedError("%s is not on the MI355X spectral path" % self.name())

    def _spectral_kinds(self, D):
        """(kind [C, C, T] int32, shape [C, C, T] float64): the radial profile phi_kind(s), s = sum_d V_d u_d^2, that stands where the Gaussian
        exp(-s/2) stands in each (channel pair, term) of `_spectral_terms(D)` (the KIND_* values of gpr/singleoutput.py), and its shape
        parameter.  Default: all Gaussian."""
        shape = self._spectral_terms(D).shape[:3]
        return np.zeros(shape, dtype=np.int32), np.zeros(shape)

    def _radial(self, D):
        """some term has a non-Gaussian profile: only then do kinds travel to the device"""
        return bool(np.any(self._spectral_kinds(self._own_dims(D))[0]))

    def _pointwise(self, D):
        """some row is a point row (dot product, gate): K(x, x) follows the point, as with an envelope, and `_point_diag` stands where
        `_spectral_diag` stood"""
        return bool(np.any(np.isin(self._spectral_kinds(self._own_dims(D))[0] & KIND_MASK, POINT_KINDS)))

    def _own_dims(self, D):
        """the composition's own input dimensions when D counts the feature columns of its FunctionKernel leaves as well (D itself otherwise)"""
        F = sum(k._features() for k in self._feature_leaves())
        return D - F if F and self.input_dims is not None and D == self.input_dims + F else D

    def _spectral_diag(self, D):
        """K_diag value per channel AS THE REFERENCE RETURNS IT (constant per channel for every spectral kernel).
        Default: the true diagonal sum_t A_cct (Delta = Psi = 0 on i == j blocks), over product groups the sum of their amplitudes' products;
        SM overrides (its K_diag differs from diag K when D > 1, reference singleoutput.py:602-605)."""
        table = self._spectral_terms(D)
        C = table.shape[0]
        kind = self._spectral_kinds(D)[0]
        if np.any(kind & KIND_TIMES):
            return np.array([group_diag(table[c, c, :, 0], kind[c, c]) for c in range(C)])
        return np.array([np.sum(table[c, c, :, 0]) for c in range(C)])

    def _spectral_diag_backward(self, gc, D):
        """accumulate d loss / d K_diag[c] = gc[c] (K_diag as `_spectral_diag` defines it) into the raw gradients.
        Default: K_diag[c] = sum_t A_cct (over groups: the product rule), so it is a table gradient on the diagonal amplitudes."""
        table = self._spectral_terms(D)
        gt = np.zeros_like(table)
        for c in range(table.shape[0]):
            gt[c, c, :, 0] = gc[c]
        self._spectral_backward(gt * _table_diag_weights(table, self._spectral_kinds(D)[0]))

    def _parts(self, D):
        """[(name, mask)]: the default partition of the kernel into addends, one level deep -- mask boolean (C, C, T) over the rows of
        `_spectral_terms(D)`.  Default: one part, the whole kernel"""
        return [(self.name(), np.ones(self._spectral_terms(D).shape[:3], dtype=bool))]

    def _row_parts(self, D, names, bounds):
        """parts that are consecutive row ranges of the table, the same in every channel pair: part i holds rows bounds[i] .. bounds[i + 1] - 1"""
        shape = self._spectral_terms(D).shape[:3]
        out = []
        for i, name in enumerate(names):
            mask = np.zeros(shape, dtype=bool)
            mask[:, :, bounds[i]:bounds[i + 1]] = True
            out.append(("%d:%s" % (i, name), mask))
        return out

    def _product_refusal(self):
        """why this kernel cannot be a factor of a MulKernel on this path (None: it can)"""
        if self.output_dims is not None:
            return "a product of multi-output kernels is not on the MI355X spectral path: MulKernel multiplies single-output kernels"
        return None

    def K(self, X1, X2=None):
        """Kernel matrix, reference gpr/kernel.py:138-150 (MO: :446-481).  Runs the HIP Gram builder."""
        from .._lib import gram
        X1k = self._kernel_format(np.asarray(X1, dtype=np.float64))
        X2k = None if X2 is None else self._kernel_format(np.asarray(X2, dtype=np.float64))
        D = X1k.shape[1] - 1                                      # the device's columns: the feature columns of a FunctionKernel included
        with terms_cache():
            table, kind, shape, _ = self._device_terms(D)
        if not np.any(kind):
            return gram(config.device, self._channels(), D, table, X1k, X2k)
        if table.shape[3] > term_width(D):
            raise NotImplementedError("a sum of enveloped (harmonizable) terms and non-Gaussian stationary kernels is not on the HIP path")
        return gram(config.device, self._channels(), D, table, X1k, X2k, kind, shape)

    def K_diag(self, X1):
        """reference gpr/kernel.py:152-163, MO :483-495.  Constant per channel for every stationary spectral kernel; with an
        envelope (MOHSM) it follows the points."""
        X1k = self._kernel_format(np.asarray(X1, dtype=np.float64))
        Dd = X1k.shape[1] - 1
        table, _, _, D = self._device_terms(Dd)
        if table.shape[3] > term_width(Dd) or self._pointwise(D):
            return self._point_diag(table, X1k, Dd)
        return self._spectral_diag(D)[X1k[:, 0].astype(np.int64)]

    @staticmethod
    def _point_env(table, Xk, D):
        """per point k (channel c) and term t: the envelope exp(-1/2 sum_d L_d (x_k,d - c_d)^2) of the diagonal pair (c, c), and x - c"""
        c = Xk[:, 0].astype(np.int64)
        rows = table[c, c]                                        # (N, T, W)
        Lv, cn = rows[..., 2 + 3 * D:2 + 4 * D], rows[..., 2 + 4 * D:2 + 5 * D]
        a = Xk[:, None, 1:] - cn                                  # (N, T, D)
        return np.exp(-0.5 * np.sum(Lv * a * a, axis=2)), a, rows

    def _point_rows(self, table, Xk, D):
        """From a table with kinds (no envelope), per point k (channel c) and row t of the diagonal pair (c, c): the row's value v on the
        diagonal -- its amplitude (every profile is 1 at zero distance, Delta = Psi = 0 there), for a dot-product row (A |x|^2 + c)^n, for
        a gate row A h(x)^2, for a weighted-dot row A sum_d V_d x_d^2 -- with dv / d(table column) for the columns that move it (N, T, W: the
        amplitude; the bias in a dot-product row's Psi slot; beta and l in a gate row's V and M slots; a weighted-dot row's V slots), and the
        groups, which are the same in every pair.  `table`, `Xk` and `D` are the device's (`_device_terms`): the feature columns included"""
        kind, shape = self._spectral_kinds(D - sum(k._features() for k in self._feature_leaves()))
        c = Xk[:, 0].astype(np.int64)
        rows = table[c, c]                                        # (N, T, W)
        kd = kind[c, c] & KIND_MASK
        dot, gate = kd == KIND_DOT, kd == KIND_GATE
        x2 = np.sum(np.square(Xk[:, 1:]), axis=1)[:, None]
        n = np.where(dot, shape[c, c], 1.0)
        b = np.where(dot, rows[..., 0] * x2 + rows[..., 1], 1.0)
        db = n * b ** (n - 1.0)
        v, dv = np.where(dot, b ** n, rows[..., 0]), np.zeros(rows.shape)
        dv[..., 0], dv[..., 1] = np.where(dot, db * x2, 1.0), np.where(dot, db, 0.0)
        if np.any(gate):                                          # h = sigmoid(beta (x - l)), dh/dz = h (1 - h); one input dimension
            A, beta, a = rows[..., 0], rows[..., 2], Xk[:, 1:2] - rows[..., 2 + D]
            z = np.where(gate, beta * a, 0.0)
            h2, hc = np.square(_sigmoid(z)), _sigmoid(-z)
            v = np.where(gate, A * h2, v)
            dv[..., 0] = np.where(gate, h2, dv[..., 0])
            dv[..., 2] = np.where(gate, 2.0 * A * h2 * hc * a, 0.0)
            dv[..., 2 + D] = np.where(gate, -2.0 * A * h2 * hc * beta, 0.0)
        wdot = kd == KIND_WDOT
        if np.any(wdot):
            xx = np.square(Xk[:, None, 1:])                          # (N, 1, D)
            q = np.sum(rows[..., 2:2 + D] * xx, axis=2)
            v = np.where(wdot, rows[..., 0] * q, v)
            dv[..., 0] = np.where(wdot, q, dv[..., 0])
            dv[..., 2:2 + D] = np.where(wdot[..., None], rows[..., 0:1] * xx, dv[..., 2:2 + D])
        return v, dv, group_slices(kind[0, 0])

    def _point_diag(self, table, Xk, D):
        """K_diag per point.  Enveloped term table: sum_t A_cct env_t(x)   (Delta = Psi = 0 on diagonal pairs); a table with kinds: the sum
        over groups of the product of the rows' diagonal values at the point (`_point_rows`)"""
        if table.shape[3] == term_width(D):
            v, _, groups = self._point_rows(table, Xk, D)
            return sum(np.prod(v[:, a:b], axis=1) for a, b in groups)
        env, _, rows = self._point_env(table, Xk, D)
        return np.sum(rows[..., 0] * env, axis=1)

    def _point_diag_table_grad(self, table, Xk, D, weights=None):
        """d [ sum_k w_k K_diag(x_k) ] / d table (w = 1: what the relative jitter, gpr/model.py:244, contributes per unit of d/d mean(diag) * N)"""
        if table.shape[3] == term_width(D):                     # kinds: the product rule inside a group; amplitude, a dot-product row's bias, a gate row's beta and l
            v, dv, groups = self._point_rows(table, Xk, D)
            w = np.ones(len(Xk)) if weights is None else np.asarray(weights, dtype=np.float64).reshape(-1)
            c = Xk[:, 0].astype(np.int64)
            gt = np.zeros_like(table)
            cols = [col for col in range(table.shape[3]) if col < 2 or np.any(dv[..., col])]
            for a, b in groups:
                for t in range(a, b):
                    others = w * np.prod(np.delete(v[:, a:b], t - a, axis=1), axis=1)
                    for col in cols:
                        gt[:, :, t, col][np.diag_indices(table.shape[0])] = np.bincount(c, weights=others * dv[:, t, col], minlength=table.shape[0])
            return gt
        env, a, rows = self._point_env(table, Xk, D)
        if weights is not None:
            env = env * np.asarray(weights, dtype=np.float64).reshape(-1, 1)
        c = Xk[:, 0].astype(np.int64)
        gt = np.zeros_like(table)
        A, Lv = rows[..., 0], rows[..., 2 + 3 * D:2 + 4 * D]
        for ch in range(table.shape[0]):
            k = c == ch
            if not np.any(k):
                continue
            gt[ch, ch, :, 0] = np.sum(env[k], axis=0)
            gt[ch, ch, :, 2 + 3 * D:2 + 4 * D] = np.sum((A[k] * env[k])[..., None] * (-0.5 * a[k] * a[k]), axis=0)
            gt[ch, ch, :, 2 + 4 * D:2 + 5 * D] = np.sum((A[k] * env[k])[..., None] * (Lv[k] * a[k]), axis=0)
        return gt

    def _point_diag_input_grad(self, table, Xk, D):
        """d K_diag(x_k) / d x_k,d per point: sum_t A env_t(x) (-L_d (x_d - c_d))   (N, D)"""
        env, a, rows = self._point_env(table, Xk, D)
        A, Lv = rows[..., 0], rows[..., 2 + 3 * D:2 + 4 * D]
        return np.sum((A * env)[..., None] * (-Lv * a), axis=1)

    def __add__(self, other):
        return AddKernel(self, other)

    def __mul__(self, other):
        return MulKernel(self, other)


class Kernels(Kernel):
    """Base kernel for list of kernels (reference gpr/kernel.py:193-230)."""

    def __init__(self, *kernels):
        super().__init__()
        kernels = self._check_kernels(kernels)
        i = 0
        while i < len(kernels):
            if isinstance(kernels[i], self.__class__):
                subkernels = list(kernels[i].kernels)
                kernels = kernels[:i] + subkernels + kernels[i + 1:]
                i += len(subkernels) - 1
            i += 1
        self.kernels = list(kernels)
        self.input_dims = kernels[0].input_dims
        output_dims = [kernel.output_dims for kernel in kernels if kernel.output_dims is not None]
        self.output_dims = None if len(output_dims) == 0 else output_dims[0]
        if any(k.output_dims != self.output_dims for k in kernels):
            raise NotImplementedError("mixing single- and multi-output kernels is not on the HIP path")

    def name(self):
        return "[%s]" % (",".join(kernel.name() for kernel in self.kernels),)

    def __getitem__(self, key):
        return self.kernels[key]

    def iterkernels(self):
        yield self
        for kernel in self.kernels:
            yield kernel


class AddKernel(Kernels):
    """Sum of kernels (reference gpr/kernel.py:232-246).  On the spectral path a sum of kernels is the
    concatenation of their term tables along T -- one fused pass instead of Q stacked N x N Grams (:243)."""

    def _spectral_diag(self, D):
        return sum(k._spectral_diag(D) for k in self.kernels)          # :245-246

    def _spectral_diag_backward(self, gc, D):
        for k in self.kernels:
            k._spectral_diag_backward(gc, D)

    @cached_terms
    def _spectral_terms(self, D):
        tabs = [k._spectral_terms(D) for k in self.kernels]
        width = max(t.shape[3] for t in tabs)                     # a sum with an enveloped kernel: everything in the wide rows
        return np.concatenate([pad_width(t, width) for t in tabs], axis=2)

    @cached_terms
    def _spectral_kinds(self, D):
        parts = [k._spectral_kinds(D) for k in self.kernels]       # along T, as the tables
        return np.concatenate([p[0] for p in parts], axis=2), np.concatenate([p[1] for p in parts], axis=2)

    def _parts(self, D):
        """one part per sub-kernel: its slice along T"""
        T = [k._spectral_terms(D).shape[2] for k in self.kernels]
        return self._row_parts(D, [k.name() for k in self.kernels], np.concatenate([[0], np.cumsum(T)]).astype(int))

    def _spectral_backward(self, gtable):
        t0 = 0
        D = self.input_dims if self.input_dims is not None else (gtable.shape[3] - 2) // 3
        for k in self.kernels:
            tab = k._spectral_terms(D)
            T = tab.shape[2]
            k._spectral_backward(gtable[:, :, t0:t0 + T, :tab.shape[3]])
            t0 += T


def _table_diag_weights(table, kind):
    """[C, C, T, 1] factor of the amplitude column's gradient when d/d(diagonal of pair (c, c)) is spread over its rows: 1 for plain rows, the
    product of the group's other amplitudes inside a product group"""
    w = np.ones(table.shape[:3] + (1,))
    if np.any(kind & KIND_TIMES):
        for c in range(table.shape[0]):
            w[c, c, :, 0] = group_diag_grad(table[c, c, :, 0], kind[c, c])
    return w


class MulKernel(Kernels):
    """Product of single-output kernels (reference gpr/kernel.py:248-262).  Every factor is a sum of groups of table rows (a plain kernel: groups
    of one); the product is the sum over the Cartesian product of the factors' groups, each combination ONE group of the concatenated rows --
    (a + b) * c = a * c + b * c.  The device multiplies the rows of a group entry by entry; at most GROUP_MAX rows per group."""

    def _plan(self, D):
        """(tables, kinds, shapes of the factors, [(factor, row)] of every produced row, flags of every produced row)"""
        for k in self.kernels:
            why = k._product_refusal()
            if why is not None:
                raise NotImplementedError(why)
        tabs = [k._spectral_terms(D) for k in self.kernels]
        if any(t.shape[0] != 1 or t.shape[3] != term_width(D) for t in tabs):
            raise NotImplementedError("a product with enveloped (harmonizable) terms is not on the MI355X spectral path")
        kinds = [k._spectral_kinds(D) for k in self.kernels]
        combos = [[]]
        for f, (kd, _) in enumerate(kinds):
            groups = [[(f, t) for t in range(a, b)] for a, b in group_slices(kd[0, 0])]
            combos = [c + g for c in combos for g in groups]
        rows, flags = [], []
        for c in combos:
            if len(c) > GROUP_MAX:
                raise NotImplementedError("a product of more than %d table rows (%s: %d) is not on the MI355X spectral path: the device multiplies "
                                          "groups of at most %d rows" % (GROUP_MAX, self.name(), len(c), GROUP_MAX))
            rows += c
            flags += [KIND_TIMES] * (len(c) - 1) + [0]
        return tabs, kinds, rows, np.array(flags, dtype=np.int32)

    @cached_terms
    def _spectral_terms(self, D):
        tabs, _, rows, _ = self._plan(D)
        return np.stack([tabs[f][0, 0, t] for f, t in rows])[None, None]

    @cached_terms
    def _spectral_kinds(self, D):
        _, kinds, rows, flags = self._plan(D)
        kind = np.array([int(kinds[f][0][0, 0, t]) & KIND_MASK for f, t in rows], dtype=np.int32) | flags
        return kind[None, None], np.array([kinds[f][1][0, 0, t] for f, t in rows])[None, None]

    def _spectral_backward(self, gtable):
        """every produced row's gradient back to the factor row it is a copy of (a row used in several groups accumulates)"""
        D = self.input_dims if self.input_dims is not None else (gtable.shape[3] - 2) // 3
        tabs, _, rows, _ = self._plan(D)
        gts = [np.zeros_like(t) for t in tabs]
        for r, (f, t) in enumerate(rows):
            gts[f][0, 0, t] += gtable[0, 0, r, :tabs[f].shape[3]]
        for k, g in zip(self.kernels, gts):
            k._spectral_backward(g)

    def _spectral_diag(self, D):
        return np.prod([k._spectral_diag(D) for k in self.kernels], axis=0)          # :261-262

    def _spectral_diag_backward(self, gc, D):
        kd = [k._spectral_diag(D) for k in self.kernels]
        for f, k in enumerate(self.kernels):
            k._spectral_diag_backward(np.asarray(gc) * np.prod([d for h, d in enumerate(kd) if h != f], axis=0), D)


class ChangePointsKernel(Kernels):
    """Change-point kernel (reference gpr/kernel.py:294-377): K(x, x') = sum_i a_i(x) a_i(x') k_i(x, x') over one input dimension, with
    a_i = sigma_i (1 - sigma_{i+1}), sigma_j(x) = sigmoid(s_j (x - l_j)) at the sorted `locations` l_1 < ... < l_n (sigma_0 = 1 - sigma_{n+1} = 1)
    and steepnesses s_j > 0, one shared or one per location.  Every weight is a product of separable factors h(x) h(x'),
    h(x) = sigmoid(beta (x - l)): beta = +s_j the rising gate of kernel j, beta = -s_j the falling gate of kernel j - 1 (1 - sigmoid(z) =
    sigmoid(-z)).  So every group of sub-kernel i travels with one (the end kernels) or two (the middle kernels) gate rows (kind 8)
    appended BEHIND its own rows -- a group's first row stays a kernel row, which is the one LMC scales; a sum inside a sub-kernel
    distributes, as in MulKernel.  At most GROUP_MAX rows per group."""

    def __init__(self, locations, steepnesses=1.0, *kernels):
        if not isinstance(locations, list):
            locations = [locations]
        if len(kernels) != len(locations) + 1:
            raise ValueError("Must pass one more kernel than the number of locations points. "
                             f"Got {len(kernels)} kernels and {len(locations)} locations points.")
        if isinstance(steepnesses, list) and len(steepnesses) > 1:
            if len(locations) != len(steepnesses):
                raise ValueError("Must pass as many locations as steepness point(s). "
                                 f"Got {len(locations)} locations and {len(steepnesses)} steepness points.")
        if not np.array_equal(np.asarray(locations, dtype=np.float64), np.sort(np.asarray(locations, dtype=np.float64))):
            raise ValueError("'locations' must be sorted ascendingly and 'steepnesses' should be ordered correspondingly.")
        super().__init__(*kernels)
        if len(self.kernels) != len(locations) + 1:
            raise NotImplementedError("a ChangePointsKernel directly inside a ChangePointsKernel is taken apart by the base class (as in the reference, "
                                      "whose K then fails): wrap the inner one in an AddKernel")
        if self.output_dims is not None:
            raise NotImplementedError("a change-point kernel over multi-output kernels is not on the MI355X spectral path: ChangePointsKernel "
                                      "weighs single-output kernels")
        if self.input_dims != 1:
            raise ValueError("Must pass kernels defined over a 1D input domain.")
        self.locations = Parameter(locations)
        self.steepness = Parameter(steepnesses, lower=config.positive_minimum)

    def _steepness_index(self, j):
        """where location j's steepness lives in the parameter: its own entry, or the one shared value"""
        return j if self.steepness.data.size > 1 else 0

    @cached_terms
    def _plan(self, D):
        """(tables and kinds of the sub-kernels, the produced rows -- (i, t): row t of sub-kernel i; (-1, j, sign): the gate at location j,
        rising (+1) or falling (-1) --, kind and shape of every produced row)"""
        if D != 1:
            raise ValueError("Must pass kernels defined over a 1D input domain.")
        tabs = [k._spectral_terms(D) for k in self.kernels]
        if any(t.shape[0] != 1 or t.shape[3] != term_width(D) for t in tabs):
            raise NotImplementedError("a change-point kernel over enveloped (harmonizable) terms is not on the MI355X spectral path")
        kinds = [k._spectral_kinds(D) for k in self.kernels]
        n = len(self.kernels)
        rows, kind, shape = [], [], []
        for i, (kd, sh) in enumerate(kinds):
            gates = ([(-1, i - 1, 1.0)] if i > 0 else []) + ([(-1, i, -1.0)] if i < n - 1 else [])
            for a, b in group_slices(kd[0, 0]):
                count = b - a + len(gates)
                if count > GROUP_MAX:
                    raise NotImplementedError("a change-point weight on a product of %d table rows (sub-kernel %d, %s: %d rows with its %d gate "
                                              "row%s) is not on the MI355X spectral path: the device multiplies groups of at most %d rows"
                                              % (b - a, i, self.kernels[i].name(), count, len(gates), "s" if len(gates) > 1 else "", GROUP_MAX))
                rows += [(i, t) for t in range(a, b)] + gates
                kind += [int(kd[0, 0, t]) & KIND_MASK for t in range(a, b)] + [KIND_GATE] * len(gates)
                shape += [float(sh[0, 0, t]) for t in range(a, b)] + [0.0] * len(gates)
                for r in range(len(kind) - count, len(kind) - 1):
                    kind[r] |= KIND_TIMES
        return tabs, kinds, rows, np.array(kind, dtype=np.int32), np.array(shape, dtype=np.float64)

    @cached_terms
    def _spectral_terms(self, D):
        tabs, _, rows, _, _ = self._plan(D)
        loc, steep = np.reshape(self.locations(), -1), np.reshape(self.steepness(), -1)
        table = np.zeros((len(rows), term_width(D)))
        for r, row in enumerate(rows):
            if row[0] >= 0:
                table[r] = tabs[row[0]][0, 0, row[1]]
            else:                                                  # [A, Psi, V, M, Delta] = [1, 0, beta, l, 0]
                _, j, sign = row
                table[r, 0], table[r, 2], table[r, 2 + D] = 1.0, sign * steep[self._steepness_index(j)], loc[j]
        return table[None, None]

    @cached_terms
    def _spectral_kinds(self, D):
        _, _, _, kind, shape = self._plan(D)
        return kind[None, None], shape[None, None]

    def _spectral_diag(self, D):
        raise NotImplementedError("%s has no diagonal value per channel: K(x, x) follows the point (Kernel._point_diag)" % self.name())

    def _spectral_backward(self, gtable):
        """a kernel row's gradient back to the sub-kernel row it copies; a gate row's V and M columns are d/dbeta and d/dl: into the
        steepness (with beta's sign) and the location that the row carries.  A gate row's amplitude is not a parameter."""
        D = 1
        tabs, _, rows, _, _ = self._plan(D)
        gts = [np.zeros_like(t) for t in tabs]
        gloc, gsteep = np.zeros(self.locations.data.size), np.zeros(self.steepness.data.size)
        for r, row in enumerate(rows):
            if row[0] >= 0:
                gts[row[0]][0, 0, row[1]] += gtable[0, 0, r, :term_width(D)]
            else:
                _, j, sign = row
                gsteep[self._steepness_index(j)] += sign * gtable[0, 0, r, 2]
                gloc[j] += gtable[0, 0, r, 2 + D]
        self.locations.accumulate_grad(np.reshape(gloc, self.locations.data.shape))
        self.steepness.accumulate_grad(np.reshape(gsteep, self.steepness.data.shape))
        for k, g in zip(self.kernels, gts):
            k._spectral_backward(g)


class MixtureKernel(AddKernel):
    """Sum of Q copies of a kernel (reference gpr/kernel.py:264-276)."""

    def __init__(self, kernel, Q):
        if not issubclass(type(kernel), Kernel):
            raise ValueError("must pass kernel")
        kernels = self._check_kernels(kernel, Q)
        super().__init__(*kernels)


class MultiOutputKernel(Kernel):
    """Base class of multi-output kernels (reference gpr/kernel.py:381-520): column 0 of X holds the
    channel id.  The channel split / pair loop / scatter of :446-481 happens inside the HIP library."""

    def __init__(self, output_dims, input_dims=None, active_dims=None):
        super().__init__(input_dims, active_dims)
        self.output_dims = output_dims

    def _check_input(self, X1, X2=None):
        """reference gpr/kernel.py:398-404 (including its slip of re-checking X1 for X2's range)"""
        X1, X2 = super()._check_input(X1, X2)
        if not np.all(X1[:, 0] == np.trunc(X1[:, 0])) or not np.all(X1[:, 0] < self.output_dims):
            raise ValueError("X must have integers for the channel IDs in the first input dimension")
        if X2 is not None and not np.all(X2[:, 0] == np.trunc(X2[:, 0])) or not np.all(X1[:, 0] < self.output_dims):
            raise ValueError("X must have integers for the channel IDs in the first input dimension")
        return X1, X2
