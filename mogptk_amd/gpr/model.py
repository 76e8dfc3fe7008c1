"""
GP inference models on the HIP path -- host-side mirror of mogptk/gpr/model.py:71-483 (CholeskyException,
Model, Exact).  The O(N^2)/O(N^3) work of every method below is one call into libmogp_hip.so; the host does
the O(C^2 Q) parameter algebra (term table, chain rule) in numpy.
"""
import sys
import numpy as np
from contextlib import contextmanager
from math import erf, sqrt

from .config import config
from .parameter import Parameter, ParameterHolder, Softplus, Sigmoid, _STRUCTURE_EPOCH
from .kernel import Kernel, MulKernel, ChangePointsKernel, terms_cache, KIND_TIMES, KIND_MASK, KIND_DOT, KIND_GATE, KIND_WDOT, group_diag_grad, group_diag, group_slices, deriv_diag, KIND_WHITE, KIND_NAMES
from .likelihood import Likelihood, GaussianLikelihood
from .mean import Mean
from .multioutput import MultiOutputSpectralMixtureKernel


class CholeskyException(Exception):
    """reference gpr/model.py:71-78"""

    def __init__(self, message, K, model):
        self.message = message
        self.K = K
        self.model = model

    def __str__(self):
        return self.message


def _to_array(X):
    if hasattr(X, "detach"):
        X = X.detach().cpu().numpy()
    return np.array(X, dtype=config.dtype)


def _leaf_kernels(kernel):
    """the kernels of a composition that carry parameters of their own"""
    subs = getattr(kernel, "kernels", None)
    if not subs or isinstance(kernel, (MulKernel, ChangePointsKernel)):      # a product, a change-point kernel: radial as a whole, whatever is inside
        return [kernel]
    return [leaf for k in subs for leaf in _leaf_kernels(k)]


def _enveloped(table, D):
    """rows of width 2 + 5 D (MOHSM): the kernel diagonal follows the points instead of being constant per channel"""
    return table.shape[3] > 2 + 3 * D


def _channel_counts(Xk, C):
    """points per channel of inputs in kernel format"""
    return np.bincount(Xk[:, 0].astype(np.int64), minlength=C).astype(np.float64)


def _lml_constant(X):
    """N/2 log 2 pi, the attribute the reference's models carry (gpr/model.py:436)"""
    return 0.5 * X.shape[0] * np.log(2.0 * np.pi)


_F64 = np.dtype(np.float64)
_STEP_KINDS = {type(None): 0, Softplus: 1, Sigmoid: 2}        # the transform kinds of the native step (include/mogp_hip.h MOGP_TRANSFORM_*)


def _step_signature(p):
    """what the native step's plan describes of one parameter: its transform's class, the transform and its fields, the shape.  The objects
    themselves are kept, so `is` decides: a bound changes through Parameter.assign, which makes a new transform"""
    t = p.transform
    return (type(t), t, getattr(t, "lower", None), getattr(t, "upper", None), getattr(t, "beta", None), getattr(t, "threshold", None), p.data.shape)


_PAIR_INDEX = {}


def _pair_index(C, lower):
    key = (C, lower)
    if key not in _PAIR_INDEX:
        _PAIR_INDEX[key] = np.tril_indices(C) if lower else tuple(np.divmod(np.arange(C * C), C))
    return _PAIR_INDEX[key]


def _gtable_from_moments(table, mom, D, lower=True, kind=None):
    """d(objective)/d(term table) from the device's gradient moments [m0, m4, m1_d, m2_d, m3_d]:
    dA = m0, dPsi = -2 pi A m4, dV_d = -1/2 A m1_d, dM_d = -2 pi A m3_d, dDelta_d = -V_d A m2_d - 2 pi M_d A m4.
    `kind` (the table's kinds, when they travelled): a dot-product row's moments are derivatives already -- dA = m0, and the bias in its Psi
    slot gets m1_0 (an even slot, which the device keeps on diagonal channel blocks); its other columns are not parameters.  A gate row's
    m1_0 and m3_0 are d/dbeta and d/dl of h_a h_b: times the row's own amplitude (1 as ChangePointsKernel writes it) they are the V and M
    columns; the other columns but the amplitude's are zero.  A weighted-dot row's m1_d is d/dV_d of sum_d V_d x_a,d x_b,d: times the row's
    own amplitude it is the V column d (FunctionKernel's magnitude on its feature columns); M, Delta and Psi are not parameters.
    lower=True: mom is indexed by lower channel pairs p = i(i+1)/2 + j (symmetric Gram, double count already
    included); lower=False: mom is indexed by all ordered pairs i*C + j (rectangular Gram)."""
    C, T = table.shape[0], table.shape[2]
    gt = np.zeros((C, C, T, table.shape[3]))
    ii, jj = _pair_index(C, lower)                      # lower: row-major lower pairs, exactly p = i(i+1)/2 + j
    tb = table[ii, jj]                                  # (P, T, W)
    A = tb[..., 0]
    V = tb[..., 2:2 + D]
    M = tb[..., 2 + D:2 + 2 * D]
    m0, m4 = mom[..., 0], mom[..., 1]
    m1, m2, m3 = mom[..., 2:2 + D], mom[..., 2 + D:2 + 2 * D], mom[..., 2 + 2 * D:2 + 3 * D]
    g = np.empty_like(tb)
    g[..., 0] = m0
    g[..., 1] = -2.0 * np.pi * A * m4
    g[..., 2:2 + D] = -0.5 * A[..., None] * m1
    g[..., 2 + D:2 + 2 * D] = -2.0 * np.pi * A[..., None] * m3
    g[..., 2 + 2 * D:2 + 3 * D] = -V * A[..., None] * m2 - 2.0 * np.pi * M * (A * m4)[..., None]
    if tb.shape[-1] > 2 + 3 * D:          # envelope exp(-1/2 L a^2), a = midpoint - c:  dL = -1/2 A m5,  dc = L A m6
        Lv = tb[..., 2 + 3 * D:2 + 4 * D]
        g[..., 2 + 3 * D:2 + 4 * D] = -0.5 * A[..., None] * mom[..., 2 + 3 * D:2 + 4 * D]
        g[..., 2 + 4 * D:2 + 5 * D] = Lv * A[..., None] * mom[..., 2 + 4 * D:2 + 5 * D]
    if kind is not None:
        dot = (kind[ii, jj] & KIND_MASK) == KIND_DOT
        if np.any(dot):
            g[dot, 1:] = 0.0
            g[dot, 1] = mom[..., 2][dot]
        gate = (kind[ii, jj] & KIND_MASK) == KIND_GATE
        if np.any(gate):
            g[gate, 1:] = 0.0
            g[gate, 2] = (A * mom[..., 2])[gate]
            g[gate, 2 + D] = (A * mom[..., 2 + 2 * D])[gate]
        wdot = (kind[ii, jj] & KIND_MASK) == KIND_WDOT
        if np.any(wdot):
            g[wdot, 1:] = 0.0
            g[wdot, 2:2 + D] = (A[..., None] * m1)[wdot]
    gt[ii, jj] = g
    return gt


class Model(ParameterHolder):
    """Base model (reference gpr/model.py:80-401)."""

    def __init__(self, kernel, X, y, likelihood=None, jitter=1e-8, mean=None):
        if likelihood is None:
            likelihood = GaussianLikelihood(1.0)
        if not issubclass(type(kernel), Kernel):
            raise ValueError("kernel must derive from mogptk_amd.gpr.Kernel")
        X, y = self._check_input(X, y)
        if mean is not None:
            mu = np.asarray(mean(X)).reshape(-1, 1)
            if mu.shape != y.shape:
                raise ValueError("mean and y data must match shapes: %s != %s" % (mu.shape, y.shape))
            if isinstance(mean, Mean):
                if any(True for _ in mean.parameters()) and not mean._has_backward():
                    raise NotImplementedError("the trainable mean %s has no backward(X, dmu): a Mean subclass with parameters implements it "
                                              "to add d loss / d m(X) to its parameters' .grad (see mogptk_amd/gpr/mean.py)" % mean.name())
            elif any(True for _ in getattr(mean, "parameters", lambda: [])()):
                raise NotImplementedError("trainable mean functions are not on the HIP path unless they derive from mogptk_amd.gpr.Mean")
        if likelihood.output_dims is not None and likelihood.output_dims != kernel.output_dims:
            raise ValueError("kernel and likelihood must have matching output dimensions")
        likelihood.validate_y(X, y)
        # limit to number of significant digits (reference gpr/model.py:106-110)
        jitter = max(jitter, 1e-6 if config.dtype == np.float32 else 1e-15)

        self.kernel = kernel
        self.X = X
        self.y = y
        self.mean = mean
        self.likelihood = likelihood
        self.jitter = jitter
        self.input_dims = X.shape[1]
        self._handle = None
        if not isinstance(self, Exact) and any(k._radial(self._D) for k in _leaf_kernels(kernel)):
            raise NotImplementedError("%s with a non-Gaussian stationary kernel (rational quadratic, Matern, exponential, periodic, locally periodic) "
                                      "or a product kernel (MulKernel) is not on the HIP path yet: its per-point input gradients need the profile's "
                                      "derivative, and a product's other factors, in a third place; gpr.Exact takes them" % self.name())

    def name(self):
        return self.__class__.__name__

    # -- trainable mean functions (gpr/mean.py, csrc/mean.hip) ---------------------------------------------------------------
    def _trainable_mean(self):
        """a gpr.Mean: the residual y - m(X) follows its parameters from evaluation to evaluation (any other mean is fixed at
        construction, as before)"""
        return isinstance(self.mean, Mean)

    def _mean_refuse(self, what):
        """the combinations a gpr.Mean is not carried through yet: raised before any device call"""
        if self._trainable_mean():
            raise NotImplementedError("a trainable mean function (%s) with %s is not on the HIP path yet" % (self.mean.name(), what))

    def _mean_has_grads(self):
        from .mean import MultiOutputMean
        return self._trainable_mean() and (any(True for _ in self.mean.parameters()) or isinstance(self.mean, MultiOutputMean))   # Q8: sub-means get .grad

    def _handle_y(self):
        """the targets the device handle is created with"""
        if self.mean is None or self._trainable_mean():
            return self.y
        return self.y - np.asarray(self.mean(self.X)).reshape(-1, 1)

    def _mean_affine(self):
        """(the mean's affine table over the model's own inputs -- with zero slopes on the feature columns of a FunctionKernel, which the device
        sees as inputs too --, whether X has a channel column)"""
        channel_col = self.kernel.output_dims is not None
        table = self.mean._affine(self.kernel._channels(), self._D, channel_col)
        F = sum(k._features() for k in self.kernel._feature_leaves())
        if table is not None and F:
            table = np.concatenate([table, np.zeros((table.shape[0], F))], axis=1)
        return table, channel_col

    def _sync_mean(self, h):
        """before an evaluation: the affine table to the device (it re-forms the residual only when the table changed), or -- a user's
        Mean -- y - m(X) when m(X) changed"""
        if not self._trainable_mean():
            return
        table, _ = self._mean_affine()
        if table is not None:
            h.set_mean(table)
            return
        mu = np.asarray(self.mean(self.X), dtype=np.float64).reshape(-1, 1)
        last = getattr(h, "host_mean", None)
        if last is None or not np.array_equal(last, mu):
            h.set_y(self.y - mu)
            h.host_mean = mu

    def _mean_backward(self, h):
        """after a gradient evaluation: d loss / d (mean parameters) from dp/dr on the device (loss = -p, r = y - m: d loss / d m = dp/dr)"""
        if not self._mean_has_grads():
            return
        table, channel_col = self._mean_affine()
        if table is not None:
            self.mean._affine_backward(np.asarray(h.mean_grad())[:, :1 + self._D], channel_col)
        else:
            self.mean.backward(self.X, h.fetch(3).reshape(-1, 1))

    def _add_mean(self, mu, X):
        """a prediction's mean plus the mean function at its inputs"""
        if self.mean is None:
            return mu
        return mu + np.asarray(self.mean(X)).reshape(-1, 1)

    # -- the host scaffold every model evaluates through ------------------------------------------------------------------------
    _device_mean = True       # _push hands a gpr.Mean to the device (the variational models refuse one at construction)
    _noise_dtype = None       # the dtype the noise scale is squared in (None: the parameter's own)

    @property
    def _D(self):
        """input dimensions without the channel column"""
        return self.X.shape[1] - (0 if self.kernel.output_dims is None else 1)

    def _device_handle(self):
        if self._handle is None:
            from .._lib import ExactHandle
            self._handle = ExactHandle(config.device, self.kernel._kernel_format(self.X), self._handle_y(), self.kernel._channels())
        return self._handle

    def _push(self, table=None):
        """what every evaluation starts with: the device handle, the mean and the term table (built here unless the caller had to look at it first)
        on the device -> (h, table, D)"""
        h = self._device_handle()
        if self._device_mean:
            self._sync_mean(h)
        D = self._D
        if table is None:
            table = self.kernel._spectral_terms(D)
        h.set_terms(table)
        return h, table, D

    @contextmanager
    def _cholesky_guard(self):
        """around every device call that factorises: not positive definite / non-finite becomes the reference's CholeskyException
        (reference gpr/model.py:245-255: report, dump parameters, raise CholeskyException(msg, K, model)); any other error passes"""
        from .._lib import MogpError, MOGP_ENOTPD, MOGP_ENONFINITE
        try:
            yield
        except MogpError as e:
            if e.code in (MOGP_ENOTPD, MOGP_ENONFINITE):
                print("ERROR:", str(e), file=sys.__stdout__)
                self.print_parameters()
                raise CholeskyException(str(e), None, self)
            raise

    def _kernel_diag(self, table, Xk, D):
        """K_diag as the device takes it: per point of Xk with enveloped terms, else per channel"""
        return self.kernel._point_diag(table, Xk, D) if _enveloped(table, D) or self.kernel._pointwise(self._D) else self.kernel._spectral_diag(self._D)

    def _train_counts(self):
        """training points per channel.  X does not change under a model (reference gpr/model.py:113-118): counted once per X and number of channels"""
        C = self.kernel._channels()
        cache = self.__dict__.get("_count_cache")
        if cache is None or cache[0] is not self.X or cache[1].shape[0] != C:
            cache = self.__dict__["_count_cache"] = (self.X, _channel_counts(self.kernel._kernel_format(self.X), C))
        return cache[1]

    def _noise_per_channel(self, s):
        return s.ndim == 1 and s.shape[0] == self.kernel._channels() and self.kernel.output_dims is not None

    def _noise_var(self):
        """sigma_c^2 per channel: the vector `_index_channel` (gpr/model.py:183-186) would gather from (a scalar scale is shared by all channels)"""
        s = np.asarray(self.likelihood.scale(), dtype=self._noise_dtype)
        if self._noise_per_channel(s):
            return np.square(s)
        s = s.reshape(-1)[0]               # (Snelson has always squared its shared scale as a power, which is not a product's bits for one float64 in a thousand)
        return np.repeat(s ** 2 if self._noise_dtype else np.square(s), self.kernel._channels())

    def _noise_backward(self, gvar):
        """gvar[c] = d LML / d sigma_c^2 -> the noise scale's .grad (loss = -LML): d / d sigma_c = 2 sigma_c gvar[c]; a shared scale takes the sum"""
        scale = self.likelihood.scale
        sc = np.asarray(scale(), dtype=self._noise_dtype)
        if self._noise_per_channel(sc):
            gsc = 2.0 * sc * gvar
        else:
            gsc = np.reshape(2.0 * sc * np.sum(gvar), sc.shape)
        scale.accumulate_grad(-gsc)

    def _get_name(self):
        return self.__class__.__name__

    def __getstate__(self):
        """device handles are never pickled; they are rebuilt lazily (reference gpr/model.py:131-136 drops
        the traced forward the same way), and so is the per-channel count"""
        state = self.__dict__.copy()
        state["_handle"] = None
        state.pop("_count_cache", None)
        return state

    def _check_input(self, X, y=None):
        """reference gpr/model.py:149-181"""
        X = _to_array(X)
        if X.ndim == 0:
            X = X.reshape(1, 1)
        elif X.ndim == 1:
            X = X.reshape(-1, 1)
        elif X.ndim != 2:
            raise ValueError("X must have dimensions (data_points,input_dims) with input_dims optional")
        if X.shape[0] == 0 or X.shape[1] == 0:
            raise ValueError("X must not be empty")
        if y is not None:
            y = _to_array(y)
            if y.ndim == 0:
                y = y.reshape(1, 1)
            elif y.ndim == 1:
                y = y.reshape(-1, 1)
            elif y.ndim != 2 or y.shape[1] != 1:
                raise ValueError("y must have one dimension (data_points,)")
            if X.shape[0] != y.shape[0]:
                raise ValueError("number of data points for X and y must match")
            return X, y
        if X.shape[1] != self.input_dims:
            raise ValueError("X must have %s input dimensions" % self.input_dims)
        return X

    def print_parameters(self, file=None):
        """reference gpr/model.py:188-240 (plain-text branch)"""
        vals = [["Name", "Range", "Value"]]
        for p in self.parameters():
            vals.append([str(p._name), "", p.numpy().tolist()])
        nameWidth = max(len(val[0]) for val in vals)
        for val in vals:
            print("%-*s  %s" % (nameWidth, val[0], val[2]), file=file)

    def log_marginal_likelihood(self):
        raise NotImplementedError()

    def log_prior(self):
        """reference gpr/model.py:268-277"""
        total = 0.0
        for p in self._parameter_list():
            if p.prior is not None:
                total = total + p.log_prior()
        return total

    def forward(self, x=None):
        """reference gpr/model.py:124-125"""
        return -self.log_marginal_likelihood() - self.log_prior()

    def compile(self):
        """reference gpr/model.py:127-129 traces the forward with torch.jit; the HIP path is already one
        native call per evaluation, so this is accepted and ignored."""
        pass

    def loss(self):
        with terms_cache():                 # parameters are frozen between the table push and the chain rule
            return self._loss_impl()

    def _loss_impl(self):
        raise NotImplementedError()

    def K(self, X1, X2=None):
        """reference gpr/model.py:294-306"""
        return self.kernel(X1, X2)

    def predict_f(self, X, full=False):
        raise NotImplementedError()

    def predict_y(self, X, ci=None, sigma=None, n=10000):
        """reference gpr/model.py:322-344"""
        X = self._check_input(X)
        mu, var = self.predict_f(X)
        if ci is None and sigma is not None:
            p = 0.5 * (1.0 + erf(sigma / sqrt(2.0)))
            ci = [1.0 - p, p]
        return self.likelihood.predict(self._likelihood_X(X), mu, var, ci, sigma=sigma, n=n)

    def _likelihood_X(self, X):
        return X

    def sample_f(self, Z, n=None, prior=False):
        """Samples of f at Z (reference gpr/model.py:346-376): from the posterior (`predict_f(Z, full=True)`, the device path) or the prior,
        drawn by torch's MultivariateNormal from torch's global generator exactly as the reference does -- the same seed gives the same
        samples.  Shape as the reference returns it: (n, data_points), or (data_points,) without n."""
        from .likelihood import _torch
        torch = _torch()
        Z = self._check_input(Z)
        S = 1 if n is None else n
        if prior:
            if self.mean is None:
                raise TypeError("sampling from the prior needs a mean function (the reference calls self.mean(Z), gpr/model.py:364)")
            mu, var = np.asarray(self.mean(Z), dtype=np.float64), np.array(self.kernel(Z), dtype=np.float64)
        else:
            mu, var = self.predict_f(Z, full=True)
        var = np.array(var, dtype=np.float64)
        var += self.jitter * np.mean(np.diagonal(var)) * np.eye(var.shape[0])
        dist = torch.distributions.multivariate_normal.MultivariateNormal(torch.tensor(np.reshape(mu, -1), dtype=torch.float64), torch.tensor(var))
        samples = dist.sample([S])
        if n is None:
            samples = samples.squeeze()
        return samples.numpy()

    def sample_y(self, Z, n=None):
        """Samples of y at Z (reference gpr/model.py:378-401): samples of f pushed through the likelihood's sampler"""
        from .likelihood import _torch
        torch = _torch()
        Z = self._check_input(Z)
        S = 1 if n is None else n
        samples_f = torch.tensor(self.sample_f(Z, n=S))
        samples_y = self.likelihood.conditional_sample(self._likelihood_X(Z), samples_f)
        if n is None:
            samples_y = samples_y.squeeze()
        return samples_y.numpy()


class Exact(Model):
    """
    Exact GP regression with a Gaussian likelihood (reference gpr/model.py:403-483):
        y ~ N(0, K + sigma^2 I)
    `variance` is a float (one trained scale) or a (channels,) array (one per channel).
    """

    def __init__(self, kernel, X, y, variance=1.0, data_variance=None, jitter=1e-8, mean=None):
        if data_variance is not None:
            data_variance = Parameter.to_tensor(data_variance)
            Xa = _to_array(X)
            if data_variance.ndim != 1 or Xa.ndim == 2 and data_variance.shape[0] != Xa.shape[0]:
                raise ValueError("data variance must have shape (data_points,)")
        self.data_variance = data_variance

        variance = Parameter.to_tensor(variance)
        channels = 1
        if kernel.output_dims is not None:
            channels = kernel.output_dims
        if 1 < variance.ndim or variance.ndim == 1 and variance.shape[0] != channels:
            raise ValueError("variance must be float or have shape (channels,)")

        super().__init__(kernel, X, y, GaussianLikelihood(np.sqrt(variance)), jitter, mean)
        self.log_marginal_likelihood_constant = _lml_constant(self.X)

    # -- device plumbing ---------------------------------------------------------------------
    def _push_terms(self):
        comm = getattr(config, "comm", None)
        if comm is not None and (comm.world > 1 or comm.force):
            self._mean_refuse("the sharded exact evaluation (use_distributed)")
        # the device's columns: the model's own and the feature columns of every FunctionKernel (none: the kernel's own table); what the
        # feature columns cannot go with is refused in there
        Dd = self._D + sum(k._features() for k in self.kernel._feature_leaves())
        table, kind, shape, D = self.kernel._device_terms(Dd)
        radial = bool(np.any(kind))
        if radial:                              # refused before any device call
            if comm is not None and (comm.world > 1 or comm.force):
                raise NotImplementedError("non-Gaussian stationary kernels (periodic ones included) and product kernels are not carried through the "
                                          "sharded exact evaluation (use_distributed)")
            if _enveloped(table, Dd):
                raise NotImplementedError("a sum of enveloped (harmonizable) terms and non-Gaussian stationary kernels is not on the HIP path")
        pointwise = radial and self.kernel._pointwise(D)
        h, table, _ = self._push(table)
        D = Dd                                  # from here on the table's columns are the device's
        if radial:
            h.set_kinds(kind, shape)
        elif getattr(h, "radial_kinds", False):
            h.set_kinds(None, None)               # the kernel was replaced by an all-Gaussian one with the same number of terms
        h.radial_kinds = radial
        h.group_kinds = kind if radial and np.any(kind & KIND_TIMES) else None      # product groups: _loss_impl's jitter term needs them
        h.point_kinds = kind if pointwise else None      # point rows (dot product, gate, weighted dot): _loss_impl's moments and jitter term need them
        if _enveloped(table, D) or h.point_kinds is not None:      # envelope, point rows: the diagonal varies from point to point and enters the relative jitter (:244)
            h.set_point_diag(self.kernel._point_diag(table, self.kernel._kernel_format(self.X), D))
            h.point_diag_set = True
        elif getattr(h, "point_diag_set", False):                # the kernel was replaced by one with a constant diagonal
            h.set_point_diag(None)
            h.point_diag_set = False
        return h, table, D

    def _refuse_sharded_loo(self, what="the leave-one-out likelihood"):
        comm = getattr(config, "comm", None)
        if comm is not None and (comm.world > 1 or comm.force):
            raise NotImplementedError("%s is not carried through the sharded exact evaluation (use_distributed): it "
                                      "reads the whole of Kj^-1, which no rank of a sharded evaluation holds" % what)

    FOLD_MAX = 128             # points per fold of the leave-fold-out evaluation: one factor tile (csrc/lfo.hip)

    def _fold_labels(self, folds):
        """`folds` -- an integer label array of length N (-1: never held out), or a sequence of index arrays -- as (labels int32 (N,), number of
        folds); what the device would refuse is refused here, by name, before any device call"""
        N = self.X.shape[0]
        arr = None
        if isinstance(folds, np.ndarray) or (len(folds) > 0 and all(np.ndim(f) == 0 for f in folds)):
            arr = np.asarray(folds)
        if arr is not None and arr.ndim == 1 and (arr.dtype.kind in "iu" or arr.dtype.kind == "f" and np.all(arr == np.floor(arr))):
            if arr.shape[0] != N:
                raise ValueError("a fold label array must hold one label per training point: %d labels for %d points" % (arr.shape[0], N))
            labels = arr.astype(np.int64)
            if np.any(labels < -1):
                raise ValueError("fold labels are -1 (never held out) or 0, 1, ...: found %d" % labels.min())
            F = int(labels.max()) + 1 if N else 0
        else:
            labels = np.full(N, -1, dtype=np.int64)
            F = len(folds)
            for f, ind in enumerate(folds):
                ind = np.asarray(ind).reshape(-1)
                if ind.size and ind.dtype.kind not in "iu":
                    raise ValueError("fold %d: indices must be integers" % f)
                ind = ind.astype(np.int64)
                if np.any(ind < 0) or np.any(ind >= N):
                    raise ValueError("fold %d: index %d is out of range for %d training points" % (f, ind[(ind < 0) | (ind >= N)][0], N))
                if np.unique(ind).size != ind.size:
                    raise ValueError("fold %d holds a point twice" % f)
                taken = labels[ind] >= 0
                if np.any(taken):
                    raise ValueError("folds %d and %d overlap (point %d): folds are disjoint" % (labels[ind][taken][0], f, ind[taken][0]))
                labels[ind] = f
        if F == 0:
            raise ValueError("no folds: at least one point must be held out")
        sizes = np.bincount(labels[labels >= 0], minlength=F)
        for f in range(F):
            if sizes[f] == 0:
                raise ValueError("fold %d is empty" % f)
            if sizes[f] > self.FOLD_MAX:
                raise ValueError("fold %d holds %d points: the limit is %d points per fold, larger folds are not on the device"
                                 % (f, sizes[f], self.FOLD_MAX))
        return labels.astype(np.int32), F

    def _eval(self, grad, score="lml", folds=None):
        """one device evaluation of the marginal likelihood ("lml"), the leave-one-out likelihood ("loo") or the leave-fold-out one ("cv", over
        `folds`): push, guard, conditioning check"""
        if score == "loo":
            self._refuse_sharded_loo()              # before any device call
        elif score == "cv":
            self._refuse_sharded_loo("leave-fold-out cross-validation")
            labels, F = self._fold_labels(folds)
        h, table, D = self._push_terms()
        with self._cholesky_guard():
            if score == "cv":
                run = lambda: h.cv(self._noise_var(), self.jitter, labels, F, grad=grad, data_var=self.data_variance)
            else:
                call = h.loo if score == "loo" else h.eval
                run = lambda: call(self._noise_var(), self.jitter, grad=grad, data_var=self.data_variance)
            res = run()
            # (the LML alone: the fast factorisation's log-determinant and z are good to ~1e-7 even at 1e8; a LOO / CV evaluation reads the inverse, like a gradient)
            again = self._check_conditioning(h, run) if grad or score != "lml" else None
            return (res if again is None else again), table, D

    CONDITION_WARN = 1e5       # on the pivot-spread estimate (max L_jj / min L_jj)^2, a LOWER bound of cond(Kj) -- 9e5 where cond is 7e7, 9e3 where it is 8e5;
                               # DESIGN 7 puts the envelope of the fast schedules at cond ~ 1e6 - 1e7

    def _check_conditioning(self, h, redo, est=None):
        """The reference's torch.linalg.cholesky is backward stable and silent; the fast schedules of this path form their panels with explicit block
        inverses and lose accuracy as K + noise becomes ill-conditioned.  The factor's own diagonal says when: the model then says so
        (once), repeats the evaluation in the backward-stable form (mogp_model_set_accurate; 25 ms against 10 at N = 8192) and stays there until the matrix is
        well-conditioned again.  `config.accurate_fallback = False` keeps the fast form and only warns."""
        if est is None:                                     # (the native step hands over the estimate it read with the evaluation)
            if not hasattr(h, "condition_estimate"):
                return None
            est = h.condition_estimate()
        if est != est:
            return None
        accurate = getattr(h, "accurate_mode", False)       # the mode lives in the device handle, so the flag lives ON the handle: a model that is copied,
        if not accurate and est > self.CONDITION_WARN:      # reloaded or re-sharded gets a new handle in the fast mode and a flag that says so
            fallback = getattr(config, "accurate_fallback", True) and hasattr(h, "set_accurate")
            if not getattr(self, "_cond_warned", False):
                self._cond_warned = True
                import warnings
                warnings.warn("the kernel matrix plus noise is ill-conditioned (cond >= %.1e from the Cholesky factor's diagonal): beyond ~1e6 - 1e7 the "
                              "fast schedules' LML and gradients leave a backward-stable factorisation's by more than 1e-9 / 1e-5 (at 1e8: ~1e-7 / ~1e-4); %s"
                              % (est, "evaluating in the backward-stable form from here on (about two and a half times slower)" if fallback
                                 else "a larger noise variance or jitter brings it back"), RuntimeWarning, stacklevel=5)
            if fallback:
                h.set_accurate(True)
                h.accurate_mode = True
                return redo()
        elif accurate and est < 0.1 * self.CONDITION_WARN:
            h.set_accurate(False)                     # the next evaluation is a fast one again
            h.accurate_mode = False
        return None

    # -- reference surface -------------------------------------------------------------------
    def log_marginal_likelihood(self):
        """reference gpr/model.py:438-453 -- one forward-only device evaluation"""
        res, _, _ = self._eval(grad=False)
        return config.dtype(res["lml"])

    # -- the native host side of a plain MOSM training step (csrc/hoststep.hip, csrc/step.hip) -----------------------------------
    def _step_plan(self, score):
        """the native step's plan (_lib.StepPlan) when this evaluation can take it, else None.  It takes the marginal likelihood of the plain MOSM
        kernel in float64 under a Gaussian likelihood with no mean function, no prior, no pegged parameter and no communicator, on a handle
        that has the native step; everything else goes the general way.  The plan lives on the device handle (which is never pickled or
        copied) and is rebuilt when what it describes changes: the parameters, their transforms and bounds, their shapes, X."""
        k = self.kernel
        if (score != "lml" or not getattr(config, "host_fast", True) or config.dtype != np.float64 or getattr(config, "comm", None) is not None
                or type(k) is not MultiOutputSpectralMixtureKernel or self.mean is not None or type(self.likelihood) is not GaussianLikelihood):
            return None
        h = self._device_handle()
        plan = getattr(h, "_step_plan", None)
        if plan is not None and plan.kernel is k and plan.likelihood is self.likelihood and plan.X is self.X and plan.epoch == _STRUCTURE_EPOCH[0]:
            for p, s in zip(plan.params, plan.sigs):
                t = p.transform
                if (t is not s[1] or p.pegged_parameter is not None or p.prior is not None or p.data.shape != s[6] or (p.data.dtype is not _F64 and p.data.dtype != _F64)
                        or (t is not None and (t.lower is not s[2] or getattr(t, "upper", None) is not s[3] or getattr(t, "beta", None) != s[4]
                                               or getattr(t, "threshold", None) != s[5]))):
                    break
            else:
                return plan
        return self._new_step_plan(h)

    def _new_step_plan(self, h):
        """check everything the native step assumes, and build its plan on the handle (None: this model goes the general way)"""
        k = self.kernel
        if not hasattr(h, "step") or getattr(h, "radial_kinds", False) or getattr(h, "point_diag_set", False):
            return None
        blocks, trained = k._step_blocks()
        params = blocks + (self.likelihood.scale,)
        epoch = _STRUCTURE_EPOCH[0]
        plist = self._parameter_list()
        if len(plist) != len(params):
            return None
        for p, q in zip(plist, params):
            if p is not q or p.pegged_parameter is not None or p.prior is not None or p.data.dtype != np.float64:
                return None
        sigs = [_step_signature(p) for p in params]
        C, D, Q = k.output_dims, k.input_dims, k.weight.shape[1]
        scale = params[5]
        shapes = [(C, Q), (C, Q, D), (C, Q, D), (C, Q, D), (C, Q), scale.shape]
        if D != self._D or scale.shape not in ((), (C,)) or any(s[6] != shape for s, shape in zip(sigs, shapes)) or any(s[0] not in _STEP_KINDS for s in sigs):
            return None
        from .._lib import StepPlan
        plan = StepPlan(C, Q, D, scale.data.size, [(_STEP_KINDS[s[0]],) + s[2:6] for s in sigs], k.twopi, k._phase_scale, self._train_counts(),
                        self.X.shape[0], trained + (True,))
        plan.params, plan.sigs, plan.X, plan.kernel, plan.likelihood, plan.epoch = params, sigs, self.X, k, self.likelihood, epoch
        h._step_plan = plan
        h.radial_kinds, h.group_kinds, h.point_kinds = False, None, None       # what _push_terms notes on the handle for an all-Gaussian table
        return plan

    def _loss_native(self, plan):
        """`_loss_impl` for the marginal likelihood through the native step: one gather, one native call (raw parameters -> table -> device
        evaluation -> raw gradient), one scatter.  `.grad` are fresh arrays of every parameter's own shape, None where the general way leaves
        None; they are disjoint views of one vector made for this step, so `p.grad.base` is shared between the parameters (the general way gives
        each an array of its own) -- writing into one never reaches another.  (No parameter has a prior here, so the loss is -LML.)"""
        h = self._handle
        for p in plan.params:                       # zero_grad(set_to_none=True): an evaluation that raises leaves no stale gradient
            p.grad = None
        plan.gather([p.data for p in plan.params])
        run = lambda: h.step(plan, self.jitter, self.data_variance)
        with self._cholesky_guard():
            run()
            self._check_conditioning(h, run, plan.condition_estimate())
        plan.scatter_grad()
        return config.dtype(-plan.out[0])

    def _loss_impl(self, score="lml", folds=None):
        """reference gpr/model.py:279-292: zero grads, loss = -LML - log prior, fresh `.grad` on every
        parameter in the graph.  Gradients come from the device's moment pass + the host chain rule.
        score "loo" / "cv": the leave-one-out / leave-fold-out likelihood L in the LML's place -- the device returns the moments, diagonal sums
        and trace of dL/dKj in the same layout, so the chain rule below is the same."""
        plan = self._step_plan(score)
        if plan is not None:
            return self._loss_native(plan)
        self.zero_grad(set_to_none=True)
        res, table, D = self._eval(grad=True, score=score, folds=folds)
        counts = self._train_counts()
        jit_rel = self.jitter * res["trG"] / self.X.shape[0]            # d LML / d (mean diag) through the jitter term (:244)

        # d LML / d table for the lower channel pairs (i >= j); zero elsewhere
        point_kinds = getattr(self._handle, "point_kinds", None)
        gt = _gtable_from_moments(table, res["moments"], D, lower=True, kind=point_kinds)
        if _enveloped(table, D) or point_kinds is not None:
            gt += jit_rel * self.kernel._point_diag_table_grad(table, self.kernel._kernel_format(self.X), D)
        else:
            kind = getattr(self._handle, "group_kinds", None)
            if kind is not None:                    # product groups: the diagonal is sum_groups prod_t A_t, not sum_t A_t
                for i in range(table.shape[0]):
                    gt[i, i, :, 0] += jit_rel * counts[i] * group_diag_grad(table[i, i, :, 0], kind[i, i])
            else:
                for i in range(table.shape[0]):
                    gt[i, i, :, 0] += jit_rel * counts[i]
        self.kernel._table_backward(-gt)                       # loss = -LML (without a FunctionKernel: _spectral_backward itself)

        # noise: d LML / d sigma_c = 2 sigma_c (sum_{k in c} G_kk + jitter n_c/N tr G)
        self._noise_backward(res["diagG"] + jit_rel * counts)
        self._mean_backward(self._handle)
        return config.dtype(-res[score] - self.log_prior())

    # -- leave-one-out predictive likelihood (Rasmussen & Williams 5.4.2; csrc/loo.hip) -----------------------------------------
    def loo(self):
        """-> (mu, var), each (N, 1): mean and variance (noise included) of the prediction of every training target from all the others"""
        res, _, _ = self._eval(grad=False, score="loo")
        return self._held_out(res)

    def _held_out(self, res):
        mu = res["mu"].reshape(-1, 1)
        if self.mean is not None and not (self._trainable_mean() and self._mean_affine()[0] is not None):
            mu = self._add_mean(mu, self.X)         # the device holds y - m(X) as its targets (an affine gpr.Mean is on the device: it holds y)
        return mu.astype(config.dtype, copy=False), res["var"].reshape(-1, 1).astype(config.dtype, copy=False)

    def loo_log_likelihood(self):
        """sum_i log p(y_i | X, y_-i): one device evaluation without gradients"""
        res, _, _ = self._eval(grad=False, score="loo")
        return config.dtype(res["loo"])

    def loo_loss(self):
        """-(leave-one-out log-likelihood) - log prior, and like `loss` a fresh `.grad` on every parameter: kernel, noise, trainable mean"""
        with terms_cache():
            return self._loss_impl(score="loo")

    # -- leave-fold-out cross-validation (csrc/lfo.hip) ----------------------------------------------------------------
    def cv(self, folds):
        """-> (mu, var), each (N, 1): mean and variance (noise included) of the prediction of every held-out target from the points outside
        its fold; NaN for a point in no fold.  `folds`: N integer labels (-1: never held out) or a sequence of index arrays, 1 .. 128 points each"""
        res, _, _ = self._eval(grad=False, score="cv", folds=folds)
        return self._held_out(res)

    def cv_log_likelihood(self, folds):
        """sum_f log p(y_Bf | X, y_-Bf), each fold predicted jointly from the points outside it: one device evaluation without gradients"""
        res, _, _ = self._eval(grad=False, score="cv", folds=folds)
        return config.dtype(res["cv"])

    def cv_loss(self, folds):
        """-(leave-fold-out log-likelihood) - log prior, and like `loss` a fresh `.grad` on every parameter: kernel, noise, trainable mean"""
        with terms_cache():
            return self._loss_impl(score="cv", folds=folds)

    # -- rolling-origin forecast from one factorisation (csrc/forecast.hip) ---------------------------------------------
    FORECAST_MAXH = 8          # cuts per point of one device call (MOGP_FORECAST_MAXH)

    def _forecast_args(self, order, cut):
        """`order` (N,): the model's row at every time position; `cut` (N,) or (H, N): per time position p the number of leading points the
        prediction of that point may use, 0 .. p, or -1 to skip it -> (order int64, cut int64 (H, N), cut was 1-D); what the device would
        refuse is refused here, by name, before any device call"""
        N = self.X.shape[0]
        order, cut = np.asarray(order), np.asarray(cut)
        if order.shape != (N,) or order.dtype.kind not in "iu":
            raise ValueError("order must hold one integer row index per training point: shape %s for %d points" % (order.shape, N))
        order = order.astype(np.int64)
        if not np.array_equal(np.sort(order), np.arange(N)):
            raise ValueError("order is not a permutation of 0 .. %d" % (N - 1))
        flat = cut.ndim == 1
        if cut.ndim not in (1, 2) or cut.shape[-1] != N or cut.dtype.kind not in "iu":
            raise ValueError("cut must hold one integer per training point, (N,) or (H, N): shape %s for %d points" % (cut.shape, N))
        cut = cut.astype(np.int64).reshape(-1, N)
        if not 1 <= cut.shape[0] <= self.FORECAST_MAXH:
            raise ValueError("cut holds %d horizons: one call takes 1 .. %d" % (cut.shape[0], self.FORECAST_MAXH))
        bad = np.argwhere((cut < -1) | (cut > np.arange(N)))
        if bad.size:
            h, p = bad[0]
            raise ValueError("cut[%d, %d] = %d: a cut is -1 (skipped) or 0 .. p, the number of points in front of time position p that are used" % (h, p, cut[h, p]))
        return order, cut, flat

    def _forecast(self, order, cut):
        self._refuse_sharded_loo("the rolling-origin forecast")      # before any device call
        order, cut, flat = self._forecast_args(order, cut)
        h, table, D = self._push_terms()
        with self._cholesky_guard():             # (no conditioning switch: this factorisation is the refined one, with substitution by L itself)
            res = h.forecast(self._noise_var(), self.jitter, order, cut, data_var=self.data_variance)
        return res, flat

    def forecast(self, order, cut):
        """-> (mu, var), each (H, N) in the model's row order ((N,) for a 1-D cut): mean and variance (noise included) of the prediction of every
        training target from the `cut` points in front of it in the order `order`; NaN where cut is -1.  One factorisation for all of them"""
        res, flat = self._forecast(order, cut)
        mu = res["mu"]
        if self.mean is not None and not (self._trainable_mean() and self._mean_affine()[0] is not None):
            mu = mu + np.asarray(self.mean(self.X)).reshape(1, -1)      # the device holds y - m(X) as its targets (as _held_out)
        mu, var = mu.astype(config.dtype, copy=False), res["var"].astype(config.dtype, copy=False)
        return (mu[0], var[0]) if flat else (mu, var)

    def forecast_log_likelihood(self, order, cut):
        """-> (H,) (a scalar for a 1-D cut): sum over the points with cut >= 0 of log p(y_p | the cut points in front of it).  With cut[p] = p
        the sum is the log marginal likelihood, whatever the order"""
        res, flat = self._forecast(order, cut)
        score = res["score"].astype(config.dtype, copy=False)
        return score[0] if flat else score

    def predict_f(self, X, full=False):
        """reference gpr/model.py:455-483"""
        X = self._check_input(X)
        h, table, D = self._push_terms()
        Xk = self.kernel._kernel_format(X)
        kss = self._kernel_diag(table, Xk, D)
        with self._cholesky_guard():
            run = lambda: h.predict(self._noise_var(), self.jitter, kss, Xk, full=full, data_var=self.data_variance)
            mu, var = run()
            again = self._check_conditioning(h, run)           # an ill-conditioned system: said once, predicted again in the refined form
            if again is not None:
                mu, var = again
        mu = self._add_mean(mu, X)
        return mu.astype(config.dtype, copy=False), var.astype(config.dtype, copy=False)

    # -- the posterior by kernel part (mogp_exact_predict_parts) -----------------------------------------------------
    PART_ROWS = 65536          # stacked test rows (parts x points) of one device call without the full covariance

    def _refuse_sharded_parts(self):
        comm = getattr(config, "comm", None)
        if comm is not None and (comm.world > 1 or comm.force):
            raise NotImplementedError("the posterior by kernel part is not carried through the sharded exact evaluation (use_distributed): "
                                      "the parts share one factorisation on one device")

    def parts(self):
        """-> [(name, mask)]: the default partition of the kernel into addends, one level deep (`Kernel._parts`), each mask a boolean
        (C, C, T) array over the rows of the device table"""
        with terms_cache():
            return self.kernel._parts(self._D)

    def _part_masks(self, masks, kind):
        """`masks` (P, T) or (P, C, C, T) as boolean (P, C, C, T); a mask that keeps part of a product group is refused by the group's rows"""
        C, _, T = kind.shape
        masks = np.asarray(masks)
        if masks.dtype != np.bool_:
            raise ValueError("masks must be boolean")
        if masks.ndim == 2 and masks.shape[1] == T:
            masks = np.broadcast_to(masks[:, None, None, :], (masks.shape[0], C, C, T))
        if masks.ndim != 4 or masks.shape[1:] != (C, C, T) or masks.shape[0] < 1:
            raise ValueError("masks must have shape (P, %d) or (P, %d, %d, %d): one flag per row of the device table" % (T, C, C, T))
        for a, b in group_slices(kind[0, 0]):
            if b - a > 1:
                g = masks[..., a:b]
                if np.any(np.any(g, axis=-1) != np.all(g, axis=-1)):
                    p = int(np.argwhere(np.any(g, axis=-1) != np.all(g, axis=-1))[0][0])
                    raise ValueError("mask %d keeps a part of the product group of rows %d .. %d: a part holds whole groups (the factors of "
                                     "a product are not addends)" % (p, a, b - 1))
        return np.ascontiguousarray(masks)

    def predict_terms(self, X, masks, full=False):
        """The posterior of the latent function of every addend K_p of the covariance, K = sum_p K_p, given ALL the data:
            mu_p = K_p(X*, X) Kj^-1 r,    var_p = diag K_p(X*, X*) - diag(K_p(X*, X) Kj^-1 K_p(X, X*))     (full: the whole matrix)
        with Kj and r = y - mean(X) the whole model's -- one factorisation and one substitution on the device for all parts.  `masks`: boolean
        (P, T) over the rows of the device table (`_device_terms`), the same in every channel pair, or (P, C, C, T); a part keeps or drops
        product groups whole.  -> (mu (P, S, 1), var (P, S, 1) or (P, S, S)).  No likelihood noise and no mean: the mean function belongs to
        no part, and sum_p mu_p + mean(X*) is `predict_f`'s mean when the masks partition the rows.  A part's prior diagonal is the TRUE
        diagonal of its masked table; the reference's `K_diag` of SpectralMixtureKernel at D > 1 (which is not diag K) is not reproduced
        for parts."""
        self._refuse_sharded_parts()                     # before any device call
        X = self._check_input(X)
        with terms_cache():
            h, table, D = self._push_terms()
            kind = self.kernel._device_terms(D)[1]
            masks = self._part_masks(masks, kind)
            P = masks.shape[0]
            tabs = np.repeat(np.asarray(table, dtype=np.float64)[None], P, axis=0)
            tabs[..., 0] = np.where(masks, tabs[..., 0], 0.0)
            tabs[..., 1] = np.where(~masks & ((kind & KIND_MASK) == KIND_DOT)[None], 0.0, tabs[..., 1])      # (0 <x, x'> + 0)^n = 0
            Xk = self.kernel._kernel_format(X)
            per_point = _enveloped(table, D) or self.kernel._pointwise(self._D)
            if per_point:
                kss = np.stack([self.kernel._point_diag(tabs[p], Xk, D) for p in range(P)])
            else:
                C = kind.shape[0]
                kss = np.array([[group_diag(tabs[p, c, c, :, 0], kind[c, c]) for c in range(C)] for p in range(P)])
        S = Xk.shape[0]
        step = S if full else max(1, self.PART_ROWS // P)
        mus, vs = [], []
        with self._cholesky_guard():
            for s0 in range(0, S, step):
                kc = kss[:, s0:s0 + step] if per_point else kss
                run = lambda: h.predict_parts(self._noise_var(), self.jitter, tabs, kc, Xk[s0:s0 + step], full=full, data_var=self.data_variance)
                mu, var = run()
                again = self._check_conditioning(h, run)
                if again is not None:
                    mu, var = again
                mus.append(mu)
                vs.append(var)
        mu = mus[0] if len(mus) == 1 else np.concatenate(mus, axis=1)
        var = vs[0] if len(vs) == 1 else np.concatenate(vs, axis=1)
        return mu.astype(config.dtype, copy=False), var.astype(config.dtype, copy=False)

    def predict_parts(self, X, full=False):
        """`predict_terms` over the default partition `parts()` -> (names, mu (P, S, 1), var (P, S, 1) or (P, S, S))"""
        self._refuse_sharded_parts()
        named = self.parts()
        mu, var = self.predict_terms(X, np.stack([m for _, m in named]), full=full)
        return [n for n, _ in named], mu, var

    # -- the posterior of df/dx (mogp_exact_predict_grad) ---------------------------------------------------------------
    def _mean_slope(self, C):
        """the slope (C, D) of the mean function, zero without one; a mean that is not affine is refused by name"""
        if self.mean is None:
            return np.zeros((C, self._D))
        table = self._mean_affine()[0] if self._trainable_mean() else None
        if table is None:
            name = self.mean.name() if self._trainable_mean() else getattr(self.mean, "__name__", type(self.mean).__name__)
            raise NotImplementedError("the derivative of the posterior needs the derivative of the mean function, and %s is not affine: only no "
                                      "mean, ConstantMean, LinearMean and a MultiOutputMean of these have one on this path" % name)
        return np.asarray(table, dtype=np.float64)[:, 1:1 + self._D]

    def predict_df(self, X):
        """The posterior of the derivative of the latent function at X: for every input dimension d
            dmu_d(x*) = j_d(x*)^T Kj^-1 r + dm/dx_d,    dvar_d(x*) = kappa_d(x*) - |L^-1 j_d(x*)|^2,
        with j_d(x*)_b = dK(x*, x_b)/dx*_d, kappa_d the prior variance of the derivative and Kj, r = y - mean(X) the model's -- one factorisation
        and one substitution on the device for all dimensions.  -> (dmu, dvar), each (S, D).  No likelihood noise.  Their joint covariance is
        `predict_df_cov`'s.  Refused by name: Matern 1/2 / exponential and white kernels (their
        sample paths are not differentiable), change-point and FunctionKernel rows (not yet), a mean that is not affine, and the sharded
        evaluation."""
        comm = getattr(config, "comm", None)
        if comm is not None and (comm.world > 1 or comm.force):      # before any device call
            raise NotImplementedError("the posterior of the derivative is not carried through the sharded exact evaluation (use_distributed): "
                                      "the row blocks share one factorisation on one device")
        X = self._check_input(X)
        with terms_cache():
            Dd = self._D + sum(k._features() for k in self.kernel._feature_leaves())
            kind = self.kernel._device_terms(Dd)[1]
            for k in (2, KIND_WHITE, KIND_GATE, KIND_WDOT):
                if np.any((kind & KIND_MASK) == k):
                    raise NotImplementedError("the posterior of the derivative is not defined for a %s row: its sample paths are not differentiable"
                                              % KIND_NAMES[k] if k in (2, KIND_WHITE) else
                                              "the posterior of the derivative does not carry a %s row yet" % KIND_NAMES[k])
            slope = self._mean_slope(kind.shape[0])
            h, table, D = self._push_terms()
            kind, shape = self.kernel._device_terms(D)[1:3]
            Xk = self.kernel._kernel_format(X)
            kappa = deriv_diag(table, kind, shape, Xk, D)
        S = Xk.shape[0]
        step = max(1, self.PART_ROWS // D)
        dmus, dvars = [], []
        with self._cholesky_guard():
            for s0 in range(0, S, step):
                run = lambda: h.predict_grad(self._noise_var(), self.jitter, np.ascontiguousarray(kappa[s0:s0 + step].T), Xk[s0:s0 + step],
                                             data_var=self.data_variance)
                dmu, dvar = run()
                again = self._check_conditioning(h, run)
                if again is not None:
                    dmu, dvar = again
                dmus.append(dmu.T)
                dvars.append(dvar.T)
        dmu = (dmus[0] if len(dmus) == 1 else np.concatenate(dmus, axis=0)) + slope[Xk[:, 0].astype(np.int64)]
        dvar = dvars[0] if len(dvars) == 1 else np.concatenate(dvars, axis=0)
        return dmu.astype(config.dtype, copy=False), dvar.astype(config.dtype, copy=False)

    # -- the joint covariance of df/dx (mogp_exact_predict_grad_cov) -------------------------------------------------------
    GRAD_COV_ROWS = 8192       # stacked rows D * S of one joint covariance (MOGP_GRAD_COV_ROWS: half a gigabyte on the device and again on the host)

    def predict_df_cov(self, X):
        """The posterior of the derivative of the latent function at X with the JOINT covariance of all its components:
            dcov[a, d, b, e] = Cov(df/dx_d(x*_a), df/dx_e(x*_b) | y) = d^2 K(x*_a, x*_b)/dx_d dx'_e - (L^-1 j_d(x*_a))^T (L^-1 j_e(x*_b)),
        j_d, L and the mean as `predict_df` has them.  -> (dmu (S, D), dcov (S, D, S, D)), dcov symmetrised on the host; its diagonal is
        `predict_df`'s dvar.  No likelihood noise.  One device call without chunks: D * S <= GRAD_COV_ROWS.  `predict_df` keeps its one
        argument -- its callers and its tests rely on there being no other -- so the covariance is a call of its own.  Refused by name as
        `predict_df` refuses."""
        comm = getattr(config, "comm", None)
        if comm is not None and (comm.world > 1 or comm.force):      # before any device call
            raise NotImplementedError("the posterior of the derivative is not carried through the sharded exact evaluation (use_distributed): "
                                      "the row blocks share one factorisation on one device")
        X = self._check_input(X)
        if self._D * X.shape[0] > self.GRAD_COV_ROWS:                # before any device call
            raise ValueError("the joint covariance of the derivative is limited to D * S <= %d stacked rows, and D * S = %d * %d = %d"
                             % (self.GRAD_COV_ROWS, self._D, X.shape[0], self._D * X.shape[0]))
        with terms_cache():
            Dd = self._D + sum(k._features() for k in self.kernel._feature_leaves())
            kind = self.kernel._device_terms(Dd)[1]
            for k in (2, KIND_WHITE, KIND_GATE, KIND_WDOT):
                if np.any((kind & KIND_MASK) == k):
                    raise NotImplementedError("the posterior of the derivative is not defined for a %s row: its sample paths are not differentiable"
                                              % KIND_NAMES[k] if k in (2, KIND_WHITE) else
                                              "the posterior of the derivative does not carry a %s row yet" % KIND_NAMES[k])
            slope = self._mean_slope(kind.shape[0])
            h, table, D = self._push_terms()
            Xk = self.kernel._kernel_format(X)
        with self._cholesky_guard():
            run = lambda: h.predict_grad(self._noise_var(), self.jitter, None, Xk, data_var=self.data_variance, full=True)
            dmu, dcov = run()
            again = self._check_conditioning(h, run)
            if again is not None:
                dmu, dcov = again
        dmu = dmu.T + slope[Xk[:, 0].astype(np.int64)]
        dcov = 0.5 * (dcov + dcov.transpose(2, 3, 0, 1))
        return dmu.astype(config.dtype, copy=False), dcov.astype(config.dtype, copy=False)

    def sample_df(self, X, n=None):
        """Joint draws of the derivative of the latent function at X, built as `sample_f` builds draws of f: torch's MultivariateNormal on
        `predict_df_cov(X)` -- mean dmu.reshape(-1), covariance dcov.reshape(S D, S D) + jitter * mean(diag) * I -- from torch's global
        generator.  -> (n, S, D), or (S, D) without n."""
        from .likelihood import _torch
        torch = _torch()
        dmu, dcov = self.predict_df_cov(X)
        S, D = dmu.shape
        cov = np.array(dcov, dtype=np.float64).reshape(S * D, S * D)
        cov += self.jitter * np.mean(np.diagonal(cov)) * np.eye(S * D)
        dist = torch.distributions.multivariate_normal.MultivariateNormal(torch.tensor(np.reshape(dmu, -1), dtype=torch.float64), torch.tensor(cov))
        samples = dist.sample([1 if n is None else n]).numpy().reshape(-1, S, D)
        return samples[0] if n is None else samples


# ---- inducing-point initialisation (reference gpr/model.py:11-69) ---------------------------------------------------
def _linspace_f32(lo, hi, n):
    """torch.linspace(lo, hi, n) in the reference runs in torch's default dtype float32 (quirk Q6, gpr/model.py:18):
    step = (end - start)/(n - 1) rounded to float32; first half start + i*step, second half end - (n-1-i)*step, each
    multiply-add rounded ONCE to float32 (torch's kernel fuses it; verified bit-exact against torch.linspace)."""
    start, end = np.float32(lo), np.float32(hi)
    if n == 1:
        return np.array([start], dtype=np.float64)
    step = np.float64(np.float32((end - start) / np.float32(n - 1)))
    i = np.arange(n)
    half = n // 2
    out = np.where(i < half, np.float64(start) + step * i, np.float64(end) - step * (n - i - 1))
    return out.astype(np.float32).astype(np.float64)


def _init_grid(N, X):
    n = np.power(N, 1.0 / X.shape[1])
    if not float(n).is_integer():
        raise ValueError("number of inducing points must equal N = n^%d" % X.shape[1])
    n = int(n)
    axes = [_linspace_f32(np.min(X[:, i]), np.max(X[:, i]), n) for i in range(X.shape[1])]
    grid = np.meshgrid(*axes, indexing="ij")
    return np.stack([g.reshape(-1) for g in grid], axis=1)


def _init_random(N, X):
    from scipy.stats import qmc
    samples = qmc.Halton(d=X.shape[1]).random(n=N)
    lo, hi = np.min(X, axis=0), np.max(X, axis=0)
    return lo + (hi - lo) * samples


def _init_density(N, X):
    from scipy.stats import gaussian_kde
    return gaussian_kde(X.T, bw_method="scott").resample(N).T


def init_inducing_points(Z, X, method="grid", output_dims=None):
    """reference gpr/model.py:36-69.  Z int / list of ints -> locations; an int means PER CHANNEL for multi-output
    kernels (quirk Q5).  Values pass through float32 like the reference's default-dtype tensor (quirk Q6)."""
    _init = {"grid": _init_grid, "random": _init_random, "density": _init_density}.get(method, _init_grid)
    if output_dims is not None:
        if isinstance(Z, (int, np.integer)) or (all(isinstance(z, (int, np.integer)) for z in Z) and len(Z) == output_dims):
            M = [int(Z)] * output_dims if isinstance(Z, (int, np.integer)) else [int(z) for z in Z]
            out = np.zeros((sum(M), X.shape[1]), dtype=np.float32)
            for j in range(len(M)):
                m0 = sum(M[:j])
                out[m0:m0 + M[j], 0] = j
                out[m0:m0 + M[j], 1:] = _init(M[j], X[X[:, 0] == j, 1:])
            return out.astype(np.float64)
    elif isinstance(Z, (int, np.integer)):
        return _init(int(Z), X)
    return Z


class _DataParallel:
    """Sparse models: the objective touches the training points only through sums over them.  Under `mogptk_amd.use_distributed()` every
    process builds its device model on every world-th training point (starting at its rank) and the library all-reduces those sums
    (mogp_titsias_eval_sharded, mogp_snelson_eval_sharded, mogp_svgp_backward_sharded): each rank gets the full model's value and gradient."""

    def _shardable(self):
        return True

    def _data_shard(self):
        """the communicator this process shards its training points over, or None"""
        comm = getattr(config, "comm", None)
        if self._shardable() and comm is not None and getattr(comm, "native", False) and (comm.world > 1 or comm.force):
            return comm
        return None

    def _local(self, a):
        """this rank's share of a per-point array (all of it without a communicator)"""
        comm = self._data_shard()
        return a if comm is None else a[comm.rank::comm.world]

    def _local_Xk(self):
        return self._local(self.kernel._kernel_format(self.X))

    def _device_handle(self):
        comm = self._data_shard()
        key = None if comm is None else (comm.rank, comm.world)
        if self._handle is None or self.__dict__.get("_handle_key") != key:
            from .._lib import ExactHandle
            if comm is not None:
                self._mean_refuse("the data-parallel form (use_distributed)")
            self._handle = ExactHandle(config.device, self._local_Xk(), self._local(self._handle_y()), self.kernel._channels())
            self.__dict__["_handle_key"] = key
        return self._handle


class _InducingPoints(_DataParallel):
    """What Titsias, Snelson and the Hensman models share on the host: the inducing inputs `Z` as a parameter (their channel column carries no
    gradient), the two kernel diagonals of a prediction, and the part of the chain rule that goes through K_uu and K_uf."""

    def _init_inducing(self, Z, Z_init):
        """the bound's constant, and -> `Z` as a parameter (the constructor assigns it: the assignment fixes its place in parameters())"""
        self.log_marginal_likelihood_constant = _lml_constant(self.X)
        Z = init_inducing_points(Z, self.X, method=Z_init, output_dims=self.kernel.output_dims)
        Z = Parameter(self._check_input(Z), name="induction_points")
        if self.kernel.output_dims is not None:
            Z.num_parameters -= Z().shape[0]
        return Z

    def _kernel_diags(self, table, Xsk, D):
        """(K_diag at this process's training points, K_diag at the test points Xsk): per point with enveloped terms, else one per channel for both"""
        if _enveloped(table, D):
            return self.kernel._point_diag(table, self._local_Xk(), D), self.kernel._point_diag(table, Xsk, D)
        kd = self.kernel._spectral_diag(D)
        return kd, kd

    def _inducing_backward(self, table, D, Zk, mom_uu, mom_uf, trGA, gZ):
        """-> d bound / d table through K_uu (moments over the lower channel pairs) and K_uf (all pairs), K_uu's relative jitter
        jitter * mean(diag K_uu) (gpr/model.py:244) included; the model adds what belongs to its bound and runs the kernel's backward.
        gZ = d bound / d Z goes to Z.grad past the channel column (None: Z is not trained)."""
        C, M = table.shape[0], Zk.shape[0]
        gt = _gtable_from_moments(table, mom_uu, D, lower=True) + _gtable_from_moments(table, mom_uf, D, lower=False)
        gz_jit = 0.0
        if _enveloped(table, D):
            # with an envelope (MOHSM) the diagonal follows the points: jitter * mean(diag Kuu) depends on A, L, c AND on Z itself (through autograd in the reference)
            gt += (self.jitter * trGA / M) * self.kernel._point_diag_table_grad(table, Zk, D)
            gz_jit = (self.jitter * trGA / M) * self.kernel._point_diag_input_grad(table, Zk, D)
        else:
            zc = _channel_counts(Zk, C)
            for i in range(C):
                gt[i, i, :, 0] += self.jitter * trGA * zc[i] / M
        if gZ is not None:
            gz = np.zeros(self.Z.data.shape)
            off = 0 if self.kernel.output_dims is None else 1
            gz[:, off:] = -(gZ + gz_jit)
            self.Z.accumulate_grad(gz)
        return gt


class Titsias(_InducingPoints, Model):
    """
    Sparse GP regression, Titsias 2009 (reference gpr/model.py:668-765): the bound
        ELBO = log N(y | 0, Kfu Kuu^-1 Kuf + s2 I) - tr(Kff - Kfu Kuu^-1 Kuf) / (2 s2)
    with trainable inducing inputs `Z` (the channel column of Z carries no gradient) and a SCALAR noise scale.
    """

    def __init__(self, kernel, X, y, Z, Z_init="grid", variance=1.0, jitter=1e-8, mean=None):
        variance = Parameter.to_tensor(variance)
        super().__init__(kernel, X, y, GaussianLikelihood(np.sqrt(variance)), jitter, mean)
        self.Z = self._init_inducing(Z, Z_init)

    def _sigma(self):
        s = np.asarray(self.likelihood.scale())
        if s.ndim != 0 and s.size != 1:
            raise ValueError("Titsias takes a scalar noise variance (reference gpr/model.py:686-689)")
        return float(s.reshape(-1)[0])

    def _run(self, grad):
        h, table, D = self._push()
        Zk = self.kernel._kernel_format(self.Z())
        kff = self._kernel_diag(table, self._local_Xk(), D)                     # envelope: per point
        with self._cholesky_guard():
            res = h.titsias_eval(Zk, self._sigma(), self.jitter, kff, grad=grad, sharded=self._data_shard() is not None)
        return res, table, D, Zk

    def elbo(self):
        res, _, _, _ = self._run(grad=False)
        return config.dtype(res["elbo"])

    def log_marginal_likelihood(self):
        """maximise the lower bound (reference gpr/model.py:726-728)"""
        return self.elbo()

    def _loss_impl(self):
        self.zero_grad(set_to_none=True)
        res, table, D, Zk = self._run(grad=True)
        C = table.shape[0]
        s2 = self._sigma() ** 2
        xc = self._train_counts()
        gt = self._inducing_backward(table, D, Zk, res["mom_uu"], res["mom_uf"], res["trGA"], res["gZ"])
        if _enveloped(table, D):
            # sum_k Kff_diag[k] is a sum over the training points (reference gpr/model.py:723 through autograd)
            self.kernel._spectral_backward(-gt + (0.5 / s2) * self.kernel._point_diag_table_grad(table, self.kernel._kernel_format(self.X), D))
        else:
            # - 1/(2 s2) sum_k Kff_diag[k]  (gpr/model.py:723): K_diag is constant per channel.  Where K_diag[c] is the sum of the diagonal amplitudes
            # (the kernels that keep Kernel._spectral_diag_backward) that is a table gradient too: ONE pass through the parameter algebra instead of two
            if type(self.kernel)._spectral_diag_backward is Kernel._spectral_diag_backward:
                for i in range(C):
                    gt[i, i, :, 0] -= 0.5 * xc[i] / s2
                self.kernel._spectral_backward(-gt)
            else:
                self.kernel._spectral_backward(-gt)
                self.kernel._spectral_diag_backward(0.5 * xc / s2, D)
        scale = self.likelihood.scale
        scale.accumulate_grad(np.reshape(-res["dsigma"], scale.data.shape))
        self._mean_backward(self._handle)
        return config.dtype(-res["elbo"] - self.log_prior())

    def predict_f(self, X, full=False):
        """reference gpr/model.py:730-765"""
        X = self._check_input(X)
        h, table, D = self._push()
        Xsk = self.kernel._kernel_format(X)
        with self._cholesky_guard():
            mu, var = h.titsias_predict(self.kernel._kernel_format(self.Z()), self._sigma(), self.jitter,
                                        Xsk, self._kernel_diag(table, Xsk, D), sharded=self._data_shard() is not None)
            if full:                                        # K_ss - a^T a + b^T b with the a, b this prediction left on the device (reference :758-760)
                var = h.sparse_predict_cov(X.shape[0])
        return self._add_mean(mu, X), var


class Snelson(_InducingPoints, Model):
    """
    Sparse GP regression with pseudo-inputs, Snelson & Ghahramani 2005 (reference gpr/model.py:485-576): the FITC marginal likelihood
        p = log N(y | 0, Qff + diag(Kff - Qff) + sigma^2 I),   Qff = Kfu Kuu^-1 Kuf,
    with trainable inducing inputs `Z` (their channel column carries no gradient) and a scalar or per-channel noise variance.
    """
    _noise_dtype = np.float64

    def __init__(self, kernel, X, y, Z=10, Z_init="grid", variance=1.0, jitter=1e-8, mean=None):
        variance = np.squeeze(Parameter.to_tensor(variance))
        if 1 < variance.ndim or variance.ndim == 1 and variance.shape[0] != kernel.output_dims:
            raise ValueError("variance must be float or have shape (channels,)")
        super().__init__(kernel, X, y, GaussianLikelihood(np.sqrt(variance)), jitter, mean)
        self.Z = self._init_inducing(Z, Z_init)

    def _run(self, grad):
        h, table, D = self._push()
        Zk = self.kernel._kernel_format(self.Z())
        if _enveloped(table, D) and self._data_shard() is not None:
            raise NotImplementedError("Snelson with an enveloped kernel (MOHSM) is single-process only: its per-point diagonal gradient is not reduced "
                                      "over the ranks of the data-parallel form")
        kff = self._kernel_diag(table, self._local_Xk(), D)
        with self._cholesky_guard():
            res = h.snelson_eval(Zk, self._noise_var(), self.jitter, kff, grad=grad, sharded=self._data_shard() is not None)
        return res, table, D, Zk

    def log_marginal_likelihood(self):
        """reference gpr/model.py:516-541"""
        res, _, _, _ = self._run(grad=False)
        return config.dtype(res["lml"])

    def _loss_impl(self):
        self.zero_grad(set_to_none=True)
        res, table, D, Zk = self._run(grad=True)
        C = table.shape[0]
        gt = self._inducing_backward(table, D, Zk, res["mom_uu"], res["mom_uf"], res["trGA"], res["gZ"])
        if _enveloped(table, D):
            # enveloped terms: dp/dKff_nn comes back per training point and goes through the per-point diagonal K_diag(x_n) = sum_t A_t env_t(x_n)
            Xk = self.kernel._kernel_format(self.X)
            h_pt = np.asarray(res["hsum"], dtype=np.float64)
            self.kernel._spectral_backward(-gt - self.kernel._point_diag_table_grad(table, Xk, D, weights=h_pt))
            hsum = np.bincount(Xk[:, 0].astype(np.int64), weights=h_pt, minlength=C).astype(np.float64)
        else:
            self.kernel._spectral_backward(-gt)
            hsum = np.asarray(res["hsum"], dtype=np.float64)                     # d p / d Kff_diag = d p / d sigma^2, summed per channel
            self.kernel._spectral_diag_backward(-hsum, D)
        self._noise_backward(hsum)
        self._mean_backward(self._handle)
        return config.dtype(-res["lml"] - self.log_prior())

    def predict_f(self, X, full=False):
        """reference gpr/model.py:543-576 (its full=True branch uses undefined names; not on this path either)"""
        if full:
            raise NotImplementedError("full predictive covariance for Snelson is not on the HIP path")
        X = self._check_input(X)
        h, table, D = self._push()
        Xsk = self.kernel._kernel_format(X)
        kd, ks = self._kernel_diags(table, Xsk, D)
        with self._cholesky_guard():
            mu, var = h.snelson_predict(self.kernel._kernel_format(self.Z()), self._noise_var(), self.jitter,
                                        Xsk, kd, ks, sharded=self._data_shard() is not None)
        return self._add_mean(mu, X), var


class OpperArchambeau(Model):
    """
    Variational Gaussian approximation of Opper & Archambeau 2009 (reference gpr/model.py:578-668): q(f) = N(K nu, (K^-1 + diag(lambda^2))^-1)
    with one `q_nu` and one positive `q_lambda` per data point;  ELBO = E_q[log p(y | f)] - kl / 2.  The O(N^3) algebra runs on the device in
    two calls around the likelihood (like the Hensman models): forward -> per-point mu, var of q(f) and the kl term; the likelihood (host,
    O(N)) returns its expectation and dE/dmu, dE/dvar; backward -> the gradients of kernel, q_nu, q_lambda.  Any likelihood of gpr/likelihood.py (its expectation and derivatives are the host's; the device algebra never sees it).
    No jitter enters (the reference's Cholesky calls here pass add_jitter=False); `jitter` is kept for the signature.
    """
    _device_mean = False

    def __init__(self, kernel, X, y, likelihood=None, jitter=1e-8, mean=None):
        if likelihood is None:
            likelihood = GaussianLikelihood(1.0)
        super().__init__(kernel, X, y, likelihood, jitter, mean)
        self._mean_refuse("OpperArchambeau (the variational expectation's derivative with respect to y)")
        n = self.X.shape[0]
        self.q_nu = Parameter(np.zeros((n, 1)))
        self.q_lambda = Parameter(np.ones((n, 1)), lower=config.positive_minimum)

    def _handle_y(self):
        return self.y                       # a mean function is subtracted on the host (_targets)

    def _forward(self):
        h, table, D = self._push()
        with self._cholesky_guard():
            res = h.oa_forward(self.q_nu(), self.q_lambda())
        return h, res, table, D

    def _targets(self, mu):
        """reference :604-607, :625-626: with a mean function both the targets and the mean of q(f) have it subtracted"""
        if self.mean is None:
            return self.y, mu
        mean = np.asarray(self.mean(self.X)).reshape(-1)
        return self.y - mean.reshape(-1, 1), mu - mean

    def elbo(self):
        h, res, _, _ = self._forward()
        y, mu = self._targets(res["mu"])
        return config.dtype(self.likelihood.variational_expectation(self._likelihood_X(self.X), y, mu, res["var"]) - 0.5 * res["kl"])

    def log_marginal_likelihood(self):
        """maximise the lower bound (reference gpr/model.py:636-638)"""
        return self.elbo()

    def _loss_impl(self):
        self.zero_grad(set_to_none=True)
        h, res, table, D = self._forward()
        y, mu = self._targets(res["mu"])
        ve, e, f, pgrads = self.likelihood.variational_expectation(self._likelihood_X(self.X), y, mu, res["var"], grad=True)
        bw = h.oa_backward(e, f)
        self.kernel._spectral_backward(-_gtable_from_moments(table, bw["mom"], D, lower=True))
        for p, g in pgrads:
            p.accumulate_grad(np.reshape(-np.asarray(g, dtype=np.float64), p.data.shape))
        self.q_nu.accumulate_grad(-np.reshape(bw["g_nu"], self.q_nu.data.shape))
        self.q_lambda.accumulate_grad(-np.reshape(bw["g_lambda"], self.q_lambda.data.shape))
        return config.dtype(-(ve - 0.5 * res["kl"]) - self.log_prior())

    def predict_f(self, X, full=False):
        """reference gpr/model.py:640-668"""
        X = self._check_input(X)
        h, _, D = self._push()
        with self._cholesky_guard():
            mu, var = h.oa_predict(self.q_nu(), self.q_lambda(), self.kernel._spectral_diag(D), self.kernel._kernel_format(X), full=full)
        return self._add_mean(mu, X), var


class SparseHensman(_InducingPoints, Model):
    """
    Sparse variational GP of Hensman et al. 2015, whitened (reference gpr/model.py:767-878): q(u) = N(L q_mu, L S S^T L^T), L L^T = Kuu,
    S = tril(q_sqrt);  ELBO = E_q[log p(y | f)] - KL(q || p).  The O(N M^2) algebra runs on the device in two calls around the
    likelihood: forward -> per-point mu, var of q(f) at the training inputs; the likelihood (host, O(N)) returns its expectation and
    dE/dmu, dE/dvar; backward -> the gradients of kernel, inducing inputs, q_mu, q_sqrt.  Any likelihood of gpr/likelihood.py (its expectation and derivatives are the host's; the device algebra never sees it).
    The KL term mirrors the reference's (:816-822), which counts only the DIAGONAL of q_sqrt in the trace and the determinant.
    """
    _device_mean = False

    def __init__(self, kernel, X, y, Z=None, Z_init="grid", likelihood=None, jitter=1e-8, mean=None):
        if likelihood is None:
            likelihood = GaussianLikelihood(1.0)
        super().__init__(kernel, X, y, likelihood, jitter, mean)
        self._mean_refuse("%s (the variational expectation's derivative with respect to y)" % self.__class__.__name__)
        self.is_sparse = Z is not None
        if self.is_sparse:
            Z = self._init_inducing(Z, Z_init)
        else:
            self.log_marginal_likelihood_constant = _lml_constant(self.X)
            Z = Parameter(self.X, train=False)              # the data points themselves, not trained (reference :812)
        n = Z.data.shape[0]
        self.q_mu = Parameter(np.zeros((n, 1)))
        self.q_sqrt = Parameter(np.eye(n))
        self.q_sqrt.num_parameters = int((n * n + n) / 2)
        self.Z = Z

    def _shardable(self):
        return self.is_sparse               # the non-sparse model lives on all data points

    def _reduce(self, value):
        """sum of a host scalar / small array over the ranks holding the other shards"""
        comm = self._data_shard()
        if comm is None:
            return value
        a = np.atleast_1d(np.array(value, dtype=np.float64))
        comm.all_reduce_host(a)
        return a if np.ndim(value) else float(a[0])

    def kl_gaussian(self, q_mu, q_sqrt):
        """reference gpr/model.py:816-822"""
        S_diag = np.diagonal(q_sqrt) ** 2
        return 0.5 * (float(np.sum(q_mu * q_mu)) - np.sum(np.log(S_diag)) + np.sum(S_diag) - q_mu.shape[0])

    def _forward(self):
        h, table, D = self._push()
        Zk = self.kernel._kernel_format(self.Z())
        if _enveloped(table, D) and self._data_shard() is not None:
            raise NotImplementedError("SparseHensman with an enveloped kernel (MOHSM) is single-process only: the per-point diagonal gradient is not "
                                      "reduced over the ranks of the data-parallel form")
        kff = self._kernel_diag(table, self._local_Xk(), D)
        with self._cholesky_guard():
            res = h.svgp_forward(Zk, self.q_mu(), self.q_sqrt(), self.jitter, kff, dense=not self.is_sparse)
        return h, res, table, D, Zk

    def _y(self):
        return self.y if self.mean is None else self.y - np.asarray(self.mean(self.X)).reshape(-1, 1)

    def _mu(self, res):
        """q(f)'s mean at the training inputs as the likelihood sees it.  The dense model (reference gpr/model.py:834-837) subtracts the mean
        function from BOTH y and q(f)'s mean, so that it cancels out of the bound -- reproduced; the sparse model (:861) shifts y only."""
        if self.is_sparse or self.mean is None:
            return res["mu"]
        return res["mu"] - self._local(np.asarray(self.mean(self.X)).reshape(-1))

    def elbo(self):
        h, res, _, _, _ = self._forward()
        ve = self.likelihood.variational_expectation(self._local(self._likelihood_X(self.X)), self._local(self._y()), self._mu(res), res["var"])
        return config.dtype(self._reduce(ve) - self.kl_gaussian(self.q_mu(), self.q_sqrt()))

    def log_marginal_likelihood(self):
        """maximise the lower bound (reference gpr/model.py:847-849)"""
        return self.elbo()

    def _loss_impl(self):
        self.zero_grad(set_to_none=True)
        h, res, table, D, Zk = self._forward()
        sharded = self._data_shard() is not None            # data-parallel: mu / var, e, f are those of this rank's points
        ve, e, f, pgrads = self.likelihood.variational_expectation(self._local(self._likelihood_X(self.X)), self._local(self._y()), self._mu(res), res["var"], grad=True)
        ve = self._reduce(ve)
        pgrads = [(p, self._reduce(g)) for p, g in pgrads]
        q_mu, q_sqrt = np.asarray(self.q_mu(), dtype=np.float64), np.asarray(self.q_sqrt(), dtype=np.float64)
        elbo = ve - self.kl_gaussian(q_mu, q_sqrt)
        bw = h.svgp_backward(e, f, sharded=sharded)
        gt = self._inducing_backward(table, D, Zk, bw["mom_uu"], bw["mom_uf"], bw["trGA"], bw["gZ"] if self.is_sparse else None)
        # var_n = K_diag(x_n) - ... goes back through the kernel diagonal with the likelihood's d/dvar_n as weights (the dense model's variance at its own
        # inputs has no such term): per point with enveloped terms, else summed per channel
        if _enveloped(table, D):
            if self.is_sparse:
                gt += self.kernel._point_diag_table_grad(table, self._local_Xk(), D, weights=f)
            self.kernel._spectral_backward(-gt)
        else:
            self.kernel._spectral_backward(-gt)
            if self.is_sparse:
                xc = self._local_Xk()[:, 0].astype(np.int64)
                self.kernel._spectral_diag_backward(-self._reduce(np.bincount(xc, weights=f, minlength=table.shape[0])), D)
        for p, g in pgrads:
            p.accumulate_grad(np.reshape(-np.asarray(g, dtype=np.float64), p.data.shape))
        self.q_mu.accumulate_grad(-(np.reshape(bw["g_qmu"], q_mu.shape) - q_mu))
        s = np.diagonal(q_sqrt)
        self.q_sqrt.accumulate_grad(-(np.tril(bw["g_qsqrt"]) - np.diag(s - 1.0 / s)))
        return config.dtype(-elbo - self.log_prior())

    def predict_f(self, X, full=False):
        """reference gpr/model.py:851-878"""
        X = self._check_input(X)
        h, table, D = self._push()
        Xsk = self.kernel._kernel_format(X)
        kd, ks = self._kernel_diags(table, Xsk, D)
        with self._cholesky_guard():
            res = h.svgp_forward(self.kernel._kernel_format(self.Z()), self.q_mu(), self.q_sqrt(), self.jitter, kd,
                                 Xs=Xsk, kss_diag=ks)
            var = h.sparse_predict_cov(X.shape[0]) if full else np.reshape(res["var"], (-1, 1))      # reference :870-872
        return self._add_mean(np.reshape(res["mu"], (-1, 1)), X), var


class Hensman(SparseHensman):
    """
    The non-sparse variational GP (reference gpr/model.py:880-886): the inducing inputs ARE the data points and are not trained; at the
    training inputs q(f) = N(L q_mu, L S S^T L^T) with L the factor of K_ff itself (reference :834-840) -- the same device algebra with
    a = L^T instead of L^-1 K_uf.  Predictions at new inputs take the sparse formula with Z = X, like the reference (:851-868).
    """

    def __init__(self, kernel, X, y, likelihood=None, jitter=1e-8, mean=None):
        super().__init__(kernel, X, y, None, "grid", likelihood, jitter, mean)
