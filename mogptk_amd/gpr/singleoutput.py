"""
Single-output spectral kernels on the HIP path -- host-side mirror of mogptk/gpr/singleoutput.py for
SpectralKernel (:520-561) and SpectralMixtureKernel (:563-605), and for the stationary kernels whose distance is a function of
s = sum_d V_d tau_d^2: SquaredExponentialKernel (:218-268), RationalQuadraticKernel (:270-323), MaternKernel (:607-655) and
ExponentialKernel (:181-216).  Those are ONE term each, M = Psi = Delta = 0, with a radial profile phi_kind(s) in place of the Gaussian
(DESIGN 1b); the device evaluates the profile per entry (csrc/gram.hip: radial_profile).
"""
import numpy as np

from .config import config
from .parameter import Parameter
from .kernel import Kernel, term_width, cached_terms, KIND_TIMES, KIND_DOT, KIND_WDOT, KIND_WHITE
from .multioutput import _accumulate

FOUR_PI2 = 4.0 * np.pi ** 2


class SpectralMixtureKernel(Kernel):
    """
    K = sum_q sum_d mag_q exp(-2 pi^2 tau_d^2 v_qd) cos(2 pi tau_d mu_qd)   (reference :594-600; the einsum
    SUMS over the input dimension d).  Each (q, d) is one spectral term that touches dimension d only.
    Parameters: magnitude (Q,), mean (Q,D), variance (Q,D).
    """

    def __init__(self, Q=1, input_dims=1, active_dims=None):
        super().__init__(input_dims, active_dims)
        self.magnitude = Parameter(np.ones(Q), lower=config.positive_minimum)
        self.mean = Parameter(np.zeros((Q, input_dims)), lower=config.positive_minimum)
        self.variance = Parameter(np.ones((Q, input_dims)), lower=config.positive_minimum)

    @cached_terms
    def _spectral_terms(self, D):
        if D != self.input_dims:
            raise ValueError("X must have %d input dimensions" % self.input_dims)
        mag, mu, var = self.magnitude(), self.mean(), self.variance()
        Q = mag.shape[0]
        table = np.zeros((1, 1, Q * D, term_width(D)))
        for q in range(Q):
            for d in range(D):
                t = q * D + d
                table[0, 0, t, 0] = mag[q]
                table[0, 0, t, 2 + d] = FOUR_PI2 * var[q, d]          # exp(-1/2 V u^2) with V = 4 pi^2 v
                table[0, 0, t, 2 + D + d] = mu[q, d]
        return table

    def _parts(self, D):
        """one part per component q: its D rows"""
        Q = self.magnitude.shape[0]
        return self._row_parts(D, [self.name()] * Q, np.arange(Q + 1) * D)

    def _spectral_diag(self, D):
        return np.array([np.sum(self.magnitude())])                      # reference :602-605 (not x D)

    def _spectral_diag_backward(self, gc, D):
        _accumulate(self.magnitude, np.full(self.magnitude.shape, float(gc[0])))

    def _spectral_backward(self, gtable):
        D = self.input_dims
        Q = self.magnitude.shape[0]
        g = gtable[0, 0].reshape(Q, D, term_width(D))
        idx = np.arange(D)
        _accumulate(self.magnitude, np.sum(g[:, :, 0], axis=1))
        _accumulate(self.mean, g[:, idx, 2 + D + idx])
        _accumulate(self.variance, FOUR_PI2 * g[:, idx, 2 + idx])


class SpectralKernel(Kernel):
    """K = mag sum_d exp(-2 pi^2 tau_d^2 v_d) cos(2 pi tau_d mu_d)   (reference :555-561)."""

    def __init__(self, input_dims=1, active_dims=None):
        super().__init__(input_dims, active_dims)
        self.magnitude = Parameter(1.0, lower=config.positive_minimum)
        self.mean = Parameter(np.zeros(input_dims), lower=config.positive_minimum)
        self.variance = Parameter(np.ones(input_dims), lower=config.positive_minimum)

    @cached_terms
    def _spectral_terms(self, D):
        if D != self.input_dims:
            raise ValueError("X must have %d input dimensions" % self.input_dims)
        mag, mu, var = self.magnitude(), self.mean(), self.variance()
        table = np.zeros((1, 1, D, term_width(D)))
        for d in range(D):
            table[0, 0, d, 0] = mag
            table[0, 0, d, 2 + d] = FOUR_PI2 * var[d]
            table[0, 0, d, 2 + D + d] = mu[d]
        return table

    def _spectral_diag(self, D):
        return np.array([float(self.magnitude())])                       # reference :558-561

    def _spectral_diag_backward(self, gc, D):
        _accumulate(self.magnitude, np.reshape(float(gc[0]), self.magnitude.shape))

    def _spectral_backward(self, gtable):
        D = self.input_dims
        g = gtable[0, 0]
        idx = np.arange(D)
        _accumulate(self.magnitude, np.sum(g[:, 0]))
        _accumulate(self.mean, g[idx, 2 + D + idx])
        _accumulate(self.variance, FOUR_PI2 * g[idx, 2 + idx])


# radial profile of a term (include/mogp_hip.h: mogp_model_set_kinds)
KIND_GAUSS, KIND_RQ, KIND_MATERN12, KIND_MATERN32, KIND_MATERN52, KIND_PERIODIC, KIND_SINC = 0, 1, 2, 3, 4, 5, 6      # (KIND_DOT = 7, KIND_GATE = 8, KIND_WDOT = 9, KIND_WHITE = 10: gpr/kernel.py)


class _RadialKernel(Kernel):
    """One term A phi_kind(sum_d V_d tau_d^2) with V_d = _vscale / l_d^2: magnitude (scalar) and lengthscale ((input_dims,), or a scalar
    shared by every dimension).  Subclasses set `_kind`, `_shape` and `_vscale`."""
    _kind = KIND_GAUSS
    _vscale = 1.0

    def _profile_shape(self):
        return 0.0

    def _precision(self, D):
        if D != self.input_dims:
            raise ValueError("X must have %d input dimensions" % self.input_dims)
        l = np.asarray(self.lengthscale(), dtype=np.float64)
        return np.broadcast_to(self._vscale / np.square(l), (D,))

    @cached_terms
    def _spectral_terms(self, D):
        table = np.zeros((1, 1, 1, term_width(D)))
        table[0, 0, 0, 0] = self.magnitude()
        table[0, 0, 0, 2:2 + D] = self._precision(D)
        return table

    @cached_terms
    def _spectral_kinds(self, D):
        return np.full((1, 1, 1), self._kind, dtype=np.int32), np.full((1, 1, 1), float(self._profile_shape()))

    def _spectral_diag(self, D):
        return np.array([float(self.magnitude())])                       # K_diag = magnitude (phi(0) = 1)

    def _spectral_diag_backward(self, gc, D):
        _accumulate(self.magnitude, np.reshape(float(gc[0]), self.magnitude.shape))

    def _spectral_backward(self, gtable):
        D = self.input_dims
        g = gtable[0, 0, 0]
        _accumulate(self.magnitude, np.reshape(g[0], self.magnitude.shape))
        l = np.asarray(self.lengthscale(), dtype=np.float64)
        gl = g[2:2 + D] * (-2.0 * self._vscale / np.broadcast_to(l, (D,)) ** 3)      # d V_d / d l_d
        _accumulate(self.lengthscale, gl if l.ndim else np.reshape(np.sum(gl), l.shape))


def _check_order(order, name):
    if 0 < order:
        raise NotImplementedError("%s with order > 0 is not on the HIP path: cross lengthscales make the precision a full matrix M = L L^T + "
                                  "diag(l)^-2, and a term of the device's table carries a diagonal V only" % name)


class SquaredExponentialKernel(_RadialKernel):
    """K = mag exp(-1/2 sum_d tau_d^2 / l_d^2) (reference :218-268): an ordinary Gaussian term (kind 0, no cosine), so it runs wherever term
    tables run.  order = 0: one lengthscale per dimension; order = -1: one for all."""

    def __init__(self, order=0, input_dims=1, active_dims=None):
        super().__init__(input_dims, active_dims)
        _check_order(order, "SquaredExponentialKernel")
        self.order = order
        self.magnitude = Parameter(1.0, lower=config.positive_minimum)
        self.lengthscale = Parameter(np.ones(input_dims) if -1 < order else 1.0, lower=config.positive_minimum)


class RationalQuadraticKernel(_RadialKernel):
    """K = mag (1 + sum_d tau_d^2 / l_d^2 / (2 alpha))^-alpha (reference :270-323); alpha is a plain float, as there."""
    _kind = KIND_RQ

    def __init__(self, alpha=1.0, order=0, input_dims=1, active_dims=None):
        super().__init__(input_dims, active_dims)
        _check_order(order, "RationalQuadraticKernel")
        self.alpha = alpha
        self.order = order
        self.magnitude = Parameter(1.0, lower=config.positive_minimum)
        self.lengthscale = Parameter(np.ones(input_dims) if -1 < order else 1.0, lower=config.positive_minimum)

    def _profile_shape(self):
        return self.alpha


def _check_one_dim(input_dims, name, distance):
    if input_dims != 1:
        raise NotImplementedError("%s with input_dims > 1 is not on the HIP path: the reference measures distance there as %s, which is not a "
                                  "function of sum_d V_d tau_d^2" % (name, distance))


class MaternKernel(_RadialKernel):
    """K = mag c_nu(r) exp(-sqrt(2 nu) r), r = |tau| / l, nu in {0.5, 1.5, 2.5} (reference :607-655); one input dimension."""

    def __init__(self, nu=0.5, input_dims=1, active_dims=None):
        super().__init__(input_dims, active_dims)
        if nu not in [0.5, 1.5, 2.5]:
            raise ValueError("nu parameter must be 0.5, 1.5, or 2.5")
        _check_one_dim(input_dims, "MaternKernel", "|sum_d tau_d / l_d|")
        self.nu = nu
        self.magnitude = Parameter(1.0, lower=1e-6)
        self.lengthscale = Parameter(np.ones(input_dims), lower=1e-6)

    @property
    def _kind(self):
        return {0.5: KIND_MATERN12, 1.5: KIND_MATERN32, 2.5: KIND_MATERN52}[self.nu]


class ExponentialKernel(_RadialKernel):
    """K = mag exp(-|tau| / (2 l)) (reference :181-216): the Matern 1/2 profile with V = 1 / (4 l^2); one input dimension."""
    _kind = KIND_MATERN12
    _vscale = 0.25

    def __init__(self, input_dims=1, active_dims=None):
        super().__init__(input_dims, active_dims)
        _check_one_dim(input_dims, "ExponentialKernel", "sum_d |tau_d| / l_d")
        self.magnitude = Parameter(1.0, lower=config.positive_minimum)
        self.lengthscale = Parameter(np.ones(input_dims), lower=config.positive_minimum)


class _MagnitudeKernel(Kernel):
    """shared by the kernels below: K_diag = magnitude (reference :64-67, :376-379, :433-436, :470-473)"""

    def _check_dims(self, D):
        if D != self.input_dims:
            raise ValueError("X must have %d input dimensions" % self.input_dims)

    def _spectral_diag(self, D):
        return np.array([float(self.magnitude())])

    def _spectral_diag_backward(self, gc, D):
        _accumulate(self.magnitude, np.reshape(float(gc[0]), self.magnitude.shape))


class ConstantKernel(_MagnitudeKernel):
    """K = mag (reference :37-67): a Gaussian term with V = M = 0, so it runs wherever term tables run; times another kernel it scales it."""

    def __init__(self, input_dims=1, active_dims=None):
        super().__init__(input_dims, active_dims)
        self.magnitude = Parameter(1.0, lower=config.positive_minimum)

    @cached_terms
    def _spectral_terms(self, D):
        self._check_dims(D)
        table = np.zeros((1, 1, 1, term_width(D)))
        table[0, 0, 0, 0] = self.magnitude()
        return table

    def _spectral_backward(self, gtable):
        _accumulate(self.magnitude, np.reshape(gtable[0, 0, 0, 0], self.magnitude.shape))


class CosineKernel(_MagnitudeKernel):
    """K = mag cos(2 pi sum_d tau_d / l_d) (reference :438-473): a Gaussian term with V = 0 and M_d = 1 / l_d -- an ordinary table row."""

    def __init__(self, input_dims=1, active_dims=None):
        super().__init__(input_dims, active_dims)
        self.magnitude = Parameter(1.0, lower=config.positive_minimum)
        self.lengthscale = Parameter(np.ones(input_dims), lower=config.positive_minimum)

    @cached_terms
    def _spectral_terms(self, D):
        self._check_dims(D)
        table = np.zeros((1, 1, 1, term_width(D)))
        table[0, 0, 0, 0] = self.magnitude()
        table[0, 0, 0, 2 + D:2 + 2 * D] = 1.0 / np.asarray(self.lengthscale(), dtype=np.float64)
        return table

    def _spectral_backward(self, gtable):
        D = self.input_dims
        g = gtable[0, 0, 0]
        _accumulate(self.magnitude, np.reshape(g[0], self.magnitude.shape))
        l = np.asarray(self.lengthscale(), dtype=np.float64)
        _accumulate(self.lengthscale, -g[2 + D:2 + 2 * D] / np.square(l))         # d M_d / d l_d


def _check_periodic(order, input_dims, name):
    _check_order(order, name)
    if input_dims != 1:
        raise NotImplementedError("%s with input_dims > 1 is not on the HIP path: the reference sums sin^2(pi tau_d / p_d) / l_d^2 over the "
                                  "dimensions, which is not a function of the one phase a term of the device's table carries" % name)


class PeriodicKernel(_MagnitudeKernel):
    """K = mag exp(-2 sin^2(pi tau / p) / l^2) = mag exp(V (cos theta - 1)), V = 1 / l^2, theta = 2 pi tau / p (reference :325-379): one row of
    kind 5, whose phase (M = 1 / p) is the ARGUMENT of the profile.  One input dimension; order 0 or -1 (the lengthscale's shape)."""

    def __init__(self, order=0, input_dims=1, active_dims=None):
        super().__init__(input_dims, active_dims)
        _check_periodic(order, input_dims, "PeriodicKernel")
        self.order = order
        self.magnitude = Parameter(1.0, lower=config.positive_minimum)
        self.period = Parameter(np.ones(input_dims), lower=config.positive_minimum)
        self.lengthscale = Parameter(np.ones(input_dims) if -1 < order else 1.0, lower=config.positive_minimum)

    def _l(self):
        return float(np.asarray(self.lengthscale(), dtype=np.float64).reshape(-1)[0])

    @cached_terms
    def _spectral_terms(self, D):
        self._check_dims(D)
        table = np.zeros((1, 1, 1, term_width(D)))
        table[0, 0, 0, 0] = self.magnitude()
        table[0, 0, 0, 2] = 1.0 / self._l() ** 2
        table[0, 0, 0, 3] = 1.0 / float(self.period()[0])
        return table

    @cached_terms
    def _spectral_kinds(self, D):
        return np.full((1, 1, 1), KIND_PERIODIC, dtype=np.int32), np.zeros((1, 1, 1))

    def _periodic_backward(self, g, gV):
        """g: the periodic row's table gradient; gV: d / d V summed over every row that carries V = 1 / l^2"""
        _accumulate(self.magnitude, np.reshape(g[0], self.magnitude.shape))
        _accumulate(self.period, np.reshape(-g[3] / float(self.period()[0]) ** 2, self.period.shape))
        _accumulate(self.lengthscale, np.reshape(-2.0 * gV / self._l() ** 3, self.lengthscale.shape))

    def _spectral_backward(self, gtable):
        g = gtable[0, 0, 0]
        self._periodic_backward(g, g[2])


class LocallyPeriodicKernel(PeriodicKernel):
    """K = mag exp(-2 sin^2(pi tau / p) / l^2) exp(-tau^2 / (2 l^2)) (reference :381-436): ONE product group of a periodic row (the magnitude on
    it) and a Gaussian row of unit amplitude; both carry V = 1 / l^2."""

    def __init__(self, order=0, input_dims=1, active_dims=None):
        Kernel.__init__(self, input_dims, active_dims)
        _check_periodic(order, input_dims, "LocallyPeriodicKernel")
        self.order = order
        self.magnitude = Parameter(1.0, lower=config.positive_minimum)
        self.period = Parameter(np.ones(input_dims), lower=config.positive_minimum)
        self.lengthscale = Parameter(np.ones(input_dims) if -1 < order else 1.0, lower=config.positive_minimum)

    @cached_terms
    def _spectral_terms(self, D):
        self._check_dims(D)
        table = np.zeros((1, 1, 2, term_width(D)))
        table[0, 0, 0, 0] = self.magnitude()
        table[0, 0, :, 2] = 1.0 / self._l() ** 2
        table[0, 0, 0, 3] = 1.0 / float(self.period()[0])
        table[0, 0, 1, 0] = 1.0
        return table

    @cached_terms
    def _spectral_kinds(self, D):
        return np.array([[[KIND_PERIODIC | KIND_TIMES, KIND_GAUSS]]], dtype=np.int32), np.zeros((1, 1, 2))

    def _spectral_backward(self, gtable):
        g = gtable[0, 0]
        self._periodic_backward(g[0], g[0, 2] + g[1, 2])


class SincKernel(_MagnitudeKernel):
    """K = mag sinc(bandwidth tau) cos(2 pi frequency tau), sinc(r) = sin(pi r) / (pi r) (reference :475-518): one row of kind 6 with
    V = bandwidth^2 and M = frequency -- an ordinary radial profile with its cosine beside it.  One input dimension."""

    def __init__(self, input_dims=1, active_dims=None):
        super().__init__(input_dims, active_dims)
        _check_one_dim(input_dims, "SincKernel", "sum_d tau_d bandwidth_d inside the sinc")
        self.magnitude = Parameter(1.0, lower=config.positive_minimum)
        self.frequency = Parameter(np.ones(input_dims), lower=config.positive_minimum)
        self.bandwidth = Parameter(np.ones(input_dims), lower=config.positive_minimum)

    @cached_terms
    def _spectral_terms(self, D):
        self._check_dims(D)
        table = np.zeros((1, 1, 1, term_width(D)))
        table[0, 0, 0, 0] = self.magnitude()
        table[0, 0, 0, 2] = float(self.bandwidth()[0]) ** 2
        table[0, 0, 0, 3] = float(self.frequency()[0])
        return table

    @cached_terms
    def _spectral_kinds(self, D):
        return np.full((1, 1, 1), KIND_SINC, dtype=np.int32), np.zeros((1, 1, 1))

    def _spectral_backward(self, gtable):
        g = gtable[0, 0, 0]
        _accumulate(self.magnitude, np.reshape(g[0], self.magnitude.shape))
        _accumulate(self.frequency, np.reshape(g[3], self.frequency.shape))
        _accumulate(self.bandwidth, np.reshape(2.0 * float(self.bandwidth()[0]) * g[2], self.bandwidth.shape))      # d V / d bandwidth


DOT_DEGREE_MAX = 8


class LinearKernel(Kernel):
    """K = mag <x, x'> + bias (reference :69-101): one dot-product row (kind 7) of degree 1 -- the magnitude in the amplitude slot, the
    bias in the Psi slot, which no cosine reads there.  Not stationary: K_diag = mag |x|^2 + bias follows the point."""
    _degree = 1

    def __init__(self, input_dims=1, active_dims=None):
        super().__init__(input_dims, active_dims)
        self.bias = Parameter(0.0, lower=0.0)
        self.magnitude = Parameter(1.0, lower=config.positive_minimum)

    @cached_terms
    def _spectral_terms(self, D):
        if D != self.input_dims:
            raise ValueError("X must have %d input dimensions" % self.input_dims)
        table = np.zeros((1, 1, 1, term_width(D)))
        table[0, 0, 0, 0] = self.magnitude()
        table[0, 0, 0, 1] = self.bias()
        return table

    @cached_terms
    def _spectral_kinds(self, D):
        return np.full((1, 1, 1), KIND_DOT, dtype=np.int32), np.full((1, 1, 1), float(self._degree))

    def _spectral_diag(self, D):
        raise NotImplementedError("%s has no diagonal value per channel: K(x, x) follows the point (Kernel._point_diag)" % self.name())

    def _spectral_backward(self, gtable):
        g = gtable[0, 0, 0]
        _accumulate(self.bias, np.reshape(g[1], self.bias.shape))
        _accumulate(self.magnitude, np.reshape(g[0], self.magnitude.shape))


class PolynomialKernel(LinearKernel):
    """K = (mag <x, x'> + bias)^degree (reference :103-138): the dot-product row of degree `degree`, a plain integer from 1 to 8 (the device
    multiplies it out)."""

    def __init__(self, degree, input_dims=1, active_dims=None):
        Kernel.__init__(self, input_dims, active_dims)
        if int(degree) != degree or not 1 <= degree <= DOT_DEGREE_MAX:
            raise NotImplementedError("PolynomialKernel with degree %r is not on the HIP path: the device multiplies the power out, an integer "
                                      "degree from 1 to %d" % (degree, DOT_DEGREE_MAX))
        self.degree = degree
        self.bias = Parameter(0.0, lower=0.0)
        self.magnitude = Parameter(1.0, lower=config.positive_minimum)

    @property
    def _degree(self):
        return int(self.degree)


class WhiteKernel(_MagnitudeKernel):
    """K(X) = mag I and K(X, X') = 0 (reference :5-35): one white row (kind 10) -- the identity by INDEX, not by distance: two
    different points with equal inputs do not see each other.  A noise term inside the kernel: per channel under
    IndependentMultiOutputKernel, or as a factor of a product (White x k = diag(mag k(x, x)))."""

    def __init__(self, input_dims=1, active_dims=None):
        super().__init__(input_dims, active_dims)
        self.magnitude = Parameter(1.0, lower=config.positive_minimum)

    @cached_terms
    def _spectral_terms(self, D):
        self._check_dims(D)
        table = np.zeros((1, 1, 1, term_width(D)))
        table[0, 0, 0, 0] = self.magnitude()
        return table

    @cached_terms
    def _spectral_kinds(self, D):
        return np.full((1, 1, 1), KIND_WHITE, dtype=np.int32), np.zeros((1, 1, 1))

    def _spectral_backward(self, gtable):
        _accumulate(self.magnitude, np.reshape(gtable[0, 0, 0, 0], self.magnitude.shape))


class FunctionKernel(Kernel):
    """K(x, x') = phi(x) diag(mag) phi(x')^T (reference :140-179): explicit basis functions.  `phi` maps a float64 array (n, input_dims) to
    (n, F); `magnitude` (F,) are the weights sigma_f^2.  phi is the user's Python and runs on the host: its values travel to the device as F
    further input columns behind the model's own (Kernel._kernel_format), and the kernel is ONE weighted-dot row (kind 9) with unit
    amplitude whose V slots on those columns hold the magnitude.  In the composition's own table (D columns) the row is [1, 0, ...]; the
    re-laying to the device's columns, and the magnitude's gradient from the row's V columns, happen at the seam (Kernel._device_terms,
    Kernel._table_backward).  The row's shape slot, which the device does not read for this kind, names the first feature column of the
    leaf it came from: that is how a row copied into a product or under LMC finds its weights.  K_diag follows the point."""
    _feature_offset = 0

    def __init__(self, phi, input_dims=1, active_dims=None):
        super().__init__(input_dims, active_dims)
        out = phi(np.ones((42, input_dims), dtype=np.float64))
        if not isinstance(out, np.ndarray) or out.dtype != np.float64:
            raise ValueError("phi must return an array of the same dtype as the input")
        if out.ndim != 2 or out.shape[0] != 42:
            raise ValueError("phi must take (data_points,input_dims) as input, and return (data_points,feature_dims) as output")
        self.magnitude = Parameter(np.ones(out.shape[1]), lower=config.positive_minimum)
        self.phi = phi

    def _features(self):
        return int(self.magnitude.data.size)

    def _phi_values(self, x):
        """phi at the inputs x (n, input_dims) -> (n, F) float64"""
        out = np.asarray(self.phi(np.ascontiguousarray(x, dtype=np.float64)), dtype=np.float64)
        if out.shape != (x.shape[0], self._features()):
            raise ValueError("phi returned %s for %d points; the kernel was built for (data_points, %d)" % (out.shape, x.shape[0], self._features()))
        return out

    @cached_terms
    def _spectral_terms(self, D):
        if D != self.input_dims:
            raise ValueError("X must have %d input dimensions" % self.input_dims)
        table = np.zeros((1, 1, 1, term_width(D)))
        table[0, 0, 0, 0] = 1.0
        return table

    def _spectral_kinds(self, D):
        return np.full((1, 1, 1), KIND_WDOT, dtype=np.int32), np.full((1, 1, 1), float(self._feature_offset))

    def _spectral_diag(self, D):
        raise NotImplementedError("%s has no diagonal value per channel: K(x, x) follows the point (Kernel._point_diag)" % self.name())

    def _spectral_backward(self, gtable):
        pass                                                   # the unit amplitude is no parameter; the magnitude's gradient comes from the device's V columns (Kernel._table_backward)
