"""
Trainable mean functions -- host-side mirror of mogptk/gpr/mean.py (Mean, MultiOutputMean, ConstantMean, LinearMean).

The mean enters the Gaussian models only through the residual r = y - m(X) (reference gpr/model.py:445-448).  Every built-in mean is
one affine table on the device (csrc/mean.hip): row c = [b_c, s_c,1 .. s_c,D], m(x) = b_c + sum_d s_c,d x_d for a point of channel c.
`_affine` builds that table from the parameters and `_affine_backward` maps the table's gradient back to them with the chain rule.

A mean written by a user implements `mean(X)` in numpy and, if it has trainable parameters, `backward(X, dmu)`: it adds
d loss / d m(x_k) = dmu[k] to the `.grad` of its parameters (Parameter.accumulate_grad).  This is the one place where the numpy host
cannot stand in for the reference's autograd: the reference differentiates any torch expression in `mean`, here the author of the
mean writes its derivative.  Such means take the host route: the model passes y - m(X) to the device when m(X) changed and hands
dp/dr (mogp_model_fetch, which = 3) to `backward`.

Quirk Q8 (reference gpr/mean.py:77): MultiOutputMean keeps its sub-means in a plain list, not a torch ModuleList, so they are not
sub-modules: `MultiOutputMean.parameters()` is empty, the model's `parameters()` does not list them, `train = ...` does not reach them,
and no optimiser moves them -- yet autograd fills their `.grad`, and since `Model.loss` zeroes only the registered parameters those
`.grad` values ADD UP from one loss() call to the next.  Reproduced as is.
"""
import numpy as np

from .config import config
from .parameter import Parameter, ParameterHolder

__all__ = ["Mean", "MultiOutputMean", "ConstantMean", "LinearMean"]


class Mean(ParameterHolder):
    """Trainable mean function, the counterpart of the kernel (reference gpr/mean.py:4-70)."""

    def __init__(self):
        pass

    def __call__(self, X):
        """mean values of shape (data_points, 1) for X of shape (data_points, input_dims)"""
        X = self._check_input(X)
        return self.mean(X)

    def name(self):
        return self.__class__.__name__

    def _get_name(self):
        return self.__class__.__name__

    def __setattr__(self, name, val):
        if name == "train":
            for p in self.parameters():
                p.train = val
            return
        super().__setattr__(name, val)

    def _check_input(self, X):
        if hasattr(X, "detach"):
            X = X.detach().cpu().numpy()
        X = np.asarray(X, dtype=config.dtype)
        if X.ndim != 2:
            raise ValueError("X should have two dimensions (data_points,input_dims)")
        if X.shape[0] == 0 or X.shape[1] == 0:
            raise ValueError("X must not be empty")
        return X

    def mean(self, X):
        raise NotImplementedError()

    def backward(self, X, dmu):
        """add d loss / d m(X[k]) = dmu[k] (dmu: (data_points, 1)) to the `.grad` of this mean's parameters"""
        raise NotImplementedError()

    def _has_backward(self):
        return type(self).backward is not Mean.backward

    # -- the affine table of the device (csrc/mean.hip); None: not affine, the host route ---------------------------------------
    def _affine(self, C, D, channel_col):
        return None

    def _affine_backward(self, g, channel_col):
        raise NotImplementedError()


class MultiOutputMean(Mean):
    """One mean per channel (reference gpr/mean.py:58-95); sub-mean c sees X[rows of channel c, 1:]."""

    def __init__(self, *means):
        super().__init__()
        if isinstance(means, tuple):
            if len(means) == 1 and isinstance(means[0], list):
                means = means[0]
            else:
                means = list(means)
        elif not isinstance(means, list):
            means = [means]
        if len(means) == 0:
            raise ValueError("must pass at least one mean")
        for mean in means:
            if not issubclass(type(mean), Mean):
                raise ValueError("must pass means")
            elif isinstance(mean, MultiOutputMean):
                raise ValueError("can not nest MultiOutputMeans")
        self.output_dims = len(means)
        object.__setattr__(self, "means", means)          # Q8: a plain list, not registered (see the module docstring)

    def name(self):
        return "[%s]" % (",".join(mean.name() for mean in self.means),)

    def _channel_indices(self, X):
        c = X[:, 0].astype(np.int64)
        return [np.nonzero(c == j)[0] for j in range(self.output_dims)]

    def mean(self, X):
        r = self._channel_indices(X)
        res = np.empty((X.shape[0], 1), dtype=config.dtype)
        for i in range(self.output_dims):
            res[r[i]] = np.reshape(self.means[i].mean(X[r[i], 1:]), (-1, 1))
        return res

    def backward(self, X, dmu):
        r = self._channel_indices(X)
        dmu = np.reshape(dmu, (-1, 1))
        for i in range(self.output_dims):
            if any(True for _ in self.means[i].parameters()):
                self.means[i].backward(X[r[i], 1:], dmu[r[i]])

    def _has_backward(self):
        return all(m._has_backward() or not any(True for _ in m.parameters()) for m in self.means)

    def _affine(self, C, D, channel_col):
        if not channel_col or self.output_dims != C:
            return None
        rows = [m._affine(1, D, False) for m in self.means]
        if any(r is None for r in rows):
            return None
        return np.concatenate(rows, axis=0)

    def _affine_backward(self, g, channel_col):
        for c, m in enumerate(self.means):
            m._affine_backward(g[c:c + 1], False)


class ConstantMean(Mean):
    """m(X) = b (reference gpr/mean.py:97-117)"""

    def __init__(self):
        super().__init__()
        self.bias = Parameter(0.0)

    def mean(self, X):
        return np.repeat(np.reshape(self.bias(), (1, 1)), X.shape[0], axis=0)

    def backward(self, X, dmu):
        self.bias.accumulate_grad(np.reshape(np.sum(dmu), self.bias.data.shape))

    def _affine(self, C, D, channel_col):
        t = np.zeros((C, 1 + D))
        t[:, 0] = float(np.reshape(self.bias(), -1)[0])
        return t

    def _affine_backward(self, g, channel_col):
        self.bias.accumulate_grad(np.reshape(np.sum(g[:, 0]), self.bias.data.shape))


class LinearMean(Mean):
    """m(X) = X a + b (reference gpr/mean.py:119-143).  Under a multi-output kernel a plain LinearMean sees the channel-id column too:
    input_dims = D + 1 there, and slope[0] multiplies the channel id."""

    def __init__(self, input_dims=1):
        super().__init__()
        self.bias = Parameter(0.0)
        self.slope = Parameter(np.zeros(input_dims))

    def mean(self, X):
        return self.bias() + X.dot(np.reshape(self.slope(), (-1, 1)))

    def backward(self, X, dmu):
        dmu = np.reshape(dmu, (-1, 1))
        self.bias.accumulate_grad(np.reshape(np.sum(dmu), self.bias.data.shape))
        self.slope.accumulate_grad(np.reshape(X.T.dot(dmu), self.slope.data.shape))

    def _affine(self, C, D, channel_col):
        s = np.reshape(self.slope(), -1)
        b = float(np.reshape(self.bias(), -1)[0])
        if s.shape[0] != D + (1 if channel_col else 0):
            return None
        t = np.zeros((C, 1 + D))
        if channel_col:                   # b_c = b + s_0 c, s_c,d = s_d (d >= 1)
            t[:, 0] = b + s[0] * np.arange(C)
            t[:, 1:] = s[1:]
        else:
            t[:, 0] = b
            t[:, 1:] = s
        return t

    def _affine_backward(self, g, channel_col):
        self.bias.accumulate_grad(np.reshape(np.sum(g[:, 0]), self.bias.data.shape))
        if channel_col:
            ds = np.concatenate([[np.dot(np.arange(g.shape[0], dtype=np.float64), g[:, 0])], np.sum(g[:, 1:], axis=0)])
        else:
            ds = np.sum(g[:, 1:], axis=0)
        self.slope.accumulate_grad(np.reshape(ds, self.slope.data.shape))
