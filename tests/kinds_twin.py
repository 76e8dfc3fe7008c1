"""
One numpy twin for every row kind of the exact path, 0 - 10, composed from what exists: oracle/table_model.py carries kinds
0 - 7 and the periodic row for D = 1, tests/changepoint_twin.py the gate row (kind 8), tests/function_twin.py the weighted-dot row
(kind 9), the white row (kind 10) and the periodic row beside further input columns (kind 5, D > 1).  The two family twins cannot both
be installed -- function_twin keeps the oracle's `row_parts` it saw at import and would lose the gate row -- so the dispatch is written
here, over the row functions themselves; the walks over channel pairs that tell the white row whether a block pairs a point set with
itself are function_twin's.  The device class is cv_twin's (eval, fetch, loo, cv) with a prediction that takes the kernel's diagonal per
test point whenever a dot-product, gate or weighted-dot row is present, as the library does.  Nothing here is edited into the oracle:
`install(monkeypatch)` puts it in place for one test and leaves nothing behind.
"""
import numpy as np
from scipy.linalg import solve_triangular

import oracle.table_model as tm
import changepoint_twin
import function_twin
import cv_twin
from function_twin import gram_from_table, moments_dense, _gram_block      # the walks that carry the "same point set" flag

KIND_PERIODIC, KIND_DOT, KIND_GATE, KIND_WDOT, KIND_WHITE = 5, 7, 8, 9, 10
POINT_KINDS = (KIND_DOT, KIND_GATE, KIND_WDOT)              # K(x, x) follows the point: kss_diag per test point
_oracle_row_parts = function_twin._oracle["row_parts"]     # the oracle's own, as function_twin saw it at its import
assert _oracle_row_parts.__module__ == tm.__name__, "the oracle's row_parts was already replaced when the family twins were imported"


def row_parts(row, kind, shape, x1, x2):
    if kind == KIND_GATE:
        assert x1.shape[1] == 1, "a gate row takes one input dimension"
        return changepoint_twin.gate_row_parts(row, x1, x2)
    if kind == KIND_WDOT:
        assert x1.shape[1] >= 2, "a weighted-dot row takes the inputs and at least one feature column"
        return function_twin.wdot_row_parts(row, x1, x2)
    if kind == KIND_WHITE:
        return function_twin.white_row_parts(row, x1, x2)
    if kind == KIND_PERIODIC and x1.shape[1] > 1:
        return function_twin.periodic_row_parts(row, x1, x2)
    return _oracle_row_parts(row, kind, shape, x1, x2)


def has_point_rows(kind):
    return kind is not None and bool(np.any(np.isin(np.asarray(kind) & tm.KIND_MASK, POINT_KINDS)))


class KindsTableDevice(cv_twin.CvTableDevice):
    """the numpy stand-in of mogptk_amd._lib.ExactHandle for tables of any kinds: eval, fetch, loo, cv, predict"""

    def predict(self, noise_var, jitter, kss_diag, Xs, full=False, data_var=None):
        if full or not has_point_rows(self.kind):
            return super().predict(noise_var, jitter, kss_diag, Xs, full=full, data_var=data_var)
        K, _ = self._Kj(noise_var, jitter, data_var)
        L = np.linalg.cholesky(K)
        Kfs = self._gram(self.X, Xs)
        alpha = solve_triangular(L.T, solve_triangular(L, self.y, lower=True), lower=False)
        v = solve_triangular(L, Kfs, lower=True)
        kdiag = np.asarray(kss_diag, dtype=np.float64).reshape(-1)
        assert kdiag.shape == (Xs.shape[0],), "with a dot-product, gate or weighted-dot row kss_diag holds one value per test point"
        return Kfs.T @ alpha, (kdiag - np.sum(v * v, axis=0)).reshape(-1, 1)


def install(monkeypatch, handle=False):
    """every kind into the oracle's walk over rows, the same-set flag into its walks over channel pairs, the device class into the
    scaffold; handle: also in the place of the device handle itself (tests without a device)"""
    import kernel_family as kf
    from mogptk_amd import _lib
    monkeypatch.setattr(tm, "row_parts", row_parts)
    monkeypatch.setattr(tm, "_gram_block", _gram_block)
    monkeypatch.setattr(tm, "gram_from_table", gram_from_table)
    monkeypatch.setattr(tm, "moments_dense", moments_dense)
    monkeypatch.setattr(kf, "gram_from_table", gram_from_table)
    monkeypatch.setattr(kf, "TableDevice", KindsTableDevice)
    if handle:
        monkeypatch.setattr(_lib, "ExactHandle", KindsTableDevice)
