"""
Predictions of every full case of the kernel families (family_cases.FAMILIES) without a device: predict_f (diagonal and full) and predict_y
of gpr.Exact over the numpy twin of the device handle (oracle/table_model.py: kinds, product groups, the per-point diagonal of dot-product
rows) against mu, var, cov, ymu, yvar of the goldens, at the tolerance the device is held to: 1e-9 relative to max(1, max |want|)
(tests/kernel_family.py).
"""
import pytest

from mogptk_amd import _lib
import kernel_family as kf
from family_cases import FAMILIES, full_cases
from oracle.table_model import TableDevice


@pytest.mark.parametrize("family,case", [(f, c) for f in FAMILIES for c in full_cases(f)])
def test_predictions_over_the_twin_match_the_reference(family, case, monkeypatch):
    monkeypatch.setattr(_lib, "ExactHandle", TableDevice)
    kf.check_predictions(family, case)
