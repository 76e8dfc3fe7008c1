"""
Golden vectors of the `function` kernel family (tests/function_cases.py): gen_family.py itself, run for that family, with one difference.

gen_family.py stores K(X) as its packed lower triangle and asserts that the reference's K equals its transpose bit for bit.  That holds for
every stationary kernel (one expression of |x - x'| per entry) but not for the reference's FunctionKernel, which forms
phi(X) (diag(sigma^2) phi(X)^T) as two matrix products: entry (a, b) multiplies phi_a (sigma^2 phi_b), entry (b, a) phi_b (sigma^2 phi_a),
and the two round differently in the last bit.  Here a square matrix the generator takes from the reference that is symmetric within 4 ulps
of its largest entry (a kernel matrix; a predictive covariance is not and stays as it is) is replaced by the mirror of its lower triangle
-- which is what tests/kernel_family.py:golden_K rebuilds from the packed triangle anyway -- so the generator's assertion (it still fails
for a matrix that is not symmetric to rounding), its packing and everything else run unchanged.
Re-run:  python tests/golden/gen_function.py [path to the reference]
"""
import os
import sys

import numpy as np

sys.argv = [sys.argv[0], "function"] + sys.argv[1:]
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_family             # noqa: E402

_to_numpy = gen_family.N_


def mirrored(t):
    a = _to_numpy(t)
    if a.ndim == 2 and a.shape[0] == a.shape[1] and np.max(np.abs(a - a.T)) <= 4.0 * np.finfo(np.float64).eps * np.max(np.abs(a)):
        a = np.tril(a) + np.tril(a, -1).T
    return a


gen_family.N_ = mirrored

if __name__ == "__main__":
    gen_family.main()
