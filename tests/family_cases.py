"""
What the cases modules of the kernel families share (stationary_cases.py, product_cases.py, trend_cases.py: each keeps its own CASES, data,
single, kernel and seeds, which define tests/golden/<family>*.npz).  numpy only: tests/golden/gen_family.py imports this beside the
reference, the tests beside this package; `G` is the reference's `mogptk.gpr` there and `mogptk_amd.gpr` here.
"""
import importlib

FAMILIES = ("stationary", "product", "trend")               # family -> tests/<family>_cases.py, tests/golden/<family>*.npz


def cases(family):
    return importlib.import_module(family + "_cases")


def full_cases(family):
    """every case but the `light` ones (the dataflow size: LML and gradients only)"""
    CASES = cases(family).CASES
    return [c for c in CASES if not CASES[c].get("light")]


def exact(family, G, case, **kw):
    mod = cases(family)
    X, y, _ = mod.data(case)
    return G.Exact(mod.kernel(G, case), X, y, variance=mod.NOISE, **kw)


def parse(single, G, expr, D, rng):
    """'a*b', 'a+b', '(a+b)*c' over the names of single(G, name, D, rng), which is called from left to right"""
    def split(s, op):
        parts, depth, cur = [], 0, ""
        for ch in s:
            depth += (ch == "(") - (ch == ")")
            if ch == op and depth == 0:
                parts.append(cur); cur = ""
            else:
                cur += ch
        return parts + [cur]

    def product(s):
        ks = [total(f[1:-1]) if f.startswith("(") else single(G, f, D, rng) for f in split(s, "*")]
        return ks[0] if len(ks) == 1 else G.MulKernel(*ks)

    def total(s):
        ks = [product(p) for p in split(s, "+")]
        return ks[0] if len(ks) == 1 else G.AddKernel(*ks)
    return total(expr)


def top(G, k):
    """The reference's Exact adds the noise IN PLACE to what the kernel returns, and autograd needs the output of a product to differentiate
    it: a MulKernel at the top of a model is wrapped in an AddKernel of one (same kernel, a fresh tensor) on both sides."""
    return G.AddKernel(k) if isinstance(k, G.MulKernel) else k
