"""TEST INFRASTRUCTURE ONLY -- the inputs and the float64 reference of the projected query (Fusion.add_projection), shared
by tests/test_projection_host.py (CPU) and tests/test_gpu_projection.py (MI355X).

Cases are oracle/field_cases.py shapes with a linear head attached to their first map.  The reference is float64:
oracle.field_ref.field64 on the SOURCE map gives the fused values v[n,C] and the per-entry rounding scale s[n,C]; the
expected output is (v - mean) W^T, and the magnitude an implementation may round at is
    A[n,j] = sum_c s[n,c] |W[j,c]| + sum_c |mean_c W[j,c]|.
The assertion is |got - ref| <= tol * A with the non-finite entries coinciding (field_ref.check).
"""
import torch

from oracle import field_cases as FC
from oracle import field_ref as R

F64 = torch.float64
EPS32 = 2.0 ** -24

# name -> (oracle/field_cases.py case, k).  Between them: patch-resolution and dense sources, fp32 and fp16 storage, a
# channel-range view, C = 65, 129, 384, 1000 and 1024, k = 1, 3, 16 and 64, 1 to 9 views, lattices, random clouds and the
# small surface-like clouds of the direct cases, eval and batch_eval.
CASES = {
    "patch V4 C384 k3": ("direct V4 C384", 3),
    "patch V1 C1000 k16": ("direct V1 C1000", 16),
    "patch V9 C65 k1": ("direct V9 C65 + C64", 1),
    "patch V2 C384 k64": ("direct V2 C384 C1024", 64),
    "channel-range view k3": ("direct channel-range view", 3),
    "patch f16 C129 k64": ("direct f16 C129 + C128", 64),
    "dense C1024 k64": ("wide dense C1024", 64),
    "dense C1024 k3": ("wide dense C1024", 3),
    "batch_eval reorder off k16": ("batch_eval, reorder off", 16),
    "lattice patch C384 k16": ("window lattice", 16),
    "lattice dense f16 C384 k3": ("sliced lattice f16", 3),
    "cloud dense C384 k16": ("sliced cloud", 16),
}
HOST_CASES = ("patch V4 C384 k3", "patch V1 C1000 k16", "patch V9 C65 k1", "patch f16 C129 k64", "channel-range view k3")


def head(m, k, seed):
    """(W [k,C] float32, mean [C] float64) for map m: N(0,1) rows and the map's own per-channel mean, as a PCA would carry."""
    C = m.shape[3]
    g = torch.Generator().manual_seed(1000 + seed)
    W = torch.randn(k, C, generator=g)
    mean = m.to(F64).mean((0, 1, 2))
    return W, mean


def build(name):
    """The field case with 'source' (name of its first map), 'head_W', 'head_mean', 'k' added; only the projected name is queried."""
    base, k = CASES[name]
    case = FC.CASES[base]()
    case["source"] = case["names"][0]
    case["head_W"], case["head_mean"] = head(case["maps"][case["source"]], k, k)
    case["k"] = k
    return case


def reference(case, rows=None, source_map=None):
    """(ref [n,k] float64, A [n,k] float64) on `rows`: (v - mean) W^T and the magnitude of the docstring above."""
    m = case["maps"][case["source"]] if source_map is None else source_map
    vals, scales = R.field64(case["obs"], case["pts"], case["H"], case["W"], case["mu"], [m], rows=rows)
    return project64(vals[0], scales[0], case["head_W"], case["head_mean"])


def project64(v, s, W, mean):
    W64 = W.to(F64)
    ref = (v - mean) @ W64.T
    A = s @ W64.abs().T + (mean.abs() @ W64.abs().T)
    return ref, A


def rounding_cap(C, V):
    """The worst-case float32 rounding of the whole chain per unit of A: C products and sums of the head, four corner
    weights and a weight per view, and the few operations of the fold and the subtraction of b."""
    return (C + 4 * V + 8) * EPS32


def tolerance(port_worst, C, V):
    """3 x the worst ratio of the float32 port on the host (the ratio field_ref.TOL / PORT_WORST uses), capped by the
    worst-case rounding bound."""
    return min(3.0 * port_worst, rounding_cap(C, V))


# ---- descriptor colours -------------------------------------------------------------------------------------------------
def colour_inputs(n=20000, NI=5, seed=11):
    """proj [n,3] float32 (three scales, as principal components have) and a one-hot mask [n,NI] float32"""
    g = torch.Generator().manual_seed(seed)
    proj = torch.randn(n, 3, generator=g) * torch.tensor([30.0, 7.0, 0.5])
    inst = torch.randint(0, NI, (n,), generator=g)
    mask = torch.nn.functional.one_hot(inst, NI).float()
    return proj, mask


def colour_rule64(proj, mask):
    """float64 [n,4] colour values BEFORE the truncation, in byte units (x * 255; alpha exactly 255), and the half-width of
    what float32 may make of them: the subtraction, the range, the division and the product each round once (2^-24
    relative of a value <= 1), so x is within 4 * 2^-24 and 255 x within 255 times that."""
    p = proj.to(F64)
    lo, hi = p.min(0).values, p.max(0).values
    rgb = (p - lo) / (hi - lo)
    rgb[mask.argmax(1) == 0] = 0.8
    val = torch.cat((torch.flip(rgb, dims=(-1,)) * 255.0, torch.full((p.shape[0], 1), 255.0, dtype=F64)), 1)
    bound = torch.full_like(val, 255.0 * 4 * EPS32)
    bound[:, 3] = 0.0
    return val, bound


def check_colours(got_u8, proj, mask, cap=0.01):
    """(ok, share of bytes that differ from the float64 rule's own byte, message): every byte is floor(255 x) for some x
    within the bound of the float64 value, and at most `cap` of the bytes differ from floor of the float64 value itself."""
    val, bound = colour_rule64(proj, mask)
    got = got_u8.cpu().to(F64)
    lo, hi = torch.floor(val - bound).clamp(0, 255), torch.floor(val + bound).clamp(0, 255)
    inside = (got >= lo) & (got <= hi)
    share = float((got != torch.floor(val).clamp(0, 255)).double().mean())
    if not bool(inside.all()):
        i = (~inside).nonzero()[0].tolist()
        return False, share, "byte %s: got %d, float64 value %.9g" % (i, int(got[tuple(i)]), float(val[tuple(i)]))
    return share <= cap, share, "share of differing bytes %.3g (cap %.3g)" % (share, cap)
