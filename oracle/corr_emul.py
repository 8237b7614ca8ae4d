"""TEST INFRASTRUCTURE ONLY -- float32 emulations of the pairwise-distance kernels of csrc/corr_kernels.hip, in numpy.

They exist to calibrate oracle/corr_ref.py's per-entry distance bound on the CPU (tests/test_corr_ref.py): each one
repeats a kernel's float32 operation sequence -- channel order, accumulator split, fused multiply-adds -- so its error
against float64 is the error the kernel makes, without a GPU.
  direct(a, b)            pairwise_dist_body: per 32-channel stage and float4 k-quad, d = a - b, then the even pair of the
                          quad into accumulator x and y (fmaf), then the odd pair; d^2 = x + y.
  contraction(a, b)       pairwise_mfma_body: |a|^2 + |b|^2 - 2 a.b.  a.b is an fmaf chain over the channels in the
                          order the MFMA comment states (stage, half r, component c, slot s: channel k0 + 4 (4 r + s) + c);
                          |a|^2 is sixteen partial sums (four waves x float4), combined (x+y)+(z+w) per wave and then
                          (w0+w1)+(w2+w3).  guard=True applies the kernel's guard: a pair with d^2 < 1/4 (|a|^2+|b|^2)
                          (or a non-finite |a|^2+|b|^2) is recomputed by its wave (64 lanes x float4, butterfly sum), or
                          the whole 64 x 64 tile in the direct form past 96 such pairs.  guard=False returns the raw
                          contraction (what the guard exists to reject).
  chain(a, b)             dist_to_target_kernel with one lane per descriptor (BCHW maps): one fmaf chain over the
                          channels in order.
Each v_mfma_f32_16x16x4_f32 is modelled as a chain of four fmaf in slot order; how the hardware rounds inside one MFMA is
not specified, so the calibrated ratio of the guarded form describes this model, and the device is held to the same bound
only by tests/test_gpu_corr.py passing on it.
fmaf(x, y, z) is emulated as float32(float64(x) * y + z): the product is exact in float64, so only the final sum is
rounded twice (a 2^-53 effect, far below the bounds calibrated here).
"""
import numpy as np

F32 = np.float32
F64 = np.float64


def _fma(x, y, z):
    return (x.astype(F64) * y + z).astype(F32)


def direct(a, b):
    """float32 d^2 [B1,B2] of pairwise_dist_body (C need not be a multiple of 32: missing channels are zeros)."""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    C = a.shape[1]
    Cp = (C + 3) // 4 * 4
    if Cp != C:
        a = np.pad(a, ((0, 0), (0, Cp - C)))
        b = np.pad(b, ((0, 0), (0, Cp - C)))
    x = np.zeros((a.shape[0], b.shape[0]), F32)
    y = np.zeros_like(x)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(0, Cp, 4):
            d = [(a[:, None, k + t] + (-b[None, :, k + t])).astype(F32) for t in range(4)]
            x = _fma(d[0], d[0], x)
            y = _fma(d[1], d[1], y)
            x = _fma(d[2], d[2], x)
            y = _fma(d[3], d[3], y)
        return (x + y).astype(F32)


def chain(a, b):
    """float32 d^2 [B1,B2] as one fmaf chain per pair in channel order (dist_to_target_kernel, G = 1)."""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    acc = np.zeros((a.shape[0], b.shape[0]), F32)
    with np.errstate(invalid="ignore", over="ignore"):
        for c in range(a.shape[1]):
            d = (a[:, None, c] - b[None, :, c]).astype(F32)
            acc = _fma(d, d, acc)
    return acc


def _norms(a):
    """|a|^2 per row as pairwise_mfma_body's stash(): wave w squares k-quads w and w + 4 of every 32-channel stage."""
    C = a.shape[1]
    parts = []
    with np.errstate(over="ignore", invalid="ignore"):
        for w in range(4):
            acc = np.zeros((a.shape[0], 4), F32)
            for k0 in range(0, C, 32):
                for k4 in (w, w + 4):
                    q = a[:, k0 + 4 * k4:k0 + 4 * k4 + 4]
                    acc = _fma(q, q, acc)
            parts.append(((acc[:, 0] + acc[:, 1]).astype(F32) + (acc[:, 2] + acc[:, 3]).astype(F32)).astype(F32))
        return ((parts[0] + parts[1]).astype(F32) + (parts[2] + parts[3]).astype(F32)).astype(F32)


def _wave_direct(a, b):
    """The guard's per-pair recompute: lane l sums k-quads l, l + 64, ... (x: components 0, 2; y: 1, 3), then a butterfly."""
    C = a.shape[0]
    lanes = np.zeros((64, 2), F32)
    for l in range(64):
        for k4 in range(l, C // 4, 64):
            d = (a[4 * k4:4 * k4 + 4] - b[4 * k4:4 * k4 + 4]).astype(F32)
            lanes[l] = _fma(d[0:2], d[0:2], lanes[l])
            lanes[l] = _fma(d[2:4], d[2:4], lanes[l])
    s = (lanes[:, 0] + lanes[:, 1]).astype(F32)
    off = 32
    while off:
        s = (s + s[np.arange(64) ^ off]).astype(F32)
        off >>= 1
    return s[0]


def contraction(a, b, guard=True):
    """float32 d^2 [B1,B2] of pairwise_mfma_body (C % 32 == 0, as the host requires for that kernel)."""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    B1, C = a.shape
    B2 = b.shape[0]
    assert C % 32 == 0
    acc = np.zeros((B1, B2), F32)
    with np.errstate(over="ignore", invalid="ignore"):
        for k0 in range(0, C, 32):
            for r in range(2):
                for c in range(4):
                    for s in range(4):
                        ch = k0 + 4 * (4 * r + s) + c
                        acc = _fma(a[:, None, ch], b[None, :, ch], acc)
        na, nb = _norms(a), _norms(b)
        nsum = (na[:, None] + nb[None, :]).astype(F32)
        d2 = _fma(np.full_like(acc, -2.0), acc, nsum)
        if not guard:
            return d2
        flag = ~((d2 >= F32(0.25) * nsum) & (nsum < np.inf))
    out = d2.copy()
    dense = None
    for i0 in range(0, B1, 64):
        for j0 in range(0, B2, 64):
            f = flag[i0:i0 + 64, j0:j0 + 64]
            n = int(f.sum())
            if n > 96:
                if dense is None:
                    dense = direct(a, b)
                out[i0:i0 + 64, j0:j0 + 64] = dense[i0:i0 + 64, j0:j0 + 64]
            elif n:
                for i, j in zip(*np.nonzero(f)):
                    out[i0 + i, j0 + j] = _wave_direct(a[i0 + i], b[j0 + j])
    return out
