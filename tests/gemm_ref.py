"""Float64 reference of the grouped GEMM's descriptor (include/mfm_hip.h, MfmGemmDesc), for tests/test_gpu_gemm_contract.py.
A plain module like tests/cases.py.  It takes every field literally -- flat host copies of the allocations that the device
pointers address, element offsets z*a_sz + m*a_sm + k*a_sk and so on -- and knows nothing about tiles, splits or layouts, so
the same call describes a contiguous matrix, a transposed view, a slice of a wider one and a batch of any of them.
tests/test_gemm_ref_host.py holds it to numpy's own products."""
import numpy as np


def flat(x):
    """the allocation as the pointer sees it: one flat float array (None stays None)"""
    return None if x is None else np.asarray(x).reshape(-1)


def bf16_round(x):
    """finite float32 values rounded to bf16 (nearest, ties to even) and back, as float64"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32).astype(np.float64)


def index(batch, rows, cols, sz, sr, sc):
    """element offsets [batch, rows, cols] of a strided, batched operand: z*sz + r*sr + c*sc"""
    z = np.arange(batch, dtype=np.int64)[:, None, None]
    r = np.arange(rows, dtype=np.int64)[None, :, None]
    c = np.arange(cols, dtype=np.int64)[None, None, :]
    return z * sz + r * sr + c * sc


def regions(size, m, n, n_valid, batch, c_sz, ldc):
    """-> (offsets of the valid elements, offsets of the pad columns [n_valid, n), boolean mask of everything else) of a C
    allocation of `size` elements"""
    idx = index(batch, m, n, c_sz, ldc, 1)
    valid, pad = idx[:, :, :n_valid].reshape(-1), idx[:, :, n_valid:].reshape(-1)
    rest = np.ones(size, dtype=bool)
    rest[valid] = False
    rest[pad] = False
    return valid, pad, rest


def expected(a, b, c, m, n, k, a_sm, a_sk, b_sk, b_sn, ldc, bias=None, bias2=None, n_valid=None, batch=1,
             a_sz=0, b_sz=0, c_sz=0, bias_sz=0, accumulate=0, split_k=1, alpha=1.0, c2=None, round_bf16=False):
    """The arguments of engine.make_gemm with host arrays in place of tensors: a, b, bias, bias2 the operands' allocations,
    c (and c2) the INITIAL contents of the outputs' allocations.  Returns the expected contents of c, or of (c, c2) when c2
    is given, as flat float64 arrays: elements the call does not own keep their initial value.

      C[z][i][j] (+)= alpha * sum_k A(z,i,k) B(z,k,j) + bias[z][j] + bias2[z][j]     for j < n_valid
      columns [n_valid, n): zeros for a plain product, untouched under accumulate

    split_k changes how the sum is dealt to workgroups, never its value; round_bf16 rounds A and B to bf16 first."""
    nv = n if n_valid is None else n_valid
    if not (m > 0 and n > 0 and k >= 0 and batch > 0 and 0 <= nv <= n):
        raise ValueError("bad dims")
    if split_k > 1 and not accumulate:
        raise ValueError("split_k needs accumulate")
    a, b, bias, bias2 = flat(a), flat(b), flat(bias), flat(bias2)
    rnd = bf16_round if round_bf16 else (lambda v: np.asarray(v, dtype=np.float64))
    acc = np.zeros((batch, m, nv), dtype=np.float64)
    if k > 0 and nv > 0:
        A = rnd(a[index(batch, m, k, a_sz, a_sm, a_sk)])         # [z, m, k]
        B = rnd(b[index(batch, k, nv, b_sz, b_sk, b_sn)])        # [z, k, n]
        for kk in range(k):
            acc += A[:, :, kk, None] * B[:, kk, None, :]
    val = float(np.float32(alpha)) * acc
    for bv in (bias, bias2):
        if bv is not None and nv > 0:
            val = val + bv[index(batch, 1, nv, bias_sz, 0, 1)].astype(np.float64)
    idx = index(batch, m, n, c_sz, ldc, 1)
    outs = []
    for c0 in (c, c2):
        if c0 is None:
            continue
        out = flat(c0).astype(np.float64).copy()
        if accumulate:
            np.add.at(out, idx[:, :, :nv], val)
        else:
            out[idx[:, :, :nv]] = val
            out[idx[:, :, nv:]] = 0.0
        outs.append(out)
    return outs[0] if c2 is None else tuple(outs)
