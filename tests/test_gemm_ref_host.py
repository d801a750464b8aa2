"""tests/gemm_ref.py against numpy's own products: the oracle of tests/test_gpu_gemm_contract.py must itself be right about
strides, batches, pad columns, the biases and accumulate before a kernel is held to it.  No GPU."""
import numpy as np
import pytest
import torch

from tests import gemm_ref as R

M, N, K = 7, 5, 9


def _rs(seed=0):
    return np.random.RandomState(seed)


def _f32(rs, *shape):
    return rs.normal(size=shape).astype(np.float32)


def _close(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max() < 1e-12


def test_contiguous_nn_nt_tn():
    rs = _rs(1)
    A, B = _f32(rs, M, K), _f32(rs, K, N)
    want = A.astype(np.float64) @ B.astype(np.float64)
    c0 = np.full(M * N, 7.0, np.float32)
    # A k-contiguous, B n-contiguous
    assert _close(R.expected(A, B, c0, M, N, K, a_sm=K, a_sk=1, b_sk=N, b_sn=1, ldc=N).reshape(M, N), want)
    # B stored transposed (k-contiguous, the x W^T form)
    Bt = np.ascontiguousarray(B.T)
    assert _close(R.expected(A, Bt, c0, M, N, K, a_sm=K, a_sk=1, b_sk=1, b_sn=K, ldc=N).reshape(M, N), want)
    # A stored transposed (m-contiguous, the dA^T X form)
    At = np.ascontiguousarray(A.T)
    assert _close(R.expected(At, B, c0, M, N, K, a_sm=1, a_sk=M, b_sk=N, b_sn=1, ldc=N).reshape(M, N), want)


def test_sliced_views_and_odd_strides():
    rs = _rs(2)
    wideA, wideB = _f32(rs, M + 2, 2 * K + 3), _f32(rs, 3 * K + 1, 2 * N + 1)
    A = wideA[1:1 + M, 1:1 + 2 * K:2]              # every second column of a wider matrix, from an inner corner
    B = wideB[2:2 + 3 * K:3, 0:2 * N:2]            # every third row, every second column
    want = A.astype(np.float64) @ B.astype(np.float64)
    a_flat = wideA.reshape(-1)[wideA.shape[1] + 1:]    # the pointer is the view's first element
    b_flat = wideB.reshape(-1)[2 * wideB.shape[1]:]
    got = R.expected(a_flat, b_flat, np.zeros(M * N, np.float32), M, N, K, a_sm=wideA.shape[1], a_sk=2,
                     b_sk=3 * wideB.shape[1], b_sn=2, ldc=N)
    assert _close(got.reshape(M, N), want)
    # the transposed view of the same slice: A^T is [K, M]; as the A operand of a K x N x M product
    B2 = _f32(rs, M, N)
    got = R.expected(a_flat, B2, np.zeros(K * N, np.float32), K, N, M, a_sm=2, a_sk=wideA.shape[1], b_sk=N, b_sn=1, ldc=N)
    assert _close(got.reshape(K, N), A.T.astype(np.float64) @ B2.astype(np.float64))


@pytest.mark.parametrize("a_shared,bias_shared", [(False, False), (True, False), (False, True)])
def test_batched_einsum_bias_alpha(a_shared, bias_shared):
    rs = _rs(3)
    Z = 3
    A, B = _f32(rs, 1 if a_shared else Z, M, K), _f32(rs, Z, K, N)
    b1, b2 = _f32(rs, 1 if bias_shared else Z, N), _f32(rs, 1 if bias_shared else Z, N)
    want = 0.5 * np.einsum("zmk,zkn->zmn", np.broadcast_to(A, (Z, M, K)).astype(np.float64), B.astype(np.float64))
    want = want + np.broadcast_to(b1, (Z, N))[:, None, :] + np.broadcast_to(b2, (Z, N))[:, None, :]
    got = R.expected(A, B, np.zeros(Z * M * N, np.float32), M, N, K, a_sm=K, a_sk=1, b_sk=N, b_sn=1, ldc=N, bias=b1,
                     bias2=b2, batch=Z, a_sz=0 if a_shared else M * K, b_sz=K * N, c_sz=M * N,
                     bias_sz=0 if bias_shared else N, alpha=0.5)
    assert _close(got.reshape(Z, M, N), want)


def test_gate_batch_of_one_buffer():
    """the weight-gradient form of tests/test_gpu_ops.py: batch over the gate axis of [rows, 4, Hp] with a_sz = Hp"""
    rs = _rs(4)
    Rr, Hp, Mv = 11, 8, 6
    dA, X = _f32(rs, Rr, 4, Hp), _f32(rs, Rr, N)
    want = np.einsum("rgm,rn->gmn", dA[:, :, :Mv].astype(np.float64), X.astype(np.float64))
    c0 = _f32(rs, 4 * Mv * N)
    got, got2 = R.expected(dA, X, c0, Mv, N, Rr, a_sm=1, a_sk=4 * Hp, b_sk=N, b_sn=1, ldc=N, batch=4, a_sz=Hp, c_sz=Mv * N,
                           accumulate=1, split_k=0, c2=np.zeros_like(c0))
    assert _close(got.reshape(4, Mv, N), want + c0.reshape(4, Mv, N))
    assert _close(got2.reshape(4, Mv, N), want)


@pytest.mark.parametrize("accumulate", [0, 1])
def test_pad_columns_ldc_gap_and_untouched_elements(accumulate):
    rs = _rs(5)
    A, B = _f32(rs, M, K), _f32(rs, K, N)
    nv, ldc = N - 2, N + 3
    c0 = _f32(rs, 4 + M * ldc + 4)                       # a frame of 4 elements on either side
    got = R.expected(A, B, c0[4:], M, N, K, a_sm=K, a_sk=1, b_sk=N, b_sn=1, ldc=ldc, n_valid=nv, accumulate=accumulate)
    body = got[:M * ldc].reshape(M, ldc)
    init = c0[4:4 + M * ldc].reshape(M, ldc).astype(np.float64)
    prod = A.astype(np.float64) @ B[:, :nv].astype(np.float64)
    assert _close(body[:, :nv], prod + (init[:, :nv] if accumulate else 0.0))
    assert np.array_equal(body[:, nv:N], init[:, nv:N] if accumulate else np.zeros((M, N - nv)))
    assert np.array_equal(body[:, N:], init[:, N:])      # the gap [n, ldc)
    assert np.array_equal(got[M * ldc:], c0[4 + M * ldc:].astype(np.float64))
    valid, pad, rest = R.regions(c0.size - 4, M, N, nv, 1, 0, ldc)
    assert valid.size == M * nv and pad.size == M * (N - nv) and rest.sum() == c0.size - 4 - M * N


def test_k_zero_and_refusals():
    rs = _rs(6)
    b1, c0 = _f32(rs, N), _f32(rs, M * N)
    one = np.zeros(1, np.float32)
    assert np.array_equal(R.expected(one, one, c0, M, N, 0, a_sm=0, a_sk=1, b_sk=1, b_sn=0, ldc=N, bias=b1).reshape(M, N),
                          np.broadcast_to(b1.astype(np.float64), (M, N)))
    assert not R.expected(one, one, c0, M, N, 0, a_sm=0, a_sk=1, b_sk=1, b_sn=0, ldc=N).any()
    got = R.expected(one, one, c0, M, N, 0, a_sm=0, a_sk=1, b_sk=1, b_sn=0, ldc=N, bias=b1, accumulate=1)
    assert _close(got.reshape(M, N), c0.reshape(M, N).astype(np.float64) + b1)
    with pytest.raises(ValueError, match="split_k needs accumulate"):
        R.expected(one, one, c0, M, N, 1, a_sm=0, a_sk=1, b_sk=1, b_sn=0, ldc=N, split_k=2)


def test_bf16_rounding_is_nearest_even():
    rs = _rs(7)
    x = np.concatenate([_f32(rs, 4096) * np.float32(10.0) ** rs.randint(-20, 20, 4096).astype(np.float32),
                        np.array([0.0, -0.0, 1.0, 1.00390625, 1.01171875, 3e38, -3e38], np.float32)])   # two exact ties
    want = torch.from_numpy(x).bfloat16().float().numpy()
    assert np.array_equal(R.bf16_round(x), want.astype(np.float64))
    A, B = _f32(rs, M, K), _f32(rs, K, N)
    got = R.expected(A, B, np.zeros(M * N, np.float32), M, N, K, a_sm=K, a_sk=1, b_sk=N, b_sn=1, ldc=N, round_bf16=True)
    bf = lambda v: torch.from_numpy(v).bfloat16().float().numpy().astype(np.float64)     # noqa: E731
    assert _close(got.reshape(M, N), bf(A) @ bf(B))
