"""The per-epoch reshuffle of train.DeviceDataset on the MI355X: `mfm_dataset_gather` through the C ABI and through
`DeviceDataset.reshuffle`, against torch indexing on the same device tensors.  It is a copy, so every comparison is of bits
(`torch.equal` on int32 views; the pools hold random bit patterns, NaNs with payloads and denormals among them): no tolerance.

Shapes (N, T, B, D), each the smallest at which a distinct path of the kernel can go wrong:
    1, 1, 1, 1          degenerate
    23, 3, 5, 7         odd D, B no power of two, a tail of 3: dword accesses
    16, 2, 4, 8         everything 16-byte aligned: 16-byte accesses
    18, 2, 4, 6         D even but no multiple of 4: dwords
    70, 20, 32, 325     the reference's shape with a tail; a row is more dwords than a wave has in flight (a second turn)
    9, 2, 4, 280        16-byte accesses, a row longer than one wave instruction (70 accesses for 64 lanes)
    9, 2, 4, 1032       ... and longer than what a wave has in flight (258 accesses: a second turn)
    3001, 3, 7, 5       more rows (8988) than the full grid takes in one turn (8192): the grid-stride loop and the index it
    3001, 3, 7, 8       requests ahead, in both forms
and, through the C ABI only, D % 4 == 0 with a base that is only 4-byte aligned (dwords, chosen on the host).

No GPU run was possible when this file was written: the kernel compiles for gfx950 and the same semantics pass on CPU tensors
(tests/test_shuffle_host.py), but these tests have not run on an MI355X yet."""
import ctypes as C

import numpy as np
import pytest
import torch

from factorized_amd import _lib, configs, engine, synth, train

pytestmark = pytest.mark.gpu
SENTINEL = 0x7FC0DEAD                 # a NaN with a payload: a store over it shows
SHAPES = [(1, 1, 1, 1), (23, 3, 5, 7), (16, 2, 4, 8), (18, 2, 4, 6), (70, 20, 32, 325), (9, 2, 4, 280), (9, 2, 4, 1032),
          (3001, 3, 7, 5), (3001, 3, 7, 8)]
LABELS = {"f32": ((), np.float32), "f32x3": ((3,), np.float32), "i64": ((), np.int64)}


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _bits(t):
    return t.contiguous().view(torch.int32)


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def _arrays(N, T, D, label="f32", seed=0):
    """X [T, N, D] float32 of random BITS, y [N, ...] of the label kind (floats: random bits too)"""
    rng = np.random.RandomState(seed + N + T + D)
    X = rng.randint(-2 ** 31, 2 ** 31, size=(T, N, D), dtype=np.int64).astype(np.int32).view(np.float32)
    shape, dtype = LABELS[label]
    y = rng.randint(-2 ** 31, 2 ** 31, size=(N,) + shape, dtype=np.int64)
    y = y.astype(np.int32).view(np.float32) if dtype == np.float32 else y
    return X, y


def _want(Xp, yp, perm, nb, B):
    """the batch layout by torch indexing on the device: X [nb, T, B, D], y [nb, B, ...]"""
    idx = perm[:nb * B].long()
    T, D = Xp.shape[1], Xp.shape[2]
    return Xp[idx].view(nb, B, T, D).permute(0, 2, 1, 3).contiguous(), yp[idx].view((nb, B) + tuple(yp.shape[1:]))


def _gather(X, y, Xp, yp, perm, nb, B):
    N, T, D = Xp.shape
    ybytes = yp[0].numel() * yp.element_size()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(_lib.lib().mfm_dataset_gather(_ptr(X), _ptr(y), _ptr(Xp), _ptr(yp), _ptr(perm), N, nb, T, B, D, ybytes, stream),
               "mfm_dataset_gather")


def _padded(n, dtype, pad):
    """n elements of `dtype` inside a buffer of sentinel dwords, `pad` dwords on either side -> (buffer as int32, the inside)"""
    words = n * torch.empty((), dtype=dtype).element_size() // 4
    buf = torch.full((pad + words + pad,), SENTINEL, dtype=torch.int32, device="cuda")
    return buf, buf[pad:pad + words].view(dtype)


def _sentinels_intact(buf, pad):
    return bool((buf[:pad] == SENTINEL).all()) and bool((buf[-pad:] == SENTINEL).all())


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%d-%d-%d-%d" % s)
def test_kernel_through_the_abi(shape):
    """random permutation -> the layout of torch indexing, bit for bit; nothing written around X and y; the pool unchanged"""
    _need_gpu()
    N, T, B, D = shape
    nb = N // B
    Xh, yh = _arrays(N, T, D)
    Xp, yp = torch.from_numpy(np.ascontiguousarray(Xh.transpose(1, 0, 2))).cuda(), torch.from_numpy(yh).cuda()
    Xp0, yp0 = Xp.clone(), yp.clone()
    perm = torch.from_numpy(np.random.RandomState(N).permutation(N)).cuda()
    pad = 64                                                    # 256 bytes: X stays 16-byte aligned
    xbuf, X = _padded(nb * T * B * D, torch.float32, pad)
    ybuf, y = _padded(nb * B, torch.float32, pad)
    _gather(X, y, Xp, yp, perm, nb, B)
    wx, wy = _want(Xp0, yp0, perm, nb, B)
    assert torch.equal(_bits(X), _bits(wx).flatten()) and torch.equal(_bits(y), _bits(wy).flatten())
    assert _sentinels_intact(xbuf, pad) and _sentinels_intact(ybuf, pad)
    assert torch.equal(_bits(Xp), _bits(Xp0)) and torch.equal(_bits(yp), _bits(yp0))


@pytest.mark.parametrize("label", list(LABELS))
def test_label_kinds_through_the_abi_and_the_dataset(label):
    _need_gpu()
    N, T, B, D = 23, 3, 5, 7
    nb = N // B
    Xh, yh = _arrays(N, T, D, label)
    ds = train.DeviceDataset.from_arrays(Xh, yh, B, "cuda", pool=True)
    p = np.random.RandomState(1).permutation(N)
    perm = torch.from_numpy(p).cuda()
    wx, wy = _want(ds.X_pool, ds.y_pool, perm, nb, B)
    # the C ABI, into padded buffers
    pad = 16
    xbuf, X = _padded(nb * T * B * D, torch.float32, pad)
    ybuf, y = _padded(wy.numel(), wy.dtype, pad)
    _gather(X, y, ds.X_pool, ds.y_pool, perm, nb, B)
    assert torch.equal(_bits(X), _bits(wx).flatten()) and torch.equal(_bits(y), _bits(wy).flatten())
    assert _sentinels_intact(xbuf, pad) and _sentinels_intact(ybuf, pad)
    # the dataset: the same layout as from_arrays on arrays permuted on the host
    assert ds.reshuffle(perm=p) is ds
    host = train.DeviceDataset.from_arrays(Xh[:, p], yh[p], B, "cuda")
    assert ds.y.dtype == host.y.dtype and ds.y.shape == host.y.shape
    assert torch.equal(_bits(ds.X), _bits(host.X)) and torch.equal(_bits(ds.y), _bits(host.y))
    assert torch.equal(_bits(ds.X), _bits(wx)) and torch.equal(_bits(ds.y), _bits(wy))


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%d-%d-%d-%d" % s)
def test_dataset_reshuffle_identity_twice_and_pool(shape):
    """identity perm = the from_arrays layout; two reshuffles with no synchronisation between them leave the second order;
    the pool keeps its bits"""
    _need_gpu()
    N, T, B, D = shape
    Xh, yh = _arrays(N, T, D)
    ds = train.DeviceDataset.from_arrays(Xh, yh, B, "cuda", pool=True)
    plain = train.DeviceDataset.from_arrays(Xh, yh, B, "cuda")
    assert ds.nb == plain.nb and torch.equal(_bits(ds.X), _bits(plain.X)) and torch.equal(_bits(ds.y), _bits(plain.y))
    Xp0, yp0 = ds.X_pool.clone(), ds.y_pool.clone()
    x_view, y_view = ds.batch(ds.nb - 1)
    ds.reshuffle(seed=1).reshuffle(seed=2)                      # (seed: nothing waits for the device in between)
    p2 = np.random.RandomState(2).permutation(N)
    host = train.DeviceDataset.from_arrays(Xh[:, p2], yh[p2], B, "cuda")
    assert torch.equal(_bits(ds.X), _bits(host.X)) and torch.equal(_bits(ds.y), _bits(host.y))
    assert torch.equal(ds.perm.cpu(), torch.from_numpy(p2))
    # views handed out earlier keep their storage and show the new order
    assert torch.equal(_bits(x_view), _bits(host.X[ds.nb - 1])) and torch.equal(_bits(y_view), _bits(host.y[ds.nb - 1]))
    ds.reshuffle(perm=torch.arange(N, device="cuda"))
    assert torch.equal(_bits(ds.X), _bits(plain.X)) and torch.equal(_bits(ds.y), _bits(plain.y))
    assert torch.equal(_bits(ds.X_pool), _bits(Xp0)) and torch.equal(_bits(ds.y_pool), _bits(yp0))


def test_unaligned_base_takes_dwords():
    """D % 4 == 0, but X (then X_pool) begins 12 bytes into a 16-byte line: the host must not pick 16-byte accesses"""
    _need_gpu()
    N, T, B, D = 16, 2, 4, 8
    nb = N // B
    Xh, yh = _arrays(N, T, D)
    perm = torch.from_numpy(np.random.RandomState(7).permutation(N)).cuda()
    yp = torch.from_numpy(yh).cuda()
    aligned = torch.from_numpy(np.ascontiguousarray(Xh.transpose(1, 0, 2))).cuda()
    pbuf, shifted = _padded(N * T * D, torch.float32, 3)
    shifted.copy_(aligned.flatten())
    for Xp, pad in ((aligned, 3), (shifted.view(N, T, D), 64)):
        xbuf, X = _padded(nb * T * B * D, torch.float32, pad)
        ybuf, y = _padded(nb * B, torch.float32, pad)
        assert (X.data_ptr() % 16 != 0) or (Xp.data_ptr() % 16 != 0)
        _gather(X, y, Xp, yp, perm, nb, B)
        wx, wy = _want(aligned, yp, perm, nb, B)
        assert torch.equal(_bits(X), _bits(wx).flatten()) and torch.equal(_bits(y), _bits(wy).flatten())
        assert _sentinels_intact(xbuf, pad) and _sentinels_intact(ybuf, pad)
    assert _sentinels_intact(pbuf, 3)


@pytest.mark.parametrize("D", [7, 8])
def test_indices_outside_the_pool_are_skipped(D):
    """rows whose index is below 0 or not below N keep their bytes and nothing is read for them (the pool here lies inside a
    larger buffer of sentinels, so a read just outside it would show as sentinels in X)"""
    _need_gpu()
    N, T, B = 12, 2, 4
    nb = N // B
    Xh, yh = _arrays(N, T, D)
    margin = 2 * T * D + (-2 * T * D) % 4                       # two samples' worth, a multiple of 4 dwords
    pbuf, Xp = _padded(N * T * D, torch.float32, margin)
    Xp = Xp.view(N, T, D)
    Xp.copy_(torch.from_numpy(np.ascontiguousarray(Xh.transpose(1, 0, 2))))
    ybuf_p, yp = _padded(N, torch.float32, 4)
    yp.copy_(torch.from_numpy(yh))
    p = np.random.RandomState(3).permutation(N)
    bad = {1: -1, 6: N, 10: N + 1, 11: -2}
    for j, v in bad.items():
        p[j] = v
    perm = torch.from_numpy(p).cuda()
    OLD = 0x12345678
    X = torch.full((nb, T, B, D), OLD, dtype=torch.int32, device="cuda").view(torch.float32)
    y = torch.full((nb, B), OLD, dtype=torch.int32, device="cuda").view(torch.float32)
    _gather(X, y, Xp, yp, perm, nb, B)
    for j in range(nb * B):
        b, r = divmod(j, B)
        if j in bad:
            assert bool((_bits(X[b, :, r]) == OLD).all()) and int(_bits(y[b, r])) == OLD, j
        else:
            assert torch.equal(_bits(X[b, :, r]), _bits(Xp[p[j]])) and torch.equal(_bits(y[b, r]), _bits(yp[p[j]])), j


def test_generator_on_a_side_stream():
    """reshuffle(generator=...) inside torch.cuda.stream(side): after waiting for `side` alone the batches hold nb * B distinct
    pool samples, each whole, labels with them"""
    _need_gpu()
    N, T, B, D = 70, 20, 32, 325
    Xh, _ = _arrays(N, T, D)
    yh = np.arange(N, dtype=np.float32)
    ds = train.DeviceDataset.from_arrays(Xh, yh, B, "cuda", pool=True)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    g = torch.Generator(device="cuda").manual_seed(5)
    with torch.cuda.stream(side):
        assert ds.reshuffle(generator=g) is ds
        assert ds.perm.is_cuda and ds.perm.dtype == torch.int64
    side.synchronize()
    ids = ds.y.flatten().long()
    assert ids.numel() == ds.nb * B and torch.unique(ids).numel() == ds.nb * B            # distinct: each at most once
    assert torch.equal(ids, ds.perm[:ds.nb * B])
    assert torch.equal(torch.sort(ds.perm).values, torch.arange(N, device="cuda"))
    assert not torch.equal(ids, torch.arange(ds.nb * B, device="cuda"))
    wx, wy = _want(ds.X_pool, ds.y_pool, ds.perm, ds.nb, B)
    assert torch.equal(_bits(ds.X), _bits(wx)) and torch.equal(_bits(ds.y), _bits(wy))


def test_reshuffle_refusals_on_the_gpu():
    _need_gpu()
    N, T, B, D = 23, 3, 5, 7
    Xh, yh = _arrays(N, T, D)
    with pytest.raises(_lib.MfmError, match="pool=True"):
        train.DeviceDataset.from_arrays(Xh, yh, B, "cuda").reshuffle(seed=0)
    ds = train.DeviceDataset.from_arrays(Xh, yh, B, "cuda", pool=True)
    before = ds.X.clone()
    for bad in (np.arange(N - 1), np.r_[np.arange(N - 1), 0], np.r_[np.arange(N - 1), N]):
        with pytest.raises(ValueError):
            ds.reshuffle(perm=bad)
    assert torch.equal(_bits(ds.X), _bits(before))
    half = train.DeviceDataset.from_arrays(Xh, yh.astype(np.float16), B, "cuda", pool=True)      # 2-byte label rows
    with pytest.raises(_lib.MfmError, match="multiple of 4 bytes"):
        half.reshuffle(seed=0)


def test_training_step_on_a_reshuffled_batch():
    """after reshuffle(seed=3) one MFM_KL_EF training step on batch(0) gives the loss of a step on the same samples assembled by
    torch indexing, from identical parameters: the reshuffled views are consumable as they are.  The inputs are bit-identical;
    the bar is the suite's 1e-4 relative for losses (the step's atomics order its sums differently from run to run)."""
    _need_gpu()
    cfgs = configs.canonical_configs(dropout=False)
    cfg = cfgs[0]
    N, T, B = 70, 20, 32
    ds = train.DeviceDataset(cfg, N, T, B, "cuda:0", seed=11, pool=True).reshuffle(seed=3)
    idx = torch.from_numpy(np.random.RandomState(3).permutation(N)[:B]).cuda()
    x_hand = ds.X_pool[idx].permute(1, 0, 2).contiguous()
    y_hand = ds.y_pool[idx].contiguous()
    x, y = ds.batch(0)
    assert torch.equal(x, x_hand) and torch.equal(y, y_hand)
    losses = []
    for xb, yb in ((x, y), (x_hand, y_hand)):
        e = engine.MFMEngine(cfgs, device="cuda:0")
        e.load_weights(synth.make_weights(e.layout.shapes, seed=1234))
        losses.append(e.loss_dict(e.train_step(xb, yb))["loss"])
    print("loss on the reshuffled view %.9g, on the hand-assembled batch %.9g" % tuple(losses))
    assert np.isfinite(losses[0]) and abs(losses[0] - losses[1]) <= 1e-4 * abs(losses[1]), losses
