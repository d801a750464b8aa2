"""train.DeviceDataset's per-epoch reshuffle without a GPU: on CPU tensors `reshuffle` is torch indexing, so its semantics --
the order, the seeds, the rotating tail, what is refused -- are checked here against `from_arrays` on arrays permuted on the
host (the only way to a new order before `reshuffle` existed), bit for bit; plus the sharded iteration and the native entry
point's host-side argument checks."""
import ctypes as C

import numpy as np
import pytest
import torch

from factorized_amd import _lib, train

N, T, B, D = 23, 3, 5, 7            # odd D, B no power of two, a tail of 3


def _arrays(n=N, t=T, d=D, label_shape=(), dtype=np.float32, seed=0):
    rng = np.random.RandomState(seed)
    X = rng.randn(t, n, d).astype(np.float32)
    y = rng.randn(*((n,) + label_shape)).astype(dtype) if dtype == np.float32 else rng.randint(0, 7, size=(n,) + label_shape).astype(dtype)
    return X, y


def _same(a, b):
    return torch.equal(a.X, b.X) and torch.equal(a.y, b.y) and a.nb == b.nb


def test_pool_leaves_the_batches_as_they_were():
    X, y = _arrays()
    plain = train.DeviceDataset.from_arrays(X, y, B, "cpu")
    pooled = train.DeviceDataset.from_arrays(X, y, B, "cpu", pool=True)
    assert _same(pooled, plain) and pooled.nb == N // B
    assert pooled.X_pool.shape == (N, T, D) and pooled.y_pool.shape == (N,)          # the tail is resident too
    assert torch.equal(pooled.X_pool, torch.from_numpy(X).transpose(0, 1)) and torch.equal(pooled.y_pool, torch.from_numpy(y))
    assert plain.X_pool is None


def test_pool_on_the_synthetic_constructor():
    from factorized_amd import configs
    cfg = configs.canonical_configs()[0]
    plain = train.DeviceDataset(cfg, 13, 2, 4, "cpu", seed=11)
    pooled = train.DeviceDataset(cfg, 13, 2, 4, "cpu", seed=11, pool=True)
    assert _same(pooled, plain) and pooled.X_pool.shape[:2] == (13, 2)
    pooled.reshuffle(perm=torch.arange(13))
    assert _same(pooled, plain)


@pytest.mark.parametrize("label_shape,dtype", [((), np.float32), ((3,), np.float32), ((), np.int64)])
def test_reshuffle_equals_from_arrays_on_permuted_arrays(label_shape, dtype):
    X, y = _arrays(label_shape=label_shape, dtype=dtype)
    ds = train.DeviceDataset.from_arrays(X, y, B, "cpu", pool=True)
    rng = np.random.RandomState(5)
    tail_seen = False
    for _ in range(4):
        p = rng.permutation(N)
        assert ds.reshuffle(perm=p) is ds
        assert _same(ds, train.DeviceDataset.from_arrays(X[:, p], y[p], B, "cpu"))
        assert torch.equal(ds.perm, torch.from_numpy(p))
        tail_seen = tail_seen or bool((p[:ds.nb * B] >= ds.nb * B).any())
    assert tail_seen                 # a sample of the original tail (index >= 20) sits in some batch
    assert np.array_equal(X, _arrays(label_shape=label_shape, dtype=dtype)[0])          # the caller's arrays are not written
    assert np.array_equal(y, _arrays(label_shape=label_shape, dtype=dtype)[1])


def test_reshuffle_accepts_a_tensor_and_earlier_views_see_the_new_order():
    X, y = _arrays()
    ds = train.DeviceDataset.from_arrays(X, y, B, "cpu", pool=True)
    x0, y0 = ds.batch(0)
    p = torch.from_numpy(np.random.RandomState(2).permutation(N)).to(torch.int32)
    ds.reshuffle(perm=p)
    want = train.DeviceDataset.from_arrays(X[:, p.numpy()], y[p.numpy()], B, "cpu")
    assert torch.equal(x0, want.X[0]) and torch.equal(y0, want.y[0])
    assert x0.data_ptr() == ds.X.data_ptr()


def test_seed_is_numpys_randomstate_permutation():
    X, y = _arrays()
    a = train.DeviceDataset.from_arrays(X, y, B, "cpu", pool=True).reshuffle(seed=3)
    b = train.DeviceDataset.from_arrays(X, y, B, "cpu", pool=True).reshuffle(seed=3)
    c = train.DeviceDataset.from_arrays(X, y, B, "cpu", pool=True).reshuffle(seed=4)
    assert _same(a, b) and not torch.equal(a.X, c.X)
    p = np.random.RandomState(3).permutation(N)
    assert _same(a, train.DeviceDataset.from_arrays(X[:, p], y[p], B, "cpu"))
    assert _same(a.reshuffle(3), b)          # positional, and from any earlier order: the pool is the source


def test_generator_gives_a_permutation():
    X, y = _arrays()
    y = np.arange(N, dtype=np.float32)
    ds = train.DeviceDataset.from_arrays(X, y, B, "cpu", pool=True)
    ds.reshuffle(generator=torch.Generator().manual_seed(1))
    assert torch.equal(torch.sort(ds.perm).values, torch.arange(N))
    assert torch.equal(ds.y.flatten().long(), ds.perm[:ds.nb * B])
    first = ds.perm.clone()
    ds.reshuffle(generator=torch.Generator().manual_seed(2))
    assert not torch.equal(ds.perm, first)


@pytest.mark.parametrize("bad", [
    np.arange(N - 1),                                    # wrong length
    np.arange(N + 1),
    np.r_[np.arange(N - 1), 0],                          # a repeated index
    np.r_[np.arange(N - 1), N],                          # out of range, above
    np.r_[np.arange(1, N), -1],                          # ... and below
    np.arange(N, dtype=np.float32),                      # not integers
    np.arange(N).reshape(1, N),                          # not one-dimensional
])
def test_bad_permutations_raise(bad):
    X, y = _arrays()
    ds = train.DeviceDataset.from_arrays(X, y, B, "cpu", pool=True)
    before = ds.X.clone()
    with pytest.raises(ValueError):
        ds.reshuffle(perm=bad)
    assert torch.equal(ds.X, before)


def test_exactly_one_source_of_order():
    X, y = _arrays()
    ds = train.DeviceDataset.from_arrays(X, y, B, "cpu", pool=True)
    with pytest.raises(ValueError, match="exactly one"):
        ds.reshuffle()
    with pytest.raises(ValueError, match="exactly one"):
        ds.reshuffle(seed=1, perm=np.arange(N))
    with pytest.raises(ValueError, match="exactly one"):
        ds.reshuffle(1, generator=torch.Generator())


def test_reshuffle_without_a_pool_raises():
    X, y = _arrays()
    ds = train.DeviceDataset.from_arrays(X, y, B, "cpu")
    with pytest.raises(_lib.MfmError, match="pool=True"):
        ds.reshuffle(seed=1)


def test_batches_are_the_sharded_batches():
    X, y = _arrays(n=37)             # 7 batches: world 2 takes 3 each and drops one
    ds = train.DeviceDataset.from_arrays(X, y, B, "cpu", pool=True).reshuffle(seed=9)
    assert ds.nb == 7
    whole = list(ds.batches())
    assert len(whole) == 7 and all(torch.equal(x, ds.X[i]) and torch.equal(t, ds.y[i]) for i, (x, t) in enumerate(whole))
    shards = [list(ds.batches(rank, 2)) for rank in range(2)]
    assert [len(s) for s in shards] == [3, 3]
    for rank, shard in enumerate(shards):
        idx = train.shard_batches(ds.nb, rank, 2)
        assert idx == [rank + 2 * i for i in range(3)]
        for i, (x, t) in zip(idx, shard):
            assert x.data_ptr() == ds.X[i].data_ptr() and t.data_ptr() == ds.y[i].data_ptr()
    ptrs = [x.data_ptr() for s in shards for x, _ in s]
    assert len(set(ptrs)) == 6          # disjoint


def test_library_exports_the_entry_point():
    L = _lib.lib()
    assert hasattr(L, "mfm_dataset_gather") and "mfm_dataset_gather" in _lib.exported_names()
    assert L.mfm_abi_version() == 5


def test_gather_launch_validates_on_the_host():
    """argument errors are caught before anything is enqueued (no device memory is touched: the pointers are never used)"""
    L = _lib.lib()
    base = 1 << 24

    def ptr(off):
        return C.c_void_p(base + off)

    good = dict(X=ptr(0), y=ptr(1 << 20), Xp=ptr(2 << 20), yp=ptr(3 << 20), perm=ptr(4 << 20), N=N, nb=N // B, T=T, B=B, D=D, ybytes=4)
    cases = [
        (dict(X=None), b"must not be null"),
        (dict(y=None), b"must not be null"),
        (dict(Xp=None), b"must not be null"),
        (dict(yp=None), b"must not be null"),
        (dict(perm=None), b"must not be null"),
        (dict(N=0), b"must be positive"),
        (dict(nb=0), b"must be positive"),
        (dict(T=0), b"must be positive"),
        (dict(B=-1), b"must be positive"),
        (dict(D=0), b"must be positive"),
        (dict(nb=N // B + 1), b"in the pool"),
        (dict(ybytes=0), b"multiple of 4"),
        (dict(ybytes=6), b"multiple of 4"),
        (dict(N=1 << 40, nb=1 << 20, T=1 << 10, B=2), b"rows"),
        (dict(X=ptr(2)), b"4-byte aligned"),
        (dict(yp=ptr((3 << 20) + 1)), b"4-byte aligned"),
        (dict(perm=ptr((4 << 20) + 4)), b"8-byte aligned"),
        (dict(X=ptr((2 << 20) + 64)), b"must not overlap"),
        (dict(y=ptr((3 << 20) + 8)), b"must not overlap"),
    ]
    for over, msg in cases:
        a = dict(good, **over)
        rc = L.mfm_dataset_gather(a["X"], a["y"], a["Xp"], a["yp"], a["perm"], a["N"], a["nb"], a["T"], a["B"], a["D"], a["ybytes"],
                                  None)
        assert rc == -1, over
        assert msg in L.mfm_last_error(), (over, L.mfm_last_error())
