"""Host-side checks of M_D.loss_and_grad (mfm_train_ablation_d, csrc/train_ablation.hip): the new symbols in the header, the
library and the binding; the workspace query; the entry's argument checks and refusals, which answer before anything touches a
device; the module surface, its argument checks, the composed path on the CPU against the oracle, and pickling.  No GPU compute
here.  Reference: oracle/mfm_oracle_extra.M_D with the weights of tests/golden/extra_M_D.npz and torch autograd on it; bound: the
project's 1e-4 relative fp32 tolerance per tensor, against the tensor's largest magnitude."""
import ctypes as C
import os
import pickle
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from factorized_amd import _lib, configs, synth
from oracle import mfm_oracle_extra as X
from tests.cases import rel_err
from tests.extra_cases import load_extra

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["mfm_train_ablation_d", "mfm_train_ablation_d_workspace_floats", "mfm_train_ablation_d_tile_rows", "mfm_train_ablation_d_mask_offset"]
SIZES = [32, 8, 80, 32, 88, 8, 8, 16, 300, 5, 20, 1]          # zl za zv zy fl fa fv fy d_l d_a d_v output_dim
ODD = [3, 5, 7, 1, 28, 1, 20, 12, 37, 3, 11, 2]
TOL = 1e-4
NP = 32


def _declared():
    src = open(os.path.join(ROOT, "include", "mfm_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return set(re.findall(r"\b(mfm_[a-z0-9_]+)\s*\(", src))


def test_new_symbols_are_declared_exported_and_bound():
    L = _lib.lib()
    declared, bound = _declared(), set(_lib.exported_names())
    for n in NEW:
        assert n in declared, "include/mfm_hip.h does not declare %s" % n
        assert hasattr(L, n), "libmfm_hip.so does not export %s" % n
        assert n in bound, "_lib.py does not bind %s" % n
    assert declared == bound
    assert L.mfm_abi_version() == 5 == _lib.ABI_VERSION


def test_the_header_documents_the_contract():
    src = open(os.path.join(ROOT, "include", "mfm_hip.h")).read()
    doc = src[src.index("One training step of the ablation M_D"):src.index("int64_t mfm_train_ablation_d_workspace_floats")]
    for word in ("32 DEVICE pointers", "enqueue nothing", "frozen", "ticket", "DROPOUT SCALES", "MFM_ERR_UNSUPPORTED", "accumulate", "no forked branches", "clamped"):
        assert word in doc, word


def _want_floats(T, N, S, cap, R):
    hp = lambda h: (h + 15) // 16 * 16
    up4 = lambda v: (v + 3) // 4 * 4
    rows = min(N, cap) if cap > 0 else N
    z, f, D, od = S[0:3], S[4:7], sum(S[8:11]), S[11]
    psize = up4(sum(a * a + a + b * a + b + b * b + b for a, b in zip(z, f)) + od * sum(f) + od)
    n = up4(T * rows * D) if rows < N else 0
    n += rows * T * 6 * sum(hp(a) for a in z) + sum(up4(rows * a) for a in z) + up4(rows * sum(f))
    return n + (rows + R - 1) // R * psize + up4(rows) + up4(rows * T) + 4


def _want_mask_offset(T, N, S, cap):
    hp = lambda h: (h + 15) // 16 * 16
    up4 = lambda v: (v + 3) // 4 * 4
    rows = min(N, cap) if cap > 0 else N
    return (up4(T * rows * sum(S[8:11])) if rows < N else 0) + rows * T * 6 * sum(hp(a) for a in S[0:3]) + sum(up4(rows * a) for a in S[0:3])


def test_workspace_query_equals_the_formula_of_the_header_and_stops_growing_at_the_row_cap():
    L = _lib.lib()
    T = 20
    r = (C.c_int32 * 1)()
    for S in (SIZES, ODD):
        sz = (C.c_int32 * 12)(*S)
        for N in (1, 33, 229):
            for cap in (0, 5, N, N + 1, 1000):
                assert L.mfm_train_ablation_d_tile_rows(N, cap, r) == 0
                assert L.mfm_train_ablation_d_workspace_floats(T, N, sz, cap) == _want_floats(T, N, S, cap, r[0]), (S, N, cap)
                assert L.mfm_train_ablation_d_mask_offset(T, N, sz, cap) == _want_mask_offset(T, N, S, cap), (S, N, cap)
    sz = (C.c_int32 * 12)(*SIZES)
    q = lambda N, cap: L.mfm_train_ablation_d_workspace_floats(T, N, sz, cap)
    assert q(4, 8) < q(6, 8) < q(8, 8)                              # grows with the rows up to the cap ...
    assert q(9, 8) == q(16, 8) == q(4000, 8)                        # ... and no further
    assert q(9, 8) - q(8, 8) == 8 * T * sum(SIZES[8:11])            # (a chunked call also holds the chunk's copy of x)
    for bad in ((0, 33, 0), (T, 0, 0), (T, 33, -1), (T, 1 << 24, 0)):
        assert L.mfm_train_ablation_d_workspace_floats(bad[0], bad[1], sz, bad[2]) == 0, bad
        assert L.mfm_train_ablation_d_mask_offset(bad[0], bad[1], sz, bad[2]) == 0, bad
    assert L.mfm_train_ablation_d_workspace_floats(T, 33, None, 0) == 0
    zero = (C.c_int32 * 12)(*[0 if i == 5 else v for i, v in enumerate(SIZES)])
    assert L.mfm_train_ablation_d_workspace_floats(T, 33, zero, 0) == 0


def test_tile_rows_query_follows_the_rule_of_the_prediction_entry():
    L = _lib.lib()
    cus = L.mfm_device_cus()
    r, ra = (C.c_int32 * 1)(), (C.c_int32 * 2)()
    for N, cap in ((1, 0), (2 * cus - 1, 0), (2 * cus, 0), (6 * cus, 2 * cus - 1), (6 * cus, 2 * cus)):
        assert L.mfm_train_ablation_d_tile_rows(N, cap, r) == 0
        assert L.mfm_predict_ablation_tile_rows(N, 1, 0, cap, ra) == 0
        assert r[0] == ra[0] == (1 if min(N, cap or N) < 2 * cus else 4), (N, cap)
    for bad in ((0, 0), (5, -1)):
        assert L.mfm_train_ablation_d_tile_rows(bad[0], bad[1], r) == -1, bad
    assert L.mfm_train_ablation_d_tile_rows(5, 0, None) == -1


def _call(T=4, N=6, sizes=SIZES, loss=0, train=0, p=(0.0, 0.0, 0.0), params=None, grads=None, accumulate=0, x=0x1000, y=0x3000,
          ws=0x2000, y_hat=0x90000, out=0x92000, cap=0, tick=0, null=()):
    """mfm_train_ablation_d on made-up (aligned, never dereferenced) addresses: every call here must be refused by the checks,
    which come before any launch"""
    L = _lib.lib()
    sz = None if "sizes" in null else (C.c_int32 * 12)(*sizes)
    prm = None if "params" in null else (C.c_void_p * NP)(*(params or [0x10000 + 64 * i for i in range(NP)]))
    grd = None if "grads" in null else (C.c_void_p * NP)(*(grads or [0x50000 + 64 * i for i in range(NP)]))
    pd = None if "p" in null else (C.c_float * 3)(*p)
    rc = L.mfm_train_ablation_d(T, N, sz, loss, train, pd, 1, 0, C.c_void_p(tick), prm, grd, accumulate, C.c_void_p(x), C.c_void_p(y),
                                C.c_void_p(ws), C.c_void_p(y_hat), C.c_void_p(out), cap, None)
    return rc, L.mfm_last_error().decode()


BIG = dict(T=4000, N=(1 << 24) - 1)       # passes every argument check and is refused by the row check behind them


def test_argument_checks_answer_without_a_device():
    ptrs = [0x10000 + 64 * i for i in range(NP)]
    for null in ("sizes", "params", "grads", "p"):
        rc, msg = _call(null=(null,))
        assert rc == -1 and "must not be null" in msg, (null, msg)
    for kw in (dict(x=0), dict(ws=0), dict(y_hat=0), dict(y=0), dict(out=0)):
        rc, msg = _call(**kw)
        assert rc == -1 and "must not be null" in msg, (kw, msg)
    for kw, word in ((dict(cap=-1), "row cap -1"), (dict(T=0), "T 0"), (dict(N=0), "N 0"), (dict(loss=2), "loss kind 2"), (dict(N=1 << 24), "2^24"),
                     (dict(sizes=[0 if i == 2 else v for i, v in enumerate(SIZES)]), "size 2 is 0"),
                     (dict(accumulate=2), "accumulate = 2"), (dict(accumulate=-1), "accumulate = -1"), (dict(train=2), "train = 2"),
                     (dict(p=(0.0, 1.0, 0.0)), "dropout probability 1"), (dict(p=(-0.1, 0.0, 0.0)), "dropout probability 0"),
                     (dict(p=(0.0, 0.0, float("nan"))), "dropout probability 2")):
        rc, msg = _call(**kw)
        assert rc == -1 and word in msg, (kw, msg)
    # a complete call gets as far as the row check; frozen parameters (null gradients) are fine, null parameters are named
    for kw in (dict(), dict(loss=1), dict(train=1, p=(0.2, 0.5, 0.7)), dict(accumulate=1), dict(grads=[0 if i % 3 else 0x50000 + 64 * i for i in range(NP)]),
               dict(tick=0x7008), dict(x=0x1004, y=0x3004)):
        rc, msg = _call(**dict(kw, **BIG))
        assert rc == -1 and "pass a row cap" in msg, (kw, msg)
    rc, msg = _call(params=[0 if i == 17 else p for i, p in enumerate(ptrs)])
    assert rc == -1 and "parameter 17 is null" in msg, msg
    rc, msg = _call(params=[p + 4 if i == 11 else p for i, p in enumerate(ptrs)])
    assert rc == -1 and "parameter 11 is misaligned" in msg, msg
    rc, msg = _call(params=[p + 4 if i in (2, 4, 14, 30) else p for i, p in enumerate(ptrs)], **BIG)      # (4 bytes: fine but for the LSTM weights)
    assert rc == -1 and "pass a row cap" in msg, msg
    rc, msg = _call(grads=[0x50002 if i == 5 else 0x50000 + 64 * i for i in range(NP)])
    assert rc == -1 and "gradient 5 is misaligned" in msg, msg
    for kw, word in ((dict(x=0x1002), "x must be 4-byte aligned"), (dict(ws=0x2004), "workspace 16-byte aligned"), (dict(out=0x92002), "misaligned"),
                     (dict(loss=1, y=0x3004), "misaligned"), (dict(tick=0x7004), "misaligned")):
        rc, msg = _call(**kw)
        assert rc == -1 and word in msg, (kw, msg)


def test_sizes_that_do_not_fit_on_chip_are_refused_as_unsupported_without_a_device():
    at = lambda i, v: [v if j == i else s for j, s in enumerate(SIZES)]
    for i in range(3):
        rc, msg = _call(sizes=at(i, 132))
        assert rc == _lib.MFM_ERR_UNSUPPORTED and "132" in msg, (i, msg)
        rc, msg = _call(sizes=at(4 + i, 132))
        assert rc == _lib.MFM_ERR_UNSUPPORTED and "f size 132" in msg, (i, msg)
        rc, msg = _call(sizes=at(i, 128), **BIG)
        assert rc == -1 and "pass a row cap" in msg, (i, msg)
    rc, msg = _call(sizes=at(3, 5000), **BIG)                  # (zy and fy are unused)
    assert rc == -1 and "pass a row cap" in msg, msg
    rc, msg = _call(sizes=at(11, 40000))
    assert rc == _lib.MFM_ERR_UNSUPPORTED and "output_dim = 40000" in msg, msg


# ----------------------------------------------------------------------------------- the module
def _pair(output_dim=None):
    """(M_D on the CPU, the oracle, x), both with the weights tests/golden/extra_M_D.npz was generated with (seed 1234)"""
    from factorized_amd import mfm_model as M
    cfgs, gold, xn, _ = load_extra("M_D", "small")
    if output_dim:
        cfgs = [dict(c) for c in cfgs]
        cfgs[0]["output_dim"] = output_dim
    ref = X.CLASSES["M_D"](*cfgs)
    if not output_dim:
        assert [n for n, _ in ref.named_parameters()] == list(gold["param_names"])
    w = synth.make_weights({k: tuple(v.shape) for k, v in ref.state_dict().items()}, seed=1234)
    ref.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in w.items()})
    model = M.M_D(*cfgs)
    model.load_state_dict(ref.state_dict())
    return model, ref, torch.from_numpy(xn), cfgs


def test_only_m_d_has_loss_and_grad():
    from factorized_amd import mfm_model as M
    assert callable(getattr(M.M_D, "loss_and_grad"))
    for name in ("M_A", "M_B", "M_C"):
        assert not hasattr(getattr(M, name), "loss_and_grad"), name


@pytest.mark.parametrize("loss,od", [("l1", None), ("ce", 3)])
def test_on_cpu_tensors_the_composed_path_gives_the_oracle_loss_and_gradients(loss, od):
    torch.set_num_threads(4)
    model, ref, x, cfgs = _pair(od)
    N = x.shape[1]
    rs = np.random.RandomState(5)
    y = torch.from_numpy(rs.standard_normal((N, 1)).astype(np.float32)) if loss == "l1" else torch.from_numpy(rs.randint(0, 3, size=N).astype(np.int64))
    y_hat = ref.forward(x)[0][3]
    want = F.l1_loss(y_hat, y) if loss == "l1" else F.cross_entropy(y_hat, y)
    want.backward()
    got = model.loss_and_grad(x, y, loss=loss)
    assert got.dim() == 0 and not got.requires_grad and got.device.type == "cpu"
    want = want.detach()
    assert abs(float(got) - float(want)) <= TOL * abs(float(want))
    assert rel_err(model.last_y_hat.numpy(), y_hat.detach().numpy()) < TOL
    names = [n for n, _ in ref.named_parameters()]
    assert len(names) == 32 and names == [n for n, _ in model.named_parameters()]
    for (n, p), (_, q) in zip(model.named_parameters(), ref.named_parameters()):
        assert p.grad is not None and rel_err(p.grad.numpy(), q.grad.numpy()) < TOL, n
    # a second call adds; a frozen parameter is left alone
    g1 = {n: p.grad.clone() for n, p in model.named_parameters()}
    model.fs_to_y.bias.requires_grad_(False)
    model.fs_to_y.bias.grad = None
    model.loss_and_grad(x, y, loss=loss)
    assert model.fs_to_y.bias.grad is None
    for n, p in model.named_parameters():
        if p.grad is not None:
            assert rel_err(p.grad.numpy(), 2 * g1[n].numpy()) < 1e-6, n
    assert not [k for k in model.__dict__ if k.startswith("_train_bufs")]
    assert model.last_dropout_masks() is None                # (the composed path keeps no masks)


def test_the_argument_checks_raise_before_any_library_call(monkeypatch):
    model, _, x, _ = _pair()
    N = x.shape[1]
    y = torch.zeros(N, 1)
    L, calls = _lib.lib(), []
    for name in NEW:
        monkeypatch.setattr(L, name, lambda *a: calls.append(1), raising=True)
    with pytest.raises(_lib.MfmError, match="float labels"):
        model.loss_and_grad(x, y[:-1])
    with pytest.raises(_lib.MfmError, match="float labels"):
        model.loss_and_grad(x, torch.zeros(N, 2))
    with pytest.raises(_lib.MfmError, match="int64 class indices"):
        model.loss_and_grad(x, y, loss="ce")
    with pytest.raises(ValueError, match="'l1' or 'ce'"):
        model.loss_and_grad(x, y, loss="mse")
    with pytest.raises(_lib.MfmError, match="max_rows"):
        model.loss_and_grad(x, y, max_rows=-1)
    with pytest.raises(_lib.MfmError, match="features per time step"):
        model.loss_and_grad(x[:, :, :-1], y)
    with pytest.raises(_lib.MfmError, match="empty split"):
        model.loss_and_grad(x[:, :0], y[:0])
    assert not calls and all(p.grad is None for p in model.parameters())
    assert model.last_dropout_masks() is None                # (before the first call)


def test_a_model_that_has_called_the_entry_pickles_without_its_buffers_and_still_works():
    model, _, x, _ = _pair()
    y = torch.zeros(x.shape[1], 1)
    keys = list(model.state_dict().keys())
    # a stubbed cache entry, as a call on the device leaves it: a ctypes table cannot be pickled, so it has to be dropped
    model._train_bufs = {(6, 12, 1024, "cuda:0"): (torch.zeros(4), (C.c_void_p * NP)())}
    model._train_last = (6, 12, 1024, "cuda:0")
    model._train_calls = 3
    model.dropout_seed = 99
    clone = pickle.loads(pickle.dumps(model))
    assert "_train_bufs" not in clone.__dict__ and "_train_bufs" in model.__dict__ and "_train_last" not in clone.__dict__
    assert clone.last_dropout_masks() is None                # (nothing to read: the buffers were dropped)
    assert clone._train_calls == 3 and clone.dropout_seed == 99 and list(clone.state_dict().keys()) == keys
    a, b = model.loss_and_grad(x, y), clone.loss_and_grad(x, y)
    assert torch.equal(a, b)
    for (n, p), (_, q) in zip(model.named_parameters(), clone.named_parameters()):
        assert torch.equal(p.grad, q.grad), n
