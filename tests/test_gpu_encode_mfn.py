"""encode of the MFN classes (MFM_KL, MFM: engine.encode -> mfm_encode_mfn) on the MI355X: the reference's golden outputs through
decode(encode(x)), each factor against the oracle on sizes where nothing is a multiple of 4 or of a tile, the composed path,
row chunks, determinism, containment and x off a 16-byte boundary through the raw ABI, side effects, capture, data that is not
unit noise, and the refusals.  Numeric bound: the project's 1e-4 relative fp32 tolerance (tests.cases.rel_err)."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import mfm_oracle as O
from factorized_amd import _lib, configs, synth
from tests import cases
from tests import data_regimes as DR
from tests.mfn_entries import bits as _bits, CANARY, canary as _canary, intact as _intact, model as _model, odd_cfgs as _odd_cfgs, ptr as _p
from tests.cases import rel_err

pytestmark = pytest.mark.gpu
TOL = 1e-4
def _same(a, b):
    return all((p is None and q is None) or torch.equal(_bits(p), _bits(q)) for p, q in zip(a, b))


def _keep(ts):
    """the engine reuses its output buffers: keep copies"""
    return [None if t is None else t.clone() for t in ts]


def _oracle(variant, cfgs, w, double=False):
    m = O.build(variant, cfgs)
    O.load_numpy_weights(m, w)
    if double:
        m = copy.deepcopy(m).double()
    m.eval()
    return m


def _oracle_encode(m, x):
    """the encoder half, composed exactly as the reference's forward does: the heads for "kl", the encoders' outputs for "mmd" """
    with torch.no_grad():
        l_last = m.encoder_l(x[:, :, :m.d_l])
        a_last = m.encoder_a(x[:, :, m.d_l:m.d_l + m.d_a])
        v_last = m.encoder_v(x[:, :, m.d_l + m.d_a:])
        y_last = m.mfn_encoder(x)
        if m.variant == "mmd":
            return [l_last, a_last, v_last, m.last_to_zy_fc1(y_last)]
        return [m.last_to_zl_fc1(l_last), m.last_to_za_fc1(a_last), m.last_to_zv_fc1(v_last), m.last_to_zy_fc1(y_last),
                m.last_to_logvarzl_fc1(l_last), m.last_to_logvarza_fc1(a_last), m.last_to_logvarzv_fc1(v_last),
                m.last_to_logvarzy_fc1(y_last)]


def _check_against(got, ref, tag):
    assert sum(t is not None for t in got) == len(ref)
    for i, (g, r) in enumerate(zip(got, ref)):
        assert g.shape == r.shape and g.dtype == torch.float32 and g.is_cuda
        err = rel_err(g.cpu().numpy(), r.double().numpy())
        print("encode_mfn %s factor %d %.3e" % (tag, i, err))
        assert err < TOL, (tag, i, err)


_SHARED = {}


def _canon(variant):
    """the canonical config at B = 33, T = 7 with its model and the fused entry's unchunked result, computed once"""
    if variant not in _SHARED:
        cfgs = configs.canonical_configs(dropout=False)
        model, w = _model(cfgs, variant)
        xn, _ = synth.make_batch(cfgs[0]["input_dims"], 33, 7, seed=5, output_dim=cfgs[0]["output_dim"])
        x = torch.from_numpy(xn).cuda()
        enc = _keep(model.engine.encode(x))
        _SHARED[variant] = dict(cfgs=cfgs, cfg=cfgs[0], model=model, e=model.engine, w=w, x=x, xn=xn, enc=enc, T=7, N=33)
    return _SHARED[variant]


# ----------------------------------------------------------------------------------- 1. the fused path is taken
@pytest.mark.parametrize("name", ["kl_b32_t20", "mmd_b32_t20"])
def test_fused_path_is_taken_and_matches_reference_golden(name):
    cs = cases.load_case(name)
    model, _ = _model(cs["cfgs"], cs["variant"])
    x = torch.from_numpy(cs["x"]).cuda()
    gold = cs["gold"]
    f = model.encode(x)
    e = model.engine
    assert e.__dict__.get("_encode_mfn_bufs") and not e.__dict__.get("_encode_bufs")
    dec = model.decode(*f[:4], cs["T"])
    d = [t.cpu().numpy() for t in dec]
    errs = dict(y_hat=rel_err(d[3], gold["y_hat"]), x_a_hat=rel_err(d[1], gold["x_a_hat"]),
                x_l_first=rel_err(d[0][0], gold["x_l_hat_first"]), x_l_last=rel_err(d[0][-1], gold["x_l_hat_last"]),
                x_v_first=rel_err(d[2][0], gold["x_v_hat_first"]), x_v_last=rel_err(d[2][-1], gold["x_v_hat_last"]),
                x_l_sum=rel_err(cases.summarize(d[0]), gold["x_l_hat_sum"]), x_v_sum=rel_err(cases.summarize(d[2]), gold["x_v_hat_sum"]))
    print("encode_mfn golden %s %s" % (name, " ".join("%s %.3e" % kv for kv in errs.items())))
    for k, v in errs.items():
        assert v < TOL, (k, v)
    if cs["variant"] == "mmd":
        assert all(t is None for t in f[4:])
        return
    reg = 0.0
    for mu, lv in zip(f[:4], f[4:]):
        mu, lv = mu.double(), lv.double()
        reg += float(-0.5 * torch.sum(1 + lv - mu * mu - lv.exp()))
    ref = float(gold["fwd_reg"])
    print("encode_mfn golden %s reg %.8g ref %.8g" % (name, reg, ref))
    assert abs(reg - ref) <= TOL * max(abs(ref), 1e-3)


# ----------------------------------------------------------------------------------- 2. each factor against the oracle
@pytest.mark.parametrize("variant", ["kl", "mmd"])
def test_each_factor_against_the_oracle_on_odd_sizes(variant):
    cfgs = _odd_cfgs()
    model, w = _model(cfgs, variant)
    m = _oracle(variant, cfgs, w)
    torch.set_num_threads(4)
    for T, N in ((1, 1), (2, 19), (9, 33)):
        xn, _ = synth.make_batch(cfgs[0]["input_dims"], N, T, seed=3 + T, output_dim=cfgs[0]["output_dim"])
        f = model.encode(torch.from_numpy(xn).cuda())
        assert model.engine._encode_mfn_bufs.get((T, N, model.engine.PREDICT_MAX_ROWS)) is not None
        _check_against(f, _oracle_encode(m, torch.from_numpy(xn)), "%s T%d N%d" % (variant, T, N))


# ----------------------------------------------------------------------------------- 3. the composed path agrees
@pytest.mark.parametrize("variant", ["kl", "mmd"])
def test_composed_path_agrees(variant):
    s = _canon(variant)
    with torch.no_grad():
        comp = s["model"]._encode_composed(s["x"])
    for i, (a, b) in enumerate(zip(s["enc"], comp)):
        assert (a is None) == (b is None)
        if a is not None:
            err = rel_err(a.cpu().numpy(), b.cpu().numpy())
            print("encode_mfn composed %s factor %d %.3e" % (variant, i, err))
            assert err < TOL, (i, err)


# ----------------------------------------------------------------------------------- 4. row chunks, determinism
@pytest.mark.parametrize("variant", ["kl", "mmd"])
def test_row_chunks_and_two_calls_are_bit_equal(variant):
    s = _canon(variant)
    L = _lib.lib()
    for cap in (1, 7, 16, None):
        assert L.mfm_encode_mfn_tile_rows(s["N"], cap or s["e"].PREDICT_MAX_ROWS) == 1          # one tile-row form throughout
        assert _same(_keep(s["e"].encode(s["x"], max_rows=cap)), s["enc"]), cap
    assert _same(_keep(s["e"].encode(s["x"])), s["enc"])


# ----------------------------------------------------------------------------------- 5. containment, x off a 16-byte boundary
def _abi(s, variant, x, cap):
    """mfm_encode_mfn through the C ABI on a canary-framed workspace and outputs -> the factors; nothing outside is touched"""
    from factorized_amd import engine
    e, c, T, N = s["e"], s["cfg"], s["T"], s["N"]
    L = _lib.lib()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    sizes = e._encode_mfn_sizes()
    zs = [c[k] for k in ("zl_size", "za_size", "zv_size", "zy_size")] * (2 if variant == "kl" else 1)
    nws = int(L.mfm_encode_mfn_workspace_floats(T, N, sizes, cap))
    assert nws > 0
    big_ws, ws = _canary(nws)
    outs = [_canary(N * z) for z in zs]
    names = engine.MFMEngine._ENCODE_MFN_TENSORS[variant]
    offs = (C.c_int64 * len(names))(*[e.layout.offsets[n] for n in names])
    optr = (C.c_void_p * 8)(*[o[1].data_ptr() for o in outs])
    assert L.mfm_encode_mfn(T, N, sizes, _p(e.params), offs, _p(x), _p(ws), optr, cap, stream) == 0, L.mfm_last_error()
    torch.cuda.synchronize()
    assert _intact(big_ws, nws)
    for (big, _), z in zip(outs, zs):
        assert _intact(big, N * z)
    return [view.view(N, z) for (_, view), z in zip(outs, zs)]


@pytest.mark.parametrize("variant,cap", [("kl", 0), ("kl", 7), ("mmd", 0), ("mmd", 7)])
def test_canaries_around_workspace_and_outputs(variant, cap):
    s = _canon(variant)
    got = _abi(s, variant, s["x"], cap)
    assert _same(got, [t for t in s["enc"] if t is not None])


@pytest.mark.parametrize("off", [1, 2, 3])
def test_x_may_start_off_a_16_byte_boundary(off):
    s = _canon("kl")
    buf = torch.zeros(s["x"].numel() + 8, dtype=torch.float32, device="cuda")
    assert buf.data_ptr() % 16 == 0
    xv = buf[off:off + s["x"].numel()].view(s["x"].shape)
    xv.copy_(s["x"])
    assert xv.data_ptr() % 16 == 4 * off
    assert _same(_abi(s, "kl", xv, 0), s["enc"])
    assert _same(_keep(s["e"].encode(xv)), s["enc"])


# ----------------------------------------------------------------------------------- 6. side effects and capture
@pytest.mark.parametrize("variant", ["kl", "mmd"])
def test_encode_leaves_plans_parameters_gradients_and_mode_alone_and_dropout_is_off(variant):
    cfgs = configs.canonical_configs(dropout=True)
    model, _ = _model(cfgs, variant)
    xn, _ = synth.make_batch(cfgs[0]["input_dims"], 33, 7, seed=5, output_dim=cfgs[0]["output_dim"])
    x = torch.from_numpy(xn).cuda()
    e = model.engine
    plans = dict(e._plans)
    before = e.params.clone()
    for p in model.parameters():
        p.grad = torch.full_like(p, 0.5)
    res = {}
    for mode in (True, False):
        model.train(mode)
        res[mode] = _keep(model.encode(x))
        assert model.training == mode
        assert all(t is None or not t.requires_grad for t in res[mode])
    torch.cuda.synchronize()
    assert e._encode_mfn_bufs and e._plans == plans
    assert torch.equal(_bits(before), _bits(e.params))
    assert all(bool((p.grad == 0.5).all()) for p in model.parameters())
    assert _same(res[True], res[False])                       # dropout is off in train mode
    assert _same(res[True], _canon(variant)["enc"])           # ... the dropout-free configuration's bits (same weights, same x)


def test_no_allocation_after_the_first_call():
    s = _canon("kl")
    model, x = s["model"], s["x"]
    for _ in range(2):
        model.decode(*model.encode(x)[:4], s["T"])
    torch.cuda.synchronize()
    allocated = torch.cuda.memory_allocated()
    count = torch.cuda.memory_stats()["allocation.all.allocated"]
    torch.cuda.set_sync_debug_mode("error")
    try:
        for _ in range(5):
            model.decode(*model.encode(x)[:4], s["T"])
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.cuda.memory_allocated() == allocated
    assert torch.cuda.memory_stats()["allocation.all.allocated"] == count


@pytest.mark.parametrize("variant", ["kl", "mmd"])
def test_encode_then_decode_in_one_captured_graph(variant):
    s = _canon(variant)
    model, T = s["model"], s["T"]
    xin = s["x"].clone()
    model.decode(*model.encode(xin)[:4], T)                  # warm-up: buffers, code objects
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        gf = model.encode(xin)
        gd = model.decode(*gf[:4], T)
    xn, _ = synth.make_batch(s["cfg"]["input_dims"], s["N"], T, seed=23, output_dim=s["cfg"]["output_dim"])
    x2 = torch.from_numpy(xn).cuda()
    xin.copy_(x2)
    graph.replay()
    torch.cuda.synchronize()
    cf, cd = _keep(gf), _keep(gd)
    ef = _keep(model.encode(x2))
    ed = _keep(model.decode(*ef[:4], T))
    assert _same(cf, ef) and _same(cd, ed)
    assert not _same(s["enc"], ef)                           # (the new input did change the result)


# ----------------------------------------------------------------------------------- 7. data that is not unit noise
@pytest.mark.parametrize("variant", ["kl", "mmd"])
def test_modality_scales_ten_thousand_apart_against_the_float64_oracle(variant):
    """regime `mixed` (modality scales 1 / 50 / 0.02): the cell states that meet in cStar, and the softmax over them, are fed by
    inputs 10^4 apart"""
    cfgs = DR.canonical()
    model, w = _model(cfgs, variant)
    xn, _ = DR.make("mixed", 19, 9)
    m = _oracle(variant, cfgs, w, double=True)
    torch.set_num_threads(4)
    f = model.encode(torch.from_numpy(xn).cuda())
    assert model.engine._encode_mfn_bufs
    _check_against(f, _oracle_encode(m, torch.from_numpy(xn).double()), "mixed " + variant)


# ----------------------------------------------------------------------------------- 8. refusals
def test_wide_h_dims_are_refused_remembered_and_composed():
    cfgs = _odd_cfgs(h_dims=[9, 136, 7])
    model, w = _model(cfgs, "kl")
    T, N = 3, 5
    xn, _ = synth.make_batch(cfgs[0]["input_dims"], N, T, seed=21, output_dim=cfgs[0]["output_dim"])
    x = torch.from_numpy(xn).cuda()
    e = model.engine
    with pytest.raises(_lib.MfmUnsupported, match="136"):
        e.encode(x)
    assert "136" in _lib.lib().mfm_last_error().decode()
    assert e._encode_mfn_refused and not e.__dict__.get("_encode_mfn_bufs")
    f = model.encode(x)
    assert not e.__dict__.get("_encode_mfn_bufs")
    _check_against(f, _oracle_encode(_oracle("kl", cfgs, w), torch.from_numpy(xn)), "composed h 136")


def test_windowsize_3_is_refused():
    s = _canon("kl")
    from factorized_amd import engine
    L = _lib.lib()
    e = s["e"]
    sizes = e._encode_mfn_sizes()
    sizes[11] = 3
    names = engine.MFMEngine._ENCODE_MFN_TENSORS["kl"]
    offs = (C.c_int64 * len(names))(*[e.layout.offsets[n] for n in names])
    nws = int(L.mfm_encode_mfn_workspace_floats(s["T"], s["N"], sizes, 0))
    big_ws, ws = _canary(nws)
    outs = [_canary(s["N"] * t.shape[1]) for t in s["enc"]]
    optr = (C.c_void_p * 8)(*[o[1].data_ptr() for o in outs])
    rc = L.mfm_encode_mfn(s["T"], s["N"], sizes, _p(e.params), offs, _p(s["x"]), _p(ws), optr, 0,
                          C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == _lib.MFM_ERR_UNSUPPORTED and "windowsize 3" in L.mfm_last_error().decode()
    torch.cuda.synchronize()
    assert bool((big_ws == CANARY).all()) and all(bool((b == CANARY).all()) for b, _ in outs)      # nothing was enqueued


def test_bad_arguments_do_not_reach_the_library_and_a_one_time_refusal_is_not_remembered(monkeypatch):
    s = _canon("kl")
    model, e, x = s["model"], s["e"], s["x"]
    L, calls = _lib.lib(), []
    real = L.mfm_encode_mfn
    monkeypatch.setattr(L, "mfm_encode_mfn", lambda *a: (calls.append(1), real(*a))[1], raising=True)
    bufs = dict(e._encode_mfn_bufs)
    bad = [lambda: e.encode(x, max_rows=0), lambda: model.encode(x.cpu()), lambda: model.encode(x[:, :, :-1]), lambda: model.encode(x[0])]
    for i, call in enumerate(bad):
        with pytest.raises(_lib.MfmError):
            call()
            pytest.fail("call %d was accepted" % i)
    assert not calls and e._encode_mfn_bufs == bufs
    assert _same(_keep(model.encode(x)), s["enc"]) and calls == [1]          # (the counter does count)
    # a refusal with legal sizes (as for the LDS of one call's shape) holds for that call alone
    monkeypatch.setattr(L, "mfm_encode_mfn", lambda *a: _lib.MFM_ERR_UNSUPPORTED, raising=True)
    with pytest.raises(_lib.MfmUnsupported):
        e.encode(x, max_rows=5)
    assert not e._encode_mfn_refused
    monkeypatch.setattr(L, "mfm_encode_mfn", real, raising=True)
    assert _same(_keep(e.encode(x, max_rows=5)), s["enc"])


# ----------------------------------------------------------------------------------- the other launch forms
@pytest.mark.parametrize("variant", ["kl", "mmd"])
def test_four_row_tiles_and_32_pair_attention_tiles(variant):
    """one chunk of N = 33 * CUs rows at T = 2: the six recurrences run on four-row tiles (6 N >= 6 CUs; the canonical sizes in the
    one launch with the per-block switch) and the attention chain takes 32 pairs per workgroup (2 N / 16 > 4 CUs).  Against the
    same split in chunks of CUs - 1 rows (one-row tiles, 16 pairs), run to run, and inside canaries."""
    s = _canon(variant)
    L = _lib.lib()
    cus = L.mfm_device_cus()
    N, T = 33 * cus, 2
    assert 2 * N > 16 * 4 * cus and L.mfm_encode_mfn_tile_rows(N, N) == 4 and L.mfm_encode_mfn_tile_rows(N, cus - 1) == 1
    xn, _ = synth.make_batch(s["cfg"]["input_dims"], N, T, seed=11, output_dim=s["cfg"]["output_dim"])
    x = torch.from_numpy(xn).cuda()
    one = _keep(s["e"].encode(x, max_rows=cus - 1))
    four = _keep(s["e"].encode(x, max_rows=N))
    for i, (a, b) in enumerate(zip(four, one)):
        if a is not None:
            err = rel_err(a.cpu().numpy(), b.cpu().numpy())
            print("encode_mfn four-row tiles %s factor %d %.3e" % (variant, i, err))
            assert err < TOL, (i, err)
    assert _same(_keep(s["e"].encode(x, max_rows=N)), four)
    assert _same(_abi(dict(s, T=T, N=N), variant, x, 0), [t for t in four if t is not None])


def test_four_row_tiles_on_odd_sizes_take_a_launch_per_lstm():
    cfgs = _odd_cfgs()
    model, w = _model(cfgs, "kl")
    cus = _lib.lib().mfm_device_cus()
    N, T = cus + 1, 3
    xn, _ = synth.make_batch(cfgs[0]["input_dims"], N, T, seed=13, output_dim=cfgs[0]["output_dim"])
    f = model.engine.encode(torch.from_numpy(xn).cuda(), max_rows=N)
    torch.set_num_threads(4)
    _check_against(f, _oracle_encode(_oracle("kl", cfgs, w), torch.from_numpy(xn)), "odd four-row tiles")
