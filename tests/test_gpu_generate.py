"""encode / decode (engine.encode / engine.decode, model.encode / model.decode, mfm_encode_klef / mfm_decode_factors) on the MI355X:
the reference's own golden outputs through decode(encode(x)), each factor against the oracle's composition, factors as
independent arguments, row chunks, determinism and containment, capture, the fallbacks and the refusals.  Numeric bound: the
project's 1e-4 relative fp32 tolerance (tests.cases.rel_err)."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import mfm_oracle as O
from factorized_amd import _lib, configs, synth
from tests import cases
from tests.cases import rel_err

pytestmark = pytest.mark.gpu
TOL = 1e-4
CANARY = 0x7FC0DEAD                   # a NaN with a payload: any store over it shows
CLS = {"kl_ef": "MFM_KL_EF", "kl": "MFM_KL", "mmd": "MFM"}
GOLDEN = [n for n in cases.KLEF_CASES if n != "klef_b229_t20"] + ["kl_b32_t20", "mmd_b32_t20"]


def _engine(cfgs, variant="kl_ef"):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from factorized_amd import engine
    e = engine.MFMEngine(cfgs, variant=variant)
    w = synth.make_weights(e.layout.shapes, seed=1234)
    e.load_weights(w)
    return e, w


def _model(cfgs, cls="MFM_KL_EF"):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from factorized_amd import mfm_model as M
    model = getattr(M, cls)(*cfgs)
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    w = synth.make_weights(shapes, seed=1234)
    model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in w.items()})
    return model.to("cuda"), w


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _same(a, b):
    return all(torch.equal(_bits(p), _bits(q)) for p, q in zip(a, b))


def _keep(ts):
    """the engine reuses its output buffers: keep copies"""
    return [None if t is None else t.clone() for t in ts]


def _oracle(variant, cfgs, w):
    m = O.build(variant, cfgs)
    O.load_numpy_weights(m, w)
    m.eval()
    return m


def _oracle_encode(m, x):
    """the encoder half, composed exactly as _Factorized.forward does (kl_ef / kl)"""
    with torch.no_grad():
        l_last = m.encoder_l(x[:, :, :m.d_l])
        a_last = m.encoder_a(x[:, :, m.d_l:m.d_l + m.d_a])
        v_last = m.encoder_v(x[:, :, m.d_l + m.d_a:])
        y_last = m.ef_encoder(x) if m.variant == "kl_ef" else m.mfn_encoder(x)
        return [m.last_to_zl_fc1(l_last), m.last_to_za_fc1(a_last), m.last_to_zv_fc1(v_last), m.last_to_zy_fc1(y_last),
                m.last_to_logvarzl_fc1(l_last), m.last_to_logvarza_fc1(a_last), m.last_to_logvarzv_fc1(v_last),
                m.last_to_logvarzy_fc1(y_last)]


def _oracle_decode(m, zl, za, zv, zy, T):
    """the generative half, composed exactly as _Factorized.forward does"""
    with torch.no_grad():
        fy = m._z_to_f("zy_to_fy", zy)
        fl = m._z_to_f("zl_to_fl", zl)
        fa = m._z_to_f("za_to_fa", za)
        fv = m._z_to_f("zv_to_fv", zv)
        return [m.decoder_l(torch.cat([fy, fl], 1), T), m.decoder_a(torch.cat([fy, fa], 1), T),
                m.decoder_v(torch.cat([fy, fv], 1), T),
                m.fy_to_y_fc2(m.fy_to_y_dropout(torch.relu(m.fy_to_y_fc1(fy))))]


_SHARED = {}


def _case(name):
    """a kl_ef golden case with its engine, the oracle, the oracle's factors and the engine's unchunked results, computed once"""
    if name not in _SHARED:
        cs = cases.load_case(name)
        e, w = _engine(cs["cfgs"])
        x = torch.from_numpy(cs["x"]).cuda()
        m = _oracle("kl_ef", cs["cfgs"], w)
        torch.set_num_threads(4)
        ref = _oracle_encode(m, torch.from_numpy(cs["x"]))
        enc = _keep(e.encode(x))
        dec = _keep(e.decode(*enc[:4], cs["T"]))
        _SHARED[name] = dict(cs=cs, e=e, w=w, x=x, m=m, ref=ref, enc=enc, dec=dec)
    return _SHARED[name]


# ----------------------------------------------------------------------------------- 1. the reference's own outputs
@pytest.mark.parametrize("name", GOLDEN)
def test_decode_of_encode_matches_reference_golden(name):
    cs = cases.load_case(name)
    model, _ = _model(cs["cfgs"], CLS[cs["variant"]])
    x = torch.from_numpy(cs["x"]).cuda()
    gold = cs["gold"]
    f = model.encode(x)
    dec = model.decode(*f[:4], cs["T"])
    d = [t.cpu().numpy() for t in dec]
    errs = dict(y_hat=rel_err(d[3], gold["y_hat"]), x_a_hat=rel_err(d[1], gold["x_a_hat"]),
                x_l_first=rel_err(d[0][0], gold["x_l_hat_first"]), x_l_last=rel_err(d[0][-1], gold["x_l_hat_last"]),
                x_v_first=rel_err(d[2][0], gold["x_v_hat_first"]), x_v_last=rel_err(d[2][-1], gold["x_v_hat_last"]),
                x_l_sum=rel_err(cases.summarize(d[0]), gold["x_l_hat_sum"]), x_v_sum=rel_err(cases.summarize(d[2]), gold["x_v_hat_sum"]))
    print("generate_golden %s %s" % (name, " ".join("%s %.3e" % kv for kv in errs.items())))
    cfg = cs["cfg"]
    assert [tuple(t.shape) for t in dec] == [(cs["T"], cs["B"], k) for k in cfg["input_dims"]] + [(cs["B"], cfg["output_dim"])]
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
    print("generate_golden %s reg %.8g ref %.8g" % (name, reg, ref))
    assert abs(reg - ref) <= TOL * max(abs(ref), 1e-3)


# ----------------------------------------------------------------------------------- 2. each factor against the oracle
@pytest.mark.parametrize("name", ["klef_b33_t7", "klef_odd_b19_t9"])
def test_each_factor_against_the_oracle(name):
    s = _case(name)
    cfg = s["cs"]["cfg"]
    sizes = [cfg[k] for k in ("zl_size", "za_size", "zv_size", "zy_size")] * 2
    names = type(s["e"].encode(s["x"]))._fields
    for fname, got, ref, size in zip(names, s["enc"], s["ref"], sizes):
        assert got.shape == (s["cs"]["B"], size) and got.dtype == torch.float32 and got.is_cuda, fname
        err = rel_err(got.cpu().numpy(), ref.numpy())
        print("factor %s %s %.3e" % (name, fname, err))
        assert err < TOL, (fname, err)


# ----------------------------------------------------------------------------------- 3. factors are independent arguments
def test_factors_are_independent_arguments_and_T_is_free():
    s = _case("klef_b33_t7")
    zl, za, zv, zy = s["enc"][:4]
    T = 11
    perm = [zl, za.flip(0).contiguous(), zv, zy.roll(1, 0).contiguous()]
    got = _keep(s["e"].decode(*perm, T))
    plain = _keep(s["e"].decode(zl, za, zv, zy, T))
    ref = _oracle_decode(s["m"], *[t.cpu() for t in perm], T)
    for i, (g, r) in enumerate(zip(got, ref)):
        assert g.shape == r.shape
        err = rel_err(g.cpu().numpy(), r.numpy())
        print("permuted factors out %d %.3e" % (i, err))
        assert err < TOL, (i, err)
    # not vacuous: the permutation changes y_hat (zy), x_a_hat (za and zy) and x_l_hat (zy)
    for i in (0, 1, 3):
        assert rel_err(got[i].cpu().numpy(), plain[i].cpu().numpy()) > TOL, i


# ----------------------------------------------------------------------------------- 4. row chunks
@pytest.mark.parametrize("max_rows", [1, 4, 32, 33, 1000])
def test_row_chunks_are_bit_equal(max_rows):
    s = _case("klef_b33_t7")
    enc = _keep(s["e"].encode(s["x"], max_rows=max_rows))
    assert _same(enc, s["enc"])
    dec = _keep(s["e"].decode(*s["enc"][:4], s["cs"]["T"], max_rows=max_rows))
    assert _same(dec, s["dec"])


# ----------------------------------------------------------------------------------- 5. determinism and containment
def test_two_calls_are_bit_equal():
    s = _case("klef_b33_t7")
    enc = _keep(s["e"].encode(s["x"]))
    dec = _keep(s["e"].decode(*enc[:4], s["cs"]["T"]))
    assert _same(enc, s["enc"]) and _same(dec, s["dec"])


def _p(t):
    return C.c_void_p(t.data_ptr())


def _canary(n, pad=256):
    big = torch.full((pad + n + pad,), CANARY, dtype=torch.int32, device="cuda")
    return big, big[pad:pad + n].view(torch.float32)


def _intact(big, n, pad=256):
    return bool((big[:pad] == CANARY).all()) and bool((big[pad + n:] == CANARY).all())


def _abi_in_canaries(e, c, T, N, x, cap, ref_enc, ref_dec):
    """both entries through the C ABI on canary-framed workspaces and outputs: nothing outside is touched, the results are
    bit-equal to `ref_enc` / `ref_dec`"""
    from factorized_amd import engine
    L = _lib.lib()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    zs = [c[k] for k in ("zl_size", "za_size", "zv_size", "zy_size")]
    d_l, d_a, d_v = c["input_dims"]
    nws = int(L.mfm_encode_klef_workspace_floats(T, N, zs[0], zs[1], zs[2], cap))
    big_ws, ws = _canary(nws)
    outs = [_canary(N * z) for z in zs + zs]
    offs = (C.c_int64 * 40)(*[e.layout.offsets[n] for n in engine.MFMEngine._ENCODE_TENSORS])
    optr = (C.c_void_p * 8)(*[o[1].data_ptr() for o in outs])
    assert L.mfm_encode_klef(T, N, d_l, d_a, d_v, zs[0], zs[1], zs[2], zs[3], _p(e.params), offs, _p(x), _p(ws), optr, cap,
                             stream) == 0
    torch.cuda.synchronize()
    assert _intact(big_ws, nws)
    for (big, view), z, ref in zip(outs, zs + zs, ref_enc):
        assert _intact(big, N * z)
        assert torch.equal(_bits(view.view(N, z)), _bits(ref))

    nws = int(L.mfm_decode_factors_workspace_floats(T, N, c["fy_size"], c["fl_size"], c["fa_size"], c["fv_size"], cap))
    big_ws, ws = _canary(nws)
    dims = [T * N * d_l, T * N * d_a, T * N * d_v, N * c["output_dim"]]
    outs = [_canary(n) for n in dims]
    offs = (C.c_int64 * 38)(*[e.layout.offsets[n] for n in engine.MFMEngine._DECODE_TENSORS])
    sizes = (C.c_int32 * 12)(zs[0], zs[1], zs[2], zs[3], c["fl_size"], c["fa_size"], c["fv_size"], c["fy_size"], d_l, d_a, d_v,
                             c["output_dim"])
    zptr = (C.c_void_p * 4)(*[t.data_ptr() for t in ref_enc[:4]])
    optr = (C.c_void_p * 4)(*[o[1].data_ptr() for o in outs])
    assert L.mfm_decode_factors(T, N, sizes, _p(e.params), offs, zptr, _p(ws), optr, cap, stream) == 0
    torch.cuda.synchronize()
    assert _intact(big_ws, nws)
    for (big, view), n, ref in zip(outs, dims, ref_dec):
        assert _intact(big, n)
        assert torch.equal(_bits(view), _bits(ref.reshape(-1)))


@pytest.mark.parametrize("name,cap", [("klef_b5_t1", 0), ("klef_b33_t7", 0), ("klef_b33_t7", 16), ("klef_odd_b19_t9", 4)])
def test_canaries_around_workspace_and_outputs(name, cap):
    s = _case(name)
    _abi_in_canaries(s["e"], s["cs"]["cfg"], s["cs"]["T"], s["cs"]["B"], s["x"], cap, s["enc"], s["dec"])


# ----------------------------------------------------------------------------------- four-row tiles
@pytest.mark.parametrize("over", [{}, cases.ODD], ids=["canonical", "odd"])
def test_four_row_tiles_from_six_workgroups_per_cu_on(over):
    """a chunk whose (LSTM, row) workgroups number 6 per CU or more runs on four-row tiles (the rule of the training
    recurrences): with N = 6 * CUs + 1 rows in one chunk both entries do, and the last tile holds one row.  Against the same split
    in chunks of 256 rows (one-row tiles: 4 * 256 < 6 * CUs on any part with more than 170 CUs), run to run, and inside canaries.
    The canonical sizes take the one launch with the per-block switch, the odd ones a launch per LSTM."""
    cfgs = configs.canonical_configs(dropout=False, **over)
    cfg = cfgs[0]
    e, _ = _engine(cfgs)
    cus = _lib.lib().mfm_device_cus()
    assert 4 * 256 < 6 * cus
    N, T = 6 * cus + 1, 2
    xn, _ = synth.make_batch(cfg["input_dims"], N, T, seed=11, output_dim=cfg["output_dim"])
    x = torch.from_numpy(xn).cuda()
    one = _keep(e.encode(x, max_rows=256))
    one_d = _keep(e.decode(*one[:4], T, max_rows=256))
    four = _keep(e.encode(x, max_rows=N))
    four_d = _keep(e.decode(*four[:4], T, max_rows=N))
    for i, (a, b) in enumerate(zip(four + four_d, one + one_d)):
        err = rel_err(a.cpu().numpy(), b.cpu().numpy())
        print("four-row tiles out %d %.3e" % (i, err))
        assert err < TOL, (i, err)
    again = _keep(e.encode(x, max_rows=N))
    again_d = _keep(e.decode(*four[:4], T, max_rows=N))
    assert _same(again, four) and _same(again_d, four_d)
    _abi_in_canaries(e, cfg, T, N, x, 0, four, four_d)


def test_encode_and_decode_leave_plans_parameters_gradients_and_mode_alone():
    cs = cases.load_case("klef_b33_t7")
    model, _ = _model(cs["cfgs"])
    x = torch.from_numpy(cs["x"]).cuda()
    e = model.engine
    before = e.params.clone()
    for p in model.parameters():
        p.grad = torch.full_like(p, 0.5)
    for mode in (True, False):
        model.train(mode)
        f = model.encode(x)
        dec = model.decode(*f[:4], cs["T"])
        assert model.training == mode
        assert all(not t.requires_grad for t in list(f) + dec)
    torch.cuda.synchronize()
    assert not e._plans
    assert torch.equal(_bits(before), _bits(e.params))
    assert all(bool((p.grad == 0.5).all()) for p in model.parameters())


def test_dropout_is_off_whatever_the_mode():
    cfgs = configs.canonical_configs(dropout=True)
    cfg = cfgs[0]
    xn, _ = synth.make_batch(cfg["input_dims"], 33, 7, seed=7, output_dim=cfg["output_dim"])
    x = torch.from_numpy(xn).cuda()
    model, _ = _model(cfgs)
    model.train()
    a = _keep(model.encode(x))
    da = _keep(model.decode(*a[:4], 7))
    assert model.training
    model.eval()
    b = _keep(model.encode(x))
    db = _keep(model.decode(*b[:4], 7))
    assert _same(a, b) and _same(da, db)
    with torch.no_grad():
        ref = model(x)[0]
    for g, r in zip(da, ref):
        assert rel_err(g.cpu().numpy(), r.cpu().numpy()) < TOL


# ----------------------------------------------------------------------------------- 6. capture
def test_encode_then_decode_in_one_captured_graph():
    cs = cases.load_case("klef_b33_t7")
    model, _ = _model(cs["cfgs"])
    T = cs["T"]
    x = torch.from_numpy(cs["x"]).cuda()
    xin = x.clone()
    model.decode(*model.encode(xin)[:4], T)                  # warm-up: buffers, code objects
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        gf = model.encode(xin)
        gd = model.decode(*gf[:4], T)
    xn, _ = synth.make_batch(cs["cfg"]["input_dims"], cs["B"], T, seed=23, output_dim=cs["cfg"]["output_dim"])
    x2 = torch.from_numpy(xn).cuda()
    xin.copy_(x2)
    graph.replay()
    torch.cuda.synchronize()
    cf, cd = _keep(gf), _keep(gd)
    ef = _keep(model.encode(x2))
    ed = _keep(model.decode(*ef[:4], T))
    assert _same(cf, ef) and _same(cd, ed)
    e0 = _keep(model.encode(x))
    assert not _same(e0, ef)                                 # (the new input did change the result)


def test_no_allocation_and_no_synchronisation_after_the_first_call():
    cs = cases.load_case("klef_b33_t7")
    model, _ = _model(cs["cfgs"])
    x = torch.from_numpy(cs["x"]).cuda()
    for _ in range(2):
        model.decode(*model.encode(x)[:4], cs["T"])
    torch.cuda.synchronize()
    allocated = torch.cuda.memory_allocated()
    count = torch.cuda.memory_stats()["allocation.all.allocated"]
    torch.cuda.set_sync_debug_mode("error")
    try:
        for _ in range(10):
            model.decode(*model.encode(x)[:4], cs["T"])
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.cuda.memory_allocated() <= allocated
    assert torch.cuda.memory_stats()["allocation.all.allocated"] == count


# ----------------------------------------------------------------------------------- 7. fallbacks
def test_forced_refusal_takes_the_composition_and_agrees():
    cs = cases.load_case("klef_b33_t7")
    model, _ = _model(cs["cfgs"])
    x = torch.from_numpy(cs["x"]).cuda()
    fast = _keep(model.encode(x))
    fdec = _keep(model.decode(*fast[:4], cs["T"]))
    e = model.engine
    assert e._encode_bufs and e._decode_bufs
    e._encode_bufs.clear()
    e._decode_bufs.clear()
    e._encode_refused = e._decode_refused = True
    slow = model.encode(x)
    sdec = model.decode(*fast[:4], cs["T"])
    assert not e._encode_bufs and not e._decode_bufs          # (the fused entries were not used)
    for a, b in zip(list(slow) + sdec, fast + fdec):
        assert a.shape == b.shape
        assert rel_err(a.cpu().numpy(), b.cpu().numpy()) < TOL
    with pytest.raises(_lib.MfmUnsupported):
        e.encode(x)


def test_wide_sizes_are_refused_by_the_entries_and_composed():
    cfgs = configs.canonical_configs(dropout=False, zv_size=96, fl_size=120)     # ef encoder h = 136, decoder l h = 136
    cfg = cfgs[0]
    B, T = 5, 3
    xn, _ = synth.make_batch(cfg["input_dims"], B, T, seed=21, output_dim=cfg["output_dim"])
    model, w = _model(cfgs)
    x = torch.from_numpy(xn).cuda()
    e = model.engine
    with pytest.raises(_lib.MfmUnsupported, match="136"):
        e.encode(x)
    with pytest.raises(_lib.MfmUnsupported, match="136"):
        e.decode(*[torch.zeros(B, cfg[k], device="cuda") for k in ("zl_size", "za_size", "zv_size", "zy_size")], T)
    assert e._encode_refused and e._decode_refused and not e.__dict__.get("_encode_bufs") and not e.__dict__.get("_decode_bufs")
    f = model.encode(x)
    dec = model.decode(*f[:4], T)
    m = _oracle("kl_ef", cfgs, w)
    ref = _oracle_encode(m, torch.from_numpy(xn))
    for a, b in zip(f, ref):
        assert rel_err(a.cpu().numpy(), b.numpy()) < TOL
    for a, b in zip(dec, _oracle_decode(m, *ref[:4], T)):
        assert rel_err(a.cpu().numpy(), b.numpy()) < TOL


@pytest.mark.parametrize("name", ["kl_b32_t20", "mmd_b32_t20"])
def test_mfn_classes_decode_through_the_fused_entry(name):
    cs = cases.load_case(name)
    model, _ = _model(cs["cfgs"], CLS[cs["variant"]])
    x = torch.from_numpy(cs["x"]).cuda()
    model.train()
    f = model.encode(x)
    assert model.training
    assert (f.logvar_zl is None) == (cs["variant"] == "mmd") and (f.logvar_zy is None) == (cs["variant"] == "mmd")
    e = model.engine
    assert not e.__dict__.get("_decode_bufs")
    model.decode(*f[:4], cs["T"])
    assert e._decode_bufs and not e.__dict__.get("_encode_bufs")


# ----------------------------------------------------------------------------------- 8. refusals
def test_refusals(monkeypatch):
    s = _case("klef_b33_t7")
    model, _ = _model(s["cs"]["cfgs"])
    e = model.engine
    zl, za, zv, zy = s["enc"][:4]
    T = s["cs"]["T"]
    torch.cuda.synchronize()
    launched = dict(e.__dict__.get("_decode_bufs", {}))
    L, calls = _lib.lib(), []
    for entry in ("mfm_encode_klef", "mfm_decode_factors"):
        real = getattr(L, entry)
        monkeypatch.setattr(L, entry, lambda *a, _real=real, _n=entry: (calls.append(_n), _real(*a))[1], raising=True)
    bad = [
        lambda: model.decode(zl.cpu(), za, zv, zy, T),                               # a CPU tensor
        lambda: model.decode(zl, za, zv[:, :-1].contiguous(), zy, T),                # wrong width
        lambda: model.decode(zl, za[:-1].contiguous(), zv, zy, T),                   # mismatched N
        lambda: model.decode(zl, za, zv, zy, 0),                                     # T < 1
        lambda: model.decode(zl, za, zv, zy[None], T),                               # wrong rank
        lambda: model.decode(zl, za, zv, zy.double()[None], T),                      # ... that .contiguous().float() cannot mend
        lambda: model.encode(s["x"].cpu()),
        lambda: model.encode(s["x"][:, :, :-1]),
        lambda: model.encode(s["x"][0]),
        lambda: e.decode(zl, za, zv, zy.t(), T),                                     # the engine takes no strided views
        lambda: e.encode(s["x"], max_rows=0),
    ]
    for i, call in enumerate(bad):
        with pytest.raises(_lib.MfmError):
            call()
            pytest.fail("call %d was accepted" % i)
    assert not calls                                         # neither entry was reached: nothing was launched
    assert e.__dict__.get("_decode_bufs", {}) == launched and not e.__dict__.get("_encode_bufs")      # ... and nothing was allocated
    model.decode(zl, za, zv, zy, T)                          # (the counter does count)
    assert calls == ["mfm_decode_factors"]
