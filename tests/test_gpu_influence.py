"""The gradient-based interpretation (engine.influence_factors, model.influence / influence_factors, mfm_influence_factors) on
the MI355X against the float64 recursion of tests/influence_ref.py on the oracle: golden cases, the three classes, factors as
independent arguments, row chunks, determinism and containment, capture, the torch fallback and the refusals.  The bound
everywhere is POINTWISE: |got - ref| <= 1e-4 |ref| for every element (the values fall by orders of magnitude over the steps, so
a measure relative to the tensor's maximum would see step 0 alone)."""
import ctypes as C

import numpy as np
import pytest
import torch

from factorized_amd import _lib, configs, synth
from tests import cases
from tests import influence_ref as R

pytestmark = pytest.mark.gpu
TOL = 1e-4
CANARY = 0x7FC0DEAD                   # a NaN with a payload: any store over it shows
CLS = {"kl_ef": "MFM_KL_EF", "kl": "MFM_KL", "mmd": "MFM"}
ZK = ("zl_size", "za_size", "zv_size", "zy_size")


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


def _both(inf):
    """Influence -> a private copy of its [2, 3, T, N] tensor (the engine reuses its buffers)"""
    return torch.stack([inf.fy, inf.fm]).clone()


def _check(tag, got, ref):
    err = R.pointwise_err(got.cpu().numpy() if torch.is_tensor(got) else got, ref)
    print("influence %s pointwise %.3e" % (tag, err))
    assert err <= TOL, (tag, err)


_SHARED = {}


def _case(name):
    """a kl_ef golden case: model, oracle, the oracle's factors (CPU and device), the float64 reference and the engine's
    unchunked result, computed once"""
    if name not in _SHARED:
        cs = cases.load_case(name)
        model, w = _model(cs["cfgs"])
        m = R.oracle_model("kl_ef", cs["cfgs"], w)
        torch.set_num_threads(4)
        z = R.oracle_z(m, torch.from_numpy(cs["x"]))
        zd = [t.cuda().contiguous() for t in z]
        ref = R.oracle_influence(m, *z, cs["T"])
        got = _both(model.engine.influence_factors(*zd, cs["T"]))
        _SHARED[name] = dict(cs=cs, model=model, e=model.engine, m=m, z=z, zd=zd, ref=ref, got=got,
                             x=torch.from_numpy(cs["x"]).cuda())
    return _SHARED[name]


# ----------------------------------------------------------------------------------- 1. the entry against the reference
@pytest.mark.parametrize("name", ["klef_b33_t7", "klef_odd_b19_t9", "klef_b5_t1", "klef_b1_t20"])
def test_entry_on_the_oracles_factors(name):
    s = _case(name)
    cs = s["cs"]
    inf = s["e"].influence_factors(*s["zd"], cs["T"])
    assert tuple(inf.fy.shape) == tuple(inf.fm.shape) == (3, cs["T"], cs["B"])
    assert inf.fy.dtype == torch.float32 and inf.fy.is_cuda
    base = inf.fy._base
    assert base is not None and inf.fm._base is base and tuple(base.shape) == (2, 3, cs["T"], cs["B"])
    assert s["ref"].min() > 1e-10                            # (every reference value is a normal float well above zero)
    _check(name, s["got"], s["ref"])


# ----------------------------------------------------------------------------------- 2. the three classes
@pytest.mark.parametrize("name", ["klef_b33_t7", "kl_b32_t20", "mmd_b32_t20"])
def test_model_influence_on_its_own_factors(name):
    cs = cases.load_case(name)
    model, w = _model(cs["cfgs"], CLS[cs["variant"]])
    x = torch.from_numpy(cs["x"]).cuda()
    model.train()
    z = [t.clone() for t in model.encode(x)[:4]]
    got = _both(model.influence(x))
    assert model.training and not got.requires_grad
    assert model.engine._influence_bufs
    m = R.oracle_model(cs["variant"], cs["cfgs"], w)
    _check(name, got, R.oracle_influence(m, *[t.cpu() for t in z], cs["T"]))


# ----------------------------------------------------------------------------------- 3. factors are independent arguments
def test_factors_are_independent_arguments_and_T_is_free():
    s = _case("klef_b33_t7")
    zl, za, zv, zy = s["zd"]
    T = 11
    perm = [zl, za.flip(0).contiguous(), zv, zy.roll(1, 0).contiguous()]
    got = _both(s["e"].influence_factors(*perm, T))
    assert tuple(got.shape) == (2, 3, T, s["cs"]["B"])
    _check("permuted", got, R.oracle_influence(s["m"], *[t.cpu() for t in perm], T))
    plain = _both(s["e"].influence_factors(zl, za, zv, zy, T))
    assert R.pointwise_err(got.cpu().numpy(), plain.cpu().numpy()) > TOL           # (not vacuous)
    assert torch.equal(_bits(plain[:, :, :s["cs"]["T"]]), _bits(s["got"]))        # (the first steps do not depend on T)


def test_factor_views_four_bytes_past_a_16_byte_boundary():
    s = _case("klef_odd_b19_t9")
    off = []
    for z in s["zd"]:
        n, w = z.shape
        buf = torch.zeros(n * w + 8, device="cuda")
        base = (-buf.data_ptr() // 4) % 4                   # floats up to the next 16-byte boundary
        v = buf[base + 1:base + 1 + n * w].view(n, w)
        v.copy_(z)
        assert v.data_ptr() % 16 == 4 and v.is_contiguous()
        off.append(v)
    got = _both(s["e"].influence_factors(*off, s["cs"]["T"]))
    assert torch.equal(_bits(got), _bits(s["got"]))


# ----------------------------------------------------------------------------------- 4. bit equality
@pytest.mark.parametrize("max_rows", [1, 4, 32, 33, 1000])
def test_row_chunks_are_bit_equal(max_rows):
    s = _case("klef_b33_t7")
    got = _both(s["e"].influence_factors(*s["zd"], s["cs"]["T"], max_rows=max_rows))
    assert torch.equal(_bits(got), _bits(s["got"]))


def test_two_calls_are_bit_equal():
    for name in ("klef_b33_t7", "klef_odd_b19_t9"):
        s = _case(name)
        assert torch.equal(_bits(_both(s["e"].influence_factors(*s["zd"], s["cs"]["T"]))), _bits(s["got"]))


# ----------------------------------------------------------------------------------- 5. containment
def _canary(n, pad=256):
    big = torch.full((pad + n + pad,), CANARY, dtype=torch.int32, device="cuda")
    return big, big[pad:pad + n].view(torch.float32)


def _intact(big, n, pad=256):
    return bool((big[:pad] == CANARY).all()) and bool((big[pad + n:] == CANARY).all())


@pytest.mark.parametrize("name,cap", [("klef_b5_t1", 0), ("klef_b33_t7", 0), ("klef_b33_t7", 16), ("klef_odd_b19_t9", 4)])
def test_canaries_around_workspace_and_output(name, cap):
    from factorized_amd import engine
    s = _case(name)
    e, c, T, N = s["e"], s["cs"]["cfg"], s["cs"]["T"], s["cs"]["B"]
    L = _lib.lib()
    sizes = (C.c_int32 * 12)(*[c[k] for k in ZK], c["fl_size"], c["fa_size"], c["fv_size"], c["fy_size"], *c["input_dims"], c["output_dim"])
    nws = int(L.mfm_influence_factors_workspace_floats(T, N, sizes, cap))
    assert nws > 0 and nws == e.influence_factors_workspace_floats(T, N, max_rows=cap or None)
    big_ws, ws = _canary(nws)
    big_out, out = _canary(2 * 3 * T * N)
    offs = (C.c_int64 * 38)(*[e.layout.offsets[n] for n in engine.MFMEngine._DECODE_TENSORS])
    zptr = (C.c_void_p * 4)(*[t.data_ptr() for t in s["zd"]])
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert L.mfm_influence_factors(T, N, sizes, C.c_void_p(e.params.data_ptr()), offs, zptr, C.c_void_p(ws.data_ptr()),
                                   C.c_void_p(out.data_ptr()), cap, stream) == 0
    torch.cuda.synchronize()
    assert _intact(big_ws, nws) and _intact(big_out, 2 * 3 * T * N)
    assert torch.equal(_bits(out.view(2, 3, T, N)), _bits(s["got"]))


def test_influence_leaves_plans_parameters_gradients_and_mode_alone():
    cs = cases.load_case("klef_b33_t7")
    model, _ = _model(cs["cfgs"])
    x = torch.from_numpy(cs["x"]).cuda()
    e = model.engine
    before = e.params.clone()
    for p in model.parameters():
        p.grad = torch.full_like(p, 0.5)
    for mode in (True, False):
        model.train(mode)
        inf = model.influence(x)
        assert model.training == mode
        assert not inf.fy.requires_grad and not inf.fm.requires_grad
    torch.cuda.synchronize()
    assert not e._plans
    assert torch.equal(_bits(before), _bits(e.params))
    assert all(bool((p.grad == 0.5).all()) for p in model.parameters())
    assert not e.__dict__.get("_decode_bufs") and not e.__dict__.get("_objective_bufs")      # (its own caches only)


def test_dropout_is_off_whatever_the_mode():
    cfgs = configs.canonical_configs(dropout=True)
    cfg = cfgs[0]
    xn, _ = synth.make_batch(cfg["input_dims"], 9, 3, seed=7, output_dim=cfg["output_dim"])
    x = torch.from_numpy(xn).cuda()
    model, _ = _model(cfgs)
    model.train()
    a = _both(model.influence(x))
    assert model.training
    model.eval()
    b = _both(model.influence(x))
    assert torch.equal(_bits(a), _bits(b))


# ----------------------------------------------------------------------------------- 6. capture and reuse
def test_encode_then_influence_in_one_captured_graph():
    cs = cases.load_case("klef_b33_t7")
    model, _ = _model(cs["cfgs"])
    T = cs["T"]
    x = torch.from_numpy(cs["x"]).cuda()
    xin = x.clone()
    model.influence_factors(*model.encode(xin)[:4], T)       # warm-up: buffers, code objects
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        gi = model.influence_factors(*model.encode(xin)[:4], T)
    xn, _ = synth.make_batch(cs["cfg"]["input_dims"], cs["B"], T, seed=23, output_dim=cs["cfg"]["output_dim"])
    x2 = torch.from_numpy(xn).cuda()
    xin.copy_(x2)
    graph.replay()
    torch.cuda.synchronize()
    captured = _both(gi)
    eager = _both(model.influence(x2))
    assert torch.equal(_bits(captured), _bits(eager))
    assert not torch.equal(_bits(_both(model.influence(x))), _bits(eager))       # (the new input did change the result)


def test_no_allocation_and_no_synchronisation_after_the_first_call():
    cs = cases.load_case("klef_b33_t7")
    model, _ = _model(cs["cfgs"])
    x = torch.from_numpy(cs["x"]).cuda()
    for _ in range(2):
        model.influence(x)
    torch.cuda.synchronize()
    allocated = torch.cuda.memory_allocated()
    count = torch.cuda.memory_stats()["allocation.all.allocated"]
    torch.cuda.set_sync_debug_mode("error")
    try:
        for _ in range(5):
            model.influence(x)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.cuda.memory_allocated() <= allocated
    assert torch.cuda.memory_stats()["allocation.all.allocated"] == count


# ----------------------------------------------------------------------------------- 7. the fallback and the refusals
def test_forced_refusal_takes_the_torch_fallback_and_agrees():
    s = _case("klef_b33_t7")
    model, _ = _model(s["cs"]["cfgs"])
    e = model.engine
    e._influence_refused = True
    slow = model.influence_factors(*s["zd"], s["cs"]["T"])
    assert not e.__dict__.get("_influence_bufs")              # (the fused entry was not used)
    assert slow.fy._base is slow.fm._base and slow.fy._base is not None
    _check("forced fallback", torch.stack([slow.fy, slow.fm]), s["ref"])
    with pytest.raises(_lib.MfmUnsupported):
        e.influence_factors(*s["zd"], s["cs"]["T"])


def test_wide_sizes_are_refused_by_the_entry_and_take_the_fallback():
    cfgs = configs.canonical_configs(dropout=False, fl_size=120)     # decoder l: h = fy + fl = 136
    cfg = cfgs[0]
    assert cfg["fy_size"] + cfg["fl_size"] == 136
    B, T = 3, 3
    model, w = _model(cfgs)
    e = model.engine
    z = [torch.randn(B, cfg[k], generator=torch.Generator().manual_seed(5)) for k in ZK]
    zd = [t.cuda() for t in z]
    with pytest.raises(_lib.MfmUnsupported, match="136"):
        e.influence_factors(*zd, T)
    assert b"136" in _lib.lib().mfm_last_error()
    assert e._influence_refused and not e.__dict__.get("_influence_bufs")
    got = model.influence_factors(*zd, T)
    _check("wide", torch.stack([got.fy, got.fm]), R.oracle_influence(R.oracle_model("kl_ef", cfgs, w), *z, T))


def test_bad_arguments_are_refused_before_anything_is_launched(monkeypatch):
    s = _case("klef_b33_t7")
    model, _ = _model(s["cs"]["cfgs"])
    e = model.engine
    zl, za, zv, zy = s["zd"]
    T = s["cs"]["T"]
    L, calls = _lib.lib(), []
    real = L.mfm_influence_factors
    monkeypatch.setattr(L, "mfm_influence_factors", lambda *a: (calls.append(1), real(*a))[1], raising=True)
    bad = [
        lambda: model.influence_factors(zl.cpu(), za, zv, zy, T),                    # a CPU tensor
        lambda: model.influence_factors(zl, za, zv[:, :-1].contiguous(), zy, T),     # wrong width
        lambda: model.influence_factors(zl, za[:-1].contiguous(), zv, zy, T),        # mixed row counts
        lambda: model.influence_factors(zl, za, zv, zy, 0),                          # T < 1
        lambda: model.influence_factors(zl, za, zv, zy[None], T),                    # wrong rank
        lambda: e.influence_factors(zl, za, zv, zy, T, max_rows=0),                  # max_rows < 1
        lambda: model.influence(s["x"].cpu()),
    ]
    for i, call in enumerate(bad):
        with pytest.raises(_lib.MfmError):
            call()
            pytest.fail("call %d was accepted" % i)
    assert not calls and not e.__dict__.get("_influence_bufs")
    model.influence_factors(zl, za, zv, zy, T)               # (the counter does count)
    assert calls == [1]
