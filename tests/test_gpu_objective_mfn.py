"""The full validation objective of the MFN classes (MFM_KL, MFM: engine.objective -> mfm_objective_mfn) on the MI355X: the fused
path is taken, the reference's own run (tests/golden/{kl,mmd}_objective_b19_t9.npz) and the canonical fixtures, the unchanged
fallback, row chunks and determinism, the MMD's tile edges, a given and a drawn Gaussian sample, both tile forms, cross entropy,
the lambdas, containment and x off a 16-byte boundary through the raw ABI, side effects, capture, data that is not unit noise,
and the refusals.  Numeric bound: the project's 1e-4 relative fp32 tolerance with the floor of test_gpu_objective.py (_check)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from oracle import mfm_oracle as O
from factorized_amd import _lib, configs, synth
from tests import cases
from tests import data_regimes as DR
from tests.mfn_entries import bits as _bits, CANARY, model as _model, odd_cfgs as _odd_cfgs, ptr as _p

pytestmark = pytest.mark.gpu
TOL = 1e-4
FIELDS = ("loss", "disc", "gen_l", "gen_a", "gen_v", "reg")
GOLD_KEYS = ("fwd_loss", "fwd_disc", "fwd_gen_l", "fwd_gen_a", "fwd_gen_v", "fwd_reg")
VARIANTS = ["kl", "mmd"]
def _zsizes(cfg):
    return [cfg["zl_size"], cfg["za_size"], cfg["zv_size"], cfg["zy_size"]]


def _gauss(cfg, N, seed=99):
    """a seeded N(0, 1) sample [N, zl + za + zv + zy] on the host"""
    return np.random.RandomState(seed).normal(size=(N, sum(_zsizes(cfg)))).astype(np.float32)


def _split(g, cfg):
    return list(torch.split(torch.from_numpy(np.ascontiguousarray(g)), _zsizes(cfg), dim=1))


def _give(model, variant, g):
    """inject the sample into the model (MFM alone has one)"""
    if variant == "mmd":
        model.mmd_gauss = None if g is None else [t.cuda() for t in _split(g, model.engine.cfg)]


def _eng_give(e, variant, g):
    """the same for a bare engine call (model.objective sets engine.gauss from the model on every call)"""
    if variant == "mmd":
        e.gauss = None if g is None else torch.from_numpy(np.ascontiguousarray(g)).cuda()


def _oracle(variant, cfgs, w, xn, yn, g=None, double=False):
    """the six numbers of the oracle in eval mode (float64 throughout with `double`)"""
    cfg = cfgs[0]
    m = O.build(variant, cfgs)
    O.load_numpy_weights(m, w)
    m.eval()
    x, y = torch.from_numpy(np.ascontiguousarray(xn)), torch.from_numpy(np.ascontiguousarray(yn))
    gs = None if g is None else _split(g, cfg)
    ce = cfg.get("loss", "l1") == "ce"
    if double:
        m, x = m.double(), x.double()
        y = y if ce else y.double()
        gs = None if gs is None else [t.double() for t in gs]
    if variant == "mmd":
        m.mmd_gauss = gs
    torch.set_num_threads(4)
    with torch.no_grad():
        ref = O.loss_terms(m, x, y, cfg, "ce" if ce else "l1")
    return [float(ref[k]) for k in FIELDS]


def _obits(obj):
    return _bits(torch.stack(list(obj)))


def _vals(obj):
    """the six fields on the host (the engine reuses its result tensor: this is the copy)"""
    return [float(v) for v in torch.stack(list(obj)).cpu()]


def _errs(got, want):
    return [abs(g - w) / max(abs(w), 1e-3) for g, w in zip(got, want)]


def _check(tag, got, want, fields=FIELDS):
    errs = _errs(got, want)
    print("%s %s" % (tag, " ".join("%s %.8g/%.8g (%.2e)" % (f, g, w, e) for f, g, w, e in zip(FIELDS, got, want, errs))))
    for f, g, w, e in zip(FIELDS, got, want, errs):
        if f in fields:
            assert e <= TOL, (tag, f, g, w, e)
    return max(errs)


_SHARED = {}


def _canon(variant):
    """the canonical config at N = 33, T = 7 with its model, a given sample, the oracle's numbers and the fused entry's
    unchunked result, computed once"""
    if variant not in _SHARED:
        cfgs = configs.canonical_configs(dropout=False)
        cfg = cfgs[0]
        model, w = _model(cfgs, variant)
        xn, yn = synth.make_batch(cfg["input_dims"], 33, 7, seed=5, output_dim=cfg["output_dim"])
        x, y = torch.from_numpy(xn).cuda(), torch.from_numpy(yn).cuda()
        g = _gauss(cfg, 33)
        _give(model, variant, g)
        ref = _oracle(variant, cfgs, w, xn, yn, g)
        obj = model.objective(x, y)
        _SHARED[variant] = dict(cfgs=cfgs, cfg=cfg, model=model, e=model.engine, w=w, x=x, y=y, xn=xn, yn=yn, g=g, ref=ref,
                                vals=_vals(obj), bits=_obits(obj), T=7, N=33)
    s = _SHARED[variant]
    _eng_give(s["e"], variant, s["g"])           # (a test before may have left its own sample on the shared engine)
    return s


# ----------------------------------------------------------------------------------- 1. the fused path is taken
@pytest.mark.parametrize("variant", VARIANTS)
def test_fused_path_is_taken(variant, monkeypatch):
    from factorized_amd import engine
    s = _canon(variant)
    model, _ = _model(s["cfgs"], variant)                    # (a model of its own: the shared one's cache has other keys)
    _give(model, variant, s["g"])
    e = model.engine
    L, calls = _lib.lib(), []
    real = L.mfm_objective_mfn
    monkeypatch.setattr(L, "mfm_objective_mfn", lambda *a: (calls.append(1), real(*a))[1], raising=True)
    obj = model.objective(s["x"], s["y"])
    assert calls == [1] and torch.equal(_obits(obj), s["bits"])
    assert isinstance(obj, engine.Objective) and obj._fields == FIELDS
    for v in obj:
        assert v.dim() == 0 and v.is_cuda and v.dtype == torch.float32 and not v.requires_grad
    assert list(e.__dict__.get("_objective_mfn_bufs", {})) == [(s["T"], s["N"], e.PREDICT_MAX_ROWS)]
    assert not e.__dict__.get("_objective_bufs") and not e._plans and not e.__dict__.get("_objective_mfn_refused")
    assert e.objective_workspace_floats(s["T"], s["N"]) == e._objective_mfn_bufs[(s["T"], s["N"], e.PREDICT_MAX_ROWS)][0].numel()
    cases.report("objective_mfn_canon_" + variant, _check("objective_mfn fused " + variant, s["vals"], s["ref"]))


# ----------------------------------------------------------------------------------- 2. the reference's own numbers
@pytest.mark.parametrize("variant", VARIANTS)
def test_reference_fixture_at_odd_sizes(variant):
    gold = np.load(os.path.join(cases.GOLDEN, "%s_objective_b19_t9.npz" % variant))
    B, T = [int(v) for v in gold["meta"]]
    assert (B, T) == (19, 9)
    cfgs = _odd_cfgs()
    cfg = cfgs[0]
    model, _ = _model(cfgs, variant)
    xn, yn = synth.make_batch(cfg["input_dims"], B, T, seed=7, output_dim=cfg["output_dim"])
    _give(model, variant, gold["mmd_gauss"] if variant == "mmd" else None)
    want = [float(gold[k]) for k in FIELDS]
    x, y = torch.from_numpy(xn).cuda(), torch.from_numpy(yn).cuda()
    cases.report("objective_mfn_reference_" + variant, _check("objective_mfn reference " + variant, _vals(model.objective(x, y)), want))
    _check("objective_mfn reference chunks " + variant, _vals(model.engine.objective(x, y, max_rows=4)), want)
    assert model.engine._objective_mfn_bufs and not model.engine._plans


@pytest.mark.parametrize("name", ["kl_b32_t20", "mmd_b32_t20"])
def test_canonical_fixtures(name):
    cs = cases.load_case(name)
    variant = cs["variant"]
    model, _ = _model(cs["cfgs"], variant)
    _give(model, variant, cs["gold"]["mmd_gauss"] if variant == "mmd" else None)
    x, y = torch.from_numpy(cs["x"]).cuda(), torch.from_numpy(cs["y"]).cuda()
    _check("objective_mfn golden " + name, _vals(model.objective(x, y)), [float(cs["gold"][k]) for k in GOLD_KEYS])
    assert model.engine._objective_mfn_bufs and not model.engine._plans


# ----------------------------------------------------------------------------------- 3. the fallback
@pytest.mark.parametrize("variant", VARIANTS)
def test_agrees_with_the_fallback(variant):
    s = _canon(variant)
    m2, _ = _model(s["cfgs"], variant)
    _give(m2, variant, s["g"])
    m2.engine._objective_mfn_refused = True
    fb = _vals(m2.objective(s["x"], s["y"]))
    assert m2.engine._plans and not m2.engine.__dict__.get("_objective_mfn_bufs")
    _check("objective_mfn vs fallback " + variant, s["vals"], fb)


# ----------------------------------------------------------------------------------- 4. edges, chunks, determinism
@pytest.mark.parametrize("variant", VARIANTS)
def test_edges_chunks_and_determinism(variant):
    cfgs = _odd_cfgs()
    cfg = cfgs[0]
    model, w = _model(cfgs, variant)
    e = model.engine
    for T, N, caps in ((1, 1, (None,)), (3, 5, (2,)), (4, 19, (None, 7, 1))):
        xn, yn = synth.make_batch(cfg["input_dims"], N, T, seed=3 + T, output_dim=cfg["output_dim"])
        x, y = torch.from_numpy(xn).cuda(), torch.from_numpy(yn).cuda()
        g = _gauss(cfg, N, seed=N)
        _eng_give(e, variant, g)
        ref = _oracle(variant, cfgs, w, xn, yn, g, double=True)
        first = None
        for cap in caps:
            runs = [_obits(e.objective(x, y, max_rows=cap)) for _ in range(5)]
            assert all(torch.equal(runs[0], r) for r in runs[1:]), (T, N, cap)
            got = [float(v) for v in runs[0].view(torch.float32)]
            _check("objective_mfn edges %s T%d N%d cap %s" % (variant, T, N, cap), got, ref)
            if first is None:
                first = got
            _check("objective_mfn chunkings %s T%d N%d cap %s" % (variant, T, N, cap), got, first, fields=FIELDS[:5])
    assert not e._plans


# ----------------------------------------------------------------------------------- 5. the MMD's tile edges
@pytest.mark.parametrize("N", [1, 31, 32, 33, 65])
def test_mmd_tile_edges_against_the_float64_oracle(N):
    s = _canon("mmd")
    cfg, T = s["cfg"], 2
    xn, yn = synth.make_batch(cfg["input_dims"], N, T, seed=17, output_dim=cfg["output_dim"])
    g = _gauss(cfg, N, seed=100 + N)
    model = s["model"]
    _give(model, "mmd", g)
    try:
        got = _vals(model.objective(torch.from_numpy(xn).cuda(), torch.from_numpy(yn).cuda()))
    finally:
        _give(model, "mmd", s["g"])
    _check("objective_mfn mmd tiles N%d" % N, got, _oracle("mmd", s["cfgs"], s["w"], xn, yn, g, double=True))


# ----------------------------------------------------------------------------------- 6. a given and a drawn sample
def test_given_and_drawn_gauss():
    s = _canon("mmd")
    model, e, x, y = s["model"], s["e"], s["x"], s["y"]
    given = [_obits(model.objective(x, y)) for _ in range(3)]
    assert all(torch.equal(s["bits"], r) for r in given)
    try:
        _give(model, "mmd", None)
        a, b = _obits(model.objective(x, y)), _obits(model.objective(x, y))
        assert e.gauss is None
    finally:
        _give(model, "mmd", s["g"])
    assert torch.equal(a[1:5], b[1:5]) and torch.equal(a[1:5], s["bits"][1:5])
    assert a[5] != b[5] and a[0] != b[0]
    va = [float(v) for v in a.view(torch.float32)]
    c = s["cfg"]
    total = va[1] + c["lda_xl"] * va[2] + c["lda_xa"] * va[3] + c["lda_xv"] * va[4] + c["lda_mmd"] * va[5]
    assert np.isfinite(va).all() and abs(va[0] - total) <= 1e-6 * abs(total)      # (the drawn sample's reg is the one in the total)
    for bad in (torch.zeros(s["N"], 3, device="cuda"), torch.zeros(s["N"] + 1, s["g"].shape[1], device="cuda"),
                torch.zeros(s["N"], s["g"].shape[1], device="cuda", dtype=torch.float64), torch.zeros(s["N"], s["g"].shape[1])):
        e.gauss = bad
        with pytest.raises(_lib.MfmError, match="gauss"):
            e.objective(x, y)
    e.gauss = None
    assert torch.equal(_obits(model.objective(x, y)), s["bits"])


# ----------------------------------------------------------------------------------- 7. both tile forms
@pytest.mark.parametrize("variant", VARIANTS)
def test_four_row_tiles_and_32_pair_attention_tiles(variant):
    """one chunk of N = CUs + 1 rows: the six recurrences (and the decoders) run on four-row tiles (6 N >= 6 CUs, the last tile
    with one row) and, with T such that T N / 16 > 4 CUs, the attention chain takes 32 pairs per workgroup."""
    s = _canon(variant)
    L = _lib.lib()
    cus = L.mfm_device_cus()
    N = cus + 1
    T = (64 * cus) // N + 2
    assert (T * N + 15) // 16 > 4 * cus and L.mfm_objective_mfn_tile_rows(N, N) == 4 and L.mfm_objective_mfn_tile_rows(cus - 1, 0) == 1
    xn, yn = synth.make_batch(s["cfg"]["input_dims"], N, T, seed=11, output_dim=s["cfg"]["output_dim"])
    g = _gauss(s["cfg"], N, seed=3)
    e = s["e"]
    _eng_give(e, variant, g)
    got = _vals(e.objective(torch.from_numpy(xn).cuda(), torch.from_numpy(yn).cuda(), max_rows=N))
    _check("objective_mfn four-row tiles " + variant, got, _oracle(variant, s["cfgs"], s["w"], xn, yn, g))


def test_four_row_tiles_on_odd_sizes_take_a_launch_per_lstm():
    cfgs = _odd_cfgs()
    cfg = cfgs[0]
    model, w = _model(cfgs, "mmd")
    cus = _lib.lib().mfm_device_cus()
    N, T = cus + 1, 3
    assert _lib.lib().mfm_objective_mfn_tile_rows(N, N) == 4
    xn, yn = synth.make_batch(cfg["input_dims"], N, T, seed=13, output_dim=cfg["output_dim"])
    g = _gauss(cfg, N, seed=5)
    _eng_give(model.engine, "mmd", g)
    got = _vals(model.engine.objective(torch.from_numpy(xn).cuda(), torch.from_numpy(yn).cuda(), max_rows=N))
    _check("objective_mfn odd four-row tiles", got, _oracle("mmd", cfgs, w, xn, yn, g))


# ----------------------------------------------------------------------------------- 8. cross entropy, lambdas
@pytest.mark.parametrize("variant", VARIANTS)
def test_cross_entropy_with_three_classes(variant):
    cfgs = _odd_cfgs(loss="ce", output_dim=3)
    cfg = cfgs[0]
    N, T = 19, 2
    xn, yn = synth.make_batch(cfg["input_dims"], N, T, seed=5, output_dim=3, classes=3)
    model, w = _model(cfgs, variant)
    g = _gauss(cfg, N)
    _give(model, variant, g)
    x, y = torch.from_numpy(xn).cuda(), torch.from_numpy(yn).cuda()
    ref = _oracle(variant, cfgs, w, xn, yn, g)
    _check("objective_mfn ce " + variant, _vals(model.objective(x, y)), ref)
    _eng_give(model.engine, variant, g)
    _check("objective_mfn ce chunks " + variant, _vals(model.engine.objective(x, y, max_rows=4)), ref)
    assert model.engine._objective_mfn_bufs and not model.engine._plans


@pytest.mark.parametrize("variant", VARIANTS)
def test_lambdas_weigh_the_total(variant):
    lda = (0.5, 2.0, 3.0, 0.25)
    cfgs = _odd_cfgs(lda_xl=lda[0], lda_xa=lda[1], lda_xv=lda[2], lda_mmd=lda[3])
    cfg = cfgs[0]
    N, T = 19, 3
    xn, yn = synth.make_batch(cfg["input_dims"], N, T, seed=9, output_dim=cfg["output_dim"])
    model, w = _model(cfgs, variant)
    g = _gauss(cfg, N)
    _give(model, variant, g)
    v = _vals(model.objective(torch.from_numpy(xn).cuda(), torch.from_numpy(yn).cuda()))
    total = v[1] + lda[0] * v[2] + lda[1] * v[3] + lda[2] * v[4] + lda[3] * v[5]
    print("objective_mfn lambdas %s loss %.9g weighted sum %.9g" % (variant, v[0], total))
    assert abs(v[0] - total) <= 1e-6 * abs(total)
    _check("objective_mfn lambdas " + variant, v, _oracle(variant, cfgs, w, xn, yn, g))


# ----------------------------------------------------------------------------------- 9. containment, x off a 16-byte boundary
def _abi(s, variant, x, y, cap, sizes=None, expect=0):
    """mfm_objective_mfn through the C ABI on a canary-framed workspace and output -> the bits of the six floats after checking
    that nothing outside them was touched; expect != 0: the return code, and nothing at all was touched"""
    from factorized_amd import engine
    e, T, N = s["e"], x.shape[0], x.shape[1]
    c = e.cfg
    L = _lib.lib()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    good = e._mfn_sizes()
    nws = int(L.mfm_objective_mfn_workspace_floats(T, N, good, cap))
    assert nws > 0 and nws == e.objective_workspace_floats(T, N, max_rows=cap or N)
    PAD = 256
    big_ws = torch.full((PAD + nws + PAD,), CANARY, dtype=torch.int32, device="cuda")
    big_o = torch.full((4 + 6 + 6,), CANARY, dtype=torch.int32, device="cuda")
    ws, out = big_ws[PAD:PAD + nws].view(torch.float32), big_o[4:10].view(torch.float32)
    names = engine.MFMEngine._ENCODE_MFN_TENSORS[variant] + engine.MFMEngine._DECODE_TENSORS
    offs = (C.c_int64 * len(names))(*[e.layout.offsets[n] for n in names])
    lda = (C.c_float * 4)(c["lda_xl"], c["lda_xa"], c["lda_xv"], c["lda_mmd"])
    g = torch.from_numpy(s["g"]).cuda() if variant == "mmd" else None
    rc = L.mfm_objective_mfn(T, N, sizes or good, lda, _p(e.params), offs, _p(x), _p(y), _p(g), _p(ws), _p(out), cap, stream)
    torch.cuda.synchronize()
    assert rc == expect, (rc, L.mfm_last_error())
    if expect != 0:
        assert bool((big_ws == CANARY).all()) and bool((big_o == CANARY).all())      # nothing was enqueued
        return None
    assert bool((big_ws[:PAD] == CANARY).all()) and bool((big_ws[PAD + nws:] == CANARY).all())
    assert bool((big_o[:4] == CANARY).all()) and bool((big_o[10:] == CANARY).all())
    return _bits(out)


@pytest.mark.parametrize("variant,cap", [("kl", 0), ("kl", 7), ("mmd", 0), ("mmd", 7)])
def test_canaries_around_workspace_and_output(variant, cap):
    s = _canon(variant)
    want = s["bits"] if cap == 0 else _obits(s["e"].objective(s["x"], s["y"], max_rows=cap))
    assert torch.equal(_abi(s, variant, s["x"], s["y"], cap), want)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("off", [1, 2, 3])
def test_x_may_start_off_a_16_byte_boundary(variant, off):
    s = _canon(variant)
    buf = torch.zeros(s["x"].numel() + 8, dtype=torch.float32, device="cuda")
    assert buf.data_ptr() % 16 == 0
    xv = buf[off:off + s["x"].numel()].view(s["x"].shape)
    xv.copy_(s["x"])
    assert xv.data_ptr() % 16 == 4 * off
    assert torch.equal(_abi(s, variant, xv, s["y"], 0), s["bits"])
    assert torch.equal(_abi(s, variant, xv, s["y"], 7), _obits(s["e"].objective(s["x"], s["y"], max_rows=7)))
    assert torch.equal(_obits(s["e"].objective(xv, s["y"])), s["bits"])


# ----------------------------------------------------------------------------------- 10. side effects, capture, allocation
@pytest.mark.parametrize("variant", VARIANTS)
def test_leaves_input_parameters_mode_plans_and_other_caches_alone(variant):
    s = _canon(variant)
    cfgs = configs.canonical_configs(dropout=True)
    model, _ = _model(cfgs, variant)
    _give(model, variant, s["g"])
    x, y = s["x"].clone(), s["y"].clone()
    e = model.engine
    e.forward(x, y, train=True, want_xhat=False)
    plan = e.plan(s["T"], s["N"])
    keys = set(e._plans)
    serial, consumed = plan.fwd_serial, plan.consumed
    model.encode(x)
    model.predict_zeros(x, y)
    enc, zer = dict(e._encode_mfn_bufs), dict(e._zeros_mfn_bufs)
    for p in model.parameters():
        p.grad = torch.full_like(p, 0.5)
    torch.cuda.synchronize()
    before = [plan.workspace.clone(), e.grads.clone(), e.params.clone(), x.clone()]
    res = {}
    for mode in (True, False):
        model.train(mode)
        obj = model.objective(x, y)
        res[mode] = _obits(obj)
        assert model.training == mode and all(not t.requires_grad and t.grad_fn is None for t in obj)
    e.objective(x, y, max_rows=16)
    torch.cuda.synchronize()
    # (dropout does not scale the eval computation: the numbers are those of the dropout-free configuration)
    assert torch.equal(res[True], res[False]) and torch.equal(res[True], s["bits"])
    for a, b in zip(before, [plan.workspace, e.grads, e.params, x]):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    assert set(e._plans) == keys and (plan.fwd_serial, plan.consumed) == (serial, consumed)
    assert all(bool((p.grad == 0.5).all()) for p in model.parameters())
    assert e._encode_mfn_bufs == enc and e._zeros_mfn_bufs == zer and len(e._objective_mfn_bufs) == 2
    assert not e.__dict__.get("_objective_bufs") and not e.__dict__.get("_predict_bufs")


@pytest.mark.parametrize("variant", VARIANTS)
def test_one_capture_replayed_twice_equals_the_eager_result(variant):
    s = _canon(variant)
    model, x, y = s["model"], s["x"], s["y"]
    model.objective(x, y)                                    # warm-up: buffers, code objects
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        gobj = model.objective(x, y)
    for _ in range(2):
        for v in gobj:
            v.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(_obits(gobj), s["bits"])


@pytest.mark.parametrize("variant", VARIANTS)
def test_no_allocation_and_no_synchronisation_after_the_first_call(variant):
    """MFM with a drawn sample: its buffer belongs to the entry's state and is refilled in place"""
    s = _canon(variant)
    model, x, y = s["model"], s["x"], s["y"]
    try:
        _give(model, variant, None)
        for _ in range(2):
            model.objective(x, y)
        torch.cuda.synchronize()
        allocated = torch.cuda.memory_allocated()
        count = torch.cuda.memory_stats()["allocation.all.allocated"]
        torch.cuda.set_sync_debug_mode("error")
        try:
            for _ in range(5):
                model.objective(x, y)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        assert torch.cuda.memory_allocated() == allocated
        assert torch.cuda.memory_stats()["allocation.all.allocated"] == count
    finally:
        _give(model, variant, s["g"])


# ----------------------------------------------------------------------------------- 11. data that is not unit noise
@pytest.mark.parametrize("regime", ["mixed", "saturated"])
@pytest.mark.parametrize("variant", VARIANTS)
def test_data_regimes_against_the_float64_oracle(variant, regime):
    cfgs = DR.canonical()
    model, w = _model(cfgs, variant)
    xn, yn = DR.make(regime, 19, 5)
    g = _gauss(cfgs[0], 19)
    _give(model, variant, g)
    ref = _oracle(variant, cfgs, w, xn, yn, g, double=True)
    got = _vals(model.objective(torch.from_numpy(xn).cuda(), torch.from_numpy(yn).cuda()))
    assert model.engine._objective_mfn_bufs and not model.engine._plans
    cases.report("objective_mfn_%s_%s" % (regime, variant), _check("objective_mfn %s %s" % (regime, variant), got, ref))


# ----------------------------------------------------------------------------------- 12. refusals
def test_windowsize_3_is_refused_nothing_is_enqueued_and_it_is_not_remembered(monkeypatch):
    s = _canon("kl")
    sizes = s["e"]._mfn_sizes()
    sizes[11] = 3
    _abi(s, "kl", s["x"], s["y"], 0, sizes=sizes, expect=_lib.MFM_ERR_UNSUPPORTED)
    assert "windowsize 3" in _lib.lib().mfm_last_error().decode()
    # a refusal with sizes below 128 holds for that call alone, and the call still answers through the fallback
    m2, _ = _model(s["cfgs"], "kl")
    e2, L = m2.engine, _lib.lib()
    real = L.mfm_objective_mfn
    monkeypatch.setattr(L, "mfm_objective_mfn", lambda *a: _lib.MFM_ERR_UNSUPPORTED, raising=True)
    fb = _vals(e2.objective(s["x"], s["y"], max_rows=5))
    assert not e2._objective_mfn_refused and not e2.__dict__.get("_objective_mfn_bufs")
    _check("objective_mfn one-time refusal fallback", fb, s["ref"])
    monkeypatch.setattr(L, "mfm_objective_mfn", real, raising=True)
    e2.objective(s["x"], s["y"], max_rows=5)
    assert (s["T"], s["N"], 5) in e2._objective_mfn_bufs


def _refused_136(cfgs, monkeypatch):
    """a configuration with a hidden size of 136: the entry refuses it through the raw ABI with the size in the reason and
    enqueues nothing -> (model, weights, x, y, xn, yn, calls): the library function now counts its calls"""
    cfg = cfgs[0]
    model, w = _model(cfgs, "kl")
    T, N = 3, 5
    xn, yn = synth.make_batch(cfg["input_dims"], N, T, seed=21, output_dim=cfg["output_dim"])
    x, y = torch.from_numpy(xn).cuda(), torch.from_numpy(yn).cuda()
    _abi(dict(e=model.engine), "kl", x, y, 0, expect=_lib.MFM_ERR_UNSUPPORTED)
    assert "136" in _lib.lib().mfm_last_error().decode()
    L, calls = _lib.lib(), []
    real = L.mfm_objective_mfn
    monkeypatch.setattr(L, "mfm_objective_mfn", lambda *a: (calls.append(1), real(*a))[1], raising=True)
    return model, w, x, y, xn, yn, calls


def test_a_wide_decoder_is_refused_remembered_and_falls_back(monkeypatch):
    """decoder l with fy + fl = 136: the eval forward on a plan takes it step by step"""
    cfgs = _odd_cfgs(fl_size=120)
    model, w, x, y, xn, yn, calls = _refused_136(cfgs, monkeypatch)
    e = model.engine
    got = _vals(model.objective(x, y))
    assert calls == [1] and e._objective_mfn_refused and not e.__dict__.get("_objective_mfn_bufs")
    _check("objective_mfn decoder 136 fallback", got, _oracle("kl", cfgs, w, xn, yn))
    model.objective(x, y)                                    # remembered: the entry is not asked again
    assert calls == [1] and not e.__dict__.get("_objective_mfn_bufs")


def test_wide_h_dims_are_refused_and_remembered(monkeypatch):
    """an h_dims entry of 136.  The fallback is the unchanged one, the eval forward on a fused plan, and the fused plan has no
    MFN LSTM above 128 (mfm_plan_create says so, as it did for objective of this configuration before the entry existed): the
    model's answer here is that error, not the oracle's numbers.  What the entry adds is checked: the refusal with its reason,
    nothing enqueued, remembered, the entry not called again."""
    cfgs = _odd_cfgs(h_dims=[9, 136, 7])
    model, w, x, y, xn, yn, calls = _refused_136(cfgs, monkeypatch)
    e = model.engine
    for _ in range(2):
        with pytest.raises(_lib.MfmError, match="MFN LSTM sizes above 128"):
            model.objective(x, y)
        assert calls == [1] and e._objective_mfn_refused and not e.__dict__.get("_objective_mfn_bufs")


def test_bad_arguments_do_not_reach_the_library(monkeypatch):
    s = _canon("mmd")
    model, e, x, y = s["model"], s["e"], s["x"], s["y"]
    N = x.shape[1]
    L, calls = _lib.lib(), []
    real = L.mfm_objective_mfn
    monkeypatch.setattr(L, "mfm_objective_mfn", lambda *a: (calls.append(1), real(*a))[1], raising=True)
    bufs = dict(e._objective_mfn_bufs)
    bad = [
        lambda: model.objective(x.cpu(), y),
        lambda: model.objective(x, y.cpu()),
        lambda: model.objective(x[:, :, :-1], y),
        lambda: model.objective(x, y[:-1].contiguous()),
        lambda: model.objective(x, torch.cat([y.view(N, -1)] * 2, dim=1).contiguous()),
        lambda: model.objective(x, y.double()),
        lambda: model.objective(x[:, :0].contiguous(), y[:0].contiguous()),
        lambda: model.objective(x, None),
        lambda: e.objective(x, y, max_rows=0),
    ]
    for i, call in enumerate(bad):
        with pytest.raises(_lib.MfmError):
            call()
            pytest.fail("call %d was accepted" % i)
    assert not calls and e._objective_mfn_bufs == bufs and not e._plans
    assert torch.equal(_obits(model.objective(x, y)), s["bits"]) and calls == [1]      # (the counter does count)
