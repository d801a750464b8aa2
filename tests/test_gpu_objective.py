"""The full validation objective (engine.objective, model.objective, mfm_objective_klef) on the MI355X: the six numbers against
the reference's own golden losses and against the eval forward, row chunks, the mode, canaries around its buffers, run-to-run
determinism, what it must leave alone, capture together with the device-side scheduler and keep-best, the fallbacks and the
refusals.  Numeric bound: the project's 1e-4 relative fp32 tolerance with the floor of test_gpu_predict.py."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import mfm_oracle as O
from factorized_amd import _lib, configs, synth
from tests import cases

pytestmark = pytest.mark.gpu
TOL = 1e-4
CANARY = 0x7FC0DEAD                   # a NaN with a payload: any store over it shows
FIELDS = ("loss", "disc", "gen_l", "gen_a", "gen_v", "reg")
GOLD_KEYS = ("fwd_loss", "fwd_disc", "fwd_gen_l", "fwd_gen_a", "fwd_gen_v", "fwd_reg")
GOLDEN = ["klef_b5_t1", "klef_b1_t20", "klef_b33_t7", "klef_b32_t20", "klef_odd_b19_t9", "klef_mosei_b64_t20", "klef_you_b32_t50"]
CLS = {"kl_ef": "MFM_KL_EF", "kl": "MFM_KL", "mmd": "MFM"}


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


def _xy(cs):
    return torch.from_numpy(cs["x"]).cuda(), torch.from_numpy(cs["y"]).cuda()


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _vals(obj):
    """the six fields on the host (the engine reuses its result tensor: this is the copy)"""
    return [float(v) for v in torch.stack(list(obj)).cpu()]


def _errs(got, want):
    return [abs(g - w) / max(abs(w), 1e-3) for g, w in zip(got, want)]


def _check(tag, got, want):
    errs = _errs(got, want)
    print("%s %s" % (tag, " ".join("%s %.8g/%.8g (%.2e)" % (f, g, w, e) for f, g, w, e in zip(FIELDS, got, want, errs))))
    for f, g, w, e in zip(FIELDS, got, want, errs):
        assert e <= TOL, (tag, f, g, w, e)
    return max(errs)


_B33 = {}


def _b33():
    """the B=33, T=7 case with its unchunked result, computed once"""
    if not _B33:
        cs = cases.load_case("klef_b33_t7")
        e, w = _engine(cs["cfgs"])
        x, y = _xy(cs)
        obj = e.objective(x, y)
        _B33.update(cs=cs, e=e, w=w, x=x, y=y, vals=_vals(obj), bits=_bits(torch.stack(list(obj))))
    return _B33


# ----------------------------------------------------------------------------------- 1. the reference's own losses
@pytest.mark.parametrize("name", GOLDEN)
def test_objective_matches_reference_golden(name):
    from factorized_amd import engine
    cs = cases.load_case(name)
    model, _ = _model(cs["cfgs"])
    x, y = _xy(cs)
    obj = model.objective(x, y)
    assert isinstance(obj, engine.Objective) and obj._fields == FIELDS
    for v in obj:
        assert v.dim() == 0 and v.is_cuda and v.dtype == torch.float32 and not v.requires_grad
    base = obj.loss.untyped_storage().data_ptr()
    assert [v.untyped_storage().data_ptr() for v in obj] == [base] * 6 and [v.storage_offset() for v in obj] == list(range(6))
    worst = _check("objective_golden " + name, _vals(obj), [float(cs["gold"][k]) for k in GOLD_KEYS])
    cases.report("objective_golden_" + name, worst)
    assert model.engine._objective_bufs and not model.engine._plans


# ----------------------------------------------------------------------------------- 2. the eval forward
def test_agrees_with_the_eval_forward():
    s = _b33()
    e2, _ = _engine(s["cs"]["cfgs"])
    l = e2.forward(s["x"], s["y"], train=False)["losses"].cpu().numpy().astype(np.float64)
    c = e2.cfg
    total = l[0] + c["lda_xl"] * l[1] + c["lda_xa"] * l[2] + c["lda_xv"] * l[3] + c["lda_mmd"] * l[4]
    _check("objective_vs_forward", s["vals"], [total] + [float(v) for v in l[:5]])


# ----------------------------------------------------------------------------------- 3. row chunks
@pytest.mark.parametrize("max_rows", [1, 4, 16, 32, 33, 64])
def test_row_chunks(max_rows):
    """every mean is over the whole split, not the chunk or a padded tile"""
    s = _b33()
    got = _vals(s["e"].objective(s["x"], s["y"], max_rows=max_rows))
    _check("objective_chunks %d" % max_rows, got, s["vals"])
    _check("objective_chunks %d gold" % max_rows, got, [float(s["cs"]["gold"][k]) for k in GOLD_KEYS])


# ----------------------------------------------------------------------------------- 4. the mode
def test_training_mode_gives_the_eval_numbers_and_is_left_alone():
    cfgs = configs.canonical_configs(dropout=True)
    cfg = cfgs[0]
    assert max(cfg[k] for k in cfg if k.endswith("_dropout")) > 0
    xn, yn = synth.make_batch(cfg["input_dims"], 33, 7, seed=7, output_dim=cfg["output_dim"])
    x, y = torch.from_numpy(xn).cuda(), torch.from_numpy(yn).cuda()
    model, _ = _model(cfgs)
    model.train()
    a = _bits(torch.stack(list(model.objective(x, y))))
    assert model.training
    model.eval()
    b = _bits(torch.stack(list(model.objective(x, y))))
    assert not model.training
    assert torch.equal(a, b)
    # (dropout does not scale the eval computation: the numbers are those of the dropout-free configuration)
    _check("objective_train_mode", [float(v) for v in b.view(torch.float32)], _b33()["vals"])


# ----------------------------------------------------------------------------------- 5. nothing outside its buffers
def _call_abi(e, x, y, ws, out, cap):
    from factorized_amd import engine
    c = e.cfg
    T, N, _ = x.shape
    offs = (C.c_int64 * 78)(*[e.layout.offsets[n] for n in engine.MFMEngine._ENCODE_TENSORS + engine.MFMEngine._DECODE_TENSORS])
    lda = (C.c_float * 4)(c["lda_xl"], c["lda_xa"], c["lda_xv"], c["lda_mmd"])
    p = lambda t: C.c_void_p(t.data_ptr())
    return _lib.lib().mfm_objective_klef(T, N, e._objective_sizes(), lda, p(e.params), offs, p(x), p(y), p(ws), p(out), cap,
                                         C.c_void_p(torch.cuda.current_stream().cuda_stream))


@pytest.mark.parametrize("name,cap", [("klef_b5_t1", 0), ("klef_b33_t7", 0), ("klef_b33_t7", 16)])
def test_canaries_around_workspace_and_output(name, cap):
    cs = cases.load_case(name)
    e, _ = _engine(cs["cfgs"])
    x, y = _xy(cs)
    T, N = cs["T"], cs["B"]
    nws = int(_lib.lib().mfm_objective_klef_workspace_floats(T, N, e._objective_sizes(), cap))
    assert nws == e.objective_workspace_floats(T, N, max_rows=cap or N)
    PAD = 256
    big_ws = torch.full((PAD + nws + PAD,), CANARY, dtype=torch.int32, device="cuda")
    big_o = torch.full((4 + 6 + 6,), CANARY, dtype=torch.int32, device="cuda")
    ws = big_ws[PAD:PAD + nws].view(torch.float32)
    out = big_o[4:10].view(torch.float32)
    assert _call_abi(e, x, y, ws, out, cap) == 0
    torch.cuda.synchronize()
    assert bool((big_ws[:PAD] == CANARY).all()) and bool((big_ws[PAD + nws:] == CANARY).all())
    assert bool((big_o[:4] == CANARY).all()) and bool((big_o[10:] == CANARY).all())
    _check("objective_canaries %s %d" % (name, cap), [float(v) for v in out.cpu()], [float(cs["gold"][k]) for k in GOLD_KEYS])


# ----------------------------------------------------------------------------------- 6. run-to-run determinism
@pytest.mark.parametrize("max_rows", [None, 64])
def test_bit_identical_from_run_to_run(max_rows):
    cs = cases.load_case("klef_b229_t20")
    e, _ = _engine(cs["cfgs"])
    x, y = _xy(cs)
    runs = [_bits(torch.stack(list(e.objective(x, y, max_rows=max_rows)))) for _ in range(5)]
    assert all(torch.equal(runs[0], r) for r in runs[1:])
    _check("objective_b229 %s" % max_rows, [float(v) for v in runs[0].view(torch.float32)], [float(cs["gold"][k]) for k in GOLD_KEYS])


# ----------------------------------------------------------------------------------- 7. it leaves training alone
def test_objective_leaves_plans_gradients_and_parameters_alone():
    cs = cases.load_case("klef_b33_t7")
    model, _ = _model(cs["cfgs"])
    x, y = _xy(cs)
    e = model.engine
    e.forward(x, y, train=True, want_xhat=False)
    plan = e.plan(cs["T"], cs["B"])
    keys = set(e._plans)
    serial, consumed = plan.fwd_serial, plan.consumed
    for p in model.parameters():
        p.grad = torch.full_like(p, 0.5)
    torch.cuda.synchronize()
    before = [plan.workspace.clone(), e.grads.clone(), e.params.clone()]
    model.objective(x, y)
    e.objective(x, y, max_rows=16)
    torch.cuda.synchronize()
    for a, b in zip(before, [plan.workspace, e.grads, e.params]):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    assert set(e._plans) == keys and (plan.fwd_serial, plan.consumed) == (serial, consumed)
    assert all(bool((p.grad == 0.5).all()) for p in model.parameters())
    assert not e.__dict__.get("_predict_bufs") and not e.__dict__.get("_encode_bufs") and not e.__dict__.get("_decode_bufs")


# ----------------------------------------------------------------------------------- 8. allocation, capture
def test_no_allocation_after_the_first_call_and_capture_follows_the_input():
    cs = cases.load_case("klef_b33_t7")
    model, _ = _model(cs["cfgs"])
    x, y = _xy(cs)
    xin = x.clone()
    for _ in range(2):
        model.objective(xin, y)
    torch.cuda.synchronize()
    allocated = torch.cuda.memory_allocated()
    count = torch.cuda.memory_stats()["allocation.all.allocated"]
    torch.cuda.set_sync_debug_mode("error")
    try:
        for _ in range(10):
            model.objective(xin, y)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.cuda.memory_allocated() <= allocated
    assert torch.cuda.memory_stats()["allocation.all.allocated"] == count
    first = _bits(torch.stack(list(model.objective(xin, y))))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        gobj = model.objective(xin, y)
    xn, _ = synth.make_batch(cs["cfg"]["input_dims"], cs["B"], cs["T"], seed=23, output_dim=cs["cfg"]["output_dim"])
    x2 = torch.from_numpy(xn).cuda()
    xin.copy_(x2)
    graph.replay()
    torch.cuda.synchronize()
    replayed = _bits(torch.stack(list(gobj)))
    assert not torch.equal(replayed, first)                  # (the new input did change the result)
    assert torch.equal(replayed, _bits(torch.stack(list(model.objective(x2, y)))))
    assert torch.equal(first, _bits(torch.stack(list(model.objective(x, y)))))


def test_epoch_tail_in_one_captured_graph():
    import factorized_amd.optim as optim
    from factorized_amd.checkpoint import KeepBest
    from factorized_amd.lr_scheduler import ReduceLROnPlateau
    cs = cases.load_case("klef_b33_t7")
    model, _ = _model(cs["cfgs"])
    x, y = _xy(cs)
    lr = torch.tensor([1e-3], device="cuda")
    optimizer = optim.Adam(model.parameters(), lr=lr, capturable=True)
    model.engine
    scheduler = ReduceLROnPlateau(optimizer, "min", patience=0)
    best = KeepBest(model)
    loss = model.objective(x, y).loss                    # warm-up: buffers, code objects, the consumers' state blocks
    scheduler.step(loss)
    best.update(loss)
    assert scheduler.last_path == "device" and best.last_path == "flat"
    torch.cuda.synchronize()
    epoch0, calls0 = scheduler.last_epoch, best.calls
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        gloss = model.objective(x, y).loss
        scheduler.step(gloss)
        best.update(gloss)
    assert gloss.dim() == 0 and gloss.is_cuda and not gloss.requires_grad
    graph.replay()
    torch.cuda.synchronize()
    first = gloss.clone()
    assert torch.equal(_bits(first), _bits(model.objective(x, y).loss.clone()))
    with torch.no_grad():
        model.decoder_l.fc1.bias.add_(0.25)              # in place: the graph reads the same storage; only gen_l sees it
    graph.replay()
    torch.cuda.synchronize()
    second = gloss.clone()
    assert not torch.equal(_bits(first), _bits(second))
    assert torch.equal(_bits(second), _bits(model.objective(x, y).loss.clone()))
    assert scheduler.last_epoch == epoch0 + 2 and best.calls == calls0 + 2


# ----------------------------------------------------------------------------------- 9. fallbacks
def test_wide_sizes_are_refused_by_the_entry_and_fall_back():
    cfgs = configs.canonical_configs(dropout=False, zv_size=96, fl_size=120)     # ef encoder h = 136, decoder l h = 136
    cfg = cfgs[0]
    B, T = 5, 3
    xn, yn = synth.make_batch(cfg["input_dims"], B, T, seed=21, output_dim=cfg["output_dim"])
    model, w = _model(cfgs)
    x, y = torch.from_numpy(xn).cuda(), torch.from_numpy(yn).cuda()
    e = model.engine
    ws = torch.empty(max(e.objective_workspace_floats(T, B), 1 << 16), device="cuda")
    out = torch.zeros(6, device="cuda")
    assert _call_abi(e, x, y, ws, out, 0) == _lib.MFM_ERR_UNSUPPORTED
    assert b"136" in _lib.lib().mfm_last_error()
    got = _vals(model.objective(x, y))
    assert e._objective_refused and not e.__dict__.get("_objective_bufs")
    m = O.build("kl_ef", cfgs)
    O.load_numpy_weights(m, w)
    m.eval()
    torch.set_num_threads(4)
    with torch.no_grad():
        ref = O.loss_terms(m, torch.from_numpy(xn), torch.from_numpy(yn), cfg, "l1")
    _check("objective_wide", got, [float(ref[k]) for k in FIELDS])


@pytest.mark.parametrize("name", ["kl_b32_t20", "mmd_b32_t20"])
def test_other_variants_take_the_eval_forward(name):
    cs = cases.load_case(name)
    model, _ = _model(cs["cfgs"], CLS[cs["variant"]])
    x, y = _xy(cs)
    if cs["variant"] == "mmd":
        cfg = cs["cfg"]
        g = torch.from_numpy(np.ascontiguousarray(cs["gold"]["mmd_gauss"]))
        model.mmd_gauss = [t.cuda() for t in torch.split(g, [cfg["zl_size"], cfg["za_size"], cfg["zv_size"], cfg["zy_size"]], dim=1)]
    model.train()
    obj = model.objective(x, y)
    assert model.training
    for v in obj:
        assert v.dim() == 0 and v.is_cuda and not v.requires_grad
    _check("objective_variant " + name, _vals(obj), [float(cs["gold"][k]) for k in GOLD_KEYS])
    assert not model.engine.__dict__.get("_objective_bufs")


# ----------------------------------------------------------------------------------- 10. refusals
def test_refusals(monkeypatch):
    s = _b33()
    model, _ = _model(s["cs"]["cfgs"])
    e = model.engine
    x, y = s["x"], s["y"]
    T, N, D = x.shape
    torch.cuda.synchronize()
    L, calls = _lib.lib(), []
    real = L.mfm_objective_klef
    monkeypatch.setattr(L, "mfm_objective_klef", lambda *a: (calls.append("mfm_objective_klef"), real(*a))[1], raising=True)
    bad = [
        lambda: model.objective(x.cpu(), y),                                         # CPU tensors
        lambda: model.objective(x, y.cpu()),
        lambda: model.objective(x[:, :, :-1], y),                                    # wrong feature count
        lambda: model.objective(x, y[:-1].contiguous()),                             # wrong label count
        lambda: model.objective(x, torch.cat([y.view(N, -1)] * 2, dim=1).contiguous()),
        lambda: model.objective(x, y.double()),
        lambda: model.objective(x[:, :0].contiguous(), y[:0].contiguous()),          # an empty split
        lambda: model.objective(x, None),
        lambda: e.objective(x, y, max_rows=0),
    ]
    for i, call in enumerate(bad):
        with pytest.raises(_lib.MfmError):
            call()
            pytest.fail("call %d was accepted" % i)
    assert not calls                                         # the entry was not reached: nothing was launched
    assert not e.__dict__.get("_objective_bufs") and not e._plans
    model.objective(x, y)                                    # (the counter does count)
    assert calls == ["mfm_objective_klef"]
