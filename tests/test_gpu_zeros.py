"""The zeroed-modality test protocol (engine.predict_zeros, model.predict_zeros, mfm_predict_zeros_klef) on the MI355X: y_hat of the
three cases, the zeroed modality's reconstruction error against the real one and the label loss per case, against the reference's
own run (tests/golden/klef_zeros_b19_t9.npz) and against the CPU oracle on zeroed copies; row chunks, cross entropy, the call
without labels, the eval forward, run-to-run determinism, canaries, what it must leave alone, capture, the fallbacks and the
refusal.  Numeric bound: the project's 1e-4 relative fp32 tolerance with the floors of test_gpu_objective.py / test_gpu_predict.py."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from factorized_amd import _lib, configs, synth
from tests import cases, zeros_ref
from tests.cases import rel_err

pytestmark = pytest.mark.gpu
TOL = 1e-4
CANARY = 0x7FC0DEAD                   # a NaN with a payload: any store over it shows
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


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _host(z):
    """the three fields on the host (the engine reuses its result tensors: these are copies)"""
    return dict(y_hat=z.y_hat.cpu().numpy().copy(), gen=z.gen.cpu().numpy().astype(np.float64),
                disc=None if z.disc is None else z.disc.cpu().numpy().astype(np.float64))


def _check(tag, got, want):
    """got / want: dicts of y_hat [3, N, od], gen [3], disc [3] or None.  Prints every figure before it asserts"""
    ey = [rel_err(got["y_hat"][c], want["y_hat"][c]) for c in range(3)]
    eg = [abs(g - w) / max(abs(w), 1e-3) for g, w in zip(got["gen"], want["gen"])]
    ed = []
    if want["disc"] is not None and got["disc"] is not None:
        ed = [abs(g - w) / max(abs(w), 1e-3) for g, w in zip(got["disc"], want["disc"])]
    print("%s y_hat %s gen %s disc %s" % (tag, " ".join("%.2e" % e for e in ey),
                                          " ".join("%.8g/%.8g (%.2e)" % (g, w, e) for g, w, e in zip(got["gen"], want["gen"], eg)),
                                          " ".join("%.2e" % e for e in ed)))
    worst = max(ey + eg + ed)
    assert worst <= TOL, (tag, ey, eg, ed)
    return worst


_B33 = {}


def _b33():
    """the B=33, T=7 case with its oracle and its unchunked result, computed once"""
    if not _B33:
        cs = cases.load_case("klef_b33_t7")
        e, w = _engine(cs["cfgs"])
        x, y = torch.from_numpy(cs["x"]).cuda(), torch.from_numpy(cs["y"]).cuda()
        ref = zeros_ref.oracle_zeros("kl_ef", cs["cfgs"], w, cs["x"], cs["y"])
        z = e.predict_zeros(x, y)
        _B33.update(cs=cs, e=e, w=w, x=x, y=y, ref=ref, got=_host(z), bits=[_bits(z.y_hat), _bits(z.gen), _bits(z.disc)])
    return _B33


# ----------------------------------------------------------------------------------- 1. the reference's own run
def test_matches_the_reference_fixture():
    """odd sizes: the recurrences take the per-LSTM launches"""
    from factorized_amd import engine
    cs = cases.load_case("klef_odd_b19_t9")
    gold = np.load(os.path.join(cases.GOLDEN, "klef_zeros_b19_t9.npz"))
    model, _ = _model(cs["cfgs"])
    x, y = torch.from_numpy(cs["x"]).cuda(), torch.from_numpy(cs["y"]).cuda()
    z = model.predict_zeros(x, y)
    assert isinstance(z, engine.Zeros)
    od = cs["cfg"]["output_dim"]
    assert tuple(z.y_hat.shape) == (3, cs["B"], od) and tuple(z.gen.shape) == (3,) and tuple(z.disc.shape) == (3,)
    for t in z:
        assert t.is_cuda and t.dtype == torch.float32 and not t.requires_grad
    worst = _check("zeros_fixture", _host(z), dict(y_hat=gold["y_hat"], gen=gold["gen"], disc=gold["disc"]))
    cases.report("zeros_fixture", worst)
    assert model.engine._zeros_bufs and not model.engine._plans


# ----------------------------------------------------------------------------------- 2. the oracle on zeroed copies
@pytest.mark.parametrize("name", ["klef_b5_t1", "klef_b1_t20", "klef_b33_t7"])
def test_matches_the_oracle(name):
    if name == "klef_b33_t7":
        s = _b33()
        _check("zeros_oracle " + name, s["got"], s["ref"])
        return
    cs = cases.load_case(name)
    e, w = _engine(cs["cfgs"])
    x, y = torch.from_numpy(cs["x"]).cuda(), torch.from_numpy(cs["y"]).cuda()
    ref = zeros_ref.oracle_zeros("kl_ef", cs["cfgs"], w, cs["x"], cs["y"])
    cases.report("zeros_oracle_" + name, _check("zeros_oracle " + name, _host(e.predict_zeros(x, y)), ref))


def test_four_row_tiles():
    """three ef recurrences per row: a chunk of 2 * CUs rows or more runs them on four-row tiles (gen_tile_rows: 3 rows >= 6 CUs),
    and the three decoders with them; N = 2 * CUs + 1 leaves one row in the last tile.  Against the oracle, and against the
    same split in chunks of 64 rows (one-row tiles: 3 * 64 < 6 * CUs on any part with more than 32 CUs)."""
    cus = _lib.lib().mfm_device_cus()
    assert 3 * 64 < 6 * cus
    N, T = 2 * cus + 1, 2
    cfgs = configs.canonical_configs(dropout=False)
    cfg = cfgs[0]
    xn, yn = synth.make_batch(cfg["input_dims"], N, T, seed=11, output_dim=cfg["output_dim"])
    e, w = _engine(cfgs)
    x, y = torch.from_numpy(xn).cuda(), torch.from_numpy(yn).cuda()
    ref = zeros_ref.oracle_zeros("kl_ef", cfgs, w, xn, yn)
    four = _host(e.predict_zeros(x, y, max_rows=N))
    _check("zeros_four_rows", four, ref)
    _check("zeros_four_rows vs one-row chunks", _host(e.predict_zeros(x, y, max_rows=64)), four)


# ----------------------------------------------------------------------------------- 3. row chunks
@pytest.mark.parametrize("max_rows", [1, 4, 32, 33, 64])
def test_row_chunks(max_rows):
    """every mean is over the whole split, not the chunk or a padded tile"""
    s = _b33()
    got = _host(s["e"].predict_zeros(s["x"], s["y"], max_rows=max_rows))
    _check("zeros_chunks %d" % max_rows, got, s["got"])
    _check("zeros_chunks %d oracle" % max_rows, got, s["ref"])


# ----------------------------------------------------------------------------------- 4. cross entropy
def test_cross_entropy_with_three_classes():
    cfgs = configs.you_configs(dropout=False)
    cfg = cfgs[0]
    assert cfg["loss"] == "ce" and cfg["output_dim"] == 3
    B, T = 9, 3
    xn, yn = synth.make_batch(cfg["input_dims"], B, T, seed=5, output_dim=3, classes=3)
    e, w = _engine(cfgs)
    x, y = torch.from_numpy(xn).cuda(), torch.from_numpy(yn).cuda()
    ref = zeros_ref.oracle_zeros("kl_ef", cfgs, w, xn, yn)
    _check("zeros_ce", _host(e.predict_zeros(x, y)), ref)
    _check("zeros_ce chunks", _host(e.predict_zeros(x, y, max_rows=4)), ref)


# ----------------------------------------------------------------------------------- 5. without labels
def test_without_labels_disc_is_none_and_the_rest_keeps_its_bits():
    s = _b33()
    z = s["e"].predict_zeros(s["x"])
    assert z.disc is None
    assert torch.equal(_bits(z.y_hat), s["bits"][0]) and torch.equal(_bits(z.gen), s["bits"][1])


# ----------------------------------------------------------------------------------- 6. the eval forward
def test_agrees_with_three_eval_forwards_on_zeroed_copies():
    s = _b33()
    e2, _ = _engine(s["cs"]["cfgs"])
    cfg = s["cs"]["cfg"]
    y_hat, gen, disc = [], [], []
    for c, (a, b) in enumerate(zeros_ref.bounds(cfg)):
        out = e2.forward(zeros_ref.zeroed(s["x"], cfg, c), s["y"], train=False)
        y_hat.append(out["y_hat"].cpu().numpy().copy())
        xh = out[("x_l_hat", "x_a_hat", "x_v_hat")[c]]
        gen.append(float((xh.double() - s["x"][:, :, a:b].double()).square().mean()))
        disc.append(float(out["losses"][0]))
    _check("zeros_vs_forward", s["got"], dict(y_hat=np.stack(y_hat), gen=np.array(gen), disc=np.array(disc)))


# ----------------------------------------------------------------------------------- 7. run-to-run determinism
@pytest.mark.parametrize("max_rows", [None, 16])
def test_two_calls_give_equal_bits(max_rows):
    s = _b33()
    runs = []
    for _ in range(2):
        z = s["e"].predict_zeros(s["x"], s["y"], max_rows=max_rows)
        runs.append([_bits(z.y_hat), _bits(z.gen), _bits(z.disc)])
    assert all(torch.equal(a, b) for a, b in zip(runs[0], runs[1]))
    if max_rows is None:
        assert all(torch.equal(a, b) for a, b in zip(runs[0], s["bits"]))


# ----------------------------------------------------------------------------------- 8. nothing outside its buffers
def _call_abi(e, x, y, ws, y_hat, gen, disc, cap):
    from factorized_amd import engine
    T, N, _ = x.shape
    offs = (C.c_int64 * 78)(*[e.layout.offsets[n] for n in engine.MFMEngine._ENCODE_TENSORS + engine.MFMEngine._DECODE_TENSORS])
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    return _lib.lib().mfm_predict_zeros_klef(T, N, e._objective_sizes(), p(e.params), offs, p(x), p(y), p(ws), p(y_hat), p(gen), p(disc),
                                             cap, C.c_void_p(torch.cuda.current_stream().cuda_stream))


@pytest.mark.parametrize("name,cap", [("klef_b5_t1", 0), ("klef_b33_t7", 0), ("klef_b33_t7", 16)])
def test_canaries_around_workspace_and_outputs(name, cap):
    cs = cases.load_case(name)
    e, w = _engine(cs["cfgs"])
    x, y = torch.from_numpy(cs["x"]).cuda(), torch.from_numpy(cs["y"]).cuda()
    T, N, od = cs["T"], cs["B"], cs["cfg"]["output_dim"]
    nws = int(_lib.lib().mfm_predict_zeros_klef_workspace_floats(T, N, e._objective_sizes(), cap))
    assert nws == e.predict_zeros_workspace_floats(T, N, max_rows=cap or N)
    PAD = 256
    big_ws = torch.full((PAD + nws + PAD,), CANARY, dtype=torch.int32, device="cuda")
    big_y = torch.full((PAD + 3 * N * od + PAD,), CANARY, dtype=torch.int32, device="cuda")
    big_o = torch.full((4 + 3 + 4 + 3 + 4,), CANARY, dtype=torch.int32, device="cuda")
    ws = big_ws[PAD:PAD + nws].view(torch.float32)
    y_hat = big_y[PAD:PAD + 3 * N * od].view(torch.float32)
    gen, disc = big_o[4:7].view(torch.float32), big_o[11:14].view(torch.float32)
    assert _call_abi(e, x, y, ws, y_hat, gen, disc, cap) == 0
    torch.cuda.synchronize()
    assert bool((big_ws[:PAD] == CANARY).all()) and bool((big_ws[PAD + nws:] == CANARY).all())
    assert bool((big_y[:PAD] == CANARY).all()) and bool((big_y[PAD + 3 * N * od:] == CANARY).all())
    assert bool((big_o[:4] == CANARY).all()) and bool((big_o[7:11] == CANARY).all()) and bool((big_o[14:] == CANARY).all())
    ref = _b33()["ref"] if name == "klef_b33_t7" else zeros_ref.oracle_zeros("kl_ef", cs["cfgs"], w, cs["x"], cs["y"])
    got = dict(y_hat=y_hat.view(3, N, od).cpu().numpy(), gen=gen.cpu().numpy().astype(np.float64), disc=disc.cpu().numpy().astype(np.float64))
    _check("zeros_canaries %s %d" % (name, cap), got, ref)


# ----------------------------------------------------------------------------------- 9. what it leaves alone
def test_leaves_input_parameters_mode_and_plans_alone():
    cs = cases.load_case("klef_b33_t7")
    cfgs = configs.canonical_configs(dropout=True)
    model, _ = _model(cfgs)
    x, y = torch.from_numpy(cs["x"]).cuda(), torch.from_numpy(cs["y"]).cuda()
    e = model.engine
    x0, p0 = x.clone(), e.params.clone()
    model.train()
    a = model.predict_zeros(x, y)
    a = [_bits(a.y_hat), _bits(a.gen), _bits(a.disc)]
    assert model.training
    model.eval()
    b = model.predict_zeros(x, y)
    b = [_bits(b.y_hat), _bits(b.gen), _bits(b.disc)]
    assert not model.training
    e.predict_zeros(x, y, max_rows=16)
    torch.cuda.synchronize()
    # (dropout does not scale the eval computation: the numbers are those of the dropout-free configuration)
    assert all(torch.equal(u, v) for u, v in zip(a, b)) and all(torch.equal(u, v) for u, v in zip(a, _b33()["bits"]))
    assert torch.equal(x.view(torch.int32), x0.view(torch.int32)) and torch.equal(e.params.view(torch.int32), p0.view(torch.int32))
    assert not e._plans
    assert not e.__dict__.get("_predict_bufs") and not e.__dict__.get("_encode_bufs") and not e.__dict__.get("_objective_bufs")


def test_predict_and_objective_keep_their_bits_around_a_call():
    """the fused fc1 / squared-error launch is shared with objective(): a call in between changes nothing of theirs"""
    cs = cases.load_case("klef_b33_t7")
    e, _ = _engine(cs["cfgs"])
    x, y = torch.from_numpy(cs["x"]).cuda(), torch.from_numpy(cs["y"]).cuda()

    def both():
        p = e.predict(x, y)
        o = e.objective(x, y)
        return [_bits(p["y_hat"]), _bits(p["loss"]), _bits(torch.stack(list(o)))]
    before = both()
    e.predict_zeros(x, y)
    e.predict_zeros(x, y, max_rows=4)
    after = both()
    assert all(torch.equal(a, b) for a, b in zip(before, after))
    gold = [float(cs["gold"][k]) for k in ("fwd_loss", "fwd_disc", "fwd_gen_l", "fwd_gen_a", "fwd_gen_v", "fwd_reg")]
    got = [float(v) for v in after[2].view(torch.float32)]
    assert all(abs(g - w) <= TOL * max(abs(w), 1e-3) for g, w in zip(got, gold)), (got, gold)


# ----------------------------------------------------------------------------------- 10. capture
def test_one_capture_replayed_twice_equals_the_eager_result():
    s = _b33()
    model, _ = _model(s["cs"]["cfgs"])
    x, y = s["x"], s["y"]
    model.predict_zeros(x, y)                                # warm-up: buffers, code objects
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        gz = model.predict_zeros(x, y)
    for _ in range(2):
        gz.y_hat.zero_(); gz.gen.zero_(); gz.disc.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip([_bits(gz.y_hat), _bits(gz.gen), _bits(gz.disc)], s["bits"]))


# ----------------------------------------------------------------------------------- 11. fallbacks
@pytest.mark.parametrize("variant", ["kl", "mmd"])
def test_other_variants_take_three_eval_forwards(variant):
    cfgs = configs.canonical_configs(dropout=False)
    cfg = cfgs[0]
    B, T = 6, 4
    xn, yn = synth.make_batch(cfg["input_dims"], B, T, seed=13, output_dim=cfg["output_dim"])
    model, w = _model(cfgs, CLS[variant])
    x, y = torch.from_numpy(xn).cuda(), torch.from_numpy(yn).cuda()
    model.train()
    z = model.predict_zeros(x, y)
    assert model.training
    for t in z:
        assert t.is_cuda and t.dtype == torch.float32 and not t.requires_grad
    assert tuple(z.y_hat.shape) == (3, B, cfg["output_dim"])
    _check("zeros_variant " + variant, _host(z), zeros_ref.oracle_zeros(variant, cfgs, w, xn, yn))
    assert model.predict_zeros(x).disc is None
    assert not model.engine.__dict__.get("_zeros_bufs")


def test_wide_sizes_are_refused_by_the_entry_and_fall_back():
    cfgs = configs.canonical_configs(dropout=False, zv_size=96, fl_size=120)     # ef encoder h = 136, decoder l h = 136
    cfg = cfgs[0]
    B, T = 5, 3
    xn, yn = synth.make_batch(cfg["input_dims"], B, T, seed=21, output_dim=cfg["output_dim"])
    model, w = _model(cfgs)
    x, y = torch.from_numpy(xn).cuda(), torch.from_numpy(yn).cuda()
    e = model.engine
    ws = torch.empty(max(e.predict_zeros_workspace_floats(T, B), 1 << 16), device="cuda")
    y_hat, gen, disc = torch.zeros(3, B, cfg["output_dim"], device="cuda"), torch.zeros(3, device="cuda"), torch.zeros(3, device="cuda")
    assert _call_abi(e, x, y, ws, y_hat, gen, disc, 0) == _lib.MFM_ERR_UNSUPPORTED
    assert b"136" in _lib.lib().mfm_last_error()
    got = _host(model.predict_zeros(x, y))
    assert e._zeros_refused and not e.__dict__.get("_zeros_bufs")
    _check("zeros_wide", got, zeros_ref.oracle_zeros("kl_ef", cfgs, w, xn, yn))
    model.predict_zeros(x, y)                                # remembered: the entry is not asked again
    assert e._zeros_refused and not e.__dict__.get("_zeros_bufs")


# ----------------------------------------------------------------------------------- 12. refusals
def test_refusals(monkeypatch):
    s = _b33()
    model, _ = _model(s["cs"]["cfgs"])
    e = model.engine
    x, y = s["x"], s["y"]
    N = x.shape[1]
    torch.cuda.synchronize()
    L, calls = _lib.lib(), []
    real = L.mfm_predict_zeros_klef
    monkeypatch.setattr(L, "mfm_predict_zeros_klef", lambda *a: (calls.append("mfm_predict_zeros_klef"), real(*a))[1], raising=True)
    bad = [
        lambda: model.predict_zeros(x.cpu(), y),                                     # CPU tensors
        lambda: model.predict_zeros(x, y.cpu()),
        lambda: model.predict_zeros(x[:, :, :-1], y),                                # wrong feature count
        lambda: model.predict_zeros(x, y[:-1].contiguous()),                         # wrong label count
        lambda: model.predict_zeros(x, torch.cat([y.view(N, -1)] * 2, dim=1).contiguous()),
        lambda: model.predict_zeros(x, y.double()),
        lambda: model.predict_zeros(x[:, :0].contiguous(), y[:0].contiguous()),      # an empty split
        lambda: e.predict_zeros(x, y, max_rows=0),
    ]
    for i, call in enumerate(bad):
        with pytest.raises(_lib.MfmError):
            call()
            pytest.fail("call %d was accepted" % i)
    assert not calls                                         # the entry was not reached: nothing was launched
    assert not e.__dict__.get("_zeros_bufs") and not e._plans
    model.predict_zeros(x, y)                                # (the counter does count)
    assert calls == ["mfm_predict_zeros_klef"]
