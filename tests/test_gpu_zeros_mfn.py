"""The zeroed-modality test protocol of the MFN classes (MFM_KL, MFM: engine.predict_zeros -> mfm_predict_zeros_mfn) on the MI355X:
the fused path is taken, sizes where nothing is a multiple of 4 or of a tile, the reference's own run (tests/golden/
{kl,mmd}_zeros_b19_t9.npz), predict() on explicitly zeroed copies and the unchanged fallback, row chunks and determinism, both
tile forms, containment and x off a 16-byte boundary through the raw ABI, side effects, capture, data that is not unit noise,
and the refusals.  Numeric bound: the project's 1e-4 relative fp32 tolerance (tests.cases.rel_err) with the floors of
test_gpu_zeros.py; the oracle is tests/zeros_ref.oracle_zeros."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from factorized_amd import _lib, configs, synth
from tests import cases, zeros_ref
from tests import data_regimes as DR
from tests.mfn_entries import bits as _bits, CANARY, canary as _canary, intact as _intact, model as _model, odd_cfgs as _odd_cfgs, ptr as _p
from tests.cases import rel_err

pytestmark = pytest.mark.gpu
TOL = 1e-4
VARIANTS = ["kl", "mmd"]
def _zbits(z):
    return [_bits(z.y_hat), _bits(z.gen)] + ([] if z.disc is None else [_bits(z.disc)])


def _host(z):
    """the three fields on the host (the engine reuses its result tensors: these are copies)"""
    return dict(y_hat=z.y_hat.cpu().numpy().copy(), gen=z.gen.cpu().numpy().astype(np.float64),
                disc=None if z.disc is None else z.disc.cpu().numpy().astype(np.float64))


def _check(tag, got, want, tol=TOL):
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
    assert worst <= tol, (tag, ey, eg, ed)
    return worst


_SHARED = {}


def _canon(variant):
    """the canonical config at N = 33, T = 7 with its model, its oracle and the fused entry's unchunked result, computed once"""
    if variant not in _SHARED:
        cfgs = configs.canonical_configs(dropout=False)
        cfg = cfgs[0]
        model, w = _model(cfgs, variant)
        xn, yn = synth.make_batch(cfg["input_dims"], 33, 7, seed=5, output_dim=cfg["output_dim"])
        x, y = torch.from_numpy(xn).cuda(), torch.from_numpy(yn).cuda()
        ref = zeros_ref.oracle_zeros(variant, cfgs, w, xn, yn)
        z = model.predict_zeros(x, y)
        _SHARED[variant] = dict(cfgs=cfgs, cfg=cfg, model=model, e=model.engine, w=w, x=x, y=y, xn=xn, yn=yn, ref=ref, got=_host(z),
                                bits=_zbits(z), T=7, N=33)
    return _SHARED[variant]


# ----------------------------------------------------------------------------------- 1. the fused path is taken
@pytest.mark.parametrize("variant", VARIANTS)
def test_fused_path_is_taken(variant):
    from factorized_amd import engine
    s = _canon(variant)
    e = s["e"]
    assert e.__dict__.get("_zeros_mfn_bufs") and (s["T"], s["N"], e.PREDICT_MAX_ROWS) in e._zeros_mfn_bufs
    assert not e.__dict__.get("_zeros_bufs") and not e._plans
    assert not e.__dict__.get("_zeros_mfn_refused")
    z = s["model"].predict_zeros(s["x"], s["y"])
    assert isinstance(z, engine.Zeros)
    assert tuple(z.y_hat.shape) == (3, s["N"], s["cfg"]["output_dim"]) and tuple(z.gen.shape) == (3,) and tuple(z.disc.shape) == (3,)
    for t in z:
        assert t.is_cuda and t.dtype == torch.float32 and not t.requires_grad
    cases.report("zeros_mfn_canon_" + variant, _check("zeros_mfn fused " + variant, s["got"], s["ref"]))
    assert e.predict_zeros_workspace_floats(s["T"], s["N"]) == e._zeros_mfn_bufs[(s["T"], s["N"], e.PREDICT_MAX_ROWS)][0].numel()


# ----------------------------------------------------------------------------------- 2. odd sizes
@pytest.mark.parametrize("variant", VARIANTS)
def test_odd_sizes_with_and_without_labels(variant):
    """the recurrences take the per-LSTM launches; every weight row and record is off 16 bytes"""
    cfgs = _odd_cfgs()
    cfg = cfgs[0]
    model, w = _model(cfgs, variant)
    e = model.engine
    for T, N in ((1, 1), (2, 19), (9, 33)):
        xn, yn = synth.make_batch(cfg["input_dims"], N, T, seed=3 + T, output_dim=cfg["output_dim"])
        x, y = torch.from_numpy(xn).cuda(), torch.from_numpy(yn).cuda()
        ref = zeros_ref.oracle_zeros(variant, cfgs, w, xn, yn)
        got = _host(model.predict_zeros(x, y))
        assert e._zeros_mfn_bufs.get((T, N, e.PREDICT_MAX_ROWS)) is not None
        _check("zeros_mfn odd %s T%d N%d" % (variant, T, N), got, ref)
        z = model.predict_zeros(x)
        assert z.disc is None
        _check("zeros_mfn odd %s T%d N%d no labels" % (variant, T, N), _host(z), dict(ref, disc=None))
    assert not e._plans and not e.__dict__.get("_zeros_bufs")


@pytest.mark.parametrize("variant", VARIANTS)
def test_cross_entropy_with_three_classes(variant):
    cfgs = _odd_cfgs(loss="ce", output_dim=3)
    cfg = cfgs[0]
    N, T = 19, 2
    xn, yn = synth.make_batch(cfg["input_dims"], N, T, seed=5, output_dim=3, classes=3)
    model, w = _model(cfgs, variant)
    x, y = torch.from_numpy(xn).cuda(), torch.from_numpy(yn).cuda()
    ref = zeros_ref.oracle_zeros(variant, cfgs, w, xn, yn)
    _check("zeros_mfn ce " + variant, _host(model.predict_zeros(x, y)), ref)
    _check("zeros_mfn ce chunks " + variant, _host(model.engine.predict_zeros(x, y, max_rows=4)), ref)
    assert model.engine._zeros_mfn_bufs


# ----------------------------------------------------------------------------------- 3. the reference's own run
@pytest.mark.parametrize("variant", VARIANTS)
def test_matches_the_reference_fixture(variant):
    gold = np.load(os.path.join(cases.GOLDEN, "%s_zeros_b19_t9.npz" % variant))
    cfgs = _odd_cfgs()
    cfg = cfgs[0]
    B, T = [int(v) for v in gold["meta"]]
    xn, yn = synth.make_batch(cfg["input_dims"], B, T, seed=7, output_dim=cfg["output_dim"])
    model, _ = _model(cfgs, variant)
    z = model.predict_zeros(torch.from_numpy(xn).cuda(), torch.from_numpy(yn).cuda())
    worst = _check("zeros_mfn fixture " + variant, _host(z), dict(y_hat=gold["y_hat"], gen=gold["gen"], disc=gold["disc"]))
    cases.report("zeros_mfn_fixture_" + variant, worst)
    assert model.engine._zeros_mfn_bufs and not model.engine._plans


# ----------------------------------------------------------------------------------- 4. against the project itself
@pytest.mark.parametrize("variant", VARIANTS)
def test_agrees_with_predict_on_zeroed_copies_and_with_the_fallback(variant):
    s = _canon(variant)
    m2, _ = _model(s["cfgs"], variant)
    y_hat = [m2.predict(zeros_ref.zeroed(s["x"], s["cfg"], c)).cpu().numpy().copy() for c in range(3)]
    for c in range(3):
        err = rel_err(s["got"]["y_hat"][c], y_hat[c])
        print("zeros_mfn vs predict %s case %d %.3e" % (variant, c, err))
        assert err <= TOL, (c, err)
    m2.engine._zeros_mfn_refused = True                  # the fallback that was the only path before: three eval forwards
    fb = _host(m2.predict_zeros(s["x"], s["y"]))
    assert not m2.engine.__dict__.get("_zeros_mfn_bufs")
    _check("zeros_mfn vs fallback " + variant, s["got"], fb)


# ----------------------------------------------------------------------------------- 5. row chunks, determinism
@pytest.mark.parametrize("variant", VARIANTS)
def test_row_chunks_and_two_calls(variant):
    s = _canon(variant)
    e, L = s["e"], _lib.lib()
    for cap in (1, 7, 16, None):
        assert L.mfm_predict_zeros_mfn_tile_rows(s["N"], cap or e.PREDICT_MAX_ROWS) == 1          # one tile-row form throughout
        z = e.predict_zeros(s["x"], s["y"], max_rows=cap)
        first = _zbits(z)
        got = _host(z)
        assert torch.equal(first[0], s["bits"][0]), cap                                            # y_hat: bit-equal
        for k in ("gen", "disc"):                                                                  # fp64 sums, another order
            for c in range(3):
                assert abs(got[k][c] - s["got"][k][c]) <= 1e-6 * abs(s["got"][k][c]), (cap, k, c, got[k][c], s["got"][k][c])
        z2 = e.predict_zeros(s["x"], s["y"], max_rows=cap)
        assert all(torch.equal(a, b) for a, b in zip(_zbits(z2), first)), cap                      # two calls: bit-equal
        assert z2.y_hat.data_ptr() == z.y_hat.data_ptr() and z2.gen.data_ptr() == z.gen.data_ptr() and z2.disc.data_ptr() == z.disc.data_ptr()
    assert all(torch.equal(a, b) for a, b in zip(_zbits(e.predict_zeros(s["x"], s["y"])), s["bits"]))
    z = e.predict_zeros(s["x"])
    assert z.disc is None and all(torch.equal(a, b) for a, b in zip(_zbits(z), s["bits"][:2]))


# ----------------------------------------------------------------------------------- 6. both tile forms
@pytest.mark.parametrize("variant", VARIANTS)
def test_four_row_tiles_and_32_triple_attention_tiles(variant):
    """one chunk of N = 11 * CUs + 1 rows at T = 2: the three recurrences (and the decoders) run on four-row tiles (3 N >= 6 CUs,
    the last tile with one row) and the attention chain takes 32 triples per workgroup (3 * 2 * N / 16 > 4 CUs)."""
    s = _canon(variant)
    L = _lib.lib()
    cus = L.mfm_device_cus()
    N, T = 11 * cus + 1, 2
    assert (3 * T * N + 15) // 16 > 4 * cus and L.mfm_predict_zeros_mfn_tile_rows(N, N) == 4
    xn, yn = synth.make_batch(s["cfg"]["input_dims"], N, T, seed=11, output_dim=s["cfg"]["output_dim"])
    x, y = torch.from_numpy(xn).cuda(), torch.from_numpy(yn).cuda()
    ref = zeros_ref.oracle_zeros(variant, s["cfgs"], s["w"], xn, yn)
    _check("zeros_mfn four-row tiles " + variant, _host(s["e"].predict_zeros(x, y, max_rows=N)), ref)


def test_four_row_tiles_on_odd_sizes_take_a_launch_per_lstm():
    cfgs = _odd_cfgs()
    cfg = cfgs[0]
    model, w = _model(cfgs, "kl")
    cus = _lib.lib().mfm_device_cus()
    N, T = 2 * cus + 1, 3
    xn, yn = synth.make_batch(cfg["input_dims"], N, T, seed=13, output_dim=cfg["output_dim"])
    got = _host(model.engine.predict_zeros(torch.from_numpy(xn).cuda(), torch.from_numpy(yn).cuda(), max_rows=N))
    _check("zeros_mfn odd four-row tiles", got, zeros_ref.oracle_zeros("kl", cfgs, w, xn, yn))


# ----------------------------------------------------------------------------------- 7. containment, x off a 16-byte boundary
def _abi(s, variant, x, y, cap, sizes=None, expect=0):
    """mfm_predict_zeros_mfn through the C ABI on canary-framed workspace and outputs -> (bits of y_hat, gen, disc) after checking
    that nothing outside them was touched; expect != 0: the return code, and nothing at all was touched"""
    from factorized_amd import engine
    e, c, T, N = s["e"], s["cfg"], x.shape[0], x.shape[1]
    od = c["output_dim"]
    L = _lib.lib()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    good = e._mfn_sizes()
    nws = int(L.mfm_predict_zeros_mfn_workspace_floats(T, N, good, cap))
    assert nws > 0 and nws == e.predict_zeros_workspace_floats(T, N, max_rows=cap or N)
    big_ws, ws = _canary(nws)
    big_y, y_hat = _canary(3 * N * od)
    big_o = torch.full((4 + 3 + 4 + 3 + 4,), CANARY, dtype=torch.int32, device="cuda")
    gen, disc = big_o[4:7].view(torch.float32), big_o[11:14].view(torch.float32)
    names = engine.MFMEngine._ENCODE_MFN_TENSORS[variant] + engine.MFMEngine._DECODE_TENSORS
    offs = (C.c_int64 * len(names))(*[e.layout.offsets[n] for n in names])
    rc = L.mfm_predict_zeros_mfn(T, N, sizes or good, _p(e.params), offs, _p(x), _p(y), _p(ws), _p(y_hat), _p(gen),
                                 _p(disc) if y is not None else None, cap, stream)
    torch.cuda.synchronize()
    assert rc == expect, (rc, L.mfm_last_error())
    if expect != 0:
        assert bool((big_ws == CANARY).all()) and bool((big_y == CANARY).all()) and bool((big_o == CANARY).all())      # nothing was enqueued
        return None
    assert _intact(big_ws, nws) and _intact(big_y, 3 * N * od)
    assert bool((big_o[:4] == CANARY).all()) and bool((big_o[7:11] == CANARY).all()) and bool((big_o[14:] == CANARY).all())
    if y is None:
        assert bool((big_o[11:14] == CANARY).all())
    return [_bits(y_hat.view(3, N, od)), _bits(gen)] + ([] if y is None else [_bits(disc)])


@pytest.mark.parametrize("variant,cap", [("kl", 0), ("kl", 7), ("mmd", 0), ("mmd", 7)])
def test_canaries_around_workspace_and_outputs(variant, cap):
    s = _canon(variant)
    got = _abi(s, variant, s["x"], s["y"], cap)
    want = s["bits"] if cap == 0 else _zbits(s["e"].predict_zeros(s["x"], s["y"], max_rows=cap))
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    assert all(torch.equal(a, b) for a, b in zip(_abi(s, variant, s["x"], None, cap), want[:2]))


@pytest.mark.parametrize("off", [1, 2, 3])
def test_x_may_start_off_a_16_byte_boundary(off):
    s = _canon("kl")
    buf = torch.zeros(s["x"].numel() + 8, dtype=torch.float32, device="cuda")
    assert buf.data_ptr() % 16 == 0
    xv = buf[off:off + s["x"].numel()].view(s["x"].shape)
    xv.copy_(s["x"])
    assert xv.data_ptr() % 16 == 4 * off
    assert all(torch.equal(a, b) for a, b in zip(_abi(s, "kl", xv, s["y"], 0), s["bits"]))
    assert all(torch.equal(a, b) for a, b in zip(_abi(s, "kl", xv, s["y"], 7), _zbits(s["e"].predict_zeros(s["x"], s["y"], max_rows=7))))
    assert all(torch.equal(a, b) for a, b in zip(_zbits(s["e"].predict_zeros(xv, s["y"])), s["bits"]))


def test_odd_sizes_inside_canaries():
    cfgs = _odd_cfgs()
    cfg = cfgs[0]
    model, w = _model(cfgs, "mmd")
    N, T = 19, 9
    xn, yn = synth.make_batch(cfg["input_dims"], N, T, seed=7, output_dim=cfg["output_dim"])
    x, y = torch.from_numpy(xn).cuda(), torch.from_numpy(yn).cuda()
    s = dict(e=model.engine, cfg=cfg)
    want = _zbits(model.engine.predict_zeros(x, y, max_rows=5))
    assert all(torch.equal(a, b) for a, b in zip(_abi(s, "mmd", x, y, 5), want))


# ----------------------------------------------------------------------------------- 8. side effects and capture
@pytest.mark.parametrize("variant", VARIANTS)
def test_leaves_input_parameters_mode_and_plans_alone(variant):
    cfgs = configs.canonical_configs(dropout=True)
    model, _ = _model(cfgs, variant)
    s = _canon(variant)
    x, y = s["x"].clone(), s["y"].clone()
    e = model.engine
    x0, p0 = x.clone(), e.params.clone()
    for p in model.parameters():
        p.grad = torch.full_like(p, 0.5)
    res = {}
    for mode in (True, False):
        model.train(mode)
        z = model.predict_zeros(x, y)
        res[mode] = _zbits(z)
        assert model.training == mode
        assert all(not t.requires_grad and t.grad_fn is None for t in z)
    e.predict_zeros(x, y, max_rows=16)
    torch.cuda.synchronize()
    # (dropout does not scale the eval computation: the numbers are those of the dropout-free configuration)
    assert all(torch.equal(u, v) for u, v in zip(res[True], res[False])) and all(torch.equal(u, v) for u, v in zip(res[True], s["bits"]))
    assert torch.equal(_bits(x), _bits(x0)) and torch.equal(_bits(e.params), _bits(p0))
    assert all(bool((p.grad == 0.5).all()) for p in model.parameters())
    assert not e._plans and e._zeros_mfn_bufs
    assert not e.__dict__.get("_zeros_bufs") and not e.__dict__.get("_encode_mfn_bufs") and not e.__dict__.get("_predict_bufs")


@pytest.mark.parametrize("variant", VARIANTS)
def test_one_capture_replayed_twice_equals_the_eager_result(variant):
    s = _canon(variant)
    model, x, y = s["model"], s["x"], s["y"]
    model.predict_zeros(x, y)                                # warm-up: buffers, code objects
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        gz = model.predict_zeros(x, y)
    for _ in range(2):
        gz.y_hat.zero_(); gz.gen.zero_(); gz.disc.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(_zbits(gz), s["bits"]))


def test_no_allocation_and_no_synchronisation_after_the_first_call():
    s = _canon("kl")
    model, x, y = s["model"], s["x"], s["y"]
    for _ in range(2):
        model.predict_zeros(x, y)
    torch.cuda.synchronize()
    allocated = torch.cuda.memory_allocated()
    count = torch.cuda.memory_stats()["allocation.all.allocated"]
    torch.cuda.set_sync_debug_mode("error")
    try:
        for _ in range(5):
            model.predict_zeros(x, y)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.cuda.memory_allocated() == allocated
    assert torch.cuda.memory_stats()["allocation.all.allocated"] == count


# ----------------------------------------------------------------------------------- 9. data that is not unit noise
@pytest.mark.parametrize("regime", ["mixed", "saturated"])
@pytest.mark.parametrize("variant", VARIANTS)
def test_data_regimes_against_the_float64_oracle(variant, regime):
    """mixed: the cell states that meet in cStar are fed by inputs 10^4 apart, and the real a record sits beside a's zero row;
    saturated: acoustic pre-activations beyond +-88.7 in the MFN's lstm_a"""
    cfgs = DR.canonical()
    model, w = _model(cfgs, variant)
    xn, yn = DR.make(regime, 19, 5)
    ref = zeros_ref.oracle_zeros(variant, cfgs, w, xn, yn, double=True)
    got = _host(model.predict_zeros(torch.from_numpy(xn).cuda(), torch.from_numpy(yn).cuda()))
    assert model.engine._zeros_mfn_bufs
    cases.report("zeros_mfn_%s_%s" % (regime, variant), _check("zeros_mfn %s %s" % (regime, variant), got, ref))


# ----------------------------------------------------------------------------------- 10. refusals
def test_windowsize_3_is_refused_and_nothing_is_enqueued():
    s = _canon("kl")
    sizes = s["e"]._mfn_sizes()
    sizes[11] = 3
    _abi(s, "kl", s["x"], s["y"], 0, sizes=sizes, expect=_lib.MFM_ERR_UNSUPPORTED)
    assert "windowsize 3" in _lib.lib().mfm_last_error().decode()


def _refused_136(cfgs, monkeypatch):
    """a configuration with a hidden size of 136: the entry refuses it through the raw ABI with the size in the reason and
    enqueues nothing -> (model, weights, x, y, xn, yn, calls): the library function now counts its calls"""
    cfg = cfgs[0]
    model, w = _model(cfgs, "kl")
    T, N = 3, 5
    xn, yn = synth.make_batch(cfg["input_dims"], N, T, seed=21, output_dim=cfg["output_dim"])
    x, y = torch.from_numpy(xn).cuda(), torch.from_numpy(yn).cuda()
    _abi(dict(e=model.engine, cfg=cfg), "kl", x, y, 0, expect=_lib.MFM_ERR_UNSUPPORTED)
    assert "136" in _lib.lib().mfm_last_error().decode()
    L, calls = _lib.lib(), []
    real = L.mfm_predict_zeros_mfn
    monkeypatch.setattr(L, "mfm_predict_zeros_mfn", lambda *a: (calls.append(1), real(*a))[1], raising=True)
    return model, w, x, y, xn, yn, calls


def test_a_wide_decoder_is_refused_remembered_and_falls_back(monkeypatch):
    """decoder l with fy + fl = 136: the three eval forwards on a plan take it step by step"""
    cfgs = _odd_cfgs(fl_size=120)
    model, w, x, y, xn, yn, calls = _refused_136(cfgs, monkeypatch)
    e = model.engine
    got = _host(model.predict_zeros(x, y))
    assert calls == [1] and e._zeros_mfn_refused and not e.__dict__.get("_zeros_mfn_bufs")
    _check("zeros_mfn decoder 136 fallback", got, zeros_ref.oracle_zeros("kl", cfgs, w, xn, yn))
    model.predict_zeros(x, y)                                # remembered: the entry is not asked again
    assert calls == [1] and not e.__dict__.get("_zeros_mfn_bufs")


def test_wide_h_dims_are_refused_and_remembered(monkeypatch):
    """an h_dims entry of 136.  The fallback is the unchanged one, three eval forwards on a fused plan, and the fused plan
    has no MFN LSTM above 128 (mfm_plan_create says so, as it did for predict_zeros of this configuration before the entry
    existed): the model's answer here is that error, not the oracle's numbers.  What the entry adds is checked: the refusal with
    its reason, nothing enqueued, remembered, the entry not called again."""
    cfgs = _odd_cfgs(h_dims=[9, 136, 7])
    model, w, x, y, xn, yn, calls = _refused_136(cfgs, monkeypatch)
    e = model.engine
    for _ in range(2):
        with pytest.raises(_lib.MfmError, match="MFN LSTM sizes above 128"):
            model.predict_zeros(x, y)
        assert calls == [1] and e._zeros_mfn_refused and not e.__dict__.get("_zeros_mfn_bufs")


def test_bad_arguments_do_not_reach_the_library_and_a_one_time_refusal_is_not_remembered(monkeypatch):
    s = _canon("kl")
    model, e, x, y = s["model"], s["e"], s["x"], s["y"]
    N = x.shape[1]
    L, calls = _lib.lib(), []
    real = L.mfm_predict_zeros_mfn
    monkeypatch.setattr(L, "mfm_predict_zeros_mfn", lambda *a: (calls.append(1), real(*a))[1], raising=True)
    bufs = dict(e._zeros_mfn_bufs)
    bad = [
        lambda: model.predict_zeros(x.cpu(), y),
        lambda: model.predict_zeros(x, y.cpu()),
        lambda: model.predict_zeros(x[:, :, :-1], y),
        lambda: model.predict_zeros(x, y[:-1].contiguous()),
        lambda: model.predict_zeros(x, y.double()),
        lambda: model.predict_zeros(x[:, :0].contiguous(), y[:0].contiguous()),
        lambda: e.predict_zeros(x, y, max_rows=0),
    ]
    for i, call in enumerate(bad):
        with pytest.raises(_lib.MfmError):
            call()
            pytest.fail("call %d was accepted" % i)
    assert not calls and e._zeros_mfn_bufs == bufs
    assert all(torch.equal(a, b) for a, b in zip(_zbits(model.predict_zeros(x, y)), s["bits"])) and calls == [1]      # (the counter does count)
    # a refusal with legal sizes (as for the LDS of one call's shape) depends on N and max_rows: it holds for that call alone,
    # and the call still answers through the fallback (on a model of its own: the fallback builds a plan)
    m2, _ = _model(s["cfgs"], "kl")
    e2 = m2.engine
    monkeypatch.setattr(L, "mfm_predict_zeros_mfn", lambda *a: _lib.MFM_ERR_UNSUPPORTED, raising=True)
    fb = _host(e2.predict_zeros(x, y, max_rows=5))
    assert not e2._zeros_mfn_refused and not e2.__dict__.get("_zeros_mfn_bufs")
    _check("zeros_mfn one-time refusal fallback", fb, s["ref"])
    monkeypatch.setattr(L, "mfm_predict_zeros_mfn", real, raising=True)
    z = e2.predict_zeros(x, y, max_rows=5)
    assert (s["T"], N, 5) in e2._zeros_mfn_bufs and torch.equal(_bits(z.y_hat), s["bits"][0])
