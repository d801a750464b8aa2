"""Label-only predict / evaluate of the MFN classes (MFM_KL, MFM: engine.predict(label_only=True) -> mfm_predict_mfn) on the
MI355X: the path taken, the oracle in eval mode on the canonical config, the golden fixtures and the reference's own runs, odd
sizes, T = 1, N = 1 and cross entropy, row chunks and determinism, both tile-row forms of the recurrence launch, the 32-pair form
of the attention chain, dead parameters, containment and x off a 16-byte boundary, data that is not unit noise, the refusals,
capture with the epoch tail, and the unchanged default.  Numeric bound: the project's 1e-4 relative fp32 tolerance
(tests.cases.rel_err on y_hat; the loss with the floor max(|want|, 1e-3), as tests/test_gpu_objective_mfn.py::_check)."""
import copy
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
from tests import offset_views as OV
from tests.cases import rel_err

pytestmark = pytest.mark.gpu
TOL = 1e-4
VARIANTS = ["kl", "mmd"]
def _oracle(variant, cfgs, w, xn, yn, double=False):
    """(y_hat [N, od], the label loss) of the oracle in eval mode (float64 throughout with `double`)"""
    cfg = cfgs[0]
    m = O.build(variant, cfgs)
    O.load_numpy_weights(m, w)
    x = torch.from_numpy(np.ascontiguousarray(xn))
    if double:
        m, x = copy.deepcopy(m).double(), x.double()
    m.eval()
    torch.set_num_threads(4)
    with torch.no_grad():
        y_hat = m.forward(x)[0][3]
    y = torch.from_numpy(np.ascontiguousarray(yn))
    if cfg.get("loss", "l1") == "ce":
        loss = float(torch.nn.functional.cross_entropy(y_hat.double(), y))
    else:
        loss = float((y_hat.double() - y.double().view_as(y_hat)).abs().mean())
    return y_hat.numpy(), loss


def _run(e, x, y=None, cap=None):
    """engine.predict(label_only=True) -> (bits of y_hat, bits of the loss or None), copies (the engine reuses its tensors)"""
    out = e.predict(x, y, max_rows=cap, label_only=True)
    return _bits(out["y_hat"]), None if out["loss"] is None else _bits(out["loss"])


def _f(bits):
    return bits.view(torch.float32).numpy()


def _check(tag, yb, lb, ref):
    """y_hat within TOL of the reference (max-norm relative) and the loss within TOL with the floor; prints before it asserts"""
    ey = rel_err(_f(yb), ref[0])
    got = float(_f(lb))
    el = abs(got - ref[1]) / max(abs(ref[1]), 1e-3)
    print("%s y_hat %.2e loss %.8g/%.8g (%.2e)" % (tag, ey, got, ref[1], el))
    assert np.isfinite(_f(yb)).all() and ey <= TOL, (tag, ey)
    assert el <= TOL, (tag, got, ref[1], el)
    return max(ey, el)


_SHARED = {}


def _canon(variant):
    """the canonical config at N = 33, T = 7 with its model, the oracle's numbers and the entry's unchunked result, computed once"""
    if variant not in _SHARED:
        cfgs = configs.canonical_configs(dropout=False)
        cfg = cfgs[0]
        model, w = _model(cfgs, variant)
        xn, yn = synth.make_batch(cfg["input_dims"], 33, 7, seed=5, output_dim=cfg["output_dim"])
        x, y = torch.from_numpy(xn).cuda(), torch.from_numpy(yn).cuda()
        yb, lb = _run(model.engine, x, y)
        _SHARED[variant] = dict(cfgs=cfgs, cfg=cfg, model=model, e=model.engine, w=w, x=x, y=y, xn=xn, yn=yn,
                                ref=_oracle(variant, cfgs, w, xn, yn), yb=yb, lb=lb, T=7, N=33)
    return _SHARED[variant]


# ----------------------------------------------------------------------------------- 1. the path taken
@pytest.mark.parametrize("variant", VARIANTS)
def test_label_only_path_is_taken(variant, monkeypatch):
    s = _canon(variant)
    model, _ = _model(s["cfgs"], variant)
    e = model.engine
    L, calls = _lib.lib(), []
    real = L.mfm_predict_mfn
    monkeypatch.setattr(L, "mfm_predict_mfn", lambda *a: (calls.append(1), real(*a))[1], raising=True)
    loss = model.evaluate(s["x"], s["y"], label_only=True)
    assert calls == [1] and loss.dim() == 0 and loss.is_cuda and loss.dtype == torch.float32 and not loss.requires_grad
    assert torch.equal(_bits(loss), s["lb"])
    key = (s["T"], s["N"], e.PREDICT_MAX_ROWS)
    assert list(e.__dict__.get("_predict_mfn_bufs", {})) == [key]
    assert not e._plans and not e.__dict__.get("_predict_mfn_refused")
    for other in ("_predict_bufs", "_encode_mfn_bufs", "_objective_mfn_bufs"):
        assert not e.__dict__.get(other), other
    assert e.predict_workspace_floats(s["T"], s["N"], label_only=True) == e._predict_mfn_bufs[key][0].numel()
    y_hat = model.predict(s["x"], label_only=True)
    assert calls == [1, 1] and tuple(y_hat.shape) == (s["N"], s["cfg"]["output_dim"]) and torch.equal(_bits(y_hat), s["yb"])
    assert list(e._predict_mfn_bufs) == [key] and not e._plans


# ----------------------------------------------------------------------------------- 2. the oracle
@pytest.mark.parametrize("variant", VARIANTS)
def test_canonical_config_against_the_oracle(variant):
    s = _canon(variant)
    cases.report("predict_mfn_canon_" + variant, _check("predict_mfn canon " + variant, s["yb"], s["lb"], s["ref"]))


@pytest.mark.parametrize("name", ["kl_b32_t20", "mmd_b32_t20"])
def test_golden_fixtures(name):
    cs = cases.load_case(name)
    model, _ = _model(cs["cfgs"], cs["variant"])
    x, y = torch.from_numpy(cs["x"]).cuda(), torch.from_numpy(cs["y"]).cuda()
    yb, lb = _run(model.engine, x, y)
    _check("predict_mfn golden " + name, yb, lb, (cs["gold"]["y_hat"].reshape(cs["B"], -1), float(cs["gold"]["fwd_disc"])))
    assert model.engine._predict_mfn_bufs and not model.engine._plans


@pytest.mark.parametrize("variant", VARIANTS)
def test_reference_runs_at_odd_sizes(variant):
    """the configs and data of tests/golden/{kl,mmd}_objective_b19_t9.npz (the reference's own run): its disc"""
    gold = np.load(os.path.join(cases.GOLDEN, "%s_objective_b19_t9.npz" % variant))
    B, T = [int(v) for v in gold["meta"]]
    assert (B, T) == (19, 9)
    cfgs = _odd_cfgs()
    cfg = cfgs[0]
    model, w = _model(cfgs, variant)
    xn, yn = synth.make_batch(cfg["input_dims"], B, T, seed=7, output_dim=cfg["output_dim"])
    x, y = torch.from_numpy(xn).cuda(), torch.from_numpy(yn).cuda()
    y_ref, _ = _oracle(variant, cfgs, w, xn, yn)
    ref = (y_ref, float(gold["disc"]))
    cases.report("predict_mfn_reference_" + variant, _check("predict_mfn reference " + variant, *_run(model.engine, x, y), ref))
    _check("predict_mfn reference chunks " + variant, *_run(model.engine, x, y, cap=4), ref)
    assert model.engine._predict_mfn_bufs and not model.engine._plans


# ----------------------------------------------------------------------------------- 3. odd sizes, edges, chunks, determinism
@pytest.mark.parametrize("variant", VARIANTS)
def test_odd_sizes_edges_chunks_and_determinism(variant):
    """N = 19, T = 9; T = 1 (the window's c_{t-1} is zero at step 0); N = 1.  max_rows 1, 5 (a last chunk of 4) and N: y_hat
    bit-identical across the chunkings (one tile-row form: asserted), the loss within tolerance; two calls of one chunking
    bit-identical in both"""
    cfgs = _odd_cfgs()
    cfg = cfgs[0]
    model, w = _model(cfgs, variant)
    e, L = model.engine, _lib.lib()
    for T, N, caps in ((9, 19, (None, 1, 5, 19)), (1, 19, (None, 5)), (1, 1, (None,)), (9, 1, (None,))):
        xn, yn = synth.make_batch(cfg["input_dims"], N, T, seed=3 + T, output_dim=cfg["output_dim"])
        x, y = torch.from_numpy(xn).cuda(), torch.from_numpy(yn).cuda()
        ref = _oracle(variant, cfgs, w, xn, yn, double=True)
        first = None
        assert len({L.mfm_predict_mfn_tile_rows(N, cap or e.PREDICT_MAX_ROWS) for cap in caps}) == 1
        for cap in caps:
            a, b = _run(e, x, y, cap), _run(e, x, y, cap)
            assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), (T, N, cap)
            _check("predict_mfn odd %s T%d N%d cap %s" % (variant, T, N, cap), a[0], a[1], ref)
            if first is None:
                first = a
            assert torch.equal(a[0], first[0]), (T, N, cap)
            assert abs(float(_f(a[1])) - float(_f(first[1]))) <= TOL * max(abs(float(_f(first[1]))), 1e-3)
        # without labels: the same y_hat, no loss
        yb, lb = _run(e, x, None)
        assert lb is None and torch.equal(yb, first[0])
    assert not e._plans


@pytest.mark.parametrize("variant", VARIANTS)
def test_cross_entropy_with_three_classes(variant):
    cfgs = _odd_cfgs(loss="ce", output_dim=3)
    cfg = cfgs[0]
    N, T = 19, 2
    xn, yn = synth.make_batch(cfg["input_dims"], N, T, seed=5, output_dim=3, classes=3)
    model, w = _model(cfgs, variant)
    x, y = torch.from_numpy(xn).cuda(), torch.from_numpy(yn).cuda()
    assert y.dtype == torch.int64
    ref = _oracle(variant, cfgs, w, xn, yn)
    _check("predict_mfn ce " + variant, *_run(model.engine, x, y), ref)
    _check("predict_mfn ce chunks " + variant, *_run(model.engine, x, y, cap=4), ref)
    loss = model.evaluate(x, y, label_only=True)
    assert abs(float(loss) - ref[1]) <= TOL * max(abs(ref[1]), 1e-3)
    assert model.engine._predict_mfn_bufs and not model.engine._plans


# ----------------------------------------------------------------------------------- 4. tile-row forms, attention forms
@pytest.mark.parametrize("variant", VARIANTS)
def test_both_tile_row_forms_of_the_recurrence_launch(variant):
    """N = 2 CUs + 1 rows, T = 2.  One chunk: four-row tiles (3 N >= 6 CUs) with a one-row last tile.  The same split at a row
    cap of 2 CUs - 1 (3 rows < 6 CUs): one-row tiles, a last chunk of two rows.  The forms are read from
    mfm_predict_mfn_tile_rows; they agree within tolerance and each is bit-identical from run to run"""
    s = _canon(variant)
    L = _lib.lib()
    cus = L.mfm_device_cus()
    N, T, small = 2 * cus + 1, 2, 2 * cus - 1
    assert L.mfm_predict_mfn_tile_rows(N, N) == 4 and L.mfm_predict_mfn_tile_rows(N, small) == 1
    assert N % 4 == 1
    xn, yn = synth.make_batch(s["cfg"]["input_dims"], N, T, seed=11, output_dim=s["cfg"]["output_dim"])
    x, y = torch.from_numpy(xn).cuda(), torch.from_numpy(yn).cuda()
    ref = _oracle(variant, s["cfgs"], s["w"], xn, yn)
    res = {}
    for cap in (N, small):
        a, b = _run(s["e"], x, y, cap), _run(s["e"], x, y, cap)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), cap
        _check("predict_mfn tile rows %s cap %d" % (variant, cap), a[0], a[1], ref)
        res[cap] = a
    _check("predict_mfn four-row against one-row tiles " + variant, res[N][0], res[N][1],
           (_f(res[small][0]), float(_f(res[small][1]))))


def test_four_row_tiles_on_odd_sizes_take_a_launch_per_lstm():
    cfgs = _odd_cfgs()
    cfg = cfgs[0]
    model, w = _model(cfgs, "mmd")
    N, T = 2 * _lib.lib().mfm_device_cus() + 1, 3
    assert _lib.lib().mfm_predict_mfn_tile_rows(N, N) == 4
    xn, yn = synth.make_batch(cfg["input_dims"], N, T, seed=13, output_dim=cfg["output_dim"])
    got = _run(model.engine, torch.from_numpy(xn).cuda(), torch.from_numpy(yn).cuda(), cap=N)
    _check("predict_mfn odd four-row tiles", got[0], got[1], _oracle("mmd", cfgs, w, xn, yn))


@pytest.mark.parametrize("variant", VARIANTS)
def test_32_pair_form_of_the_attention_chain(variant):
    """T * N pairs above 64 x CUs (16 pairs per workgroup would give every CU more than four workgroups): 32 per workgroup"""
    s = _canon(variant)
    cus = _lib.lib().mfm_device_cus()
    T = 20
    N = (64 * cus) // T + 5
    assert (T * N + 15) // 16 > 4 * cus and (T * 33 + 15) // 16 <= 4 * cus       # (the other tests take the 16-pair form)
    xn, yn = synth.make_batch(s["cfg"]["input_dims"], N, T, seed=17, output_dim=s["cfg"]["output_dim"])
    got = _run(s["e"], torch.from_numpy(xn).cuda(), torch.from_numpy(yn).cuda(), cap=N)
    _check("predict_mfn 32-pair attention " + variant, got[0], got[1], _oracle(variant, s["cfgs"], s["w"], xn, yn))


# ----------------------------------------------------------------------------------- 5. dead parameters
@pytest.mark.parametrize("variant", VARIANTS)
def test_parameters_off_the_label_path_are_not_read(variant):
    """every tensor the entry's offsets table does not list -- the encoders and their heads, the logvar heads, the modalities'
    z -> f MLPs, the decoders -- overwritten with NaN in the flat buffer: the same bits"""
    from factorized_amd import engine
    s = _canon(variant)
    model, _ = _model(s["cfgs"], variant)
    e = model.engine
    before = _run(e, s["x"], s["y"], cap=8)
    live = set(engine.MFMEngine._PREDICT_MFN_TENSORS)
    dead = [n for n in e.layout.offsets if n not in live]
    assert all(any(n.startswith(p) for n in dead) for p in ("encoder_l.", "encoder_a.", "encoder_v.", "decoder_l.", "decoder_a.",
                                                            "decoder_v.", "zl_to_fl_fc1.", "za_to_fa_fc2.", "zv_to_fv_fc1."))
    if variant == "kl":
        assert all(any(n.startswith(p) for n in dead) for p in ("last_to_zl_fc1.", "last_to_logvarzl_fc1.", "last_to_logvarzy_fc1."))
    views = e.param_views()
    with torch.no_grad():
        for n in dead:
            views[n].fill_(float("nan"))
    poisoned = int(torch.isnan(e.params).sum())
    assert poisoned == sum(views[n].numel() for n in dead) and poisoned > 0
    after = _run(e, s["x"], s["y"], cap=8)
    assert torch.equal(before[0], after[0]) and torch.equal(before[1], after[1])
    assert torch.equal(_run(e, s["x"], s["y"])[0], s["yb"])


# ----------------------------------------------------------------------------------- 6. containment, x off a 16-byte boundary
def _abi(e, x, y, cap, sizes=None, expect=0, with_loss=True):
    """mfm_predict_mfn through the C ABI on canary-framed workspace, y_hat and loss -> (bits of y_hat, bits of the loss word, the
    workspace) after checking that nothing outside them was touched; expect != 0: the return code, and nothing at all was touched"""
    from factorized_amd import engine
    T, N = x.shape[0], x.shape[1]
    od = e.cfg["output_dim"]
    L = _lib.lib()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    good = e._mfn_sizes()
    nws = int(L.mfm_predict_mfn_workspace_floats(T, N, good, cap))
    assert nws > 0 and nws == e.predict_workspace_floats(T, N, max_rows=cap or N, label_only=True)
    PAD = 256
    big_ws = torch.full((PAD + nws + PAD,), CANARY, dtype=torch.int32, device="cuda")
    big_y = torch.full((8 + N * od + 8,), CANARY, dtype=torch.int32, device="cuda")
    big_l = torch.full((4 + 1 + 4,), CANARY, dtype=torch.int32, device="cuda")
    ws, y_hat, loss = big_ws[PAD:PAD + nws].view(torch.float32), big_y[8:8 + N * od].view(torch.float32), big_l[4:5].view(torch.float32)
    names = engine.MFMEngine._PREDICT_MFN_TENSORS
    offs = (C.c_int64 * len(names))(*[e.layout.offsets[n] for n in names])
    rc = L.mfm_predict_mfn(T, N, sizes or good, _p(e.params), offs, _p(x), _p(y) if with_loss else None, _p(ws), _p(y_hat),
                           _p(loss) if with_loss else None, cap, stream)
    torch.cuda.synchronize()
    assert rc == expect, (rc, L.mfm_last_error())
    if expect != 0:
        assert bool((big_ws == CANARY).all()) and bool((big_y == CANARY).all()) and bool((big_l == CANARY).all())
        return None
    assert bool((big_ws[:PAD] == CANARY).all()) and bool((big_ws[PAD + nws:] == CANARY).all())
    assert bool((big_y[:8] == CANARY).all()) and bool((big_y[8 + N * od:] == CANARY).all())
    assert bool((big_l[:4] == CANARY).all()) and bool((big_l[5:] == CANARY).all())
    if not with_loss:
        assert int(big_l[4]) == CANARY                              # no labels: no loss is written
    else:
        assert int(big_ws[PAD + nws - 2]) == 0                      # the ticket word is back at 0
    return _bits(y_hat.view(N, od)), _bits(loss.view(())), big_ws


@pytest.mark.parametrize("variant,cap", [("kl", 0), ("kl", 7), ("mmd", 0), ("mmd", 7)])
def test_canaries_around_workspace_y_hat_and_loss(variant, cap):
    s = _canon(variant)
    want = (s["yb"], s["lb"]) if cap == 0 else _run(s["e"], s["x"], s["y"], cap)
    yb, lb, _ = _abi(s["e"], s["x"], s["y"], cap)
    assert torch.equal(yb, want[0]) and torch.equal(lb, want[1])
    yb, _, _ = _abi(s["e"], s["x"], None, cap, with_loss=False)
    assert torch.equal(yb, want[0])


@pytest.mark.parametrize("variant", VARIANTS)
def test_x_may_start_off_a_16_byte_boundary(variant):
    """4, 8 and 12 bytes off, a batch view of a dataset and a time crop x[k:]: the bits of an aligned copy"""
    s = _canon(variant)
    e, x, y = s["e"], s["x"], s["y"]
    OV.forget_views()
    for r in (4, 8, 12):
        xv = OV.at_residue(x, r)
        assert torch.equal(_abi(e, xv, y, 0)[0], s["yb"])
        got = _run(e, xv, y)
        assert torch.equal(got[0], s["yb"]) and torch.equal(got[1], s["lb"])
        got7, want7 = _run(e, xv, y, 7), _run(e, x, y, 7)
        assert torch.equal(got7[0], want7[0]) and torch.equal(got7[1], want7[1])
    T, N, D = x.shape
    ds = torch.randn(3, T, N, D, device="cuda")
    ds[1].copy_(x)
    assert ds[1].is_contiguous() and ds[1].data_ptr() % 16 != 0
    got = _run(e, ds[1], y)
    assert torch.equal(got[0], s["yb"]) and torch.equal(got[1], s["lb"])
    long = torch.randn(T + 1, N, D, device="cuda")
    long[1:].copy_(x)
    assert long[1:].is_contiguous() and long[1:].data_ptr() % 16 != 0
    got = _run(e, long[1:], y)
    assert torch.equal(got[0], s["yb"]) and torch.equal(got[1], s["lb"])
    assert OV.check_guards() == 3


# ----------------------------------------------------------------------------------- 7. data that is not unit noise
def _row_err(got, ref):
    """max over rows of max|got - ref| over the row's own max|ref| (floored at 1e-3), as tests/test_gpu_data_regimes.py"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float((np.abs(got - ref).max(axis=1) / np.maximum(np.abs(ref).max(axis=1), 1e-3)).max())


@pytest.mark.parametrize("regime", DR.REGIMES)
@pytest.mark.parametrize("variant", VARIANTS)
def test_data_regimes_against_the_float64_oracle(variant, regime):
    """the six regimes of tests/data_regimes.py (zero biases with vanishing inputs are left out there);
    outlier is judged row by row as well"""
    cfgs = DR.canonical()
    model, w = _model(cfgs, variant)
    xn, yn = DR.make(regime, 19, 5)
    ref = _oracle(variant, cfgs, w, xn, yn, double=True)
    yb, lb = _run(model.engine, torch.from_numpy(xn).cuda(), torch.from_numpy(yn).cuda())
    assert model.engine._predict_mfn_bufs and not model.engine._plans
    cases.report("predict_mfn_%s_%s" % (regime, variant), _check("predict_mfn %s %s" % (regime, variant), yb, lb, ref))
    if regime == "outlier":
        re = _row_err(_f(yb), ref[0])
        print("predict_mfn outlier %s worst row %.2e" % (variant, re))
        assert re <= TOL, re


# ----------------------------------------------------------------------------------- 8. refusals
def test_a_refusal_at_resident_sizes_falls_back_and_is_not_remembered(monkeypatch):
    s = _canon("kl")
    model, _ = _model(s["cfgs"], "kl")
    e, L, log = model.engine, _lib.lib(), []
    real = L.mfm_predict_mfn

    def fn(*a):
        log.append(1)
        return _lib.MFM_ERR_UNSUPPORTED if len(log) <= 1 else real(*a)
    monkeypatch.setattr(L, "mfm_predict_mfn", fn, raising=True)
    out = e.predict(s["x"], s["y"], label_only=True)
    assert log == [1] and len(e._plans) == 1                         # the entry was asked, the plan's forward answered
    _check("predict_mfn refused once", _bits(out["y_hat"]), _bits(out["loss"]), s["ref"])
    assert e._predict_mfn_refused is False and not e.__dict__.get("_predict_mfn_bufs")
    again = _run(e, s["x"], s["y"])
    assert log == [1, 1] and len(e._predict_mfn_bufs) == 1
    assert torch.equal(again[0], s["yb"]) and torch.equal(again[1], s["lb"])


def test_windowsize_3_is_refused_and_nothing_is_enqueued():
    s = _canon("kl")
    sizes = s["e"]._mfn_sizes()
    sizes[11] = 3
    _abi(s["e"], s["x"], s["y"], 0, sizes=sizes, expect=_lib.MFM_ERR_UNSUPPORTED)
    assert "windowsize 3" in _lib.lib().mfm_last_error().decode()


def test_wide_h_dims_are_refused_and_remembered(monkeypatch):
    """an h_dims entry of 136 through the real entry: refused with the size in the reason, nothing enqueued, remembered, the
    entry not asked again.  The fallback is the unchanged default path, the eval forward on a fused plan, and the fused plan has
    no MFN LSTM above 128 (mfm_plan_create says so, as it does for the default predict of this configuration): the answer is
    that error on both paths, pinned here side by side."""
    cfgs = _odd_cfgs(h_dims=[9, 136, 7])
    cfg = cfgs[0]
    model, w = _model(cfgs, "kl")
    e = model.engine
    T, N = 3, 5
    xn, yn = synth.make_batch(cfg["input_dims"], N, T, seed=21, output_dim=cfg["output_dim"])
    x, y = torch.from_numpy(xn).cuda(), torch.from_numpy(yn).cuda()
    _abi(e, x, y, 0, expect=_lib.MFM_ERR_UNSUPPORTED)
    assert "136" in _lib.lib().mfm_last_error().decode()
    L, calls = _lib.lib(), []
    real = L.mfm_predict_mfn
    monkeypatch.setattr(L, "mfm_predict_mfn", lambda *a: (calls.append(1), real(*a))[1], raising=True)
    with pytest.raises(_lib.MfmError, match="MFN LSTM sizes above 128"):
        model.evaluate(x, y)                                         # the default path of this configuration
    assert calls == []
    for _ in range(2):
        with pytest.raises(_lib.MfmError, match="MFN LSTM sizes above 128"):
            model.evaluate(x, y, label_only=True)
        assert calls == [1] and e._predict_mfn_refused is True and not e.__dict__.get("_predict_mfn_bufs")


def test_wide_tail_layers_keep_the_entry(monkeypatch):
    """fy, zy and output_dim do not bound the recurrences: zy = 136 stays on the entry, and its numbers are right"""
    cfgs = _odd_cfgs(zy_size=136)
    cfg = cfgs[0]
    model, w = _model(cfgs, "mmd")
    T, N = 3, 5
    xn, yn = synth.make_batch(cfg["input_dims"], N, T, seed=21, output_dim=cfg["output_dim"])
    got = _run(model.engine, torch.from_numpy(xn).cuda(), torch.from_numpy(yn).cuda())
    _check("predict_mfn zy 136", got[0], got[1], _oracle("mmd", cfgs, w, xn, yn))
    assert model.engine._predict_mfn_bufs and not model.engine._plans


# ----------------------------------------------------------------------------------- 9. capture, allocation
@pytest.mark.parametrize("variant", VARIANTS)
def test_epoch_tail_in_one_captured_graph(variant):
    """evaluate(label_only=True) -> ReduceLROnPlateau.step -> KeepBest.update in one graph; two replays with different contents
    copied into x give the eager call's bits each time, and the arrival ticket is back at 0 between them"""
    import factorized_amd.optim as optim
    from factorized_amd.checkpoint import KeepBest
    from factorized_amd.lr_scheduler import ReduceLROnPlateau
    s = _canon(variant)
    model, _ = _model(s["cfgs"], variant)
    e = model.engine
    x, y = s["x"].clone(), s["y"].clone()
    x2n, _ = synth.make_batch(s["cfg"]["input_dims"], s["N"], s["T"], seed=77, output_dim=s["cfg"]["output_dim"])
    x2 = torch.from_numpy(x2n).cuda()
    lr = torch.tensor([1e-3], device="cuda")
    optimizer = optim.Adam(model.parameters(), lr=lr, capturable=True)
    scheduler = ReduceLROnPlateau(optimizer, "min", patience=0)
    best = KeepBest(model)
    loss = model.evaluate(x, y, label_only=True)             # warm-up: buffers, code objects, the consumers' state blocks
    scheduler.step(loss)
    best.update(loss)
    torch.cuda.synchronize()
    want1 = _bits(loss)
    assert torch.equal(want1, s["lb"])
    want2 = _bits(model.evaluate(x2, y, label_only=True))
    assert not torch.equal(want1, want2)
    epoch0, calls0 = scheduler.last_epoch, best.calls
    ws = e._predict_mfn_bufs[(s["T"], s["N"], e.PREDICT_MAX_ROWS)][0]
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        gloss = model.evaluate(x, y, label_only=True)
        scheduler.step(gloss)
        best.update(gloss)
    for src, want in ((x2, want2), (s["x"], want1)):
        x.copy_(src)
        gloss.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(_bits(gloss), want)
        assert int(ws.view(torch.int32)[-2]) == 0            # the ticket word
    assert scheduler.last_epoch == epoch0 + 2 and best.calls == calls0 + 2
    assert not e._plans


@pytest.mark.parametrize("variant", VARIANTS)
def test_no_allocation_and_no_synchronisation_after_the_first_call(variant):
    s = _canon(variant)
    model, x, y = s["model"], s["x"], s["y"]
    for _ in range(2):
        model.evaluate(x, y, label_only=True)
        model.predict(x, label_only=True)
    torch.cuda.synchronize()
    allocated = torch.cuda.memory_allocated()
    count = torch.cuda.memory_stats()["allocation.all.allocated"]
    torch.cuda.set_sync_debug_mode("error")
    try:
        for _ in range(5):
            model.evaluate(x, y, label_only=True)
            model.predict(x, label_only=True)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.cuda.memory_allocated() == allocated
    assert torch.cuda.memory_stats()["allocation.all.allocated"] == count


# ----------------------------------------------------------------------------------- 10. the unchanged default
@pytest.mark.parametrize("name", ["kl_b32_t20", "mmd_b32_t20"])
def test_default_is_still_the_eval_forward_bit_for_bit(name):
    cs = cases.load_case(name)
    variant = cs["variant"]
    model, _ = _model(cs["cfgs"], variant)
    x, y = torch.from_numpy(cs["x"]).cuda(), torch.from_numpy(cs["y"]).cuda()
    if variant == "mmd":
        cfg = cs["cfg"]
        g = torch.from_numpy(np.ascontiguousarray(cs["gold"]["mmd_gauss"]))
        model.mmd_gauss = [t.cuda() for t in torch.split(g, [cfg["zl_size"], cfg["za_size"], cfg["zv_size"], cfg["zy_size"]], dim=1)]
    model.eval()
    with torch.no_grad():
        ref = model(x)[0][3].clone()
    assert torch.equal(_bits(model.predict(x)), _bits(ref))
    assert torch.equal(_bits(model.predict(x, label_only=False)), _bits(ref))
    assert model.engine._plans and not model.engine.__dict__.get("_predict_mfn_bufs")
    lo = model.predict(x, label_only=True).clone()
    assert rel_err(lo.cpu().numpy(), ref.cpu().numpy()) <= TOL
    assert torch.equal(_bits(model.predict(x)), _bits(ref))          # (and the default again, behind the label-only call)
    # any other loss function is applied to the label-only y_hat
    mse = model.evaluate(x, y.view_as(lo), torch.nn.MSELoss(), label_only=True)
    assert torch.equal(_bits(mse), _bits(torch.nn.MSELoss()(model.predict(x, label_only=True), y.view_as(lo))))


def test_label_only_changes_nothing_for_mfm_kl_ef():
    cs = cases.load_case("klef_b33_t7")
    model, _ = _model(cs["cfgs"], "kl_ef")
    x, y = torch.from_numpy(cs["x"]).cuda(), torch.from_numpy(cs["y"]).cuda()
    want_y, want_l = _bits(model.predict(x)), _bits(model.evaluate(x, y))
    assert torch.equal(_bits(model.predict(x, label_only=True)), want_y)
    assert torch.equal(_bits(model.evaluate(x, y, label_only=True)), want_l)
    e = model.engine
    assert len(e._predict_bufs) == 1 and not e.__dict__.get("_predict_mfn_bufs") and not e._plans
    assert e.predict_workspace_floats(7, 33, label_only=True) == e.predict_workspace_floats(7, 33)


def test_bad_arguments_do_not_reach_the_library(monkeypatch):
    s = _canon("mmd")
    model, e, x, y = s["model"], s["e"], s["x"], s["y"]
    N = x.shape[1]
    L, calls = _lib.lib(), []
    real = L.mfm_predict_mfn
    monkeypatch.setattr(L, "mfm_predict_mfn", lambda *a: (calls.append(1), real(*a))[1], raising=True)
    bad = [
        lambda: model.evaluate(x.cpu(), y, label_only=True),
        lambda: model.evaluate(x, y.cpu(), label_only=True),
        lambda: model.predict(x[:, :, :-1], label_only=True),
        lambda: model.evaluate(x, y[:-1].contiguous(), label_only=True),
        lambda: model.evaluate(x, torch.cat([y.view(N, -1)] * 2, dim=1).contiguous(), label_only=True),
        lambda: model.predict(x[:, :0].contiguous(), label_only=True),
        lambda: e.predict(x, y, max_rows=0, label_only=True),
    ]
    for i, call in enumerate(bad):
        with pytest.raises(_lib.MfmError):
            call()
            pytest.fail("call %d was accepted" % i)
    assert not calls and not e._plans
