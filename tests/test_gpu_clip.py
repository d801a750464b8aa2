"""factorized_amd.nn_utils on the MI355X: the clip kernels through the C ABI against numpy / torch on raw buffers (spans that end
anywhere, poisoned padding, non-finite values, the guard word, capture), and the reference's unchanged loop with the usual line

    loss.backward(); clip_grad_norm_(model.parameters(), MAX_NORM); optimizer.step()

against the reference's own clipped trajectory (klef_clip_b32_t20, tests/golden/make_golden_clip.py) and against torch's
function on twins: the flat path, the tensors it skips, the fallbacks, no synchronisation, the guard."""
import ctypes as C
import math

import numpy as np
import pytest
import torch
import torch.nn as nn

import factorized_amd.optim as optim
from factorized_amd import _lib, configs, nn_utils, synth
from tests import cases
from tests.test_gpu_sgd import _assert_flat, _model, _param_err, _summaries, _trace_err

pytestmark = pytest.mark.gpu
TOL = 1e-4                      # the project's fp32 contract (model level)
# total_norm against a float64 norm: fp32 unit round-off 6e-8, a reduction tree over at most 2^20 terms is about 20 roundings
# deep (1.2e-6), margin about 8x
NORM_TOL = 1e-5
KINDS = {"l2": (_lib.MFM_NORM_L2, 2.0), "inf": (_lib.MFM_NORM_INF, math.inf), "l1": (_lib.MFM_NORM_L1, 1.0)}
NAN = float("nan")


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


# ----------------------------------------------------------------------------------- the kernels through the C ABI
# 20 spans: 1, 3 and 4 elements, around the 1024-element tile, several tiles, ends that are no multiple of 4
LENGTHS = [1, 3, 4, 1023, 1024, 1025, 2, 5, 7, 63, 64, 65, 255, 257, 1000, 2047, 2049, 4097, 6, 130]


def _layout():
    """[(begin, end)], total: begins are multiples of 4; the gap behind a span is 0 (the next span starts in the float4 right
    behind this one's last -- after a length that is a multiple of 4: at its very end), 4, 60 or 8 elements"""
    spans, cur = [], 64
    for k, n in enumerate(LENGTHS):
        spans.append((cur, cur + n))
        cur = (cur + n + 3) // 4 * 4 + (0, 4, 60, 8)[k % 4]
    return spans, cur + 64


def _poisoned(spans, total, seed, scale=1.0):
    """fp32 [total]: N(0, scale) inside the spans, NaN and 1e30 alternating everywhere else; and the mask of the inside"""
    gen = torch.Generator().manual_seed(seed)
    g = torch.randn(total, generator=gen) * scale
    inside = torch.zeros(total, dtype=torch.bool)
    for a, e in spans:
        inside[a:e] = True
    out = (~inside).nonzero().flatten()
    g[out[0::2]] = NAN
    g[out[1::2]] = 1e30
    return g, inside


def _table(spans):
    arr = (_lib.ClipSpan * len(spans))()
    for j, (a, e) in enumerate(spans):
        arr[j].begin, arr[j].end = a, e
    return arr


def _ptr(t):
    return C.c_void_p(t.data_ptr() if t is not None else None)


def _ws():
    return torch.empty(int(_lib.lib().mfm_clip_workspace_floats()), dtype=torch.float32, device="cuda")


def _clip_norm(g, spans, kind, max_norm, guard=None, ws=None, total=None):
    ws = _ws() if ws is None else ws
    total = torch.zeros((), device="cuda") if total is None else total
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(_lib.lib().mfm_clip_grad_norm_flat_spans(_ptr(g), _table(spans), len(spans), kind, max_norm, _ptr(ws), _ptr(total),
                                                        _ptr(guard), stream), "mfm_clip_grad_norm_flat_spans")
    return total


def _clip_value(g, spans, c, guard=None):
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(_lib.lib().mfm_clip_grad_value_flat_spans(_ptr(g), _table(spans), len(spans), c, _ptr(guard), stream),
               "mfm_clip_grad_value_flat_spans")


def _true_norm(g0, inside, name):
    v = np.abs(g0[inside].numpy().astype(np.float64))
    return {"l2": math.sqrt(float((v * v).sum())), "inf": float(v.max()), "l1": float(v.sum())}[name]


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _f32(x):
    return float(np.float32(x))


def _torch_clip(g0, spans, max_norm, norm_type):
    """torch.nn.utils.clip_grad_norm_ on CPU, one parameter per span -> (total_norm, [gradient of each span])"""
    ps = []
    for a, e in spans:
        p = nn.Parameter(torch.zeros(e - a))
        p.grad = g0[a:e].clone()
        ps.append(p)
    total = torch.nn.utils.clip_grad_norm_(ps, max_norm, norm_type)
    return total, [p.grad for p in ps]


def _check_scaled(gc, g0, inside, total, max_norm, scale):
    """the buffer after a norm clip: inside the spans g0 * coef with coef from the kernel's own norm through torch's formula in
    fp32; outside, every bit as it was (NaN padding included)"""
    coef = torch.clamp(_f32(max_norm) / (total.cpu() + 1e-6), max=1.0)
    assert coef.dtype == torch.float32
    torch.testing.assert_close(gc[inside], g0[inside] * coef, rtol=1e-6, atol=0)
    if scale > 1.0:
        assert float(coef) == 1.0 and torch.equal(_bits(gc)[inside], _bits(g0)[inside])
    else:
        assert float(coef) < 1.0
    assert torch.equal(_bits(gc)[~inside], _bits(g0)[~inside])


@pytest.mark.parametrize("scale", [0.5, 2.0])
@pytest.mark.parametrize("name", list(KINDS))
def test_norm_and_scaled_values_over_spans_with_poisoned_padding(name, scale):
    _need_gpu()
    spans, total_len = _layout()
    assert len(spans) == 20 and all(a % 4 == 0 for a, _ in spans) and any(e % 4 for _, e in spans)
    g0, inside = _poisoned(spans, total_len, seed=10)
    true = _true_norm(g0, inside, name)
    max_norm = scale * true
    g = g0.cuda()
    total = _clip_norm(g, spans, KINDS[name][0], max_norm)
    torch.cuda.synchronize()
    err = abs(float(total) - true) / true
    cases.report("clip_kernel_norm_rel_%s" % name, err)
    print("clip_kernel_norm_rel_%s %.3e" % (name, err))
    assert err < NORM_TOL, (float(total), true)
    if name == "inf":
        assert float(total) == true                  # a maximum of fp32 values: exact
    _check_scaled(g.cpu(), g0, inside, total, max_norm, scale)


def test_two_runs_give_the_same_bits():
    _need_gpu()
    spans, total_len = _layout()
    g0, _ = _poisoned(spans, total_len, seed=11)
    runs = []
    for _ in range(2):
        g = g0.cuda()
        total = _clip_norm(g, spans, _lib.MFM_NORM_L2, 1.0)
        torch.cuda.synchronize()
        runs.append((_bits(total.reshape(1)), _bits(g)))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    assert not torch.equal(runs[0][1], _bits(g0))                 # (and it did clip)


def test_non_finite_gradients_behave_like_torch():
    _need_gpu()
    spans, total_len = _layout()
    g0, inside = _poisoned(spans, total_len, seed=12)
    at = spans[5][0] + 1001                                       # in the second tile of the 1025-element span
    # one inf under L2: the norm is inf, the coefficient 0; finite elements become 0 and inf * 0 is NaN
    gi = g0.clone()
    gi[at] = float("inf")
    g = gi.cuda()
    total = _clip_norm(g, spans, _lib.MFM_NORM_L2, 1.0)
    gc = g.cpu()
    assert math.isinf(float(total)) and float(total) > 0
    assert math.isnan(float(gc[at]))
    rest = inside.clone()
    rest[at] = False
    assert bool((gc[rest] == 0).all())
    rt, rg = _torch_clip(gi, spans, 1.0, 2.0)
    assert math.isinf(float(rt))
    for (a, e), r in zip(spans, rg):
        torch.testing.assert_close(gc[a:e], r, rtol=0, atol=0, equal_nan=True)
    assert torch.equal(_bits(gc)[~inside], _bits(gi)[~inside])
    # one NaN under each kind: the norm is NaN (the maximum too) and so is every element of every span
    gn = g0.clone()
    gn[at] = NAN
    for name, (kind, norm_type) in KINDS.items():
        g = gn.cuda()
        total = _clip_norm(g, spans, kind, 1.0)
        gc = g.cpu()
        assert math.isnan(float(total)), name
        assert bool(torch.isnan(gc[inside]).all()), name
        rt, rg = _torch_clip(gn, spans, 1.0, norm_type)
        assert math.isnan(float(rt)) and all(bool(torch.isnan(r).all()) for r in rg)
        assert torch.equal(_bits(gc)[~inside], _bits(gn)[~inside])


def test_guard_word_leaves_the_gradients_alone_and_reports_nan():
    _need_gpu()
    spans, total_len = _layout()
    g0, inside = _poisoned(spans, total_len, seed=13)
    true = _true_norm(g0, inside, "l2")
    g = g0.cuda()
    guard = torch.full((1,), NAN, device="cuda")
    for word in (NAN, 1.0):
        guard.fill_(word)
        total = _clip_norm(g, spans, _lib.MFM_NORM_L2, 0.5 * true, guard=guard)
        assert math.isnan(float(total)), word
        assert torch.equal(_bits(g), _bits(g0)), word
        _clip_value(g, spans, 0.5, guard=guard)
        assert torch.equal(_bits(g), _bits(g0)), word
    guard.zero_()
    total = _clip_norm(g, spans, _lib.MFM_NORM_L2, 0.5 * true, guard=guard)
    torch.cuda.synchronize()
    assert abs(float(total) - true) / true < NORM_TOL
    _check_scaled(g.cpu(), g0, inside, total, 0.5 * true, 0.5)


def test_value_clip_matches_torch_clamp():
    _need_gpu()
    spans, total_len = _layout()
    g0, inside = _poisoned(spans, total_len, seed=14)
    g0[spans[3][0] + 5] = NAN                                     # a NaN inside a span stays a NaN
    g0[spans[17][1] - 1] = float("inf")
    g0[spans[0][0]] = -float("inf")
    c = 0.5
    g = g0.cuda()
    guard = torch.zeros(1, device="cuda")
    _clip_value(g, spans, c, guard=guard)
    gc = g.cpu()
    want = torch.clamp(g0, min=-c, max=c)
    torch.testing.assert_close(gc[inside], want[inside], rtol=0, atol=0, equal_nan=True)
    assert int(torch.isnan(gc[inside]).sum()) == 1
    assert int((gc[inside].abs() == c).sum()) > 100
    assert torch.equal(_bits(gc)[~inside], _bits(g0)[~inside])
    g = g0.cuda()
    _clip_value(g, spans, c)                                      # unguarded form
    assert torch.equal(_bits(g), _bits(gc))


def test_every_tensor_of_mfm_kl_as_its_own_span():
    """the largest fused model (MFM_KL, 104 tensors): their exact extents as 104 spans, the padding between them poisoned"""
    _need_gpu()
    from factorized_amd import mfm_model as M
    model = M.MFM_KL(*configs.canonical_configs(dropout=False)).cuda()
    lay = model.engine.layout
    spans = sorted((o, o + n) for o, n, _ in lay.slots)
    assert len(spans) == 104 and all(e <= lay.guard for _, e in spans)
    g0, inside = _poisoned(spans, lay.total, seed=15)
    assert int((~inside).sum()) > 104                             # (there is padding to keep)
    true = _true_norm(g0, inside, "l2")
    g = g0.cuda()
    total = _clip_norm(g, spans, _lib.MFM_NORM_L2, 0.5 * true)
    gc = g.cpu()
    rt, rg = _torch_clip(g0, spans, 0.5 * true, 2.0)
    assert abs(float(total) - true) / true < NORM_TOL and abs(float(rt) - true) / true < NORM_TOL
    # torch's coefficient comes from torch's own fp32 norm: the two norms are each within NORM_TOL of the exact one, so the
    # coefficients differ by at most 2 * NORM_TOL, plus one rounding of the product on either side
    for (a, e), r in zip(spans, rg):
        torch.testing.assert_close(gc[a:e], r, rtol=2 * NORM_TOL + 2e-7, atol=0)
    assert torch.equal(_bits(gc)[~inside], _bits(g0)[~inside])
    g = g0.cuda()
    _clip_value(g, spans, 0.25)
    gc = g.cpu()
    assert torch.equal(gc[inside], torch.clamp(g0[inside], -0.25, 0.25))
    assert torch.equal(_bits(gc)[~inside], _bits(g0)[~inside])


def test_both_entry_points_replay_from_a_captured_graph():
    _need_gpu()
    spans, total_len = _layout()
    base, inside = _poisoned(spans, total_len, seed=16)
    max_norm = _true_norm(base, inside, "l2")
    c = 0.75
    gn, gv = base.cuda(), base.cuda()                             # static buffers: norm clip on one, value clip on the other
    ws, total = _ws(), torch.zeros((), device="cuda")
    _clip_norm(gn, spans, _lib.MFM_NORM_L2, max_norm, ws=ws, total=total)         # (code objects loaded before the capture)
    _clip_value(gv, spans, c)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _clip_norm(gn, spans, _lib.MFM_NORM_L2, max_norm, ws=ws, total=total)
        _clip_value(gv, spans, c)
    for k, scale in enumerate((3.0, 0.2, 1.5)):                   # above, below and above the threshold again
        new = base.clone()
        new[inside] = base[inside] * scale + 0.01 * k
        gn.copy_(new)
        gv.copy_(new)
        graph.replay()
        torch.cuda.synchronize()
        rt, rg = _torch_clip(new, spans, max_norm, 2.0)
        assert (float(rt) > max_norm) == (scale > 1.0)
        assert abs(float(total) - float(rt)) / float(rt) < 2 * NORM_TOL, (k, float(total), float(rt))
        gc = gn.cpu()
        for (a, e), r in zip(spans, rg):
            torch.testing.assert_close(gc[a:e], r, rtol=2 * NORM_TOL + 2e-7, atol=0)
        if scale < 1.0:
            assert torch.equal(_bits(gc), _bits(new))
        assert torch.equal(_bits(gc)[~inside], _bits(new)[~inside])
        vc = gv.cpu()
        assert torch.equal(vc[inside], torch.clamp(new[inside], -c, c))
        assert torch.equal(_bits(vc)[~inside], _bits(new)[~inside])


# ----------------------------------------------------------------------------------- the reference loop
def _clip_loop(model, optimizer, X, y, config, steps, clip, stage_of=None, before_clip=None):
    """tests/test_gpu_sgd.py's _reference_loop (mfm_mosi.py:424-442, :278-281) with the one clipping line added; returns the
    trace and what `clip(model.parameters())` returned in every step"""
    criterion = nn.L1Loss()
    gen_criterion = nn.MSELoss()
    d_l, d_a, d_v = config["input_dims"]
    model.train()
    trace, norms = [], []
    for step in range(steps):
        optimizer.zero_grad()
        batch_X = X
        batch_y = y
        decoded, mmd_loss, missing_loss = model.forward(batch_X)
        [x_l_hat, x_a_hat, x_v_hat, y_hat] = decoded
        batch_X_l = batch_X[:, :, :d_l]
        batch_X_a = batch_X[:, :, d_l:d_l + d_a]
        batch_X_v = batch_X[:, :, d_l + d_a:]
        gen_loss = config["lda_xl"] * gen_criterion(x_l_hat, batch_X_l) + config["lda_xa"] * gen_criterion(x_a_hat, batch_X_a) \
            + config["lda_xv"] * gen_criterion(x_v_hat, batch_X_v)
        disc_loss = criterion(y_hat.squeeze(1), batch_y)
        stage = stage_of(step) if stage_of else 0
        if stage == 1:
            loss = gen_loss + config["lda_mmd"] * mmd_loss
        elif stage == 2:
            loss = disc_loss + config["lda_mmd"] * mmd_loss
        else:
            loss = disc_loss + gen_loss + config["lda_mmd"] * mmd_loss + missing_loss
        loss.backward()
        if before_clip is not None:
            before_clip(step)
        norms.append(clip(model.parameters()))
        optimizer.step()
        trace.append([loss.item(), disc_loss.item(), gen_loss.item(), mmd_loss.item()])
    return np.array(trace), np.array([float(n) for n in norms])


def _clip_case():
    cs = cases.load_case("klef_b32_t20")
    gold = np.load(cases.GOLDEN + "/klef_clip_b32_t20.npz")
    return cs, gold, float(gold["meta"][5])


def _norm_err(norms, ref):
    return float(np.max(np.abs(norms - ref) / np.abs(ref)))


def _sgd_model(cs):
    cfg = cs["cfg"]
    model = _model(cs["cfgs"])
    optimizer = optim.SGD(model.parameters(), lr=cfg["lr"], momentum=cfg["momentum"])     # :404, before .to(device)
    model = model.to("cuda")
    return model, optimizer, torch.from_numpy(cs["x"]).cuda(), torch.from_numpy(cs["y"]).cuda()


def _flat_only(monkeypatch):
    """torch's functions raise: whatever runs under this took the flat path"""
    def refuse(*a, **k):
        raise AssertionError("torch.nn.utils clipping was called: not the flat path")
    monkeypatch.setattr(torch.nn.utils, "clip_grad_norm_", refuse)
    monkeypatch.setattr(torch.nn.utils, "clip_grad_value_", refuse)


def test_unchanged_reference_loop_with_clipping_follows_reference_trajectory(monkeypatch):
    _need_gpu()
    cs, gold, max_norm = _clip_case()
    cfg = cs["cfg"]
    assert (cfg["lr"], cfg["momentum"]) == (0.01, 0.9)
    steps = int(gold["meta"][2])
    model, optimizer, X, y = _sgd_model(cs)
    _flat_only(monkeypatch)
    clip = lambda params: nn_utils.clip_grad_norm_(params, max_norm)
    first, n1 = _clip_loop(model, optimizer, X, y, cfg, 1, clip)
    perr1 = _param_err(_summaries(model), gold["param_after1"])
    cases.report("clip_param_rel_step1", perr1)
    print("clip_param_rel_step1 %.3e" % perr1)
    assert perr1 < TOL, perr1
    rest, n2 = _clip_loop(model, optimizer, X, y, cfg, steps - 1, clip)
    trace, norms = np.concatenate([first, rest]), np.concatenate([n1, n2])
    terr = _trace_err(trace, gold["trace"])
    nerr = _norm_err(norms, gold["total_norm"])
    perr = _param_err(_summaries(model), gold["param_after_last"])
    for key, val in (("clip_trace_rel", terr), ("clip_norm_rel", nerr), ("clip_param_rel", perr)):
        cases.report(key, val)
        print("%s %.3e" % (key, val))
    assert terr < TOL, (trace[:, 0], gold["trace"][:, 0])
    assert nerr < TOL, (norms, gold["total_norm"])
    assert perr < TOL, perr
    # both branches of the coefficient were taken, here as in the fixture
    for n in (norms, gold["total_norm"]):
        assert (n > max_norm).any() and (n < max_norm).any()
    _assert_flat(model, optimizer)


def test_staged_loop_leaves_tensors_without_gradient_out_of_norm_and_update(monkeypatch):
    """train_beta_vae's stage losses: a tensor the stage loss does not reach is in no norm and does not move"""
    _need_gpu()
    cs, gold, max_norm = _clip_case()
    cfg = cs["cfg"]
    n1, n2 = int(gold["meta"][3]), int(gold["meta"][4])
    model, optimizer, X, y = _sgd_model(cs)
    _flat_only(monkeypatch)
    clip = lambda params: nn_utils.clip_grad_norm_(params, max_norm)
    named = dict(model.named_parameters())
    disc = [n for n in named if n.startswith("fy_to_y_")]
    dec = [n for n in named if n.startswith(("decoder_", "zl_to_fl_", "za_to_fa_", "zv_to_fv_"))]
    assert disc and dec
    snap = lambda names: {n: named[n].detach().clone() for n in names}
    before = snap(disc)
    t1, na = _clip_loop(model, optimizer, X, y, cfg, n1, clip, stage_of=lambda s: 1)
    for n in disc:                                                # gen + reg never reaches the classifier
        assert torch.equal(named[n].detach(), before[n]), n
    perr1 = _param_err(_summaries(model), gold["staged_param_after_stage1"])
    assert perr1 < TOL, perr1
    before = snap(dec)
    present = []
    t2, nb = _clip_loop(model, optimizer, X, y, cfg, n2, clip, stage_of=lambda s: 2,
                        before_clip=lambda s: present.append(model._grad_present.copy()))
    for n in dec:                                                 # disc + reg never reaches the decoders (momentum included)
        assert torch.equal(named[n].detach(), before[n]), n
    assert not present[-1].all() and present[-1].any()
    trace, norms = np.concatenate([t1, t2]), np.concatenate([na, nb])
    terr = _trace_err(trace, gold["staged_trace"])
    nerr = _norm_err(norms, gold["staged_total_norm"])
    perr = _param_err(_summaries(model), gold["staged_param_after_stage2"])
    for key, val in (("clip_staged_trace_rel", terr), ("clip_staged_norm_rel", nerr), ("clip_staged_param_rel", perr)):
        cases.report(key, val)
        print("%s %.3e" % (key, val))
    assert terr < TOL, (trace[:, 0], gold["staged_trace"][:, 0])
    assert nerr < TOL, (norms, gold["staged_total_norm"])
    assert perr < TOL, perr
    # the last norm is the norm over exactly the tensors that have a gradient (the buffer now holds them scaled by the coefficient)
    lay, flat = model.engine.layout, model._grad_flat.detach().cpu().double()
    sq = sum(float((flat[o:o + n] ** 2).sum()) for i, (o, n, _) in enumerate(lay.slots) if present[-1][i])
    coef = min(max_norm / (norms[-1] + 1e-6), 1.0)
    assert abs(math.sqrt(sq) / coef - norms[-1]) / norms[-1] < 2 * NORM_TOL
    _assert_flat(model, optimizer)


def test_gpu_twin_with_adam_and_torchs_clip_sees_the_same_norms():
    _need_gpu()
    cs, _, max_norm = _clip_case()
    cfg = cs["cfg"]
    X, y = torch.from_numpy(cs["x"]).cuda(), torch.from_numpy(cs["y"]).cuda()
    a = _model(cs["cfgs"])
    oa = optim.Adam(a.parameters(), lr=1e-3)
    a = a.to("cuda")
    b = _model(cs["cfgs"], fast=False).to("cuda")
    ob = torch.optim.Adam(b.parameters(), lr=1e-3)
    ta, na = _clip_loop(a, oa, X, y, cfg, 5, lambda ps: nn_utils.clip_grad_norm_(ps, max_norm))
    tb, nb = _clip_loop(b, ob, X, y, cfg, 5, lambda ps: torch.nn.utils.clip_grad_norm_(ps, max_norm))
    nerr = _norm_err(na, nb)
    cases.report("clip_adam_twin_norm_rel", nerr)
    print("clip_adam_twin_norm_rel %.3e" % nerr, na, nb)
    assert nerr < TOL, (na, nb)
    assert _trace_err(ta, tb) < TOL
    assert (na > max_norm).any()
    _assert_flat(a, oa)


def _one_backward(model, optimizer, X, y, cfg):
    """zero_grad, forward, joint loss, backward: the gradients of one step, not yet clipped or applied"""
    _clip_loop(model, _NoStep(optimizer), X, y, cfg, 1, lambda ps: 0.0)


class _NoStep:
    def __init__(self, opt):
        self.opt = opt

    def zero_grad(self):
        self.opt.zero_grad()

    def step(self):
        pass


def test_subset_of_parameters_takes_the_flat_path_and_touches_nothing_else(monkeypatch):
    _need_gpu()
    cs, _, _ = _clip_case()
    model, optimizer, X, y = _sgd_model(cs)
    _one_backward(model, optimizer, X, y, cs["cfg"])
    subset = list(model.decoder_l.parameters())
    ids = {id(p) for p in subset}
    g0 = model._grad_flat.detach().cpu().clone()
    ref = [nn.Parameter(torch.zeros_like(p, device="cpu")) for p in subset]
    for r, p in zip(ref, subset):
        r.grad = p.grad.detach().cpu().clone()
    true = float(torch.nn.utils.clip_grad_norm_(ref, math.inf))
    rt = torch.nn.utils.clip_grad_norm_(ref, 0.5 * true)
    state = (model._guarded, model._grad_present.copy(), model._grad_fresh)
    _flat_only(monkeypatch)
    total = nn_utils.clip_grad_norm_(subset, 0.5 * true)
    assert total.dim() == 0 and total.is_cuda and abs(float(total) - float(rt)) / float(rt) < 2 * NORM_TOL
    for r, p in zip(ref, subset):
        torch.testing.assert_close(p.grad.detach().cpu(), r.grad, rtol=2 * NORM_TOL + 2e-7, atol=0)
    g1 = model._grad_flat.detach().cpu()
    keep = torch.ones(g0.numel(), dtype=torch.bool)
    for p, (o, n, _) in zip(model._plist, model.engine.layout.slots):
        if id(p) in ids:
            keep[o:o + n] = False
    assert int((~keep).sum()) == sum(p.numel() for p in subset)
    assert torch.equal(_bits(g1)[keep], _bits(g0)[keep])
    # the model's gradient bookkeeping is as it was
    assert model._guarded is state[0] and np.array_equal(model._grad_present, state[1]) and model._grad_fresh == state[2]
    # value clip of the same subset
    nn_utils.clip_grad_value_(subset, 1e-4)
    g2 = model._grad_flat.detach().cpu()
    assert torch.equal(_bits(g2)[keep], _bits(g0)[keep])
    assert torch.equal(g2[~keep], torch.clamp(g1[~keep], -1e-4, 1e-4)) and float(g1[~keep].abs().max()) > 1e-4


def _twin_of(params):
    """CPU parameters with clones of the gradients of `params` (None stays None)"""
    out = []
    for p in params:
        q = nn.Parameter(torch.zeros_like(p, device="cpu"), requires_grad=p.requires_grad)
        q.grad = None if p.grad is None else p.grad.detach().cpu().clone()
        out.append(q)
    return out


def _assert_equals_torch_on_twin(params, max_norm_scale, norm_type):
    twin = _twin_of(params)
    true = float(torch.nn.utils.clip_grad_norm_(_twin_of(params), math.inf, norm_type))
    rt = torch.nn.utils.clip_grad_norm_(twin, max_norm_scale * true, norm_type)
    total = nn_utils.clip_grad_norm_(params, max_norm_scale * true, norm_type)
    # torch's own function ran on the same values, on the GPU instead of the CPU: its reduction order is the only difference
    assert abs(float(total) - float(rt)) / float(rt) < 2 * NORM_TOL, (float(total), float(rt))
    for p, q in zip(params, twin):
        assert (p.grad is None) == (q.grad is None)
        if p.grad is not None:
            torch.testing.assert_close(p.grad.detach().cpu(), q.grad, rtol=2 * NORM_TOL + 2e-7, atol=1e-30)


def _calls_torch(monkeypatch):
    """count the calls of torch.nn.utils.clip_grad_norm_ (the fallback goes there, whole)"""
    real, calls = torch.nn.utils.clip_grad_norm_, []

    def counting(*a, **k):
        calls.append(1)
        return real(*a, **k)
    monkeypatch.setattr(torch.nn.utils, "clip_grad_norm_", counting)
    return calls


def test_other_norm_types_go_to_torch(monkeypatch):
    _need_gpu()
    cs, _, _ = _clip_case()
    model, optimizer, X, y = _sgd_model(cs)
    _one_backward(model, optimizer, X, y, cs["cfg"])
    assert model._grad_views_attached()
    calls = _calls_torch(monkeypatch)
    _assert_equals_torch_on_twin(list(model.parameters()), 0.5, 3.0)
    assert len(calls) == 3                           # two on the twin, ONE from nn_utils


def test_a_frozen_parameter_goes_to_torch(monkeypatch):
    _need_gpu()
    cs, _, _ = _clip_case()
    model, optimizer, X, y = _sgd_model(cs)
    _one_backward(model, optimizer, X, y, cs["cfg"])                 # a flat step first: the gradient views are attached
    frozen = dict(model.named_parameters())["decoder_a.lstm.weight_hh"]
    frozen.requires_grad_(False)
    _one_backward(model, optimizer, X, y, cs["cfg"])
    assert not model._fast_last
    calls = _calls_torch(monkeypatch)
    _assert_equals_torch_on_twin(list(model.parameters()), 0.5, 2.0)
    assert len(calls) == 3


def test_a_composed_model_of_mfm_extra_goes_to_torch(monkeypatch):
    _need_gpu()
    from factorized_amd import mfm_extra as X_
    cs, _, _ = _clip_case()
    torch.manual_seed(3)
    model = X_.M_D(*cs["cfgs"]).cuda()
    X, y = torch.from_numpy(cs["x"]).cuda(), torch.from_numpy(cs["y"]).cuda()
    decoded, _, _ = model.forward(X)
    nn.L1Loss()(decoded[3].squeeze(1), y).backward()
    calls = _calls_torch(monkeypatch)
    _assert_equals_torch_on_twin(list(model.parameters()), 0.5, 2.0)
    assert len(calls) == 3


def test_parameters_of_two_fused_models_in_one_call_go_to_torch(monkeypatch):
    _need_gpu()
    cs, _, _ = _clip_case()
    a, oa, X, y = _sgd_model(cs)
    b, ob, _, _ = _sgd_model(cs)
    _one_backward(a, oa, X, y, cs["cfg"])
    _one_backward(b, ob, X, y, cs["cfg"])
    assert a._grad_views_attached() and b._grad_views_attached()
    calls = _calls_torch(monkeypatch)
    _assert_equals_torch_on_twin(list(a.parameters()) + list(b.parameters()), 0.5, 2.0)
    assert len(calls) == 3


def test_flat_path_does_not_synchronise(monkeypatch):
    _need_gpu()
    cs, _, max_norm = _clip_case()
    model, optimizer, X, y = _sgd_model(cs)
    _one_backward(model, optimizer, X, y, cs["cfg"])
    _flat_only(monkeypatch)
    nn_utils.clip_grad_norm_(model.parameters(), max_norm)          # (first call: workspace and span table are built)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        total = nn_utils.clip_grad_norm_(model.parameters(), max_norm)
        inf = nn_utils.clip_grad_norm_(model.parameters(), max_norm, norm_type="inf")
        assert nn_utils.clip_grad_value_(model.parameters(), 1e-3) is None
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert total.is_cuda and math.isfinite(float(total)) and 0.0 < float(inf) <= float(total)
    # (the clamp is at clip_value as an fp32 number, which is what torch clamps an fp32 tensor at too)
    assert float(model._grad_flat[:model.engine.layout.guard].abs().max()) == _f32(1e-3)


def test_guard_word_at_model_level(monkeypatch):
    """a NaN in the flat gradient buffer's guard word (what a hand-over that gave up leaves there): clipping leaves the
    gradients alone and returns NaN, the guarded optimizer step leaves the parameters alone; word back to 0: training goes on"""
    _need_gpu()
    cs, _, max_norm = _clip_case()
    cfg = cs["cfg"]
    model, optimizer, X, y = _sgd_model(cs)
    _flat_only(monkeypatch)
    clip = lambda params: nn_utils.clip_grad_norm_(params, max_norm)
    _clip_loop(model, optimizer, X, y, cfg, 1, clip)
    gw = model.engine.layout.guard
    p0 = model.engine.params.detach().clone()
    seen = {}

    def poison(step):
        model._grad_flat[gw] = NAN
        seen["g"] = _bits(model._grad_flat)

    class Checked:
        def zero_grad(self):
            optimizer.zero_grad()

        def step(self):
            seen["after_clip"] = _bits(model._grad_flat)
            optimizer.step()
    _, norms = _clip_loop(model, Checked(), X, y, cfg, 1, clip, before_clip=poison)
    assert math.isnan(norms[0])
    assert torch.equal(seen["g"], seen["after_clip"])
    assert torch.equal(_bits(model.engine.params), _bits(p0))
    model._grad_flat[gw] = 0.0
    _, norms = _clip_loop(model, optimizer, X, y, cfg, 1, clip)
    assert math.isfinite(norms[0]) and norms[0] > 0
    assert not torch.equal(_bits(model.engine.params), _bits(p0))
    _assert_flat(model, optimizer)
