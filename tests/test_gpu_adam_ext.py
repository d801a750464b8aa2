"""factorized_amd.optim.Adam / AdamW with torch.optim.Adam's other options on the MI355X: the span kernel through the C ABI
against torch.optim.Adam / AdamW, and the reference's unchanged loop with

    optim.AdamW(model.parameters(), lr=1e-3, weight_decay=1e-2)
    optim.Adam(model.parameters(), lr=1e-3, weight_decay=1e-4, amsgrad=True)
    optim.AdamW([{"params": encoders, "lr": 1e-4}, {"params": rest}], lr=1e-3, weight_decay=1e-2)

against the reference's own trajectories (klef_adamw_b32_t20, tests/golden/make_golden_adamw.py) and against the CPU oracle
with torch's optimizers: one flat launch per step, per-group hyper-parameters, skipped tensors, fallbacks, state, hand-overs."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn as nn

import factorized_amd.optim as optim
from factorized_amd import _lib, configs, synth
from tests import cases

pytestmark = pytest.mark.gpu
TOL = 1e-4


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


# ----------------------------------------------------------------------------------- the kernel through the C ABI
def _flags(s):
    return ((_lib.MFM_ADAMX_MAXIMIZE if s["maximize"] else 0) | (_lib.MFM_ADAMX_AMSGRAD if s["amsgrad"] else 0)
            | (_lib.MFM_ADAMX_DECOUPLED if s["decoupled"] else 0))


def _launch(p, g, m, v, vmax, spans, guard=None, grad_scale=1.0):
    arr = (_lib.AdamExtSpan * len(spans))()
    for j, s in enumerate(spans):
        arr[j].begin, arr[j].end, arr[j].step, arr[j].flags = s["begin"], s["end"], s["step"], _flags(s)
        arr[j].lr, arr[j].beta1, arr[j].beta2, arr[j].eps, arr[j].weight_decay = s["lr"], s["b1"], s["b2"], s["eps"], s["wd"]
    L = _lib.lib()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = lambda t: C.c_void_p(t.data_ptr() if t is not None else None)
    if guard is None:
        _lib.check(L.mfm_adam_ext_flat_spans(ptr(p), ptr(g), ptr(m), ptr(v), ptr(vmax), arr, len(spans), grad_scale, stream),
                   "mfm_adam_ext_flat_spans")
    else:
        _lib.check(L.mfm_adam_ext_flat_spans_guarded(ptr(p), ptr(g), ptr(m), ptr(v), ptr(vmax), arr, len(spans), grad_scale, ptr(guard),
                                                     stream), "mfm_adam_ext_flat_spans_guarded")
    torch.cuda.synchronize()


def _flag_spans():
    """every combination of maximize / amsgrad / decay style, weight decay zero and not, steps 1 and 7, with gaps between spans
    and lengths that are not multiples of the 1024-element tile; lr 1e-2 and 1e-1 (an absolute 1e-6 on p is at most 1e-4 of an
    update)"""
    spans, cur = [], 64
    rs = np.random.RandomState(3)
    for maximize in (False, True):
        for amsgrad in (False, True):
            for decoupled in (False, True):
                for wd in (0.0, 1e-2):
                    for step in (1, 7):
                        n = 4 * int(rs.randint(1, 700))
                        b1, b2 = ((0.9, 0.999), (0.8, 0.99))[int(rs.randint(0, 2))]
                        spans.append(dict(begin=cur, end=cur + n, step=step, lr=float(rs.choice([0.01, 0.1])), b1=b1, b2=b2,
                                          eps=float(rs.choice([1e-8, 1e-6])), wd=wd, maximize=maximize, amsgrad=amsgrad,
                                          decoupled=decoupled))
                        cur += n + 4 * int(rs.randint(0, 40))          # (a gap: elements nobody updates)
    return spans, cur + 64


def _torch_span(p0, g0, m0, v0, x0, s):
    """torch.optim.Adam (AdamW for decoupled decay) on CPU for one span, entered at the span's step count with its state"""
    p = nn.Parameter(p0.clone())
    kw = dict(lr=s["lr"], betas=(s["b1"], s["b2"]), eps=s["eps"], weight_decay=s["wd"], amsgrad=s["amsgrad"], maximize=s["maximize"])
    opt = torch.optim.AdamW([p], **kw) if s["decoupled"] else torch.optim.Adam([p], **kw)
    st = dict(step=torch.tensor(float(s["step"] - 1)), exp_avg=m0.clone(), exp_avg_sq=v0.clone())
    if s["amsgrad"]:
        st["max_exp_avg_sq"] = x0.clone()
    opt.state[p] = st
    p.grad = g0.clone()
    opt.step()
    return p.detach(), st["exp_avg"], st["exp_avg_sq"], st.get("max_exp_avg_sq", x0)


def _data(total, seed):
    """parameters, gradients, first moments; second moments and their running maximum non-negative, neither dominating"""
    torch.manual_seed(seed)
    return torch.randn(total), torch.randn(total), 0.1 * torch.randn(total), torch.rand(total), torch.rand(total)


def _check_spans(spans, host, dev):
    p0, g0, m0, v0, x0 = host
    pc, mc, vc, xc = (t.cpu() for t in dev)
    inside = torch.zeros(p0.numel(), dtype=torch.bool)
    close = lambda a, b, what, s: torch.testing.assert_close(a, b, rtol=1e-6, atol=1e-6, msg=lambda t: "%s %s: %s" % (what, s, t))
    for s in spans:
        a, e = s["begin"], s["end"]
        inside[a:e] = True
        rp, rm, rv, rx = _torch_span(p0[a:e], g0[a:e], m0[a:e], v0[a:e], x0[a:e], s)
        close(pc[a:e], rp, "p", s)
        close(mc[a:e], rm, "m", s)
        close(vc[a:e], rv, "v", s)
        if s["amsgrad"]:
            close(xc[a:e], rx, "vmax", s)
        else:
            assert torch.equal(xc[a:e], x0[a:e]), s          # no AMSGRAD: vmax is neither read nor written
    out = ~inside
    assert torch.equal(pc[out], p0[out]) and torch.equal(mc[out], m0[out]) and torch.equal(vc[out], v0[out])
    assert torch.equal(xc[out], x0[out])


def test_kernel_matches_torch_adam_over_spans():
    _need_gpu()
    spans, total = _flag_spans()
    assert len(spans) == 32 <= _lib.MFM_ADAMX_MAX_SPANS
    host = _data(total, 0)
    p, g, m, v, x = (t.cuda() for t in host)
    _launch(p, g, m, v, x, spans)
    _check_spans(spans, host, (p, m, v, x))


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def _launch_plain_spans(p, g, m, v, spans, grad_scale=1.0, guard=None):
    """mfm_adam_flat_spans[_guarded] over [(begin, end, step)], lr 0.01 and torch's default betas / eps"""
    arr = (_lib.AdamSpan * len(spans))()
    for a, (b, e, st) in zip(arr, spans):
        a.begin, a.end, a.step = b, e, st
    L = _lib.lib()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    head = (_ptr(p), _ptr(g), _ptr(m), _ptr(v), arr, len(spans), 0.01, 0.9, 0.999, 1e-8, grad_scale)
    if guard is None:
        _lib.check(L.mfm_adam_flat_spans(*head, stream), "mfm_adam_flat_spans")
    else:
        _lib.check(L.mfm_adam_flat_spans_guarded(*head, _ptr(guard), stream), "mfm_adam_flat_spans_guarded")
    torch.cuda.synchronize()


def test_span_without_options_matches_mfm_adam_flat():
    """every Adam entry point computes the bits of mfm_adam_flat (five workgroups, a partial last tile), and mfm_adam_flat's
    scalar tail (n % 4 elements) the bits of its float4 loop"""
    _need_gpu()
    n4 = 4 * 1237
    n = n4 + 3
    host = [t.clone() for t in _data(n, 4)[:4]]
    for t in host:
        t[n4:] = t[:3]                                           # the tail repeats elements 0..2
    L = _lib.lib()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    none = dict(lr=0.01, b1=0.9, b2=0.999, eps=1e-8, wd=0.0, maximize=False, amsgrad=False, decoupled=False)
    guard = torch.zeros(1, device="cuda")
    for step in (1, 9):
        for gs in (1.0, 1.0 / 3.0):
            hyper = (0.01, 0.9, 0.999, 1e-8, gs)
            p, g, m, v = (t.cuda() for t in host)
            _lib.check(L.mfm_adam_flat(_ptr(p), _ptr(g), _ptr(m), _ptr(v), n, step, *hyper, stream), "mfm_adam_flat")
            torch.cuda.synchronize()
            for t in (p, m, v):
                assert torch.equal(t[n4:], t[:3]), (step, gs)
            want = (p[:n4].clone(), m[:n4].clone(), v[:n4].clone())
            assert not torch.equal(want[0], host[0][:n4].cuda())
            step_dev = torch.full((1,), step - 1, dtype=torch.int32, device="cuda")
            lr_dev = torch.full((1,), 0.01, device="cuda")
            entries = {
                "guarded": lambda q, qg, qm, qv: _lib.check(L.mfm_adam_flat_guarded(
                    _ptr(q), _ptr(qg), _ptr(qm), _ptr(qv), n4, step, *hyper, _ptr(guard), stream), "mfm_adam_flat_guarded"),
                "dev": lambda q, qg, qm, qv: _lib.check(L.mfm_adam_flat_dev(
                    _ptr(q), _ptr(qg), _ptr(qm), _ptr(qv), n4, _ptr(step_dev), _ptr(lr_dev), 0.9, 0.999, 1e-8, gs, None, stream),
                    "mfm_adam_flat_dev"),
                "one span": lambda q, qg, qm, qv: _launch_plain_spans(q, qg, qm, qv, [(0, n4, step)], gs),
                "three spans": lambda q, qg, qm, qv: _launch_plain_spans(
                    q, qg, qm, qv, [(1024, 1024 + 4 * 300, step), (0, 1024, step), (1024 + 4 * 300, n4, step)], gs),
                "ext span": lambda q, qg, qm, qv: _launch(q, qg, qm, qv, None, [dict(none, begin=0, end=n4, step=step)],
                                                          grad_scale=gs),
            }
            for name, run in entries.items():
                q, qg, qm, qv = (t[:n4].cuda() for t in host)
                run(q, qg, qm, qv)
                torch.cuda.synchronize()
                for a, b, what in zip((q, qm, qv), want, "pmv"):
                    assert torch.equal(a, b), (name, what, step, gs, float((a - b).abs().max()))
            assert int(step_dev.item()) == step


def test_adam_flat_spans_descending_with_gaps():
    """mfm_adam_flat_spans at its maximum of 8 spans, handed over in descending order, with gaps, a span shorter than a tile,
    one of exactly a tile and mixed step counts: torch.optim.Adam inside, untouched outside; a raised guard writes nothing"""
    _need_gpu()
    spans, cur = [], 64
    for k, (n, step) in enumerate(((4, 1), (1024, 2), (1200, 7), (2052, 1), (5000, 2), (36, 7), (3076, 1), (1028, 2))):
        spans.append(dict(begin=cur, end=cur + n, step=step, lr=0.01, b1=0.9, b2=0.999, eps=1e-8, wd=0.0, maximize=False,
                          amsgrad=False, decoupled=False))
        cur += n + 4 * (1 + 5 * k)                               # (a gap: elements nobody updates)
    assert len(spans) == _lib.MFM_ADAM_MAX_SPANS
    table = [(s["begin"], s["end"], s["step"]) for s in reversed(spans)]
    host = _data(cur + 64, 5)
    dev = [t.cuda() for t in host]
    p, g, m, v, x = dev
    guard = torch.empty(1, device="cuda")
    for word in (float("nan"), 1.0):
        guard.fill_(word)
        _launch_plain_spans(p, g, m, v, table, guard=guard)
        for t, t0 in zip(dev, host):
            assert torch.equal(t.cpu(), t0)
    _launch_plain_spans(p, g, m, v, table)
    _check_spans(spans, host, (p, m, v, x))
    p, g, m, v, x = (t.cuda() for t in host)
    guard.zero_()
    _launch_plain_spans(p, g, m, v, table, guard=guard)
    _check_spans(spans, host, (p, m, v, x))


def test_kernel_guard_and_launch_without_vmax():
    _need_gpu()
    spans, total = _flag_spans()
    host = _data(total, 1)
    dev = [t.cuda() for t in host]
    p, g, m, v, x = dev
    guard = torch.full((1,), float("nan"), device="cuda")
    for word in (float("nan"), 1.0):
        guard.fill_(word)
        _launch(p, g, m, v, x, spans, guard=guard)
        for t, t0 in zip(dev, host):
            assert torch.equal(t.cpu(), t0)                   # anything but 0.0 in the guard word: nothing written
    guard.zero_()
    _launch(p, g, m, v, x, spans, guard=guard)
    _check_spans(spans, host, (p, m, v, x))
    plain = [dict(s, amsgrad=False) for s in spans]
    p, g, m, v, _ = (t.cuda() for t in host)
    _launch(p, g, m, v, None, plain, guard=guard)              # no vmax buffer at all when no span has AMSGRAD
    _check_spans(plain, host, (p, m, v, host[4]))


def test_kernel_takes_every_tensor_of_mfm_kl_as_its_own_span():
    """the largest fused model (MFM_KL, 104 tensors), every tensor its own span with alternating settings so that nothing
    merges: more spans than one argument block holds, so the table goes out in consecutive launches"""
    _need_gpu()
    from factorized_amd import mfm_model as M
    model = M.MFM_KL(*configs.canonical_configs(dropout=False)).cuda()
    lay = model.engine.layout
    order = sorted(range(len(lay.slots)), key=lambda i: lay.slots[i][0])
    starts = [lay.slots[i][0] for i in order] + [lay.guard]
    spans = [dict(begin=starts[k], end=starts[k + 1], step=1 + k % 5, lr=0.01 * (1 + 9 * (k % 2)), b1=0.9, b2=0.999, eps=1e-8,
                  wd=1e-2 * (k % 2), maximize=False, amsgrad=bool(k % 2), decoupled=bool(k % 4 == 1)) for k in range(len(order))]
    assert len(spans) == 104
    host = _data(lay.total, 2)
    p, g, m, v, x = (t.cuda() for t in host)
    for k in range(0, len(spans), _lib.MFM_ADAMX_MAX_SPANS):
        _launch(p, g, m, v, x, spans[k:k + _lib.MFM_ADAMX_MAX_SPANS])
    _check_spans(spans, host, (p, m, v, x))


# ----------------------------------------------------------------------------------- the reference loop
def _model(cfgs, fast=True, cls="MFM_KL_EF"):
    from factorized_amd import mfm_model as M
    model = getattr(M, cls)(*cfgs)
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    w = synth.make_weights(shapes, seed=1234)
    model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in w.items()})
    model.fast_grads = fast
    return model


def _reference_loop(model, optimizer, X, y, config, steps, stage_of=None, zero_kw=None, before_step=None):
    """mfm_mosi.py:424-442 (and :278-281 for the stage losses), statement by statement (tests/test_gpu_dropin.py)"""
    criterion = nn.L1Loss()
    gen_criterion = nn.MSELoss()
    d_l, d_a, d_v = config["input_dims"]
    model.train()
    trace = []
    for step in range(steps):
        optimizer.zero_grad(**(zero_kw or {}))
        if before_step is not None:
            before_step(step)
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
        optimizer.step()
        trace.append([loss.item(), disc_loss.item(), gen_loss.item(), mmd_loss.item()])
    return np.array(trace)


def _summaries(model):
    return np.stack([cases.summarize(p.detach().cpu().numpy()) for p in model.parameters()])


def _trace_err(trace, ref):
    return float(np.max(np.abs(trace - ref) / np.maximum(np.abs(ref), 1e-2)))


def _param_err(pl, ref):
    return float(np.max(np.abs(pl - ref) / np.maximum(np.abs(ref[:, :1]), 1e-3)))


def _assert_flat(model, optimizer):
    """the flat path really ran: hand-overs allowed (the model's `_guarded` refers to this optimizer), nothing through torch,
    gradients are views of ONE buffer"""
    assert model._handover_ok() and callable(model._guarded) and model._guarded() is optimizer
    assert optimizer._fallback is None
    assert model._grad_views_attached()
    g = model._grad_flat
    assert all(g.data_ptr() <= p.grad.data_ptr() < g.data_ptr() + 4 * g.numel() for p in model.parameters())


ENCODERS = ("encoder_l.", "encoder_a.", "encoder_v.", "ef_encoder.")


def _two_groups(m):
    enc = [p for n, p in m.named_parameters() if n.startswith(ENCODERS)]
    rest = [p for n, p in m.named_parameters() if not n.startswith(ENCODERS)]
    return [{"params": enc, "lr": 1e-4}, {"params": rest}]


RUNS = {
    "adamw": lambda o, m: o.AdamW(m.parameters(), lr=1e-3, weight_decay=1e-2),
    "amsgrad": lambda o, m: o.Adam(m.parameters(), lr=1e-3, weight_decay=1e-4, amsgrad=True),
    "groups": lambda o, m: o.AdamW(_two_groups(m), lr=1e-3, weight_decay=1e-2),
}


def _case():
    return cases.load_case("klef_b32_t20"), np.load(cases.GOLDEN + "/klef_adamw_b32_t20.npz")


@pytest.mark.parametrize("run", list(RUNS))
def test_unchanged_reference_loop_follows_the_reference_trajectories(run):
    """Measured on an MI355X, relative errors against the reference's own runs (bound 0.5 * TOL = 5e-5 each), as parameters
    after step 1 / loss trace / parameters after step 20: adamw 5.1e-6 / 6.1e-7 / 9.5e-7, amsgrad 2.1e-6 / 5.8e-7 / 7.2e-7,
    groups 5.1e-7 / 6.3e-7 / 8.1e-7 (profiles/adamw_kernel_stats.txt)."""
    _need_gpu()
    cs, gold = _case()
    cfg = cs["cfg"]
    model = _model(cs["cfgs"])
    optimizer = RUNS[run](optim, model)                                   # before .to(device), as the reference builds it
    model = model.to("cuda")
    X, y = torch.from_numpy(cs["x"]).cuda(), torch.from_numpy(cs["y"]).cuda()
    first = _reference_loop(model, optimizer, X, y, cfg, 1)
    perr1 = _param_err(_summaries(model), gold[run + "_param_after1"])
    trace = np.concatenate([first, _reference_loop(model, optimizer, X, y, cfg, int(gold["meta"][2]) - 1)])
    terr = _trace_err(trace, gold[run + "_trace"])
    perr = _param_err(_summaries(model), gold[run + "_param_after_last"])
    for key, val in (("param_rel_step1", perr1), ("trace_rel", terr), ("param_rel", perr)):
        cases.report("dropin_adam_ext_%s_%s" % (run, key), val)
        print("dropin_adam_ext_%s_%s %.3e" % (run, key, val))
    assert perr1 < 0.5 * TOL, perr1
    assert terr < 0.5 * TOL, (trace[:, 0], gold[run + "_trace"][:, 0])
    assert perr < 0.5 * TOL, perr
    _assert_flat(model, optimizer)
    st = optimizer._fused[model]
    assert (st["vmax"] is not None) == (run == "amsgrad") and (st["steps"] == 20).all()


def test_plain_adam_allocates_no_vmax_and_still_meets_the_reference_trajectory():
    _need_gpu()
    cs = cases.load_case("klef_b32_t20")
    cfg, gold = cs["cfg"], cs["gold"]
    model = _model(cs["cfgs"])
    optimizer = optim.Adam(model.parameters())
    model = model.to("cuda")
    X, y = torch.from_numpy(cs["x"]).cuda(), torch.from_numpy(cs["y"]).cuda()
    trace = _reference_loop(model, optimizer, X, y, cfg, cs["steps"])
    assert _trace_err(trace, gold["trace"]) < 0.1 * TOL
    assert _param_err(_summaries(model), gold["param_after_last"]) < 0.5 * TOL
    _assert_flat(model, optimizer)
    st = optimizer._fused[model]
    assert st["vmax"] is None and "runs" not in st and set(optimizer.state_dict()["fused"][0]) == {"m", "v", "steps"}


# ----------------------------------------------------------------------------------- against the CPU oracle
def _oracle(variant, cfgs, gauss=None):
    from oracle import mfm_oracle as O
    m = O.build(variant, cfgs)
    shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    O.load_numpy_weights(m, synth.make_weights(shapes, seed=1234))
    if gauss is not None:
        m.mmd_gauss = gauss
    return m


def _oracle_loop(model, optimizer, x, y, cfg, steps, stage_of=None, zero_kw=None, before_step=None):
    from oracle import mfm_oracle as O
    model.train()
    trace = []
    for step in range(steps):
        optimizer.zero_grad(**(zero_kw or {}))
        if before_step is not None:
            before_step(step)
        terms = O.loss_terms(model, x, y, cfg)
        loss = O.stage_loss(terms, cfg, stage_of(step) if stage_of else 0)
        loss.backward()
        optimizer.step()
        trace.append([loss.item(), terms["disc"].item(), terms["gen"].item(), terms["reg"].item()])
    return np.array(trace)


def _compare_with_oracle(cls, variant, make_opt, steps=5, stage_of=None, zero_kw=None, gauss_case=None, hooks=None, flat=True):
    """the same loop on our model (GPU, factorized_amd.optim) and on the oracle (CPU, torch.optim) with the same optimizer
    line `make_opt(optim module, model)`; returns (ours, oracle, our optimizer, torch's optimizer)"""
    cfgs = configs.canonical_configs(dropout=False)
    cfg = cfgs[0]
    xn, yn = synth.make_batch(cfg["input_dims"], 32, 20, seed=7)
    gauss = None
    if gauss_case is not None:
        g = torch.from_numpy(np.ascontiguousarray(np.load(cases.GOLDEN + "/%s.npz" % gauss_case)["mmd_gauss"]))
        gauss = list(torch.split(g, [cfg["zl_size"], cfg["za_size"], cfg["zv_size"], cfg["zy_size"]], dim=1))
    ref = _oracle(variant, cfgs, gauss)
    ropt = make_opt(torch.optim, ref)
    ours = _model(cfgs, True, cls)
    oopt = make_opt(optim, ours)
    ours = ours.cuda()
    if gauss is not None:
        ours.mmd_gauss = [t.cuda() for t in gauss]
    rhook, ohook = (hooks(ref), hooks(ours)) if hooks else (None, None)
    tr = _oracle_loop(ref, ropt, torch.from_numpy(xn), torch.from_numpy(yn), cfg, steps, stage_of, zero_kw, rhook)
    to = _reference_loop(ours, oopt, torch.from_numpy(xn).cuda(), torch.from_numpy(yn).cuda(), cfg, steps, stage_of, zero_kw,
                         ohook)
    terr = _trace_err(to, tr)
    assert terr < 0.5 * TOL, (to[:, 0], tr[:, 0])
    perr = _param_err(_summaries(ours), np.stack([cases.summarize(p.detach().numpy()) for p in ref.parameters()]))
    assert perr < 0.5 * TOL, perr
    if flat:
        _assert_flat(ours, oopt)
    return ours, ref, oopt, ropt


@pytest.mark.parametrize("cls,variant,gauss", [("MFM_KL", "kl", None), ("MFM", "mmd", "mmd_b32_t20")])
def test_mfm_kl_and_mfm_follow_the_oracle_under_adamw(cls, variant, gauss):
    _need_gpu()
    ours, _, _, _ = _compare_with_oracle(cls, variant, lambda o, m: o.AdamW(m.parameters()), gauss_case=gauss)
    if cls == "MFM_KL":
        # the unused MFN output layers never receive a gradient: skipped, decoupled decay included -- never moved
        w0 = synth.make_weights({k: tuple(v.shape) for k, v in ours.state_dict().items()}, seed=1234)
        assert np.array_equal(ours.mfn_encoder.out_fc1.weight.detach().cpu().numpy(), w0["mfn_encoder.out_fc1.weight"])


def test_every_option_in_three_groups_stays_on_the_flat_path():
    _need_gpu()

    def make(o, m):
        enc = [p for n, p in m.named_parameters() if n.startswith(ENCODERS)]
        dec = [p for n, p in m.named_parameters() if n.startswith("decoder_")]
        ids = {id(p) for p in enc + dec}
        rest = [p for p in m.parameters() if id(p) not in ids]
        return o.Adam([dict(params=enc, lr=5e-4, amsgrad=True, weight_decay=1e-3),
                       dict(params=dec, betas=(0.8, 0.99), eps=1e-6, weight_decay=1e-2, decoupled_weight_decay=True),
                       dict(params=rest)], lr=1e-3)
    ours, _, oopt, _ = _compare_with_oracle("MFM_KL_EF", "kl_ef", make, steps=6)
    assert len(oopt._fused[ours]["runs"][3]) <= 8                     # a handful of spans: one launch


def test_two_plain_groups_stay_on_the_flat_path():
    """the issue's last line: no new option, the encoders in a group of their own"""
    _need_gpu()
    _compare_with_oracle("MFM_KL_EF", "kl_ef", lambda o, m: o.Adam(_two_groups(m)), steps=5)


def test_maximize_and_l2_decay_with_amsgrad_follow_the_oracle():
    _need_gpu()
    _compare_with_oracle("MFM_KL_EF", "kl_ef", lambda o, m: o.Adam(m.parameters(), weight_decay=1e-3, amsgrad=True), steps=4)
    ours, _, oopt, _ = _compare_with_oracle("MFM_KL_EF", "kl_ef", lambda o, m: o.Adam(m.parameters(), maximize=True), steps=3)
    assert oopt._fused[ours]["vmax"] is None


def test_staged_loop_skips_tensors_without_gradient_with_all_their_state():
    """train_beta_vae's stage losses with zero_grad() (set_to_none) under AdamW + AMSGrad: a tensor the stage loss does not
    reach keeps parameter (no decoupled decay), moments, vmax and step count -- torch's trajectory, and checked directly"""
    _need_gpu()
    make = lambda o, m: o.AdamW(m.parameters(), lr=1e-3, weight_decay=1e-2, amsgrad=True)
    ours, _, oopt, _ = _compare_with_oracle("MFM_KL_EF", "kl_ef", make, steps=4, stage_of=lambda s: 1)
    st = oopt._fused[ours]
    names = [n for n, _ in ours.named_parameters()]
    w0 = synth.make_weights({k: tuple(v.shape) for k, v in ours.state_dict().items()}, seed=1234)
    skipped = [i for i in range(len(names)) if st["steps"][i] == 0]
    assert skipped and any(names[i].startswith("fy_to_y") for i in skipped)        # stage 1: the classifier gets no gradient
    assert set(np.unique(st["steps"])) == {0, 4}
    for i in skipped:
        o, n, _ = ours.engine.layout.slots[i]
        assert np.array_equal(ours._plist[i].detach().cpu().numpy(), w0[names[i]]), names[i]
        for key in ("m", "v", "vmax"):
            assert float(st[key][o:o + n].abs().max()) == 0.0, (names[i], key)
    # and the whole schedule (gen + reg, then disc + reg: the classifier joins at its own step 1)
    _compare_with_oracle("MFM_KL_EF", "kl_ef", make, steps=8, stage_of=lambda s: 1 if s < 4 else 2)


def test_partial_coverage_takes_the_inner_optimizer_and_leaves_the_rest_alone():
    _need_gpu()
    cs, _ = _case()
    cfg = cs["cfg"]
    X, y = torch.from_numpy(cs["x"]).cuda(), torch.from_numpy(cs["y"]).cuda()

    def groups(m):
        return [dict(params=list(m.encoder_l.parameters()), lr=1e-3, amsgrad=True),
                dict(params=list(m.fy_to_y_fc2.parameters()), weight_decay=0.1)]
    ours, ref = _model(cs["cfgs"]).cuda(), _model(cs["cfgs"]).cuda()
    opt, ropt = optim.AdamW(groups(ours)), torch.optim.AdamW(groups(ref))
    to = _reference_loop(ours, opt, X, y, cfg, 4)
    tr = _reference_loop(ref, ropt, X, y, cfg, 4)
    assert _trace_err(to, tr) < 1e-6
    for (n, p), q in zip(ours.named_parameters(), ref.parameters()):
        torch.testing.assert_close(p, q, rtol=1e-6, atol=1e-7, msg=n)
    assert opt._fallback is not None and not ours._handover_ok() and ours not in opt._fused
    fg = opt._fallback.param_groups
    assert (fg[0]["amsgrad"], fg[0]["weight_decay"], fg[1]["amsgrad"], fg[1]["weight_decay"]) == (True, 1e-2, False, 0.1)
    assert all(g["decoupled_weight_decay"] for g in fg)
    w0 = synth.make_weights({k: tuple(v.shape) for k, v in ours.state_dict().items()}, seed=1234)
    covered = {id(p) for g in groups(ours) for p in g["params"]}
    moved = 0
    for n, p in ours.named_parameters():
        same = np.array_equal(p.detach().cpu().numpy(), w0[n])
        if id(p) in covered:
            moved += not same
        else:
            assert same, n
    assert moved == len(covered)


def test_mixed_optimizer_uses_the_inner_optimizer_for_the_extra_layer_only():
    _need_gpu()
    torch.manual_seed(5)
    head, head_ref = nn.Linear(4, 3), nn.Linear(4, 3)
    head_ref.load_state_dict(head.state_dict())
    head = head.cuda()
    xh = torch.randn(8, 4)

    def mine(m):
        return hasattr(m, "_plist")

    def make(o, m):
        return o.AdamW(list(m.parameters()) + list((head if mine(m) else head_ref).parameters()), lr=1e-3, amsgrad=True)

    def hooks(m):
        h, x = (head, xh.cuda()) if mine(m) else (head_ref, xh)
        return lambda step: (h(x) ** 2).mean().backward()        # (after zero_grad: the extra layer's own loss)

    ours, _, opt, _ = _compare_with_oracle("MFM_KL_EF", "kl_ef", make, steps=4, hooks=hooks, flat=False)
    assert opt._fallback is not None
    assert {id(p) for g in opt._fallback.param_groups for p in g["params"]} == {id(p) for p in head.parameters()}
    assert ours._handover_ok() and ours._grad_views_attached() and opt._fused[ours]["vmax"] is not None
    torch.testing.assert_close(head.weight.detach().cpu(), head_ref.weight.detach(), rtol=1e-6, atol=1e-7)


# ----------------------------------------------------------------------------------- state
def test_freeze_then_unfreeze_carries_vmax_both_ways():
    """a parameter frozen for two steps (the model steps through the inner torch.optim.Adam, max_exp_avg_sq moves there with
    the moments) and trainable again (all of it comes back): torch's trajectory"""
    _need_gpu()

    def hooks(m):
        p = dict(m.named_parameters())["decoder_a.lstm.weight_hh"]

        def before(step):
            p.requires_grad_(step not in (2, 3))
        return before
    make = lambda o, m: o.Adam(m.parameters(), lr=1e-3, weight_decay=1e-3, amsgrad=True)
    ours, ref, opt, ropt = _compare_with_oracle("MFM_KL_EF", "kl_ef", make, steps=7, hooks=hooks, flat=False)
    assert ours._handover_ok() and ours._grad_views_attached()
    st = opt._fused[ours]
    assert not any(p in opt._fallback.state for p in ours.parameters())
    for i, (p, q) in enumerate(zip(ours.parameters(), ref.parameters())):
        if "max_exp_avg_sq" not in ropt.state.get(q, {}):
            continue
        o, n, shp = ours.engine.layout.slots[i]
        want = ropt.state[q]["max_exp_avg_sq"]
        got = st["vmax"][o:o + n].view(shp).cpu()
        scale = float(want.abs().max()) + 1e-30
        assert float((got - want).abs().max()) / scale < 1e-3, i


def test_state_dict_resume_continues_identically():
    _need_gpu()
    cs, _ = _case()
    cfg = cs["cfg"]
    X, y = torch.from_numpy(cs["x"]).cuda(), torch.from_numpy(cs["y"]).cuda()
    kw = dict(lr=1e-3, weight_decay=1e-2, amsgrad=True)
    a = _model(cs["cfgs"]).cuda()
    oa = optim.AdamW(a.parameters(), **kw)
    _reference_loop(a, oa, X, y, cfg, 3)
    sd = oa.state_dict()
    assert len(sd["fused"]) == 1 and sd["fused"][0]["vmax"] is not None and set(sd["fused"][0]["steps"]) == {3}
    b = _model(cs["cfgs"]).cuda()
    b.load_state_dict(a.state_dict())
    ob = optim.AdamW(b.parameters(), **kw)
    ob.load_state_dict(sd)
    assert ob.state_dict()["fused"][0]["vmax"] is not None          # loaded, not stepped yet: still the state
    ta = _reference_loop(a, oa, X, y, cfg, 3)
    tb = _reference_loop(b, ob, X, y, cfg, 3)
    # (identical up to the rounding of the backward's atomic sums; restarted moments would differ in the first digits)
    assert _trace_err(tb, ta) < 1e-6, (ta[:, 0], tb[:, 0])
    for p, q in zip(a.parameters(), b.parameters()):
        torch.testing.assert_close(q, p, rtol=1e-5, atol=1e-7)
    xa, xb = oa._fused[a]["vmax"], ob._fused[b]["vmax"]
    assert float((xa - xb).abs().max()) < 1e-4 * float(xa.abs().max())
    # a fused state of another flat layout is refused, not silently restarted -- a vmax of another size too
    for bad_entry in (dict(sd["fused"][0], vmax=sd["fused"][0]["vmax"][:-64]),
                      dict(sd["fused"][0], steps=sd["fused"][0]["steps"][:-1])):
        c = _model(cs["cfgs"]).cuda()
        oc = optim.AdamW(c.parameters(), **kw)
        oc.load_state_dict(dict(sd, fused=[bad_entry]))
        with pytest.raises(_lib.MfmError, match="does not fit"):
            _reference_loop(c, oc, X, y, cfg, 1)
    # a state saved without vmax loads into an optimizer without AMSGrad as before
    d = _model(cs["cfgs"]).cuda()
    od = optim.Adam(d.parameters())
    _reference_loop(d, od, X, y, cfg, 2)
    e = _model(cs["cfgs"]).cuda()
    e.load_state_dict(d.state_dict())
    oe = optim.Adam(e.parameters())
    oe.load_state_dict(od.state_dict())
    assert _trace_err(_reference_loop(e, oe, X, y, cfg, 2), _reference_loop(d, od, X, y, cfg, 2)) < 1e-6
    assert oe._fused[e]["vmax"] is None


def test_reduce_lr_on_plateau_is_honoured_on_the_flat_path():
    _need_gpu()
    cs, _ = _case()
    cfg = cs["cfg"]
    X, y = torch.from_numpy(cs["x"]).cuda(), torch.from_numpy(cs["y"]).cuda()
    model = _model(cs["cfgs"]).cuda()
    opt = optim.AdamW(model.parameters(), lr=1e-3, weight_decay=1e-2)
    sched = optim.ReduceLROnPlateau(opt, "min", patience=0, factor=0.1)
    _reference_loop(model, opt, X, y, cfg, 2)
    sched.step(1e9)
    sched.step(1e10)                       # no improvement: lr 1e-3 -> 1e-4
    assert abs(opt.param_groups[0]["lr"] - 1e-4) < 1e-15
    n = model.engine.layout.guard
    p0 = model.engine.params.clone()
    st = opt._fused[model]
    m0, v0 = st["m"].clone(), st["v"].clone()
    _reference_loop(model, opt, X, y, cfg, 1)
    g = model._grad_flat.double()
    # the third step of AdamW in double precision with the LOWERED rate
    m1 = m0.double() + 0.1 * (g - m0.double())
    v1 = 0.999 * v0.double() + 0.001 * g * g
    want = p0.double() * (1 - 1e-4 * 1e-2) - (1e-4 / (1 - 0.9 ** 3)) * m1 / (v1.sqrt() / (1 - 0.999 ** 3) ** 0.5 + 1e-8)
    got = model.engine.params.double()
    moved = (got[:n] - p0.double()[:n]).abs().max()
    assert float((got[:n] - want[:n]).abs().max()) < 1e-3 * float(moved) + 1e-7      # (at lr 1e-3 the step is 10 x larger)
    _assert_flat(model, opt)


def test_capturable_with_a_new_option_or_a_second_group_is_refused():
    _need_gpu()
    cfgs = configs.canonical_configs(dropout=False)
    model = _model(cfgs)
    for make in (lambda: optim.Adam(model.parameters(), weight_decay=1e-2, capturable=True),
                 lambda: optim.Adam(model.parameters(), amsgrad=True, capturable=True),
                 lambda: optim.Adam(model.parameters(), maximize=True, capturable=True),
                 lambda: optim.AdamW(model.parameters(), capturable=True),
                 lambda: optim.Adam(_two_groups(model), capturable=True)):
        with pytest.raises(ValueError, match="capturable"):
            make()
    optim.Adam(model.parameters(), capturable=True)                 # the plain capturable update is still built


# ----------------------------------------------------------------------------------- hand-overs
def test_foreign_torch_adamw_still_revokes_the_handovers():
    _need_gpu()
    cs, _ = _case()
    cfg = cs["cfg"]
    X, y = torch.from_numpy(cs["x"]).cuda(), torch.from_numpy(cs["y"]).cuda()
    model = _model(cs["cfgs"]).cuda()
    ours = optim.AdamW(model.parameters())
    _reference_loop(model, ours, X, y, cfg, 1)
    assert model._handover_ok()
    foreign = torch.optim.AdamW(model.parameters())
    _reference_loop(model, foreign, X, y, cfg, 1)
    assert not model._handover_ok()
    _reference_loop(model, ours, X, y, cfg, 1)           # our optimizer steps the model again: it answers for the guard
    assert model._handover_ok()
