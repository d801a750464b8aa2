"""factorized_amd.optim.SGD on the MI355X: the span kernel through the C ABI against torch.optim.SGD, and the reference's
unchanged loop with its commented-out optimizer line

    optimizer = optim.SGD(model.parameters(), lr=config["lr"], momentum=config["momentum"])      # mfm_mosi.py:404

against the reference's own trajectory (klef_sgd_b32_t20, tests/golden/make_golden_sgd.py) and against the CPU oracle with
torch.optim.SGD: one flat launch per step, per-group hyper-parameters, skipped tensors, fallbacks, state and hand-overs."""
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
def _launch(p, g, buf, spans, guard=None):
    arr = (_lib.SgdSpan * len(spans))()
    for j, s in enumerate(spans):
        arr[j].begin, arr[j].end = s["begin"], s["end"]
        arr[j].lr, arr[j].weight_decay, arr[j].momentum, arr[j].dampening = s["lr"], s["wd"], s["mom"], s["damp"]
        arr[j].flags = ((_lib.MFM_SGD_NESTEROV if s["nesterov"] else 0) | (_lib.MFM_SGD_MAXIMIZE if s["maximize"] else 0)
                        | (_lib.MFM_SGD_FIRST if s["first"] else 0))
    L = _lib.lib()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = lambda t: C.c_void_p(t.data_ptr() if t is not None else None)
    if guard is None:
        _lib.check(L.mfm_sgd_flat_spans(ptr(p), ptr(g), ptr(buf), arr, len(spans), 1.0, stream), "mfm_sgd_flat_spans")
    else:
        _lib.check(L.mfm_sgd_flat_spans_guarded(ptr(p), ptr(g), ptr(buf), arr, len(spans), 1.0, ptr(guard), stream),
                   "mfm_sgd_flat_spans_guarded")
    torch.cuda.synchronize()


def _flag_spans():
    """every combination of momentum / first / nesterov / maximize / weight decay / dampening, with gaps between spans and
    lengths that are not multiples of the 1024-element tile"""
    spans, cur = [], 64
    rs = np.random.RandomState(3)
    for mom in (0.0, 0.9):
        for first in (False, True):
            for nesterov in (False, True):
                for maximize in (False, True):
                    for wd in (0.0, 1e-2):
                        if (nesterov and mom == 0.0) or (first and mom == 0.0):
                            continue
                        damp = 0.0 if nesterov else float(rs.choice([0.0, 0.25]))
                        n = 4 * int(rs.randint(1, 700))
                        spans.append(dict(begin=cur, end=cur + n, lr=float(rs.choice([0.01, 0.1])), wd=wd, mom=mom, damp=damp,
                                          nesterov=nesterov, maximize=maximize, first=first))
                        cur += n + 4 * int(rs.randint(0, 40))          # (a gap: elements nobody updates)
    return spans, cur + 64


def _torch_span(p0, g0, b0, s):
    """torch.optim.SGD on CPU for one span: a fresh optimizer whose buffer exists unless the span is a first step"""
    p = nn.Parameter(p0.clone())
    opt = torch.optim.SGD([p], lr=s["lr"], momentum=s["mom"], dampening=s["damp"], weight_decay=s["wd"],
                          nesterov=s["nesterov"], maximize=s["maximize"])
    if s["mom"] != 0.0 and not s["first"]:
        opt.state[p]["momentum_buffer"] = b0.clone()
    p.grad = g0.clone()
    opt.step()
    b = opt.state[p].get("momentum_buffer")
    return p.detach(), (b if b is not None else b0)


def test_kernel_matches_torch_sgd_over_spans():
    _need_gpu()
    spans, total = _flag_spans()
    assert len(spans) <= _lib.MFM_SGD_MAX_SPANS
    torch.manual_seed(0)
    p0, g0, b0 = torch.randn(total), torch.randn(total), torch.randn(total)
    p, g, buf = p0.cuda(), g0.cuda(), b0.cuda()
    _launch(p, g, buf, spans)
    pc, bc = p.cpu(), buf.cpu()
    inside = torch.zeros(total, dtype=torch.bool)
    for s in spans:
        a, e = s["begin"], s["end"]
        inside[a:e] = True
        rp, rb = _torch_span(p0[a:e], g0[a:e], b0[a:e], s)
        torch.testing.assert_close(pc[a:e], rp, rtol=1e-6, atol=1e-6, msg=lambda m: "p %s: %s" % (s, m))
        if s["mom"] == 0.0:
            assert torch.equal(bc[a:e], b0[a:e]), s          # momentum 0: the buffer is neither read nor written
        else:
            torch.testing.assert_close(bc[a:e], rb, rtol=1e-6, atol=1e-6, msg=lambda m: "buf %s: %s" % (s, m))
    assert torch.equal(pc[~inside], p0[~inside]) and torch.equal(bc[~inside], b0[~inside])


def test_kernel_guard_and_momentum_free_launch():
    _need_gpu()
    spans, total = _flag_spans()
    torch.manual_seed(1)
    p0, g0, b0 = torch.randn(total), torch.randn(total), torch.randn(total)
    p, g, buf = p0.cuda(), g0.cuda(), b0.cuda()
    guard = torch.full((1,), float("nan"), device="cuda")
    _launch(p, g, buf, spans, guard=guard)
    assert torch.equal(p.cpu(), p0) and torch.equal(buf.cpu(), b0)      # a NaN guard word: nothing written
    guard.fill_(1.0)
    _launch(p, g, buf, spans, guard=guard)
    assert torch.equal(p.cpu(), p0) and torch.equal(buf.cpu(), b0)
    guard.zero_()
    plain = [dict(s, mom=0.0, nesterov=False, first=False) for s in spans]
    _launch(p, g, None, plain, guard=guard)                              # no buffer at all when no span has momentum
    for s in plain[:4]:
        a, e = s["begin"], s["end"]
        rp, _ = _torch_span(p0[a:e], g0[a:e], b0[a:e], s)
        torch.testing.assert_close(p.cpu()[a:e], rp, rtol=1e-6, atol=1e-6)


def test_kernel_takes_every_tensor_of_mfm_kl_as_its_own_span():
    """the largest fused model (MFM_KL, 104 tensors): one launch, one span per tensor, alternating hyper-parameters"""
    _need_gpu()
    from factorized_amd import mfm_model as M
    model = M.MFM_KL(*configs.canonical_configs(dropout=False)).cuda()
    lay = model.engine.layout
    order = sorted(range(len(lay.slots)), key=lambda i: lay.slots[i][0])
    starts = [lay.slots[i][0] for i in order] + [lay.guard]
    spans = [dict(begin=starts[k], end=starts[k + 1], lr=0.01 * (1 + k % 3), wd=0.0, mom=0.9 * (k % 2), damp=0.0,
                  nesterov=False, maximize=False, first=bool(k % 4 == 1)) for k in range(len(order))]
    assert len(spans) == 104
    torch.manual_seed(2)
    p0, g0, b0 = torch.randn(lay.total), torch.randn(lay.total), torch.randn(lay.total)
    p, g, buf = p0.cuda(), g0.cuda(), b0.cuda()
    _launch(p, g, buf, spans)
    pc, bc = p.cpu(), buf.cpu()
    for s in spans:
        a, e = s["begin"], s["end"]
        rp, rb = _torch_span(p0[a:e], g0[a:e], b0[a:e], s)
        torch.testing.assert_close(pc[a:e], rp, rtol=1e-6, atol=1e-6)
        torch.testing.assert_close(bc[a:e], rb, rtol=1e-6, atol=1e-6)
    assert torch.equal(pc[lay.guard:], p0[lay.guard:])


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
    """the fast path really ran: hand-overs allowed, nothing through torch, gradients are views of ONE buffer"""
    assert model._handover_ok() and optimizer._fallback is None
    assert model._grad_views_attached()
    g = model._grad_flat
    assert all(g.data_ptr() <= p.grad.data_ptr() < g.data_ptr() + 4 * g.numel() for p in model.parameters())


def _sgd_case():
    cs = cases.load_case("klef_b32_t20")
    gold = np.load(cases.GOLDEN + "/klef_sgd_b32_t20.npz")
    return cs, gold


def test_unchanged_reference_loop_with_dropin_sgd_follows_reference_trajectory():
    _need_gpu()
    cs, gold = _sgd_case()
    cfg = cs["cfg"]
    assert (cfg["lr"], cfg["momentum"]) == (0.01, 0.9)
    model = _model(cs["cfgs"])
    optimizer = optim.SGD(model.parameters(), lr=cfg["lr"], momentum=cfg["momentum"])     # :404, before .to(device)
    model = model.to("cuda")
    X, y = torch.from_numpy(cs["x"]).cuda(), torch.from_numpy(cs["y"]).cuda()
    first = _reference_loop(model, optimizer, X, y, cfg, 1)
    perr1 = _param_err(_summaries(model), gold["param_after1"])          # the first step: buffers created from the gradient
    cases.report("dropin_sgd_param_rel_step1", perr1)
    assert perr1 < 0.1 * TOL, perr1
    trace = np.concatenate([first, _reference_loop(model, optimizer, X, y, cfg, int(gold["meta"][2]) - 1)])
    terr = _trace_err(trace, gold["trace"])
    cases.report("dropin_sgd_trace_rel", terr)
    assert terr < 0.1 * TOL, (trace[:, 0], gold["trace"][:, 0])
    perr = _param_err(_summaries(model), gold["param_after_last"])
    cases.report("dropin_sgd_param_rel", perr)
    assert perr < 0.5 * TOL, perr
    _assert_flat(model, optimizer)


def test_staged_loop_skips_tensors_without_gradient_like_the_reference():
    """train_beta_vae's stage losses with zero_grad() (set_to_none): a tensor the stage loss does not reach is skipped, its
    momentum buffer included -- pinned to the reference's staged trajectory"""
    _need_gpu()
    cs, gold = _sgd_case()
    cfg = cs["cfg"]
    B, T, _, n1, n2 = (int(v) for v in gold["meta"])
    model = _model(cs["cfgs"])
    optimizer = optim.SGD(model.parameters(), lr=cfg["lr"], momentum=cfg["momentum"])
    model = model.to("cuda")
    X, y = torch.from_numpy(cs["x"]).cuda(), torch.from_numpy(cs["y"]).cuda()
    t1 = _reference_loop(model, optimizer, X, y, cfg, n1, stage_of=lambda s: 1)
    perr1 = _param_err(_summaries(model), gold["staged_param_after_stage1"])     # the classifier has not moved yet
    assert perr1 < 0.5 * TOL, perr1
    trace = np.concatenate([t1, _reference_loop(model, optimizer, X, y, cfg, n2, stage_of=lambda s: 2)])
    terr = _trace_err(trace, gold["staged_trace"])
    cases.report("dropin_sgd_staged_trace_rel", terr)
    assert terr < 0.5 * TOL, (trace[:, 0], gold["staged_trace"][:, 0])
    perr = _param_err(_summaries(model), gold["staged_param_after_stage2"])
    assert perr < 0.5 * TOL, perr
    _assert_flat(model, optimizer)


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


def _compare_with_oracle(cls, variant, make_groups, steps=5, stage_of=None, zero_kw=None, gauss_case=None, hooks=None,
                         flat=True):
    """the same loop on our model (GPU, factorized_amd.optim.SGD) and on the oracle (CPU, torch.optim.SGD) with the same
    parameter groups; returns (ours, oracle, optimizer)"""
    cfgs = configs.canonical_configs(dropout=False)
    cfg = cfgs[0]
    xn, yn = synth.make_batch(cfg["input_dims"], 32, 20, seed=7)
    gauss = None
    if gauss_case is not None:
        g = torch.from_numpy(np.ascontiguousarray(np.load(cases.GOLDEN + "/%s.npz" % gauss_case)["mmd_gauss"]))
        gauss = list(torch.split(g, [cfg["zl_size"], cfg["za_size"], cfg["zv_size"], cfg["zy_size"]], dim=1))
    ref = _oracle(variant, cfgs, gauss)
    ropt = torch.optim.SGD(make_groups(ref))
    ours = _model(cfgs, True, cls)
    oopt = optim.SGD(make_groups(ours))
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
    return ours, ref, oopt


def _one_group(lr=0.01, momentum=0.9, **kw):
    return lambda m: [dict(params=list(m.parameters()), lr=lr, momentum=momentum, **kw)]


@pytest.mark.parametrize("cls,variant,gauss", [("MFM_KL", "kl", None), ("MFM", "mmd", "mmd_b32_t20")])
def test_mfm_kl_and_mfm_follow_the_oracle(cls, variant, gauss):
    _need_gpu()
    ours, _, _ = _compare_with_oracle(cls, variant, _one_group(), gauss_case=gauss)
    if cls == "MFM_KL":
        # the unused MFN output layers never receive a gradient: skipped, never moved
        w0 = synth.make_weights({k: tuple(v.shape) for k, v in ours.state_dict().items()}, seed=1234)
        assert np.array_equal(ours.mfn_encoder.out_fc1.weight.detach().cpu().numpy(), w0["mfn_encoder.out_fc1.weight"])


def test_staged_loop_legacy_zero_grad_keeps_moving_on_momentum():
    """zero_grad(set_to_none=False) (the reference's PyTorch 0.4): a tensor with a zero gradient keeps moving on its momentum"""
    _need_gpu()
    _compare_with_oracle("MFM_KL_EF", "kl_ef", _one_group(), steps=8, stage_of=lambda s: 1 if s < 4 else 2,
                         zero_kw={"set_to_none": False})


def _three_groups(m):
    enc = [p for n, p in m.named_parameters() if n.startswith(("encoder_", "ef_encoder"))]
    dec = [p for n, p in m.named_parameters() if n.startswith("decoder_")]
    ids = {id(p) for p in enc + dec}
    rest = [p for p in m.parameters() if id(p) not in ids]
    return [dict(params=enc, lr=0.005, momentum=0.9, nesterov=True), dict(params=dec, lr=0.02, momentum=0.5, dampening=0.1),
            dict(params=rest, lr=0.01, momentum=0.0, weight_decay=1e-3)]


def test_several_groups_covering_the_model_stay_on_the_flat_path():
    _need_gpu()
    _compare_with_oracle("MFM_KL_EF", "kl_ef", _three_groups, steps=6)


def test_partial_coverage_takes_the_fallback_and_leaves_the_rest_alone():
    """the reference's grouped example (an encoder and the classifier, mfm_mosi.py:242-245) on MFM_KL_EF: a model only partly
    in the optimizer keeps torch.optim.SGD's behaviour on the same model and separate launches; what is not in the optimizer
    never moves"""
    _need_gpu()
    cs, _ = _sgd_case()
    cfg = cs["cfg"]
    X, y = torch.from_numpy(cs["x"]).cuda(), torch.from_numpy(cs["y"]).cuda()

    def groups(m):
        return [dict(params=list(m.encoder_l.parameters()), lr=cfg["lr"]),
                dict(params=list(m.fy_to_y_fc2.parameters()), lr=cfg["lr"])]
    ours, ref = _model(cs["cfgs"]).cuda(), _model(cs["cfgs"]).cuda()
    opt, ropt = optim.SGD(groups(ours), momentum=0.9), torch.optim.SGD(groups(ref), momentum=0.9)
    to = _reference_loop(ours, opt, X, y, cfg, 4)
    tr = _reference_loop(ref, ropt, X, y, cfg, 4)
    assert _trace_err(to, tr) < 1e-6
    for (n, p), q in zip(ours.named_parameters(), ref.parameters()):
        torch.testing.assert_close(p, q, rtol=1e-6, atol=1e-7, msg=n)
    assert opt._fallback is not None and not ours._handover_ok()
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


def test_mixed_optimizer_uses_the_fallback_for_the_extra_layer_only():
    """an extra nn.Linear in the same optimizer: that layer goes through the inner torch.optim.SGD, the model stays flat"""
    _need_gpu()
    torch.manual_seed(5)
    head, head_ref = nn.Linear(4, 3), nn.Linear(4, 3)
    head_ref.load_state_dict(head.state_dict())
    head = head.cuda()
    xh = torch.randn(8, 4)

    def mine(m):
        return hasattr(m, "_plist")

    def groups(m):
        return [dict(params=list(m.parameters()) + list((head if mine(m) else head_ref).parameters()), lr=0.01, momentum=0.9)]

    def hooks(m):
        h, x = (head, xh.cuda()) if mine(m) else (head_ref, xh)
        return lambda step: (h(x) ** 2).mean().backward()        # (after zero_grad: the extra layer's own loss)

    ours, _, opt = _compare_with_oracle("MFM_KL_EF", "kl_ef", groups, steps=4, hooks=hooks, flat=False)
    assert opt._fallback is not None
    assert {id(p) for g in opt._fallback.param_groups for p in g["params"]} == {id(p) for p in head.parameters()}
    assert ours._handover_ok() and ours._grad_views_attached()
    torch.testing.assert_close(head.weight.detach().cpu(), head_ref.weight.detach(), rtol=1e-6, atol=1e-7)


# ----------------------------------------------------------------------------------- state
def test_freeze_unfreeze_freeze_keeps_the_momentum():
    _need_gpu()

    def hooks(m):
        p = dict(m.named_parameters())["decoder_a.lstm.weight_hh"]

        def before(step):
            p.requires_grad_(step not in (2, 3, 6))
        return before
    _compare_with_oracle("MFM_KL_EF", "kl_ef", _one_group(momentum=0.9, dampening=0.2), steps=8, hooks=hooks, flat=False)


def test_frozen_from_the_start_then_unfrozen_keeps_the_momentum():
    """a parameter frozen from the first step (the model starts on the inner torch.optim.SGD) and trainable again from step 2:
    the flat path takes over the inner optimizer's buffers instead of starting every tensor's momentum again"""
    _need_gpu()

    def hooks(m):
        p = dict(m.named_parameters())["decoder_a.lstm.weight_hh"]

        def before(step):
            p.requires_grad_(step >= 2)
        return before
    ours, _, opt = _compare_with_oracle("MFM_KL_EF", "kl_ef", _one_group(momentum=0.9), steps=5, hooks=hooks, flat=False)
    st = opt._fused[ours]
    assert ours._handover_ok() and ours._grad_views_attached() and ours not in opt._away
    assert st["have"].all() and not any(p in opt._fallback.state for p in ours.parameters())


def test_guard_skipped_first_step_with_dampening_is_rolled_back():
    """the guard word holds a NaN at the first step (a hand-over gave up): nothing moves, the buffers do not exist afterwards,
    and the next step is torch's first step -- with dampening, where a buffer left marked as existing would differ"""
    _need_gpu()
    cfgs = configs.canonical_configs(dropout=False)
    cfg = cfgs[0]
    xn, yn = synth.make_batch(cfg["input_dims"], 32, 20, seed=7)
    kw = dict(lr=0.01, momentum=0.9, dampening=0.5)
    ref = _oracle("kl_ef", cfgs)
    tr = _oracle_loop(ref, torch.optim.SGD(ref.parameters(), **kw), torch.from_numpy(xn), torch.from_numpy(yn), cfg, 2)
    ours = _model(cfgs).cuda()
    opt = optim.SGD(ours.parameters(), **kw)
    p0 = [p.detach().clone() for p in ours.parameters()]

    class SkipFirst:
        """the optimizer, with a NaN in the flat gradient's guard word at its first step"""
        n = 0

        def zero_grad(self, **k):
            opt.zero_grad(**k)

        def step(self):
            if self.n == 0:
                g = ours.engine.layout.guard
                ours._grad_flat[g] = float("nan")
                opt.step()
                st = opt._fused[ours]
                assert st["have"].all() and st["pending"] is not None       # (not known yet: the guard is read later)
                opt.state_dict()                                             # reads it
                assert not st["have"].any() and float(st["buf"].abs().max()) == 0.0
                for p, q in zip(ours.parameters(), p0):
                    assert torch.equal(p, q)
                ours._grad_flat[g] = 0.0
            else:
                opt.step()
            self.n += 1
    to = _reference_loop(ours, SkipFirst(), torch.from_numpy(xn).cuda(), torch.from_numpy(yn).cuda(), cfg, 3)
    assert _trace_err(to[1:], tr) < 0.5 * TOL, (to[:, 0], tr[:, 0])
    perr = _param_err(_summaries(ours), np.stack([cases.summarize(p.detach().numpy()) for p in ref.parameters()]))
    assert perr < 0.5 * TOL, perr
    assert opt._fused[ours]["have"].all()


def test_state_dict_resume_continues_identically():
    _need_gpu()
    cs, _ = _sgd_case()
    cfg = cs["cfg"]
    X, y = torch.from_numpy(cs["x"]).cuda(), torch.from_numpy(cs["y"]).cuda()
    a = _model(cs["cfgs"]).cuda()
    oa = optim.SGD(a.parameters(), lr=0.01, momentum=0.9, dampening=0.1)
    _reference_loop(a, oa, X, y, cfg, 3)
    sd = oa.state_dict()
    assert len(sd["fused"]) == 1 and sd["fused"][0]["buf"] is not None and all(sd["fused"][0]["have"])
    b = _model(cs["cfgs"]).cuda()
    b.load_state_dict(a.state_dict())
    ob = optim.SGD(b.parameters(), lr=0.01, momentum=0.9, dampening=0.1)
    ob.load_state_dict(sd)
    ta = _reference_loop(a, oa, X, y, cfg, 3)
    tb = _reference_loop(b, ob, X, y, cfg, 3)
    # (identical up to the rounding of the backward's atomic sums, ~1e-8; a momentum restarted from zero would differ by
    #  0.9 * lr * buf per step)
    assert _trace_err(tb, ta) < 1e-6, (ta[:, 0], tb[:, 0])
    for p, q in zip(a.parameters(), b.parameters()):
        torch.testing.assert_close(q, p, rtol=1e-5, atol=1e-7)
    # a fused state of another flat layout (another model / library version) is refused, not silently restarted
    bad = dict(sd, fused=[dict(sd["fused"][0], total=sd["fused"][0]["total"] + 64)])
    c = _model(cs["cfgs"]).cuda()
    oc = optim.SGD(c.parameters(), lr=0.01, momentum=0.9, dampening=0.1)
    oc.load_state_dict(bad)
    with pytest.raises(_lib.MfmError, match="does not fit"):
        _reference_loop(c, oc, X, y, cfg, 1)


def test_reduce_lr_on_plateau_is_honoured_on_the_flat_path():
    _need_gpu()
    cs, _ = _sgd_case()
    cfg = cs["cfg"]
    X, y = torch.from_numpy(cs["x"]).cuda(), torch.from_numpy(cs["y"]).cuda()
    model = _model(cs["cfgs"]).cuda()
    opt = optim.SGD(model.parameters(), lr=0.01, momentum=0.9)
    sched = optim.ReduceLROnPlateau(opt, "min", patience=0, factor=0.1)
    _reference_loop(model, opt, X, y, cfg, 2)
    sched.step(1e9)
    sched.step(1e10)                       # no improvement: lr 0.01 -> 0.001
    assert abs(opt.param_groups[0]["lr"] - 0.001) < 1e-12
    p0 = model.engine.params.clone()
    buf0 = opt._fused[model]["buf"].clone()
    _reference_loop(model, opt, X, y, cfg, 1)
    g = model._grad_flat
    # p1 = p0 - lr * (0.9 * buf0 + g): the step used the lowered rate
    want = p0 - 0.001 * (0.9 * buf0 + g)
    n = model.engine.layout.guard
    torch.testing.assert_close(model.engine.params[:n], want[:n], rtol=1e-5, atol=1e-7)
    _assert_flat(model, opt)


def test_step_inside_a_stream_capture_is_refused():
    _need_gpu()
    cs, _ = _sgd_case()
    model = _model(cs["cfgs"]).cuda()
    opt = optim.SGD(model.parameters(), lr=0.01, momentum=0.9)
    s = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with pytest.raises(_lib.MfmError, match="stream capture"):
            with torch.cuda.graph(graph, stream=s):
                opt.step()


# ----------------------------------------------------------------------------------- hand-overs
def test_foreign_torch_sgd_still_revokes_the_handovers():
    _need_gpu()
    cs, _ = _sgd_case()
    cfg = cs["cfg"]
    X, y = torch.from_numpy(cs["x"]).cuda(), torch.from_numpy(cs["y"]).cuda()
    model = _model(cs["cfgs"]).cuda()
    ours = optim.SGD(model.parameters(), lr=0.01, momentum=0.9)
    _reference_loop(model, ours, X, y, cfg, 1)
    assert model._handover_ok()
    foreign = torch.optim.SGD(model.parameters(), lr=0.01, momentum=0.9)
    _reference_loop(model, foreign, X, y, cfg, 1)
    assert not model._handover_ok()
    _reference_loop(model, ours, X, y, cfg, 1)           # our optimizer steps the model again: it answers for the guard
    assert model._handover_ok()
