"""The prediction-only path (engine.predict, model.predict / model.evaluate, mfm_predict_klef) on the MI355X: y_hat and the
discriminative loss against the reference's own golden outputs, partial tiles and row chunks, canaries around its buffers,
run-to-run determinism, what it must leave alone (plans, gradients, parameters), capture together with the device-side
scheduler and keep-best, and the fallbacks.  Numeric bound: the project's 1e-4 relative fp32 tolerance (tests.cases.rel_err)."""
import ctypes as C
import io

import numpy as np
import pytest
import torch

from oracle import mfm_oracle as O
from factorized_amd import _lib, configs, synth
from tests import cases
from tests.cases import grad_err, rel_err

pytestmark = pytest.mark.gpu
TOL = 1e-4
CANARY = 0x7FC0DEAD                   # a NaN with a payload: any store over it shows


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
    return model.to("cuda")


def _xy(cs):
    return torch.from_numpy(cs["x"]).cuda(), torch.from_numpy(cs["y"]).cuda()


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _take(out):
    """the engine reuses its output buffers: keep a copy"""
    return out["y_hat"].clone(), (None if out["loss"] is None else out["loss"].clone())


_B33 = {}


def _b33():
    """the B=33, T=7 case with its unchunked result, computed once"""
    if not _B33:
        cs = cases.load_case("klef_b33_t7")
        e, _ = _engine(cs["cfgs"])
        x, y = _xy(cs)
        yh, loss = _take(e.predict(x, y))
        _B33.update(cs=cs, e=e, x=x, y=y, y_hat=yh.cpu().numpy(), loss=float(loss))
    return _B33


# ----------------------------------------------------------------------------------- 1. the reference's own outputs
@pytest.mark.parametrize("name", cases.KLEF_CASES)
def test_predict_matches_reference_golden(name):
    cs = cases.load_case(name)
    e, _ = _engine(cs["cfgs"])
    x, y = _xy(cs)
    out = e.predict(x, y)
    gold = cs["gold"]
    err = rel_err(out["y_hat"].cpu().numpy(), gold["y_hat"])
    ref = float(gold["fwd_disc"])
    got = float(out["loss"])
    print("predict_golden %s y_hat %.3e loss %.8g ref %.8g" % (name, err, got, ref))
    assert out["y_hat"].shape == (cs["B"], cs["cfg"]["output_dim"]) and out["loss"].dim() == 0 and out["loss"].is_cuda
    assert err < TOL
    assert abs(got - ref) <= TOL * max(abs(ref), 1e-3)
    assert e.predict(x)["loss"] is None
    assert not e._plans


# ----------------------------------------------------------------------------------- 2. dropout is off
def test_dropout_is_off_whatever_the_mode():
    cfgs = configs.canonical_configs(dropout=True)
    cfg = cfgs[0]
    xn, yn = synth.make_batch(cfg["input_dims"], 33, 7, seed=7, output_dim=cfg["output_dim"])
    x, y = torch.from_numpy(xn).cuda(), torch.from_numpy(yn).cuda()
    e, _ = _engine(cfgs)
    a, la = _take(e.predict(x, y))
    b, lb = _take(e.predict(x, y))
    ref = e.forward(x, y, train=False)["y_hat"]
    assert rel_err(a.cpu().numpy(), ref.cpu().numpy()) < TOL
    assert torch.equal(_bits(a), _bits(b)) and torch.equal(_bits(la), _bits(lb))
    model = _model(cfgs)
    model.train()
    c = model.predict(x).clone()
    assert model.training
    model.eval()
    d = model.predict(x).clone()
    assert torch.equal(_bits(c), _bits(d)) and torch.equal(_bits(c), _bits(a))


# ----------------------------------------------------------------------------------- 3. partial tiles and chunks
@pytest.mark.parametrize("k", [1, 2, 3, 4, 5, 8, 31, 32])
def test_first_k_rows(k):
    s = _b33()
    xk = s["x"][:, :k].contiguous()
    yk = s["y"][:k].contiguous()
    out = s["e"].predict(xk, yk)
    assert rel_err(out["y_hat"].cpu().numpy(), s["y_hat"][:k]) < TOL
    want = float(np.abs(s["y_hat"][:k].astype(np.float64) - s["cs"]["y"][:k].reshape(k, -1)).mean())
    assert abs(float(out["loss"]) - want) <= TOL * max(abs(want), 1e-3)


@pytest.mark.parametrize("max_rows", [1, 4, 16, 32, 33, 64])
def test_row_chunks(max_rows):
    s = _b33()
    out = s["e"].predict(s["x"], s["y"], max_rows=max_rows)
    assert rel_err(out["y_hat"].cpu().numpy(), s["y_hat"]) < TOL
    # the mean over all 33 rows, not a mean of chunk means (the last chunk is short)
    want = float(np.abs(s["y_hat"].astype(np.float64) - s["cs"]["y"].reshape(33, -1)).mean())
    got = float(out["loss"])
    assert abs(got - want) <= TOL * max(abs(want), 1e-3), (got, want)
    assert abs(got - s["loss"]) <= TOL * max(abs(s["loss"]), 1e-3)


# ----------------------------------------------------------------------------------- 4. nothing outside its buffers
def _call_abi(e, x, y, ws, y_hat, loss, cap):
    from factorized_amd import engine
    c = e.cfg
    T, N, D = x.shape
    h = c["zl_size"] + c["za_size"] + c["zv_size"]
    offs = (C.c_int64 * 16)(*[e.layout.offsets[n] for n in engine.MFMEngine._PREDICT_TENSORS])
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(None)
    return _lib.lib().mfm_predict_klef(T, N, D, h, c["zy_size"], c["fy_size"], c["output_dim"],
                                       1 if c.get("loss", "l1") == "ce" else 0, p(e.params), offs, p(x), p(y), p(ws), p(y_hat),
                                       p(loss), cap, C.c_void_p(torch.cuda.current_stream().cuda_stream))


@pytest.mark.parametrize("name,cap", [("klef_b5_t1", 0), ("klef_b33_t7", 0), ("klef_b33_t7", 16)])
def test_canaries_around_workspace_and_output(name, cap):
    cs = cases.load_case(name)
    e, _ = _engine(cs["cfgs"])
    x, y = _xy(cs)
    T, N, od = cs["T"], cs["B"], cs["cfg"]["output_dim"]
    h = sum(cs["cfg"][k] for k in ("zl_size", "za_size", "zv_size"))
    nws = int(_lib.lib().mfm_predict_klef_workspace_floats(T, N, h, cap))
    PAD = 256
    big_ws = torch.full((PAD + nws + PAD,), CANARY, dtype=torch.int32, device="cuda")
    big_y = torch.full((PAD + N * od + PAD,), CANARY, dtype=torch.int32, device="cuda")
    big_l = torch.full((9,), CANARY, dtype=torch.int32, device="cuda")
    ws = big_ws[PAD:PAD + nws].view(torch.float32)
    y_hat = big_y[PAD:PAD + N * od].view(torch.float32).view(N, od)
    loss = big_l[4:5].view(torch.float32)
    assert _call_abi(e, x, y, ws, y_hat, loss, cap) == 0
    torch.cuda.synchronize()
    for big, n in ((big_ws, nws), (big_y, N * od)):
        assert bool((big[:PAD] == CANARY).all()) and bool((big[PAD + n:] == CANARY).all())
    assert bool((big_l[:4] == CANARY).all()) and bool((big_l[5:] == CANARY).all())
    assert rel_err(y_hat.cpu().numpy(), cs["gold"]["y_hat"]) < TOL
    ref = float(cs["gold"]["fwd_disc"])
    assert abs(float(loss) - ref) <= TOL * max(abs(ref), 1e-3)
    assert int(big_ws[PAD + nws - 4]) == 0               # the ticket word is back at 0


# ----------------------------------------------------------------------------------- 5. run-to-run determinism
@pytest.mark.parametrize("max_rows", [None, 64])
def test_bit_identical_from_run_to_run(max_rows):
    cs = cases.load_case("klef_b229_t20")
    e, _ = _engine(cs["cfgs"])
    x, y = _xy(cs)
    a, la = _take(e.predict(x, y, max_rows=max_rows))
    b, lb = _take(e.predict(x, y, max_rows=max_rows))
    assert torch.equal(_bits(a), _bits(b)) and torch.equal(_bits(la), _bits(lb))
    ref = float(cs["gold"]["fwd_disc"])
    assert abs(float(la) - ref) <= TOL * max(abs(ref), 1e-3)


# ----------------------------------------------------------------------------------- 6. it leaves training alone
def test_predict_leaves_plans_gradients_and_parameters_alone():
    cs = cases.load_case("klef_b32_t20")
    e, w = _engine(cs["cfgs"])
    x, y = _xy(cs)
    e.forward(x, y, train=True, want_xhat=False)
    plan = e.plan(20, 32)
    keys = set(e._plans)
    serial, consumed = plan.fwd_serial, plan.consumed
    before = [plan.workspace.clone(), e.grads.clone(), e.params.clone()]
    big = cases.load_case("klef_b229_t20")
    xb, yb = _xy(big)
    e.predict(x, y)
    e.predict(xb, yb)
    torch.cuda.synchronize()
    for a, b in zip(before, [plan.workspace, e.grads, e.params]):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    assert set(e._plans) == keys and (plan.fwd_serial, plan.consumed) == (serial, consumed)
    e.backward(x, y, stage=0)
    m = O.build("kl_ef", cs["cfgs"])
    O.load_numpy_weights(m, w)
    m.train()
    torch.set_num_threads(4)
    O.loss_terms(m, torch.from_numpy(cs["x"]), torch.from_numpy(cs["y"]), cs["cfg"], cs["loss_kind"])["loss"].backward()
    gv = e.grad_views()
    worst = max(grad_err(gv[n].cpu().numpy(), p.grad.numpy()) for n, p in m.named_parameters())
    assert worst < TOL, worst


# ----------------------------------------------------------------------------------- 7. capture
def _tail_setup():
    import factorized_amd.optim as optim
    from factorized_amd.checkpoint import KeepBest
    from factorized_amd.lr_scheduler import ReduceLROnPlateau
    cs = cases.load_case("klef_b33_t7")
    model = _model(cs["cfgs"])
    x, y = _xy(cs)
    lr = torch.tensor([1e-3], device="cuda")
    optimizer = optim.Adam(model.parameters(), lr=lr, capturable=True)
    model.engine
    scheduler = ReduceLROnPlateau(optimizer, "min", patience=0)
    best = KeepBest(model)
    return model, x, y, scheduler, best


def test_epoch_tail_in_one_captured_graph():
    model, x, y, scheduler, best = _tail_setup()
    loss = model.evaluate(x, y)                          # warm-up: buffers, code objects, the consumers' state blocks
    scheduler.step(loss)
    best.update(loss)
    assert scheduler.last_path == "device" and best.last_path == "flat"
    torch.cuda.synchronize()
    epoch0, calls0 = scheduler.last_epoch, best.calls
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        gloss = model.evaluate(x, y)
        scheduler.step(gloss)
        best.update(gloss)
    assert gloss.dim() == 0 and gloss.is_cuda and not gloss.requires_grad
    graph.replay()
    torch.cuda.synchronize()
    first = gloss.clone()
    assert torch.equal(_bits(first), _bits(model.evaluate(x, y).clone()))
    with torch.no_grad():
        model.fy_to_y_fc2.bias.add_(0.25)                # in place: the graph reads the same storage
    graph.replay()
    torch.cuda.synchronize()
    second = gloss.clone()
    assert not torch.equal(_bits(first), _bits(second))
    assert torch.equal(_bits(second), _bits(model.evaluate(x, y).clone()))
    assert scheduler.last_epoch == epoch0 + 2 and best.calls == calls0 + 2


def test_no_allocation_and_no_synchronisation_after_the_first_call():
    model, x, y, scheduler, best = _tail_setup()
    for _ in range(2):
        loss = model.evaluate(x, y)
        scheduler.step(loss)
        best.update(loss)
        model.predict(x)
    torch.cuda.synchronize()
    allocated = torch.cuda.memory_allocated()
    count = torch.cuda.memory_stats()["allocation.all.allocated"]
    torch.cuda.set_sync_debug_mode("error")
    try:
        for _ in range(20):
            loss = model.evaluate(x, y)
            scheduler.step(loss)
            best.update(loss)
            model.predict(x)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    del loss
    assert torch.cuda.memory_allocated() <= allocated
    assert torch.cuda.memory_stats()["allocation.all.allocated"] == count


# ----------------------------------------------------------------------------------- 8. fallbacks
def test_wide_hidden_size_falls_back_and_the_entry_names_the_size():
    cfgs = configs.canonical_configs(dropout=False, zv_size=96)           # ef encoder h = 32 + 8 + 96 = 136 > 128
    cfg = cfgs[0]
    B, T = 5, 3
    xn, yn = synth.make_batch(cfg["input_dims"], B, T, seed=21, output_dim=cfg["output_dim"])
    x, y = torch.from_numpy(xn).cuda(), torch.from_numpy(yn).cuda()
    e, w = _engine(cfgs)
    out = e.predict(x, y)
    m = O.build("kl_ef", cfgs)
    O.load_numpy_weights(m, w)
    m.eval()
    with torch.no_grad():
        ref = m(torch.from_numpy(xn))[0][3].numpy()
    assert rel_err(out["y_hat"].cpu().numpy(), ref) < TOL
    want = float(np.abs(ref.astype(np.float64) - yn.reshape(B, -1)).mean())
    assert out["loss"].dim() == 0 and out["loss"].is_cuda
    assert abs(float(out["loss"]) - want) <= TOL * max(abs(want), 1e-3)
    ws = torch.empty(1 << 16, device="cuda")
    y_hat = torch.empty(B, cfg["output_dim"], device="cuda")
    rc = _call_abi(e, x, None, ws, y_hat, None, 0)
    assert rc == _lib.MFM_ERR_UNSUPPORTED
    assert b"136" in _lib.lib().mfm_last_error()


@pytest.mark.parametrize("name,cls", [("kl_b32_t20", "MFM_KL"), ("mmd_b32_t20", "MFM")])
def test_mfn_classes_predict_through_the_eval_forward(name, cls):
    cs = cases.load_case(name)
    model = _model(cs["cfgs"], cls)
    x, y = _xy(cs)
    if cs["variant"] == "mmd":
        cfg = cs["cfg"]
        g = torch.from_numpy(np.ascontiguousarray(cs["gold"]["mmd_gauss"]))
        model.mmd_gauss = [t.cuda() for t in torch.split(g, [cfg["zl_size"], cfg["za_size"], cfg["zv_size"], cfg["zy_size"]], dim=1)]
    model.eval()
    with torch.no_grad():
        ref = model(x)[0][3].clone()
    got = model.predict(x)
    assert torch.equal(_bits(got), _bits(ref))
    loss = model.evaluate(x, y)
    assert loss.dim() == 0 and loss.is_cuda and not loss.requires_grad
    want = float(torch.nn.L1Loss()(ref, y.view_as(ref)))
    assert abs(float(loss) - want) <= TOL * max(abs(want), 1e-3)


# ----------------------------------------------------------------------------------- 9. module surface
def test_module_surface():
    cs = cases.load_case("klef_b33_t7")
    model = _model(cs["cfgs"])
    x, y = _xy(cs)
    model.eval()
    with torch.no_grad():
        ref = model(x)[0][3].clone()
    got = model.predict(x).clone()
    assert rel_err(got.cpu().numpy(), ref.cpu().numpy()) < TOL
    loss = model.evaluate(x, y)
    assert loss.dim() == 0 and loss.is_cuda and not loss.requires_grad
    ref_loss = float(cs["gold"]["fwd_disc"])
    assert abs(float(loss) - ref_loss) <= TOL * max(abs(ref_loss), 1e-3)
    mse = model.evaluate(x, y.view(33, -1), loss_fn=torch.nn.MSELoss())
    assert torch.equal(_bits(mse), _bits(torch.nn.MSELoss()(model.predict(x), y.view(33, -1))))
    buf = io.BytesIO()
    torch.save(model, buf)
    buf.seek(0)
    back = torch.load(buf, weights_only=False)
    assert torch.equal(_bits(back.predict(x)), _bits(got))
    with pytest.raises(_lib.MfmError):
        model.predict(x.cpu())
    with pytest.raises(_lib.MfmError):
        model.evaluate(x, y.double())


# ----------------------------------------------------------------------------------- four-row tiles
def test_four_row_tiles_from_six_workgroups_per_cu_on():
    """a chunk of 6 * CUs rows or more runs on four-row tiles (the rule of the training recurrences); N = 6 * CUs + 1 leaves
    the last tile with one row.  Against the same split in chunks of 512 rows (one-row tiles)."""
    cfgs = configs.canonical_configs(dropout=False)
    cfg = cfgs[0]
    e, _ = _engine(cfgs)
    N, T = 6 * _lib.lib().mfm_device_cus() + 1, 2
    xn, yn = synth.make_batch(cfg["input_dims"], N, T, seed=11, output_dim=cfg["output_dim"])
    x, y = torch.from_numpy(xn).cuda(), torch.from_numpy(yn).cuda()
    one, l1 = _take(e.predict(x, y, max_rows=512))
    four, l4 = _take(e.predict(x, y, max_rows=N))
    again, l4b = _take(e.predict(x, y, max_rows=N))
    assert rel_err(four.cpu().numpy(), one.cpu().numpy()) < TOL
    assert abs(float(l4) - float(l1)) <= TOL * max(abs(float(l1)), 1e-3)
    assert torch.equal(_bits(four), _bits(again)) and torch.equal(_bits(l4), _bits(l4b))
    want = float(np.abs(one.cpu().numpy().astype(np.float64) - yn.reshape(N, -1)).mean())
    assert abs(float(l4) - want) <= TOL * max(abs(want), 1e-3)
