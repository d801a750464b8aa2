"""predict / evaluate of the ablations M_B and M_D (mfm_predict_ablation, csrc/ablation.hip) on the MI355X: y_hat, the three
reconstruction errors and the label loss against the oracle in eval mode and the reference's own output summaries; edges, row
chunks, four-row tiles, odd hidden sizes, the arrival tickets (repeat calls, graph replays, the epoch tail), containment,
unaligned x, the composed path and allocation.  Numeric bounds: the project's 1e-4 relative fp32 tolerance against the oracle
(scalars against float64 reductions of the oracle's outputs), 5e-4 against the golden summaries.

Cross-entropy labels need more than one class and the committed fixtures were generated with output_dim = 1, so the `ce` parity
cases run a model of the fixture's sizes with output_dim = 3 on the fixture's x, against the oracle alone."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import mfm_oracle_extra as X
from factorized_amd import _lib, configs, synth
from tests import cases, offset_views
from tests.cases import rel_err
from tests.extra_cases import EXTRA_SIZES, SIZES, load_extra

pytestmark = pytest.mark.gpu
TOL = 1e-4
CANARY = 0x7FC0DEAD                   # a NaN with a payload: any store over it shows
CLASSES = ("M_B", "M_D")
FAMILY = {"M_B": 0, "M_D": 1}


def _pair(name, cfgs, seed=1234):
    """(model on the GPU, oracle in eval mode) with the same synthetic weights"""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from factorized_amd import mfm_model as M
    ref = X.CLASSES[name](*cfgs)
    w = synth.make_weights({k: tuple(v.shape) for k, v in ref.state_dict().items()}, seed=seed)
    ref.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in w.items()})
    ref.eval()
    model = getattr(M, name)(*cfgs)
    model.load_state_dict(ref.state_dict())
    return model.cuda(), ref


def _want(ref, name, x, y, loss="l1"):
    """(y_hat, gen [3] or None, disc or None) of the oracle's eval forward: the scalars as float64 reductions of its outputs"""
    with torch.no_grad():
        out = ref.forward(x)[0]
    y_hat = out[3]
    gen = None
    if name == "M_B":
        gen = [float(F.mse_loss(xh.double(), xm.double())) for xh, xm in zip(out[:3], ref._split(x))]
    disc = None
    if y is not None:
        disc = float(F.l1_loss(y_hat.double(), y.double()) if loss == "l1" else F.cross_entropy(y_hat.double(), y))
    return y_hat, gen, disc


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _same(a, b):
    assert len(a) == len(b)
    return all((p is None and q is None) or (p is not None and q is not None and torch.equal(_bits(p), _bits(q))) for p, q in zip(a, b))


def _keep(r):
    """predict reuses its output buffers: keep copies"""
    return type(r)(*[None if t is None else t.clone() for t in r])


def _check(got, want, what, gen=True):
    y_hat, wgen, disc = want
    if not gen:
        wgen = None
    assert (got.gen is None) == (wgen is None) and (got.disc is None) == (disc is None), what
    assert tuple(got.y_hat.shape) == tuple(y_hat.shape), what
    assert got.y_hat.dtype == torch.float32 and got.y_hat.is_cuda and not got.y_hat.requires_grad
    err = rel_err(got.y_hat.cpu().numpy(), y_hat.numpy())
    print("ablation %s y_hat %.3e" % (what, err))
    assert err < TOL, (what, err)
    if wgen is not None:
        assert tuple(got.gen.shape) == (3,) and got.gen.dtype == torch.float32 and got.gen.is_cuda
        for m, g, w in zip("lav", got.gen.tolist(), wgen):
            err = abs(g - w) / max(abs(w), 1e-30)
            print("ablation %s gen_%s %.6e want %.6e err %.3e" % (what, m, g, w, err))
            assert err < TOL, (what, m, g, w)
    if disc is not None:
        assert got.disc.dim() == 0 and got.disc.dtype == torch.float32 and got.disc.is_cuda
        err = abs(float(got.disc) - disc) / max(abs(disc), 1e-30)
        print("ablation %s disc %.6e want %.6e err %.3e" % (what, float(got.disc), disc, err))
        assert err < TOL, (what, float(got.disc), disc)


def _labels(N, od, seed=5):
    return torch.from_numpy(np.random.RandomState(seed).standard_normal((N, od)).astype(np.float32))


def _classes(N, od, seed=6):
    return torch.from_numpy(np.random.RandomState(seed).randint(0, od, size=N).astype(np.int64))


_SHARED = {}


def _case(name, size):
    """a parity case with its model, the oracle, labels, the oracle's numbers and the uncapped result, computed once"""
    key = (name, size)
    if key not in _SHARED:
        cfgs, gold, xn, _ = load_extra(name, size)
        model, ref = _pair(name, cfgs)
        torch.set_num_threads(4)
        xc = torch.from_numpy(xn)
        yc = _labels(xc.shape[1], cfgs[0]["output_dim"])
        x, y = xc.cuda(), yc.cuda()
        _SHARED[key] = dict(cfgs=cfgs, cfg=cfgs[0], gold=gold, xc=xc, yc=yc, x=x, y=y, model=model, ref=ref, want=_want(ref, name, xc, yc),
                            full=_keep(model.predict(x, y)))
    return _SHARED[key]


def _fresh(name, s, N, T, seed):
    """a batch of another shape for the model of a shared case, and the oracle's numbers for it"""
    xn, _ = synth.make_batch(s["cfg"]["input_dims"], N, T, seed=seed)
    xc, yc = torch.from_numpy(xn), _labels(N, s["cfg"]["output_dim"], seed=seed + 1)
    return xc.cuda(), yc.cuda(), _want(s["ref"], name, xc, yc)


# ----------------------------------------------------------------------------------- 1. against the oracle and the reference
@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("name", CLASSES)
def test_l1_matches_the_oracle_and_the_reference_golden(name, size):
    s = _case(name, size)
    N, od = s["xc"].shape[1], s["cfg"]["output_dim"]
    assert tuple(s["xc"].shape[:2]) == ((6, 12) if size == "small" else (20, 33))
    assert tuple(s["full"].y_hat.shape) == (N, od)
    _check(s["full"], s["want"], "%s %s" % (name, size))
    # row 3 of out_summary: y_hat of the flattened forward outputs (generated with dropout 0: train mode equals eval)
    gold = s["gold"]["out_summary"]
    got = cases.summarize(s["full"].y_hat.cpu().numpy())
    err = float(np.max(np.abs(got - gold[3]) / max(abs(gold[3, 0]), 1e-6)))
    print("ablation golden %s %s %.3e" % (name, size, err))
    assert err < 5 * TOL, err


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("name", CLASSES)
def test_cross_entropy_matches_the_oracle(name, size):
    s = _case(name, size)
    sizes = {k: s["cfg"][k] for k in EXTRA_SIZES}
    cfgs = configs.canonical_configs(dropout=False, output_dim=3, **sizes)
    model, ref = _pair(name, cfgs)
    N = s["xc"].shape[1]
    yc = _classes(N, 3)
    y = yc.cuda()
    want = _want(ref, name, s["xc"], yc, loss="ce")
    got = _keep(model.predict(s["x"], y, loss="ce"))
    _check(got, want, "%s %s ce" % (name, size))
    _check(model.predict(s["x"], y, loss="ce", max_rows=5), want, "%s %s ce chunks" % (name, size))
    assert torch.equal(_bits(model.evaluate(s["x"], y, loss="ce")), _bits(got.disc))
    with pytest.raises(_lib.MfmError, match="int64 class indices"):
        model.predict(s["x"], y.float(), loss="ce")
    with pytest.raises(_lib.MfmError, match="float labels"):
        model.predict(s["x"], y, loss="l1")


# ----------------------------------------------------------------------------------- 2. evaluate, gen or not, labels or not, M_D
@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("name", CLASSES)
def test_evaluate_and_the_label_path_keep_the_bits_of_predict(name, size):
    s = _case(name, size)
    model, x, y = s["model"], s["x"], s["y"]
    nogen = _keep(model.predict(x, y, gen=False))
    assert nogen.gen is None and _same((nogen.y_hat, nogen.disc), (s["full"].y_hat, s["full"].disc))
    ev = model.evaluate(x, y)
    assert ev.dim() == 0 and ev.is_cuda and torch.equal(_bits(ev), _bits(nogen.disc))
    nolab = model.predict(x)
    assert nolab.disc is None and _same((nolab.y_hat, nolab.gen), (s["full"].y_hat, s["full"].gen))


def test_m_d_has_no_gen():
    s = _case("M_D", "small")
    assert s["full"].gen is None
    got = s["model"].predict(s["x"], s["y"], gen=True)
    assert got.gen is None and _same((got.y_hat, got.disc), (s["full"].y_hat, s["full"].disc))
    assert all(k[2] is False for k in s["model"]._ablation_bufs)          # (one cache entry whatever `gen` says)
    assert tuple(_case("M_B", "small")["full"].gen.shape) == (3,)


# ----------------------------------------------------------------------------------- 3. edges, chunks, four-row tiles, odd sizes
@pytest.mark.parametrize("T,N", [(1, 1), (6, 1)], ids=["T1N1", "T6N1"])
@pytest.mark.parametrize("name", CLASSES)
def test_edges_against_the_oracle(name, T, N):
    s = _case(name, "small")
    x, y, want = _fresh(name, s, N, T, seed=31)
    _check(s["model"].predict(x, y), want, "%s T%d N%d" % (name, T, N))
    _check(s["model"].predict(x, y, gen=False), want, "%s T%d N%d label path" % (name, T, N), gen=False)


@pytest.mark.parametrize("name", CLASSES)
def test_row_chunks_of_5_5_and_2(name):
    """N = 12 with max_rows = 5: y_hat keeps the bits of the uncapped call, gen / disc differ in the grouping of the fp64 sums"""
    s = _case(name, "small")
    assert s["x"].shape[1] == 12
    got = _keep(s["model"].predict(s["x"], s["y"], max_rows=5))
    assert _same((got.y_hat,), (s["full"].y_hat,))
    for a, b in ((got.gen, s["full"].gen), (got.disc, s["full"].disc)):
        assert (a is None) == (b is None)
        if a is not None:
            assert bool(((a.double() - b.double()).abs() <= TOL * b.double().abs()).all()), (a, b)
    _check(got, s["want"], "%s chunks of 5" % name)
    assert torch.equal(_bits(s["model"].evaluate(s["x"], s["y"], max_rows=5)), _bits(got.disc))


@pytest.mark.parametrize("name", CLASSES)
def test_four_row_tiles_with_a_ragged_last_tile(name):
    """T = 2 at three rows past the smallest N for which the library reports four-row tiles (so N mod 4 != 0); against the
    oracle, and against chunks of 32 rows (one-row tiles)"""
    s = _case(name, "small")
    L = _lib.lib()
    gen = int(name == "M_B")
    tr = (C.c_int32 * 2)()
    N0 = None
    for n in range(1, 4097):
        assert L.mfm_predict_ablation_tile_rows(n, FAMILY[name], gen, 0, tr) == 0
        if tr[0] == 4:
            N0 = n
            break
    assert N0 is not None, "no N up to 4096 reaches the four-row form on %d CUs" % L.mfm_device_cus()
    N = N0 + 3
    assert N % 4 and N0 % 4 == 0
    assert L.mfm_predict_ablation_tile_rows(N, FAMILY[name], gen, N, tr) == 0 and list(tr) == [4, 4 * gen]
    assert L.mfm_predict_ablation_tile_rows(N, FAMILY[name], gen, 32, tr) == 0 and list(tr) == [1, gen]
    x, y, want = _fresh(name, s, N, 2, seed=11)
    four = _keep(s["model"].predict(x, y, max_rows=N))
    _check(four, want, "%s four-row N%d" % (name, N))
    _check(s["model"].predict(x, y, max_rows=32), want, "%s one-row N%d" % (name, N))
    assert _same(four, s["model"].predict(x, y, max_rows=N))


@pytest.mark.parametrize("sizes", [dict(fa_size=1), dict(zl_size=3, za_size=5, zv_size=7)], ids=["fa1", "z357"])
@pytest.mark.parametrize("name", CLASSES)
def test_hidden_sizes_that_are_no_multiple_of_4(name, sizes):
    """the concatenated f row at odd offsets (fa = 1), and recurrences whose hidden size is odd"""
    s = _case(name, "small")
    cfgs = configs.canonical_configs(dropout=False, **dict(EXTRA_SIZES, **sizes))
    model, ref = _pair(name, cfgs)
    want = _want(ref, name, s["xc"], s["yc"])
    got = _keep(model.predict(s["x"], s["y"]))
    _check(got, want, "%s %s" % (name, sorted(sizes.items())))
    assert _same((got.y_hat,), (model.predict(s["x"], s["y"], max_rows=5).y_hat,))
    assert model._ablation_bufs and all(v is not False for v in model._ablation_bufs.values())      # (the entry took them)


# ----------------------------------------------------------------------------------- 4. the tickets
def _ticket_words(model, key):
    """the ticket words of a cached workspace: round_up(rows, 4) per-tile words, then (behind the fp64 sum) the chunk's"""
    ws = model._ablation_bufs[key][0].view(torch.int32)
    rows = min(key[1], key[4])
    n = (rows + 3) // 4 * 4
    return torch.cat([ws[-(n + 4):-4], ws[-2:-1]])


@pytest.mark.parametrize("name", CLASSES)
def test_two_calls_are_bit_equal_and_leave_the_tickets_at_zero(name):
    s = _case(name, "small")
    model, x, y = s["model"], s["x"], s["y"]
    a = _keep(model.predict(x, y))
    b = model.predict(x, y)
    assert _same(a, b) and _same(a, s["full"])
    for key in model._ablation_bufs:
        assert int(_ticket_words(model, key).abs().sum()) == 0, key


@pytest.mark.parametrize("name", CLASSES)
def test_three_replays_of_a_captured_call_give_the_eager_bits(name):
    s = _case(name, "small")
    model, _ = _pair(name, s["cfgs"])
    x, y = s["x"], s["y"]
    T, N = x.shape[:2]
    xin = x.clone()
    model.predict(xin, y, max_rows=5)                        # warm-up: buffers, code objects
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        g = model.predict(xin, y, max_rows=5)
    xn, _ = synth.make_batch(s["cfg"]["input_dims"], N, T, seed=23)
    x2 = torch.from_numpy(xn).cuda()
    eager2 = _keep(model.predict(x2, y, max_rows=5))
    eager1 = _keep(model.predict(x, y, max_rows=5))
    assert not _same(eager1, eager2)
    key = [k for k in model._ablation_bufs][0]
    for src, want in ((x2, eager2), (x, eager1), (x2, eager2)):
        xin.copy_(src)
        for t in g:
            if t is not None:
                t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert _same(g, want)
        assert int(_ticket_words(model, key).abs().sum()) == 0


def _epoch_tail(name):
    import factorized_amd.optim as optim
    from factorized_amd.checkpoint import KeepBest
    from factorized_amd.lr_scheduler import ReduceLROnPlateau
    s = _case(name, "canonical")
    model, _ = _pair(name, s["cfgs"])
    lr = torch.tensor([1e-3], device="cuda")
    optimizer = optim.Adam(model.parameters(), lr=lr, capturable=True)
    return s, model, ReduceLROnPlateau(optimizer, "min", patience=0), KeepBest(model)


@pytest.mark.parametrize("name", CLASSES)
def test_evaluate_and_the_scheduler_step_in_one_captured_graph(name):
    """evaluate -> ReduceLROnPlateau.step as one graph, the loss never on the host; KeepBest.update takes the replayed device loss
    behind the graph, on its torch path"""
    s, model, scheduler, best = _epoch_tail(name)
    x, y = s["x"].clone(), s["y"]
    x2n, _ = synth.make_batch(s["cfg"]["input_dims"], x.shape[1], x.shape[0], seed=77)
    x2 = torch.from_numpy(x2n).cuda()
    loss = model.evaluate(x, y)                              # warm-up: buffers, code objects, the scheduler's state block
    scheduler.step(loss)
    torch.cuda.synchronize()
    assert scheduler.last_path == "device"
    want1 = _bits(loss)
    assert torch.equal(want1, _bits(s["full"].disc))
    want2 = _bits(model.evaluate(x2, y))
    assert not torch.equal(want1, want2)
    epoch0 = scheduler.last_epoch
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        gloss = model.evaluate(x, y)
        scheduler.step(gloss)
    for i, (src, want) in enumerate(((x2, want2), (s["x"], want1), (x2, want2))):
        x.copy_(src)
        gloss.zero_()
        graph.replay()
        best.update(gloss)
        torch.cuda.synchronize()
        assert torch.equal(_bits(gloss), want)
    assert scheduler.last_epoch == epoch0 + 3 and best.calls == 3
    assert best.value == min(float(want1.view(torch.float32)), float(want2.view(torch.float32)))


@pytest.mark.parametrize("name", CLASSES)
def test_epoch_tail_in_one_captured_graph(name):
    """evaluate -> ReduceLROnPlateau.step -> KeepBest.update in ONE graph; three replays with other weights and other contents
    copied into x give the eager call's bits each time, the tickets are back at 0 between them, and KeepBest keeps the weights of the best replay
    (a composed module: its captured update works on the state block and the buffers the warm-up call left beside the model)"""
    s, model, scheduler, best = _epoch_tail(name)
    x, y = s["x"].clone(), s["y"]
    x2n, _ = synth.make_batch(s["cfg"]["input_dims"], x.shape[1], x.shape[0], seed=77)
    x2 = torch.from_numpy(x2n).cuda()
    loss = model.evaluate(x, y)                              # warm-up: buffers, code objects, the consumers' state blocks
    scheduler.step(loss)
    best.update(loss)
    torch.cuda.synchronize()
    assert scheduler.last_path == "device" and best.last_path == "torch"
    want1 = _bits(loss)
    assert torch.equal(want1, _bits(s["full"].disc))
    want2 = _bits(model.evaluate(x2, y))
    assert not torch.equal(want1, want2)
    v1 = float(want1.view(torch.float32))
    epoch0, calls0 = scheduler.last_epoch, best.calls
    assert calls0 == 1 and best.value == v1
    key = list(model._ablation_bufs)[0]
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        gloss = model.evaluate(x, y)
        scheduler.step(gloss)
        took = best.update(gloss)
    assert best.last_path == "tensors"
    p0 = next(model.parameters())
    marks, seen = [p0.detach().clone()], [v1]
    for i, src in enumerate((x2, s["x"], x2)):
        with torch.no_grad():
            p0.add_(0.01)                                    # (other weights every epoch: the snapshot tells which one was kept)
        marks.append(p0.detach().clone())
        want = _bits(model.evaluate(src, y))
        assert want.item() not in (want1.item(), want2.item())
        x.copy_(src)
        gloss.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(_bits(gloss), want), i
        assert int(_ticket_words(model, key).abs().sum()) == 0
        assert int(took) == int(_fp(gloss) <= min(seen)), (i, float(gloss), seen)
        seen.append(_fp(gloss))
    assert scheduler.last_epoch == epoch0 + 3 and best.calls == calls0 + 3
    assert best.value == min(seen)
    last_take = max(i for i in range(4) if i == 0 or seen[i] <= min(seen[:i]))      # (call 0: the warm-up's snapshot)
    assert best.epoch == last_take
    best.restore()
    assert torch.equal(_bits(p0), _bits(marks[last_take]))


def _fp(t):
    return float(t.detach().cpu())


# ----------------------------------------------------------------------------------- 5. containment
def _canary(n, pad=256):
    big = torch.full((pad + n + pad,), CANARY, dtype=torch.int32, device="cuda")
    return big, big[pad:pad + n].view(torch.float32)


def _intact(big, n, pad=256):
    return bool((big[:pad] == CANARY).all()) and bool((big[pad + n:] == CANARY).all())


@pytest.mark.parametrize("gen,cap", [(1, 0), (1, 5), (0, 5)])
@pytest.mark.parametrize("name", CLASSES)
def test_canaries_around_workspace_outputs_and_parameters(name, gen, cap):
    """the entry through the C ABI on caller-owned, canary-framed buffers, the parameters copied into one framed block: nothing
    outside the workspace and the outputs is touched, parameters and x keep their bits, the results are the module's"""
    s = _case(name, "small")
    model, x, y = s["model"], s["x"], s["y"]
    fam = FAMILY[name]
    gen = gen if fam == 0 else 0
    T, N = x.shape[:2]
    L = _lib.lib()
    sz = model._ablation_sizes()
    sizes = (C.c_int32 * 12)(*sz)
    nws = int(L.mfm_predict_ablation_workspace_floats(T, N, sizes, fam, gen, 1, cap))
    assert nws > 0
    big_ws, ws = _canary(nws)
    ny = N * sz[11]
    (big_y, y_hat), (big_g, gen_out), (big_d, disc) = _canary(ny), _canary(3), _canary(1)
    # every parameter on a 16-byte boundary of one block, canaries in the gaps and around
    params = model._ablation_params(bool(gen))
    offs, total = [], 0
    for p in params:
        offs.append(total)
        total += 0 if p is None else (p.numel() + 3) // 4 * 4 + 4
    big_p, block = _canary(total)
    for p, o in zip(params, offs):
        if p is not None:
            block[o:o + p.numel()].copy_(p.detach().reshape(-1))
    before = big_p.clone()
    xk = x.clone()
    prm = (C.c_void_p * 52)(*[None if p is None else block.data_ptr() + 4 * o for p, o in zip(params, offs)])
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = L.mfm_predict_ablation(T, N, sizes, fam, 0, gen, prm, C.c_void_p(xk.data_ptr()), C.c_void_p(y.data_ptr()), C.c_void_p(ws.data_ptr()),
                                C.c_void_p(y_hat.data_ptr()), C.c_void_p(gen_out.data_ptr()) if gen else None, C.c_void_p(disc.data_ptr()),
                                cap, stream)
    assert rc == 0, L.mfm_last_error().decode()
    torch.cuda.synchronize()
    assert _intact(big_ws, nws) and _intact(big_y, ny) and _intact(big_g, 3) and _intact(big_d, 1)
    assert torch.equal(big_p, before) and torch.equal(_bits(xk), _bits(x))
    if not gen:
        assert bool((big_g == CANARY).all())
    assert torch.equal(_bits(y_hat), _bits(s["full"].y_hat.reshape(-1)))
    pairs = [(disc[0], s["full"].disc)] + ([(gen_out, s["full"].gen)] if gen else [])
    for a, b in pairs:
        if cap == 0:
            assert torch.equal(_bits(a), _bits(b))
        else:
            assert rel_err(a.cpu().numpy(), b.cpu().numpy()) < TOL
    n = (min(N, cap or N) + 3) // 4 * 4
    assert int(ws.view(torch.int32)[-(n + 4):-4].abs().sum()) == 0 and int(ws.view(torch.int32)[-2]) == 0      # the tickets


# ----------------------------------------------------------------------------------- 6. x off a 16-byte boundary
@pytest.mark.parametrize("name", CLASSES)
def test_an_x_off_a_16_byte_boundary_gives_the_same_bits(name):
    s = _case(name, "small")
    offset_views.forget_views()
    for r in (4, 8, 12):
        view = offset_views.at_residue(s["x"], r)
        assert _same(s["model"].predict(view, s["y"]), s["full"]), r
        assert _same((s["model"].predict(view, s["y"], max_rows=5).y_hat,), (s["full"].y_hat,)), r
    assert offset_views.check_guards() == 3


# ----------------------------------------------------------------------------------- 7. refusal takes the composition
@pytest.mark.parametrize("name", CLASSES)
def test_a_hidden_size_of_136_takes_the_composed_path(name, monkeypatch):
    cfgs = configs.canonical_configs(dropout=False, **dict(EXTRA_SIZES, zl_size=136))
    model, ref = _pair(name, cfgs)
    T, N = 3, 5
    xn, _ = synth.make_batch(cfgs[0]["input_dims"], N, T, seed=21)
    xc, yc = torch.from_numpy(xn), _labels(N, cfgs[0]["output_dim"], seed=22)
    x, y = xc.cuda(), yc.cuda()
    L, calls = _lib.lib(), []
    real = L.mfm_predict_ablation
    monkeypatch.setattr(L, "mfm_predict_ablation", lambda *a: (calls.append(1), real(*a))[1], raising=True)
    want = _want(ref, name, xc, yc)
    _check(model.predict(x, y), want, "%s zl 136" % name)
    assert calls == [1] and model._ablation_refused == {False, True} and not model.__dict__.get("_ablation_bufs")
    _check(model.predict(x, y, gen=False), want, "%s zl 136 label path" % name, gen=False)
    ev = model.evaluate(x, y)
    assert abs(float(ev) - want[2]) < TOL * abs(want[2])
    assert calls == [1] and not model.__dict__.get("_ablation_bufs")      # (remembered: no second call into the entry)


@pytest.mark.parametrize("name", CLASSES)
def test_a_refusal_for_one_shape_is_remembered(name, monkeypatch):
    s = _case(name, "small")
    model, _ = _pair(name, s["cfgs"])
    L, calls = _lib.lib(), []
    monkeypatch.setattr(L, "mfm_predict_ablation", lambda *a: (calls.append(1), _lib.MFM_ERR_UNSUPPORTED)[1], raising=True)
    for _ in range(2):
        _check(model.predict(s["x"], s["y"]), s["want"], "%s refused shape, composed" % name)
        assert calls == [1] and not model.__dict__.get("_ablation_refused") and list(model._ablation_bufs.values()) == [False]


# ----------------------------------------------------------------------------------- 8. no allocation after the first call
@pytest.mark.parametrize("name", CLASSES)
def test_no_allocation_and_no_synchronisation_after_the_first_call(name):
    s = _case(name, "small")
    model, x, y = s["model"], s["x"], s["y"]
    for _ in range(2):
        model.predict(x, y)
        model.evaluate(x, y)
    torch.cuda.synchronize()
    allocated = torch.cuda.memory_allocated()
    count = torch.cuda.memory_stats()["allocation.all.allocated"]
    torch.cuda.set_sync_debug_mode("error")
    try:
        for _ in range(5):
            model.predict(x, y)
            model.evaluate(x, y)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.cuda.memory_allocated() == allocated
    assert torch.cuda.memory_stats()["allocation.all.allocated"] == count


# ----------------------------------------------------------------------------------- 9. errors, and what a call leaves alone
@pytest.mark.parametrize("name", CLASSES)
def test_errors_reach_no_kernel_and_training_is_left_as_found(name, monkeypatch):
    s = _case(name, "small")
    model, x, y = s["model"], s["x"], s["y"]
    L, calls = _lib.lib(), []
    real = L.mfm_predict_ablation
    monkeypatch.setattr(L, "mfm_predict_ablation", lambda *a: (calls.append(1), real(*a))[1], raising=True)
    bufs = dict(model._ablation_bufs)
    with pytest.raises(_lib.MfmError, match="features per time step"):
        model.predict(x[:, :, :-1], y)
    with pytest.raises(_lib.MfmError, match="input is on cpu"):
        model.predict(x.cpu(), y)
    with pytest.raises(_lib.MfmError, match="empty split"):
        model.predict(x[:, :0], y)
    with pytest.raises(_lib.MfmError, match="max_rows"):
        model.evaluate(x, y, max_rows=0)
    with pytest.raises(ValueError, match="'l1' or 'ce'"):
        model.predict(x, y, loss="l2")
    with pytest.raises(_lib.MfmError, match="float labels"):
        model.predict(x, y[:-1])
    with pytest.raises(_lib.MfmError, match="labels must be a tensor on"):
        model.evaluate(x, y.cpu())
    assert not calls and model._ablation_bufs == bufs        # the entry was not reached, nothing was allocated
    model.train()
    got = model.predict(x, y)
    assert model.training and all(mod.training for mod in model.modules())
    model.eval()
    assert calls == [1] and _same(got, s["full"])            # (eval computation whatever the mode)
    assert all(p.grad is None for p in model.parameters()) and not [k for k in model.state_dict() if "ablation" in k]
