"""predict / evaluate of the ablations M_A and M_C (mfm_predict_ablation_mfn, csrc/ablation_mfn.hip) on the MI355X: y_hat, the
three reconstruction errors and the label loss against the oracle in eval mode and the reference's own output summaries; edges,
row chunks, four-row tiles, seams of the embedding block off a multiple of 4, the label path shared with mfm_predict_mfn, the
loss ticket (repeat calls, graph replays, the epoch tail), containment, unaligned x, the composed path and allocation.  Numeric
bounds: the project's 1e-4 relative fp32 tolerance against the oracle (scalars against float64 reductions of the oracle's
outputs), 5e-4 against the golden summaries.

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
CLASSES = ("M_A", "M_C")
FAMILY = {"M_A": 0, "M_C": 1}
NP = 66


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


def _want(ref, x, y, loss="l1"):
    """(y_hat, gen [3], disc or None) of the oracle's eval forward: the scalars as float64 reductions of its outputs"""
    with torch.no_grad():
        out = ref.forward(x)[0]
    y_hat = out[3]
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
    print("ablation mfn %s y_hat %.3e" % (what, err))
    assert err < TOL, (what, err)
    if wgen is not None:
        assert tuple(got.gen.shape) == (3,) and got.gen.dtype == torch.float32 and got.gen.is_cuda
        for m, g, w in zip("lav", got.gen.tolist(), wgen):
            err = abs(g - w) / max(abs(w), 1e-30)
            print("ablation mfn %s gen_%s %.6e want %.6e err %.3e" % (what, m, g, w, err))
            assert err < TOL, (what, m, g, w)
    if disc is not None:
        assert got.disc.dim() == 0 and got.disc.dtype == torch.float32 and got.disc.is_cuda
        err = abs(float(got.disc) - disc) / max(abs(disc), 1e-30)
        print("ablation mfn %s disc %.6e want %.6e err %.3e" % (what, float(got.disc), disc, err))
        assert err < TOL, (what, float(got.disc), disc)


def _labels(N, od, seed=5):
    return torch.from_numpy(np.random.RandomState(seed).standard_normal((N, od)).astype(np.float32))


def _classes(N, od, seed=6):
    return torch.from_numpy(np.random.RandomState(seed).randint(0, od, size=N).astype(np.int64))


def _took_the_entry(model):
    """the entry, not the composed path, served every shape so far"""
    return bool(model._ablation_bufs) and all(v is not False for v in model._ablation_bufs.values()) and not model.__dict__.get("_ablation_refused")


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
        _SHARED[key] = dict(cfgs=cfgs, cfg=cfgs[0], gold=gold, xc=xc, yc=yc, x=x, y=y, model=model, ref=ref, want=_want(ref, xc, yc),
                            full=_keep(model.predict(x, y)))
        assert _took_the_entry(model)
    return _SHARED[key]


def _fresh(s, N, T, seed):
    """a batch of another shape for the model of a shared case, and the oracle's numbers for it"""
    xn, _ = synth.make_batch(s["cfg"]["input_dims"], N, T, seed=seed)
    xc, yc = torch.from_numpy(xn), _labels(N, s["cfg"]["output_dim"], seed=seed + 1)
    return xc.cuda(), yc.cuda(), _want(s["ref"], xc, yc)


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
    print("ablation mfn golden %s %s %.3e" % (name, size, err))
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
    want = _want(ref, s["xc"], yc, loss="ce")
    got = _keep(model.predict(s["x"], y, loss="ce"))
    _check(got, want, "%s %s ce" % (name, size))
    _check(model.predict(s["x"], y, loss="ce", max_rows=5), want, "%s %s ce chunks" % (name, size))
    assert torch.equal(_bits(model.evaluate(s["x"], y, loss="ce")), _bits(got.disc))
    assert _took_the_entry(model)
    with pytest.raises(_lib.MfmError, match="int64 class indices"):
        model.predict(s["x"], y.float(), loss="ce")
    with pytest.raises(_lib.MfmError, match="float labels"):
        model.predict(s["x"], y, loss="l1")


# ----------------------------------------------------------------------------------- 2. evaluate, gen or not, labels or not
@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("name", CLASSES)
def test_evaluate_and_the_label_path_keep_the_bits_of_predict(name, size):
    s = _case(name, size)
    model, x, y = s["model"], s["x"], s["y"]
    nogen = _keep(model.predict(x, y, gen=False))
    assert nogen.gen is None and _same((nogen.y_hat, nogen.disc), (s["full"].y_hat, s["full"].disc))
    _check(nogen, s["want"], "%s %s label path" % (name, size), gen=False)
    ev = model.evaluate(x, y)
    assert ev.dim() == 0 and ev.is_cuda and torch.equal(_bits(ev), _bits(nogen.disc))
    nolab = model.predict(x)
    assert nolab.disc is None and _same((nolab.y_hat, nolab.gen), (s["full"].y_hat, s["full"].gen))


def test_the_label_path_is_the_code_of_mfm_predict_mfn():
    """M_C.predict(gen=False).y_hat has the bits of MFM.predict(label_only=True) of a model with the same MFN, last_to_zy_fc1,
    zy_to_fy and fy_to_y weights (small fixture: one-row tiles in both)"""
    from factorized_amd import mfm_model as M
    s = _case("M_C", "small")
    L = _lib.lib()
    tr = (C.c_int32 * 2)()
    N = s["x"].shape[1]
    assert L.mfm_predict_ablation_mfn_tile_rows(N, 1, 0, 0, tr) == 0 and tr[0] == 1 and L.mfm_predict_mfn_tile_rows(N, 0) == 1
    mfm = M.MFM(*s["cfgs"])
    w = synth.make_weights({k: tuple(v.shape) for k, v in mfm.state_dict().items()}, seed=99)
    sd = {k: torch.from_numpy(v.copy()) for k, v in w.items()}
    shared = {k: v.detach().cpu().clone() for k, v in s["model"].state_dict().items()
              if k.split(".")[0] in ("mfn_encoder", "last_to_zy_fc1", "zy_to_fy_fc1", "zy_to_fy_fc2", "fy_to_y_fc1", "fy_to_y_fc2")}
    assert len(shared) == 12 + 2 * 10 + 10 and all(tuple(sd[k].shape) == tuple(v.shape) for k, v in shared.items())
    sd.update(shared)
    mfm.load_state_dict(sd)
    mfm = mfm.to("cuda")
    want = mfm.predict(s["x"], label_only=True).clone()
    assert mfm.engine.__dict__.get("_predict_mfn_bufs") and not mfm.engine.__dict__.get("_predict_mfn_refused")
    got = s["model"].predict(s["x"], s["y"], gen=False)
    assert torch.equal(_bits(got.y_hat), _bits(want))
    assert torch.equal(_bits(got.disc), _bits(mfm.evaluate(s["x"], s["y"], label_only=True)))


# ----------------------------------------------------------------------------------- 3. edges, chunks, four-row tiles, seams
@pytest.mark.parametrize("T,N", [(1, 1), (6, 1)], ids=["T1N1", "T6N1"])
@pytest.mark.parametrize("name", CLASSES)
def test_edges_against_the_oracle(name, T, N):
    """T = 1: the attention's prev_c half is all zeros"""
    s = _case(name, "small")
    x, y, want = _fresh(s, N, T, seed=31)
    _check(s["model"].predict(x, y), want, "%s T%d N%d" % (name, T, N))
    _check(s["model"].predict(x, y, gen=False), want, "%s T%d N%d label path" % (name, T, N), gen=False)
    assert _took_the_entry(s["model"])


@pytest.mark.parametrize("name", CLASSES)
def test_row_chunks_of_5_5_and_2(name):
    """N = 12 with max_rows = 5: y_hat keeps the bits of the uncapped call, gen / disc differ in the grouping of the fp64 sums"""
    s = _case(name, "small")
    assert s["x"].shape[1] == 12
    got = _keep(s["model"].predict(s["x"], s["y"], max_rows=5))
    assert _same((got.y_hat,), (s["full"].y_hat,))
    for a, b in ((got.gen, s["full"].gen), (got.disc, s["full"].disc)):
        assert bool(((a.double() - b.double()).abs() <= TOL * b.double().abs()).all()), (a, b)
    _check(got, s["want"], "%s chunks of 5" % name)
    assert torch.equal(_bits(s["model"].evaluate(s["x"], s["y"], max_rows=5)), _bits(got.disc))


@pytest.mark.parametrize("name", CLASSES)
def test_four_row_tiles_with_a_ragged_last_tile(name):
    """T = 2 at three rows past the smallest N for which the library reports four-row tiles (so N mod 4 != 0); against the
    oracle, and against chunks of 32 rows (one-row tiles).  Both tile-row outputs are looked at: the recurrence launch's and
    the decoders'"""
    s = _case(name, "small")
    L = _lib.lib()
    fam = FAMILY[name]
    tr = (C.c_int32 * 2)()
    N0 = None
    for n in range(1, 4097):
        assert L.mfm_predict_ablation_mfn_tile_rows(n, fam, 1, 0, tr) == 0
        if tr[0] == 4:
            N0 = n
            break
    assert N0 is not None, "no N up to 4096 reaches the four-row form on %d CUs" % L.mfm_device_cus()
    N = N0 + 3
    assert N % 4 and N0 % 4 == 0
    assert L.mfm_predict_ablation_mfn_tile_rows(N, fam, 1, N, tr) == 0 and list(tr) == [4, 4]
    assert L.mfm_predict_ablation_mfn_tile_rows(N, fam, 0, N, tr) == 0 and list(tr) == [4, 0]
    assert L.mfm_predict_ablation_mfn_tile_rows(N, fam, 1, 32, tr) == 0 and list(tr) == [1, 1]
    x, y, want = _fresh(s, N, 2, seed=11)
    four = _keep(s["model"].predict(x, y, max_rows=N))
    _check(four, want, "%s four-row N%d" % (name, N))
    _check(s["model"].predict(x, y, max_rows=32), want, "%s one-row N%d" % (name, N))
    assert _same(four, s["model"].predict(x, y, max_rows=N))
    nogen = s["model"].predict(x, y, gen=False, max_rows=N)
    assert _same((nogen.y_hat, nogen.disc), (four.y_hat, four.disc))
    assert _took_the_entry(s["model"])


@pytest.mark.parametrize("sizes", [dict(fy_size=5, fl_size=3), dict(fy_size=1), dict(zl_size=7)], ids=["fy5fl3", "fy1", "zl7"])
@pytest.mark.parametrize("name", CLASSES)
def test_seams_off_a_multiple_of_4(name, sizes):
    """fl at an odd column of the embedding block (decoder h = 8 for M_A), a one-column fy, an odd encoder_l"""
    s = _case(name, "small")
    cfgs = configs.canonical_configs(dropout=False, **dict(EXTRA_SIZES, **sizes))
    model, ref = _pair(name, cfgs)
    if sizes.get("fl_size") == 3 and name == "M_A":
        assert model.decoder_l.h == 8
    want = _want(ref, s["xc"], s["yc"])
    got = _keep(model.predict(s["x"], s["y"]))
    _check(got, want, "%s %s" % (name, sorted(sizes.items())))
    assert _same((got.y_hat,), (model.predict(s["x"], s["y"], max_rows=5).y_hat,))
    nogen = model.predict(s["x"], s["y"], gen=False)
    assert _same((nogen.y_hat, nogen.disc), (got.y_hat, got.disc))
    assert _took_the_entry(model)                            # (the entry took them, not the fallback)


# ----------------------------------------------------------------------------------- 4. the ticket
def _ticket_word(model, key):
    """the ticket word of a cached workspace: the third of its last four floats"""
    return int(model._ablation_bufs[key][0].view(torch.int32)[-2])


@pytest.mark.parametrize("name", CLASSES)
def test_two_calls_are_bit_equal_and_leave_the_ticket_at_zero(name):
    s = _case(name, "small")
    model, x, y = s["model"], s["x"], s["y"]
    a = _keep(model.predict(x, y))
    b = model.predict(x, y)
    assert _same(a, b) and _same(a, s["full"])
    labelled = [key for key in model._ablation_bufs if key[3]]      # (a call without labels draws no ticket and clears none)
    assert labelled
    for key in labelled:
        assert _ticket_word(model, key) == 0, key


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
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert _same(g, want)
        assert _ticket_word(model, key) == 0


def _fp(t):
    return float(t.detach().cpu())


@pytest.mark.parametrize("name", CLASSES)
def test_epoch_tail_in_one_captured_graph(name):
    """evaluate -> ReduceLROnPlateau.step -> KeepBest.update in ONE graph; three replays with other weights and other contents
    copied into x give the eager call's bits each time, the ticket is back at 0 between them, and KeepBest keeps the weights of
    the best replay, as the eager sequence would"""
    import factorized_amd.optim as optim
    from factorized_amd.checkpoint import KeepBest
    from factorized_amd.lr_scheduler import ReduceLROnPlateau
    s = _case(name, "canonical")
    model, _ = _pair(name, s["cfgs"])
    lr = torch.tensor([1e-3], device="cuda")
    optimizer = optim.Adam(model.parameters(), lr=lr, capturable=True)
    scheduler, best = ReduceLROnPlateau(optimizer, "min", patience=0), KeepBest(model)
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
    p0 = model.last_to_zy_fc1.weight                         # (on the label path: the first parameter, encoder_l's or a decoder's, is not)
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
        assert _ticket_word(model, key) == 0
        assert int(took) == int(_fp(gloss) <= min(seen)), (i, float(gloss), seen)
        seen.append(_fp(gloss))
    assert scheduler.last_epoch == epoch0 + 3 and best.calls == calls0 + 3
    assert best.value == min(seen)
    last_take = max(i for i in range(4) if i == 0 or seen[i] <= min(seen[:i]))      # (call 0: the warm-up's snapshot)
    assert best.epoch == last_take
    best.restore()
    assert torch.equal(_bits(p0), _bits(marks[last_take]))


# ----------------------------------------------------------------------------------- 5. containment
def _canary(n, pad=256):
    big = torch.full((pad + n + pad,), CANARY, dtype=torch.int32, device="cuda")
    return big, big[pad:pad + n].view(torch.float32)


def _intact(big, n, pad=256):
    return bool((big[:pad] == CANARY).all()) and bool((big[pad + n:] == CANARY).all())


@pytest.mark.parametrize("gen,cap", [(1, 0), (1, 5), (0, 0), (0, 5)])
@pytest.mark.parametrize("name", CLASSES)
def test_canaries_around_workspace_outputs_and_parameters(name, gen, cap):
    """the entry through the C ABI on caller-owned, canary-framed buffers, the parameters copied into one framed block: nothing
    outside the workspace and the outputs is touched, parameters and x keep their bits, the results are the module's.  Without
    gen the tensors of encoder_l, zl_to_fl and the decoders are handed over all the same, filled with NaN: y_hat and disc keep
    their bits, so nothing of them was read"""
    s = _case(name, "small")
    model, x, y = s["model"], s["x"], s["y"]
    fam = FAMILY[name]
    T, N = x.shape[:2]
    L = _lib.lib()
    sz = model._ablation_sizes()
    sizes = (C.c_int32 * 23)(*sz)
    nws = int(L.mfm_predict_ablation_mfn_workspace_floats(T, N, sizes, fam, gen, 1, cap))
    assert nws > 0
    big_ws, ws = _canary(nws)
    ny = N * sz[21]
    (big_y, y_hat), (big_g, gen_out), (big_d, disc) = _canary(ny), _canary(3), _canary(1)
    # every parameter on a 16-byte boundary of one block, canaries in the gaps and around
    params = model._ablation_params(True)
    offs, total = [], 0
    for p in params:
        offs.append(total)
        total += 0 if p is None else (p.numel() + 3) // 4 * 4 + 4
    big_p, block = _canary(total)
    for i, (p, o) in enumerate(zip(params, offs)):
        if p is not None:
            if gen or i < 38:
                block[o:o + p.numel()].copy_(p.detach().reshape(-1))
            else:
                block[o:o + p.numel()].fill_(float("nan"))
    before = big_p.clone()
    xk = x.clone()
    prm = (C.c_void_p * NP)(*[None if p is None else block.data_ptr() + 4 * o for p, o in zip(params, offs)])
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = L.mfm_predict_ablation_mfn(T, N, sizes, fam, gen, prm, C.c_void_p(xk.data_ptr()), C.c_void_p(y.data_ptr()), C.c_void_p(ws.data_ptr()),
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
    assert int(ws.view(torch.int32)[-2]) == 0                # the ticket


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
def test_an_h_dims_entry_of_136_takes_the_composed_path(name, monkeypatch):
    cfgs = configs.canonical_configs(dropout=False, **dict(EXTRA_SIZES, h_dims=[136, 12, 20]))
    model, ref = _pair(name, cfgs)
    T, N = 3, 5
    xn, _ = synth.make_batch(cfgs[0]["input_dims"], N, T, seed=21)
    xc, yc = torch.from_numpy(xn), _labels(N, cfgs[0]["output_dim"], seed=22)
    x, y = xc.cuda(), yc.cuda()
    L, calls = _lib.lib(), []
    real = L.mfm_predict_ablation_mfn
    monkeypatch.setattr(L, "mfm_predict_ablation_mfn", lambda *a: (calls.append(1), real(*a))[1], raising=True)
    want = _want(ref, xc, yc)
    _check(model.predict(x, y), want, "%s h_dims 136" % name)
    assert calls == [1] and model._ablation_refused == {False, True} and not model.__dict__.get("_ablation_bufs")
    _check(model.predict(x, y, gen=False), want, "%s h_dims 136 label path" % name, gen=False)
    ev = model.evaluate(x, y)
    assert abs(float(ev) - want[2]) < TOL * abs(want[2])
    assert calls == [1] and not model.__dict__.get("_ablation_bufs")      # (remembered: no second call into the entry)


@pytest.mark.parametrize("name", CLASSES)
def test_a_decoder_width_of_132_takes_the_composed_path_with_gen_alone(name, monkeypatch):
    """fy + fl = 12 + 120 (M_A) / fy = 132 (M_C): the calls with gen are refused and remembered, the label path stays the entry's"""
    sizes = dict(fl_size=120) if name == "M_A" else dict(fy_size=132)
    cfgs = configs.canonical_configs(dropout=False, **dict(EXTRA_SIZES, **sizes))
    model, ref = _pair(name, cfgs)
    assert model.decoder_l.h == 132
    T, N = 3, 5
    xn, _ = synth.make_batch(cfgs[0]["input_dims"], N, T, seed=21)
    xc, yc = torch.from_numpy(xn), _labels(N, cfgs[0]["output_dim"], seed=22)
    x, y = xc.cuda(), yc.cuda()
    L, calls = _lib.lib(), []
    real = L.mfm_predict_ablation_mfn
    monkeypatch.setattr(L, "mfm_predict_ablation_mfn", lambda *a: (calls.append(1), real(*a))[1], raising=True)
    want = _want(ref, xc, yc)
    for _ in range(2):
        _check(model.predict(x, y), want, "%s decoder 132" % name)
        assert calls == [1] and model._ablation_refused == {True} and not model.__dict__.get("_ablation_bufs")
    _check(model.predict(x, y, gen=False), want, "%s decoder 132 label path" % name, gen=False)
    assert calls == [1, 1] and list(model._ablation_bufs) == [(T, N, False, True, model.ABLATION_MAX_ROWS, x.device)]


@pytest.mark.parametrize("name", CLASSES)
def test_a_refusal_for_one_shape_is_remembered(name, monkeypatch):
    s = _case(name, "small")
    model, _ = _pair(name, s["cfgs"])
    L, calls = _lib.lib(), []
    monkeypatch.setattr(L, "mfm_predict_ablation_mfn", lambda *a: (calls.append(1), _lib.MFM_ERR_UNSUPPORTED)[1], raising=True)
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
    real = L.mfm_predict_ablation_mfn
    monkeypatch.setattr(L, "mfm_predict_ablation_mfn", lambda *a: (calls.append(1), real(*a))[1], raising=True)
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
