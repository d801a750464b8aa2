"""predict_missing of MFM_missing, seq2seq and basic_missing (mfm_predict_missing, csrc/missing.hip) on the MI355X: per missing
case the label from the other two modalities, the error of the rebuilt modality and the label loss against the oracle's
sub-modules and the reference's own output summaries; agreement with impute; the missing columns; "each" against the single
calls, row chunks, four-row tiles, edges, determinism, containment, unaligned x, labels, capture, the composed path and
allocation.  Numeric bounds: the project's 1e-4 relative fp32 tolerance against the oracle (scalars against float64 reductions
of the oracle's outputs), 5e-4 against the golden summaries.

The missing columns: `gen` of a case is the squared error AGAINST the missing modality's columns, so a single-case call on NaN
there cannot return the clean call's gen.  What is checked is everything that can hold: on NaN in those columns y_hat and disc
keep the clean call's bits and gen is NaN (the columns reached the squared error and nothing else); on ZEROS there y_hat and
disc keep their bits again and gen is the oracle's mean(x_hat^2) -- x_hat was rebuilt without them."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import mfm_oracle_extra as X
from factorized_amd import _lib, configs, synth
from tests import cases
from tests.cases import rel_err
from tests.extra_cases import EXTRA_SIZES, SIZES, load_extra

pytestmark = pytest.mark.gpu
TOL = 1e-4
CANARY = 0x7FC0DEAD                   # a NaN with a payload: any store over it shows
MS = ("l", "a", "v")
CLASSES = ("MFM_missing", "seq2seq", "basic_missing")
FAMILY = {"MFM_missing": 0, "seq2seq": 1, "basic_missing": 2}
PAIR = {"l": "av", "a": "lv", "v": "la"}


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


def _columns(ref, x, m):
    return ref._split(x)[MS.index(m)]


def _oracle(ref, name, x, m):
    """(x_hat_m, y_hat_m) of case m from the oracle's own sub-modules; None for what the class does not have"""
    x_l, x_a, x_v = ref._split(x)
    pair = torch.cat({"l": [x_a, x_v], "a": [x_l, x_v], "v": [x_l, x_a]}[m], 2)
    with torch.no_grad():
        if name == "basic_missing":
            zy = getattr(ref, "encoder_%s_to_y" % PAIR[m])(pair)
            tag = "zy_no%s_to_y" % m
            return None, getattr(ref, tag + "_fc2")(F.relu(getattr(ref, tag + "_fc1")(zy)))
        fm = ref._z_to_f("z%s_to_f%s" % (m, m), getattr(ref, "encoder_%s_to_%s" % (PAIR[m], m))(pair))
        if name == "seq2seq":
            return getattr(ref, "decoder_" + m)(fm, x.shape[0]), None
        fy = ref._z_to_f("zy_to_fy", getattr(ref, "encoder_%s_to_y" % PAIR[m])(pair))
        return getattr(ref, "decoder_" + m)(torch.cat([fy, fm], 1), x.shape[0]), ref._classify(fy)


def _want(ref, name, x, y, m, loss="l1"):
    """(y_hat, gen, disc) of case m: the scalars as float64 reductions of the oracle's outputs"""
    x_hat, y_hat = _oracle(ref, name, x, m)
    gen = None if x_hat is None else float(F.mse_loss(x_hat.double(), _columns(ref, x, m).double()))
    disc = None
    if y_hat is not None and y is not None:
        disc = float(F.l1_loss(y_hat.double(), y.double()) if loss == "l1" else F.cross_entropy(y_hat.double(), y))
    return y_hat, gen, disc


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _same(a, b):
    assert len(a) == len(b)
    return all((p is None and q is None) or torch.equal(_bits(p), _bits(q)) for p, q in zip(a, b))


def _keep(r):
    """predict_missing reuses its output buffers: keep copies"""
    return type(r)(*[None if t is None else t.clone() for t in r])


def _at(r, i):
    """case i of an "each" result"""
    return type(r)(*[None if t is None else t[i] for t in r])


def _check(got, want, what):
    y_hat, gen, disc = want
    assert (got.y_hat is None) == (y_hat is None) and (got.gen is None) == (gen is None) and (got.disc is None) == (disc is None), what
    if y_hat is not None:
        assert tuple(got.y_hat.shape) == tuple(y_hat.shape), what
        assert got.y_hat.dtype == torch.float32 and got.y_hat.is_cuda and not got.y_hat.requires_grad
        err = rel_err(got.y_hat.cpu().numpy(), y_hat.numpy())
        print("missing %s y_hat %.3e" % (what, err))
        assert err < TOL, (what, err)
    for part, g, w in (("gen", got.gen, gen), ("disc", got.disc, disc)):
        if w is not None:
            assert g.dim() == 0 and g.dtype == torch.float32 and g.is_cuda
            err = abs(float(g) - w) / max(abs(w), 1e-30)
            print("missing %s %s %.6e want %.6e err %.3e" % (what, part, float(g), w, err))
            assert err < TOL, (what, part, float(g), w)


def _labels(N, od, seed=5):
    return torch.from_numpy(np.random.RandomState(seed).standard_normal((N, od)).astype(np.float32))


_SHARED = {}


def _case(name, size):
    """a parity case with its model, the oracle, labels, the oracle's numbers and the uncapped results, computed once"""
    key = (name, size)
    if key not in _SHARED:
        cfgs, gold, xn, _ = load_extra(name, size)
        model, ref = _pair(name, cfgs)
        torch.set_num_threads(4)
        xc = torch.from_numpy(xn)
        yc = _labels(xc.shape[1], cfgs[0]["output_dim"])
        x, y = xc.cuda(), yc.cuda()
        want = {m: _want(ref, name, xc, yc, m) for m in MS}
        _SHARED[key] = dict(cfgs=cfgs, cfg=cfgs[0], gold=gold, xc=xc, yc=yc, x=x, y=y, model=model, ref=ref, want=want,
                            single={m: _keep(_call(model, x, y, m)) for m in MS}, each=_keep(_call(model, x, y, "each")))
    return _SHARED[key]


def _call(model, x, y, missing, **kw):
    if FAMILY[type(model).__name__] == 1:
        return model.predict_missing(x, missing=missing, **kw)
    return model.predict_missing(x, y, missing=missing, **kw)


# ----------------------------------------------------------------------------------- 1. against the oracle and the reference
@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("name", CLASSES)
def test_each_and_single_match_the_oracle(name, size):
    s = _case(name, size)
    N, od = s["xc"].shape[1], s["cfg"]["output_dim"]
    if name != "seq2seq":
        assert tuple(s["each"].y_hat.shape) == (3, N, od) and tuple(s["each"].disc.shape) == (3,)
    if name != "basic_missing":
        assert tuple(s["each"].gen.shape) == (3,)
    for i, m in enumerate(MS):
        _check(s["single"][m], s["want"][m], "%s %s no%s" % (name, size, m))
        _check(_at(s["each"], i), s["want"][m], "%s %s each no%s" % (name, size, m))


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("name", ["MFM_missing", "basic_missing"])
def test_y_hat_summaries_match_the_reference_golden(name, size):
    """the rows of out_summary that hold y_hat of the cases no l, no a, no v (the flattened forward outputs)"""
    s = _case(name, size)
    gold = s["gold"]["out_summary"]
    for i, m in enumerate(MS):
        row = 4 * (1 + i) + 3 if name == "MFM_missing" else i
        got = cases.summarize(s["each"].y_hat[i].cpu().numpy())
        scale = max(abs(gold[row, 0]), 1e-6)
        err = float(np.max(np.abs(got - gold[row]) / scale))
        print("missing golden %s %s no%s row %d %.3e" % (name, size, m, row, err))
        assert err < 5 * TOL, (m, row, err)


# ----------------------------------------------------------------------------------- 2. agreement with impute
@pytest.mark.parametrize("size", SIZES)
def test_mfm_missing_agrees_with_impute(size):
    s = _case("MFM_missing", size)
    L = _lib.lib()
    N = s["x"].shape[1]
    ti, tp = (C.c_int32 * 2)(), (C.c_int32 * 2)()
    for i, m in enumerate(MS):
        assert L.mfm_impute_missing_tile_rows(N, 1 << i, s["model"].IMPUTE_MAX_ROWS, ti) == 0
        assert L.mfm_predict_missing_tile_rows(N, 0, 1 << i, s["model"].MISSING_MAX_ROWS, tp) == 0
        assert list(ti) == list(tp)
        imp = s["model"].impute(s["x"], m)
        assert torch.equal(_bits(imp.y_hat), _bits(s["single"][m].y_hat)), m
        want = float(F.mse_loss(imp.x_hat.double(), _columns(s["ref"], s["x"], m).double()))
        got = float(s["single"][m].gen)
        print("missing vs impute %s no%s gen %.6e want %.6e" % (size, m, got, want))
        assert abs(got - want) < TOL * abs(want), (m, got, want)


# ----------------------------------------------------------------------------------- 3. the missing columns
@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("name", CLASSES)
def test_the_missing_columns_reach_the_squared_error_alone(name, m):
    s = _case(name, "small")
    d_l, d_a, d_v = s["cfg"]["input_dims"]
    lo, hi = {"l": (0, d_l), "a": (d_l, d_l + d_a), "v": (d_l + d_a, d_l + d_a + d_v)}[m]
    clean = s["single"][m]
    for poison in (float("nan"), 0.0):
        x = s["x"].clone()
        x[:, :, lo:hi] = poison
        got = _keep(_call(s["model"], x, s["y"], m))
        assert _same((got.y_hat, got.disc), (clean.y_hat, clean.disc)), (name, m, poison)
        if got.y_hat is not None:
            assert bool(torch.isfinite(got.y_hat).all()) and bool(torch.isfinite(got.disc))
        if got.gen is not None and poison != 0.0:
            assert bool(torch.isnan(got.gen)), (name, m)
        elif got.gen is not None:
            xz = s["xc"].clone()
            xz[:, :, lo:hi] = 0.0
            x_hat, _ = _oracle(s["ref"], name, xz, m)
            want = float((x_hat.double() ** 2).mean())
            assert abs(float(got.gen) - want) < TOL * want, (name, m, float(got.gen), want)
            assert not torch.equal(_bits(got.gen), _bits(clean.gen))


# ----------------------------------------------------------------------------------- 4. "each" equals the three single calls
@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("name", CLASSES)
def test_each_equals_the_three_single_calls(name, size):
    s = _case(name, size)
    L = _lib.lib()
    N = s["x"].shape[1]
    t1, t7 = (C.c_int32 * 2)(), (C.c_int32 * 2)()
    assert L.mfm_predict_missing_tile_rows(N, FAMILY[name], 1, 1024, t1) == 0 and L.mfm_predict_missing_tile_rows(N, FAMILY[name], 7, 1024, t7) == 0
    assert list(t1) == list(t7)                    # (both on the same tile rows)
    for i, m in enumerate(MS):
        assert _same(_at(s["each"], i), s["single"][m]), (name, m)


# ----------------------------------------------------------------------------------- 5. row chunks
@pytest.mark.parametrize("cap", [1, 5])
@pytest.mark.parametrize("name", CLASSES)
def test_row_chunks(name, cap):
    """N = 12 in chunks of 5 (a tail chunk of 2) and of 1: y_hat keeps its bits, gen / disc differ in the grouping of the fp64 sums"""
    s = _case(name, "small")
    assert s["x"].shape[1] == 12

    def close(a, b):
        if a is None:
            return b is None
        return bool(((a.double() - b.double()).abs() <= 1e-6 * b.double().abs()).all())
    got = _keep(_call(s["model"], s["x"], s["y"], "each", max_rows=cap))
    assert _same((got.y_hat,), (s["each"].y_hat,))
    assert close(got.gen, s["each"].gen) and close(got.disc, s["each"].disc), (got, s["each"])
    for m in MS:
        one = _call(s["model"], s["x"], s["y"], m, max_rows=cap)
        assert _same((one.y_hat,), (s["single"][m].y_hat,)), m
        assert close(one.gen, s["single"][m].gen) and close(one.disc, s["single"][m].disc), m


# ----------------------------------------------------------------------------------- 6. four-row tiles, a ragged last tile
@pytest.mark.parametrize("name", CLASSES)
def test_four_row_tiles_with_a_ragged_last_tile(name):
    """T = 3 at the smallest N with N mod 4 != 0 at which every recurrence launch of "each" runs on four-row tiles (the threshold
    differs with the LSTMs per launch, hence per family); against the oracle, and against chunks of 32 rows (one-row tiles)"""
    s = _case(name, "small")
    L = _lib.lib()
    cap = s["model"].MISSING_MAX_ROWS
    tr = (C.c_int32 * 2)()
    N = None
    for n in range(1, cap + 1):
        assert L.mfm_predict_missing_tile_rows(n, FAMILY[name], 7, cap, tr) == 0
        if n % 4 and tr[0] == 4 and tr[1] in (0, 4):
            N = n
            break
    assert N is not None, "no N up to %d reaches the four-row form on %d CUs" % (cap, L.mfm_device_cus())
    assert L.mfm_predict_missing_tile_rows(N, FAMILY[name], 7, 32, tr) == 0 and tr[0] == 1 and tr[1] in (0, 1)
    T = 3
    xn, _ = synth.make_batch(s["cfg"]["input_dims"], N, T, seed=11)
    xc, yc = torch.from_numpy(xn), _labels(N, s["cfg"]["output_dim"], seed=12)
    x, y = xc.cuda(), yc.cuda()
    four = _keep(_call(s["model"], x, y, "each"))
    one = _keep(_call(s["model"], x, y, "each", max_rows=32))
    for i, m in enumerate(MS):
        want = _want(s["ref"], name, xc, yc, m)
        _check(_at(four, i), want, "%s four-row N%d no%s" % (name, N, m))
        _check(_at(one, i), want, "%s one-row N%d no%s" % (name, N, m))


# ----------------------------------------------------------------------------------- 7. edges
@pytest.mark.parametrize("T,N", [(1, 12), (6, 1), (1, 1)], ids=["T1", "N1", "T1N1"])
@pytest.mark.parametrize("name", CLASSES)
def test_edges_against_the_oracle(name, T, N):
    s = _case(name, "small")
    xn, _ = synth.make_batch(s["cfg"]["input_dims"], N, T, seed=31)
    xc, yc = torch.from_numpy(xn), _labels(N, s["cfg"]["output_dim"], seed=32)
    x, y = xc.cuda(), yc.cuda()
    each = _keep(_call(s["model"], x, y, "each"))
    for i, m in enumerate(MS):
        want = _want(s["ref"], name, xc, yc, m)
        _check(_call(s["model"], x, y, m), want, "%s T%d N%d no%s" % (name, T, N, m))
        _check(_at(each, i), want, "%s T%d N%d each no%s" % (name, T, N, m))


# ----------------------------------------------------------------------------------- 8. repeat calls
@pytest.mark.parametrize("name", CLASSES)
def test_two_calls_are_bit_equal(name):
    s = _case(name, "small")
    a = _keep(_call(s["model"], s["x"], s["y"], "each"))
    b = _call(s["model"], s["x"], s["y"], "each")
    assert _same(a, b) and _same(a, s["each"])
    for m in MS:
        assert _same(_call(s["model"], s["x"], s["y"], m), s["single"][m])


# ----------------------------------------------------------------------------------- 9. canaries
def _canary(n, pad=256):
    big = torch.full((pad + n + pad,), CANARY, dtype=torch.int32, device="cuda")
    return big, big[pad:pad + n].view(torch.float32)


def _intact(big, n, pad=256):
    return bool((big[:pad] == CANARY).all()) and bool((big[pad + n:] == CANARY).all())


@pytest.mark.parametrize("bits,cap", [(2, 0), (7, 0), (7, 5)])
@pytest.mark.parametrize("name", CLASSES)
def test_canaries_around_workspace_and_outputs(name, bits, cap):
    """the entry through the C ABI on caller-owned, canary-framed buffers: nothing outside is touched, the results are the
    module's"""
    s = _case(name, "small")
    model, x, y = s["model"], s["x"], s["y"]
    fam = FAMILY[name]
    T, N = x.shape[:2]
    ms = [m for i, m in enumerate(MS) if bits >> i & 1]
    L = _lib.lib()
    sz = model._missing_sizes()
    sizes = (C.c_int32 * 12)(*sz)
    nws = int(L.mfm_predict_missing_workspace_floats(T, N, sizes, fam, bits, 1, cap))
    assert nws > 0
    big_ws, ws = _canary(nws)
    ny = len(ms) * N * sz[11]
    (big_y, y_hat), (big_g, gen), (big_d, disc) = _canary(ny), _canary(3), _canary(3)
    prm = (C.c_void_p * 74)(*[None if p is None else p.data_ptr() for p in model._missing_params(ms)])
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = lambda t, have: C.c_void_p(t.data_ptr()) if have else None
    rc = L.mfm_predict_missing(T, N, sizes, fam, bits, 0, prm, C.c_void_p(x.data_ptr()), ptr(y, fam != 1), C.c_void_p(ws.data_ptr()),
                               ptr(y_hat, fam != 1), ptr(gen, fam != 2), ptr(disc, fam != 1), cap, stream)
    assert rc == 0, L.mfm_last_error().decode()
    torch.cuda.synchronize()
    assert _intact(big_ws, nws) and _intact(big_y, ny) and _intact(big_g, 3) and _intact(big_d, 3)
    # what the family does not have was not written at all
    if fam == 1:
        assert bool((big_y == CANARY).all()) and bool((big_d == CANARY).all())
    if fam == 2:
        assert bool((big_g == CANARY).all())
    ref = s["each"] if bits == 7 else s["single"][ms[0]]
    i0 = MS.index(ms[0])
    if fam != 1:
        assert torch.equal(_bits(y_hat), _bits(ref.y_hat.reshape(-1)))
        d = disc if bits == 7 else disc[i0]
        assert torch.equal(_bits(d), _bits(ref.disc)) if cap == 0 else rel_err(d.cpu().numpy(), ref.disc.cpu().numpy()) < 1e-6
    if fam != 2:
        g = gen if bits == 7 else gen[i0]
        assert torch.equal(_bits(g), _bits(ref.gen)) if cap == 0 else rel_err(g.cpu().numpy(), ref.gen.cpu().numpy()) < 1e-6


# ----------------------------------------------------------------------------------- 10. x off a 16-byte boundary
@pytest.mark.parametrize("name", CLASSES)
def test_a_batch_view_off_a_16_byte_boundary_gives_the_same_bits(name):
    s = _case(name, "small")
    x = s["x"]
    flat = torch.zeros(x.numel() + 8, dtype=torch.float32, device="cuda")
    assert flat.data_ptr() % 16 == 0
    for k in (1, 2, 3):
        view = flat[k:k + x.numel()].view(x.shape)
        view.copy_(x)
        assert view.is_contiguous() and view.data_ptr() % 16 == 4 * k
        assert _same(_call(s["model"], view, s["y"], "each"), s["each"]), k
        assert _same(_call(s["model"], view, s["y"], "a"), s["single"]["a"]), k


# ----------------------------------------------------------------------------------- 11. labels
@pytest.mark.parametrize("name", ["MFM_missing", "basic_missing"])
def test_cross_entropy_labels(name):
    cfgs = configs.canonical_configs(dropout=False, output_dim=3, **EXTRA_SIZES)
    model, ref = _pair(name, cfgs)
    T, N = 4, 9
    xn, _ = synth.make_batch(cfgs[0]["input_dims"], N, T, seed=41)
    xc = torch.from_numpy(xn)
    yc = torch.from_numpy(np.random.RandomState(42).randint(0, 3, size=N).astype(np.int64))
    x, y = xc.cuda(), yc.cuda()
    each = _keep(model.predict_missing(x, y, missing="each", loss="ce"))
    chunks = _keep(model.predict_missing(x, y, missing="each", loss="ce", max_rows=4))
    for i, m in enumerate(MS):
        want = _want(ref, name, xc, yc, m, loss="ce")
        _check(_at(each, i), want, "%s ce each no%s" % (name, m))
        _check(_at(chunks, i), want, "%s ce chunks no%s" % (name, m))
        _check(model.predict_missing(x, y, missing=m, loss="ce"), want, "%s ce no%s" % (name, m))
    with pytest.raises(_lib.MfmError, match="int64 class indices"):
        model.predict_missing(x, y.float(), missing="each", loss="ce")
    with pytest.raises(_lib.MfmError, match="float labels"):
        model.predict_missing(x, y, missing="each", loss="l1")


@pytest.mark.parametrize("name", ["MFM_missing", "basic_missing"])
def test_without_labels_there_is_no_disc(name):
    s = _case(name, "small")
    model, _ = _pair(name, s["cfgs"])
    got = model.predict_missing(s["x"], missing="each")
    assert got.disc is None and _same((got.y_hat, got.gen), (s["each"].y_hat, s["each"].gen))
    one = model.predict_missing(s["x"], missing="v")
    assert one.disc is None and _same((one.y_hat, one.gen), (s["single"]["v"].y_hat, s["single"]["v"].gen))
    assert sorted(k[3] for k in model._missing_bufs) == [False, False]          # (the label-free cache keys alone)


def test_seq2seq_has_no_label_path():
    s = _case("seq2seq", "small")
    assert s["each"].y_hat is None and s["each"].disc is None and s["single"]["l"].y_hat is None
    assert _case("basic_missing", "small")["each"].gen is None


# ----------------------------------------------------------------------------------- 12. capture
@pytest.mark.parametrize("name", CLASSES)
def test_each_in_a_captured_graph(name):
    s = _case(name, "small")
    model, _ = _pair(name, s["cfgs"])
    x, y = s["x"], s["y"]
    T, N = x.shape[:2]
    xin = x.clone()
    _call(model, xin, y, "each")                             # warm-up: buffers, code objects
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        g = _call(model, xin, y, "each")
    xn, _ = synth.make_batch(s["cfg"]["input_dims"], N, T, seed=23)
    x2 = torch.from_numpy(xn).cuda()
    xin.copy_(x2)
    graph.replay()
    torch.cuda.synchronize()
    first = _keep(g)
    graph.replay()
    torch.cuda.synchronize()
    second = _keep(g)
    eager = _keep(_call(model, x2, y, "each"))
    assert _same(first, eager) and _same(second, eager)
    assert not _same(eager, s["each"])                       # (the new input did change the result)


# ----------------------------------------------------------------------------------- 13. refusal takes the composition
@pytest.mark.parametrize("name,wide", [("MFM_missing", "zv_size"), ("seq2seq", "zv_size"), ("basic_missing", "zy_size")])
def test_a_hidden_size_of_132_takes_the_composed_path(name, wide, monkeypatch):
    cfgs = configs.canonical_configs(dropout=False, **dict(EXTRA_SIZES, **{wide: 132}))
    model, ref = _pair(name, cfgs)
    T, N = 3, 5
    xn, _ = synth.make_batch(cfgs[0]["input_dims"], N, T, seed=21)
    xc, yc = torch.from_numpy(xn), _labels(N, cfgs[0]["output_dim"], seed=22)
    x, y = xc.cuda(), yc.cuda()
    L, calls = _lib.lib(), []
    real = L.mfm_predict_missing
    monkeypatch.setattr(L, "mfm_predict_missing", lambda *a: (calls.append(1), real(*a))[1], raising=True)
    each = _call(model, x, y, "each")
    assert calls == [1] and model._missing_refused and not model.__dict__.get("_missing_bufs")
    for i, m in enumerate(MS):
        want = _want(ref, name, xc, yc, m)
        _check(_at(each, i), want, "%s wide each no%s" % (name, m))
        _check(_call(model, x, y, m), want, "%s wide no%s" % (name, m))
    assert calls == [1] and not model.__dict__.get("_missing_bufs")      # (remembered: no second call into the entry)


@pytest.mark.parametrize("name", CLASSES)
def test_a_refusal_for_one_shape_is_remembered(name, monkeypatch):
    s = _case(name, "small")
    model, _ = _pair(name, s["cfgs"])
    L, calls = _lib.lib(), []
    monkeypatch.setattr(L, "mfm_predict_missing", lambda *a: (calls.append(1), _lib.MFM_ERR_UNSUPPORTED)[1], raising=True)
    for _ in range(2):
        got = _call(model, s["x"], s["y"], "l")
        _check(got, s["want"]["l"], "%s refused shape, composed" % name)
        assert calls == [1] and not model._missing_refused and list(model._missing_bufs.values()) == [False]


# ----------------------------------------------------------------------------------- 14. no allocation after the first call
@pytest.mark.parametrize("name", CLASSES)
def test_no_allocation_and_no_synchronisation_after_the_first_call(name):
    s = _case(name, "small")
    model, x, y = s["model"], s["x"], s["y"]
    for _ in range(2):
        _call(model, x, y, "each")
        _call(model, x, y, "a")
    torch.cuda.synchronize()
    allocated = torch.cuda.memory_allocated()
    count = torch.cuda.memory_stats()["allocation.all.allocated"]
    torch.cuda.set_sync_debug_mode("error")
    try:
        for _ in range(5):
            _call(model, x, y, "each")
            _call(model, x, y, "a")
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.cuda.memory_allocated() == allocated
    assert torch.cuda.memory_stats()["allocation.all.allocated"] == count


# ----------------------------------------------------------------------------------- 15. errors, and what a call leaves alone
@pytest.mark.parametrize("name", CLASSES)
def test_errors_reach_no_kernel_and_training_is_left_as_found(name, monkeypatch):
    s = _case(name, "small")
    model, x, y = s["model"], s["x"], s["y"]
    L, calls = _lib.lib(), []
    real = L.mfm_predict_missing
    monkeypatch.setattr(L, "mfm_predict_missing", lambda *a: (calls.append(1), real(*a))[1], raising=True)
    bufs = dict(model._missing_bufs)
    with pytest.raises(ValueError, match="'l', 'a', 'v' or 'each'"):
        _call(model, x, y, "la")
    with pytest.raises(_lib.MfmError, match="features per time step"):
        _call(model, x[:, :, :-1], y, "l")
    with pytest.raises(_lib.MfmError, match="input is on cpu"):
        _call(model, x.cpu(), y, "v")
    with pytest.raises(_lib.MfmError, match="empty split"):
        _call(model, x[:, :0], y, "each")
    with pytest.raises(_lib.MfmError, match="max_rows"):
        _call(model, x, y, "a", max_rows=0)
    if name != "seq2seq":
        with pytest.raises(ValueError, match="'l1' or 'ce'"):
            model.predict_missing(x, y, loss="l2")
        with pytest.raises(_lib.MfmError, match="float labels"):
            model.predict_missing(x, y[:-1])
        with pytest.raises(_lib.MfmError, match="labels must be a tensor on"):
            model.predict_missing(x, y.cpu())
    assert not calls and model._missing_bufs == bufs         # the entry was not reached, nothing was allocated
    model.train()
    got = _call(model, x, y, "each")
    assert model.training and all(mod.training for mod in model.modules())
    model.eval()
    assert calls == [1] and _same(got, s["each"])             # (eval computation whatever the mode)
    assert all(p.grad is None for p in model.parameters()) and not [k for k in model.state_dict() if "missing_bufs" in k]
