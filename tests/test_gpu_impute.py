"""MFM_missing.impute (mfm_impute_missing, csrc/impute.hip) on the MI355X: a missing modality and the label from the other two
modalities against the oracle's forward and the reference's own output summaries; the missing columns are never read; "each"
against the single calls, row chunks, determinism, edges, four-row tiles, containment, capture, the composed path and the
refusals.  Numeric bounds: the project's 1e-4 relative fp32 tolerance against the oracle, 5e-4 against the golden summaries (the
constants of test_gpu_extra_models.py)."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import mfm_oracle_extra as X
from factorized_amd import _lib, configs, synth
from tests import cases
from tests.cases import grad_err, rel_err
from tests.extra_cases import SIZES, extra_configs, load_extra

pytestmark = pytest.mark.gpu
TOL = 1e-4
CANARY = 0x7FC0DEAD                   # a NaN with a payload: any store over it shows
MS = ("l", "a", "v")


def _pair(cfgs, seed=1234):
    """(model on the GPU, oracle in eval mode) with the same synthetic weights, set up as test_gpu_extra_models.py does"""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from factorized_amd import mfm_model as M
    ref = X.CLASSES["MFM_missing"](*cfgs)
    w = synth.make_weights({k: tuple(v.shape) for k, v in ref.state_dict().items()}, seed=seed)
    ref.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in w.items()})
    ref.eval()
    model = M.MFM_missing(*cfgs)
    model.load_state_dict(ref.state_dict())
    return model.cuda(), ref


def _oracle_impute(ref, x, m):
    """what forward() computes for decoded_no<m>[index of m] and decoded_no<m>[3], from the oracle's own sub-modules (pinned to
    forward() bit for bit in test 1)"""
    x_l, x_a, x_v = ref._split(x)
    pair, name = {"l": ([x_a, x_v], "av"), "a": ([x_l, x_v], "lv"), "v": ([x_l, x_a], "la")}[m]
    with torch.no_grad():
        pair = torch.cat(pair, 2)
        zm, zy = getattr(ref, "encoder_%s_to_%s" % (name, m))(pair), getattr(ref, "encoder_%s_to_y" % name)(pair)
        fy, fm = ref._z_to_f("zy_to_fy", zy), ref._z_to_f("z%s_to_f%s" % (m, m), zm)
        return getattr(ref, "decoder_" + m)(torch.cat([fy, fm], 1), x.shape[0]), ref._classify(fy)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _same(a, b):
    return all(torch.equal(_bits(p), _bits(q)) for p, q in zip(a, b))


def _keep(r):
    """impute reuses its output buffers: keep copies"""
    if isinstance(r, dict):
        return {m: _keep(v) for m, v in r.items()}
    return type(r)(*[t.clone() for t in r])


def _check(got, want, what):
    for g, r, part in zip(got, want, ("x_hat", "y_hat")):
        assert tuple(g.shape) == tuple(r.shape), (what, part)
        assert g.dtype == torch.float32 and g.is_cuda and not g.requires_grad
        err = rel_err(g.cpu().numpy(), r.numpy())
        print("impute %s %s %.3e" % (what, part, err))
        assert err < TOL, (what, part, err)


_SHARED = {}


def _case(size):
    """a parity case with its model, the oracle, the oracle's forward and the uncapped single results, computed once"""
    if size not in _SHARED:
        cfgs, gold, xn, gauss = load_extra("MFM_missing", size)
        model, ref = _pair(cfgs)
        torch.set_num_threads(4)
        xc = torch.from_numpy(xn)
        ref.mmd_gauss = gauss
        with torch.no_grad():
            flat = X.flatten_outputs(ref.forward(xc))
        x = xc.cuda()
        single = {m: _keep(model.impute(x, m)) for m in MS}
        _SHARED[size] = dict(cfgs=cfgs, cfg=cfgs[0], gold=gold, xc=xc, x=x, model=model, ref=ref, flat=flat, single=single,
                             gauss=gauss)
    return _SHARED[size]


def _rows(i):
    return 4 * (1 + i) + i, 4 * (1 + i) + 3


# ----------------------------------------------------------------------------------- 1. against the oracle
@pytest.mark.parametrize("size", SIZES)
def test_each_case_matches_the_oracle_forward(size):
    s = _case(size)
    T, B = s["xc"].shape[:2]
    for i, m in enumerate(MS):
        ix, iy = _rows(i)
        _check(s["single"][m], (s["flat"][ix], s["flat"][iy]), "%s no%s" % (size, m))
        assert tuple(s["single"][m].x_hat.shape) == (T, B, s["cfg"]["input_dims"][i])
        assert tuple(s["single"][m].y_hat.shape) == (B, s["cfg"]["output_dim"])
        # (the helper the edge tests lean on is forward(), bit for bit)
        assert _same(_oracle_impute(s["ref"], s["xc"], m), (s["flat"][ix], s["flat"][iy]))


# ----------------------------------------------------------------------------------- 2. against the reference itself
@pytest.mark.parametrize("size", SIZES)
def test_summaries_match_the_reference_golden(size):
    s = _case(size)
    gold = s["gold"]["out_summary"]
    for i, m in enumerate(MS):
        for row, t in zip(_rows(i), s["single"][m]):
            got = cases.summarize(t.cpu().numpy())
            scale = max(abs(gold[row, 0]), 1e-6)
            err = float(np.max(np.abs(got - gold[row]) / scale))
            print("impute golden %s no%s row %d %.3e" % (size, m, row, err))
            assert err < 5 * TOL, (m, row, err)


# ----------------------------------------------------------------------------------- 3. the missing modality is never read
@pytest.mark.parametrize("m", MS)
def test_the_missing_columns_are_never_read(m):
    s = _case("small")
    d_l, d_a, d_v = s["cfg"]["input_dims"]
    lo, hi = {"l": (0, d_l), "a": (d_l, d_l + d_a), "v": (d_l + d_a, d_l + d_a + d_v)}[m]
    for poison in (float("nan"), 1e30):
        x = s["x"].clone()
        x[:, :, lo:hi] = poison
        got = _keep(s["model"].impute(x, m))
        assert all(bool(torch.isfinite(t).all()) for t in got)
        assert _same(got, s["single"][m]), (m, poison)


def _poisoned(x, cfg, m, poison):
    d_l, d_a, d_v = cfg["input_dims"]
    lo, hi = {"l": (0, d_l), "a": (d_l, d_l + d_a), "v": (d_l + d_a, d_l + d_a + d_v)}[m]
    x = x.clone()
    x[:, :, lo:hi] = poison
    return x


@pytest.mark.parametrize("m", MS)
def test_the_composed_path_never_reads_the_missing_columns_either(m):
    """with the forced-refusal switch: the composition of the granular operations gives, on poisoned columns, the bits it gives
    on the clean x"""
    s = _case("small")
    model, _ = _pair(s["cfgs"])
    model._impute_refused = True
    clean = _keep(model.impute(s["x"], m))
    _check(clean, [t.cpu() for t in s["single"][m]], "composed clean no%s" % m)
    for poison in (float("nan"), 1e30):
        got = _keep(model.impute(_poisoned(s["x"], s["cfg"], m, poison), m))
        assert all(bool(torch.isfinite(t).all()) for t in got), (m, poison)
        assert _same(got, clean), (m, poison)
    assert not model.__dict__.get("_impute_bufs")


def test_the_wide_model_never_reads_the_missing_columns():
    """canonical sizes with zv_size = 136 (case v refused by the entry, composed): k = 305 and k = 25 are no multiples of 4, so
    a 16-byte fetch of a column SLICE would reach the missing columns; the composition reads a copy"""
    cfgs = configs.canonical_configs(dropout=False, zv_size=136)
    model, ref = _pair(cfgs)
    T, N = 3, 4
    xn, _ = synth.make_batch(cfgs[0]["input_dims"], N, T, seed=21)
    xc = torch.from_numpy(xn)
    x = xc.cuda()
    model.impute(x, "v")                                     # (refused for h = 136: remembered, every case composes from here on)
    assert model._impute_refused
    clean = {m: _keep(model.impute(x, m)) for m in MS}
    for m in MS:
        _check(clean[m], _oracle_impute(ref, xc, m), "wide clean no%s" % m)
        for poison in (float("nan"), 1e30):
            got = _keep(model.impute(_poisoned(x, cfgs[0], m, poison), m))
            assert all(bool(torch.isfinite(t).all()) for t in got), (m, poison)
            assert _same(got, clean[m]), (m, poison)
    assert not model.__dict__.get("_impute_bufs")


# ----------------------------------------------------------------------------------- 4. "each" equals the three single calls
@pytest.mark.parametrize("size", SIZES)
def test_each_equals_the_three_single_calls(size):
    s = _case(size)
    each = _keep(s["model"].impute(s["x"], "each"))
    assert sorted(each) == ["a", "l", "v"]
    for m in MS:
        assert _same(each[m], s["single"][m]), m


# ----------------------------------------------------------------------------------- 5. row chunks
@pytest.mark.parametrize("cap", [1, 5, 12])
def test_row_chunks_are_bit_equal(cap):
    s = _case("small")
    for m in MS:
        assert _same(s["model"].impute(s["x"], m, max_rows=cap), s["single"][m]), m
    each = s["model"].impute(s["x"], "each", max_rows=cap)
    for m in MS:
        assert _same(each[m], s["single"][m]), m


# ----------------------------------------------------------------------------------- 6. repeat calls
def test_two_calls_are_bit_equal():
    s = _case("small")
    for m in MS:
        a = _keep(s["model"].impute(s["x"], m))
        b = s["model"].impute(s["x"], m)
        assert _same(a, b) and _same(a, s["single"][m])


# ----------------------------------------------------------------------------------- 7. edges
@pytest.mark.parametrize("T,N", [(1, 12), (6, 1), (6, 5)], ids=["T1", "N1", "N5"])
def test_edges_against_the_oracle(T, N):
    s = _case("small")
    xn, _ = synth.make_batch(s["cfg"]["input_dims"], N, T, seed=31)
    xc = torch.from_numpy(xn)
    x = xc.cuda()
    each = _keep(s["model"].impute(x, "each"))
    for m in MS:
        want = _oracle_impute(s["ref"], xc, m)
        _check(s["model"].impute(x, m), want, "T%d N%d no%s" % (T, N, m))
        _check(each[m], want, "T%d N%d each no%s" % (T, N, m))


def test_a_contiguous_view_on_a_4_byte_boundary_is_taken():
    """x[1:] of a [T + 1, N, D] tensor with N * D odd starts on a 4-byte boundary: the entry reads x element by element"""
    s = _case("small")
    T, N = 4, 5
    xn, _ = synth.make_batch(s["cfg"]["input_dims"], N, T + 1, seed=33)
    big = torch.from_numpy(xn).cuda()
    x = big[1:]
    assert (N * x.shape[2]) % 2 == 1 and x.is_contiguous() and x.data_ptr() % 16 != 0
    each = _keep(s["model"].impute(x, "each"))
    for m in MS:
        _check(each[m], _oracle_impute(s["ref"], torch.from_numpy(xn[1:]), m), "view no%s" % m)


# ----------------------------------------------------------------------------------- 8. four-row tiles
def test_four_row_tiles_from_six_workgroups_per_cu_on():
    """a single case is two encoder recurrences: from 3 * CUs rows on their launch runs on four-row tiles (the rule of
    gen_tile_rows).  N odd, so the last tile is not full."""
    s = _case("small")
    L = _lib.lib()
    cus = L.mfm_device_cus()
    N, T = 771, 2
    if 2 * N < 6 * cus:
        N = 3 * cus + (1 if (3 * cus) % 2 == 0 else 2)
    assert N % 2 == 1 and 2 * N >= 6 * cus
    tr = (C.c_int32 * 2)()
    assert L.mfm_impute_missing_tile_rows(N, 2, s["model"].IMPUTE_MAX_ROWS, tr) == 0
    assert tr[0] == 4, "N = %d on %d CUs did not reach the four-row form" % (N, cus)
    assert L.mfm_impute_missing_tile_rows(N, 2, 64, tr) == 0 and list(tr) == [1, 1]
    xn, _ = synth.make_batch(s["cfg"]["input_dims"], N, T, seed=11)
    xc = torch.from_numpy(xn)
    x = xc.cuda()
    for m in MS:
        four = _keep(s["model"].impute(x, m))
        _check(four, _oracle_impute(s["ref"], xc, m), "four-row no%s" % m)
        assert _same(s["model"].impute(x, m), four)
        _check(s["model"].impute(x, m, max_rows=64), [t.cpu() for t in four], "four-row vs one-row no%s" % m)


def test_four_row_tiles_of_each_on_canonical_sizes():
    """all three cases are six encoder and three decoder recurrences: from 2 * CUs rows on BOTH launches of "each" run on four-row
    tiles, at the canonical sizes the two instantiations with the per-block switch.  N odd: the last tile holds one row.
    Against the oracle, run to run, and against the same split in chunks of 64 rows (one-row tiles)."""
    s = _case("canonical")
    L = _lib.lib()
    cus = L.mfm_device_cus()
    N, T = 2 * cus + 1, 2
    tr = (C.c_int32 * 2)()
    assert L.mfm_impute_missing_tile_rows(N, 7, s["model"].IMPUTE_MAX_ROWS, tr) == 0
    assert list(tr) == [4, 4], "N = %d on %d CUs did not reach the four-row forms" % (N, cus)
    assert L.mfm_impute_missing_tile_rows(N, 7, 64, tr) == 0 and list(tr) == [1, 1]
    xn, _ = synth.make_batch(s["cfg"]["input_dims"], N, T, seed=13)
    xc = torch.from_numpy(xn)
    x = xc.cuda()
    four = _keep(s["model"].impute(x, "each"))
    again = s["model"].impute(x, "each")
    one = _keep(s["model"].impute(x, "each", max_rows=64))
    for m in MS:
        _check(four[m], _oracle_impute(s["ref"], xc, m), "four-row each no%s" % m)
        assert _same(again[m], four[m]), m
        _check(one[m], [t.cpu() for t in four[m]], "four-row vs one-row each no%s" % m)


# ----------------------------------------------------------------------------------- 9. eval whatever the mode
def test_dropout_is_off_whatever_the_mode():
    cfgs = configs.canonical_configs(dropout=True)
    model, ref = _pair(cfgs)
    xn, _ = synth.make_batch(cfgs[0]["input_dims"], 9, 5, seed=7)
    xc = torch.from_numpy(xn)
    x = xc.cuda()
    model.train()
    each = _keep(model.impute(x, "each"))
    assert model.training and all(mod.training for mod in model.modules())
    for m in MS:
        _check(each[m], _oracle_impute(ref, xc, m), "train-mode no%s" % m)
    model.eval()
    again = model.impute(x, "each")
    assert not model.training
    for m in MS:
        assert _same(again[m], each[m])


# ----------------------------------------------------------------------------------- 10. leaves everything alone
def test_impute_leaves_parameters_gradients_and_training_alone():
    cfgs, _, xn, gauss = load_extra("MFM_missing", "small")
    model, _ = _pair(cfgs)
    model.train()
    model.mmd_gauss = [g.cuda() for g in gauss]
    x = torch.from_numpy(xn).cuda()
    before = {n: p.detach().clone() for n, p in model.named_parameters()}
    out = model.impute(x, "each")
    assert all(p.grad is None for p in model.parameters())
    assert all(not t.requires_grad for m in MS for t in out[m])

    def step():
        for p in model.parameters():
            p.grad = None
        o = model.forward(x)
        X.test_objective(o).backward()
        return ([t.detach().clone() for t in X.flatten_outputs(o)],
                {n: None if p.grad is None else p.grad.detach().clone() for n, p in model.named_parameters()})
    o1, g1 = step()
    for m in MS:
        model.impute(x, m)
    model.impute(x, "each")
    torch.cuda.synchronize()
    for n, p in model.named_parameters():
        assert torch.equal(_bits(p), _bits(before[n])), n
        assert (p.grad is None) == (g1[n] is None), n
        if p.grad is not None:
            assert torch.equal(_bits(p.grad), _bits(g1[n])), n          # (the call touched no gradient either)
    o2, g2 = step()
    for i, (a, b) in enumerate(zip(o2, o1)):
        if b.numel() and float(b.abs().max()) > 0:
            assert rel_err(a.cpu().numpy(), b.cpu().numpy()) < TOL, i
    for n in g1:
        assert (g1[n] is None) == (g2[n] is None), n
        if g1[n] is not None:
            assert grad_err(g2[n].cpu().numpy(), g1[n].cpu().numpy(), abs_slack=1e-8) < TOL, n
    assert "_impute_bufs" in model.__dict__
    assert not [k for k in model.state_dict() if "impute" in k]


# ----------------------------------------------------------------------------------- 11. canaries
def _canary(n, pad=256):
    big = torch.full((pad + n + pad,), CANARY, dtype=torch.int32, device="cuda")
    return big, big[pad:pad + n].view(torch.float32)


def _intact(big, n, pad=256):
    return bool((big[:pad] == CANARY).all()) and bool((big[pad + n:] == CANARY).all())


@pytest.mark.parametrize("bits,cap", [(1, 0), (2, 0), (4, 5), (7, 0), (7, 5)])
def test_canaries_around_workspace_and_outputs(bits, cap):
    """the entry through the C ABI on caller-owned, canary-framed buffers: nothing outside is touched, the results are the
    module's, bit for bit"""
    s = _case("small")
    model, x = s["model"], s["x"]
    T, N = x.shape[:2]
    ms = [m for i, m in enumerate(MS) if bits >> i & 1]
    L = _lib.lib()
    sz = model._impute_sizes()
    sizes = (C.c_int32 * 12)(*sz)
    nws = int(L.mfm_impute_missing_workspace_floats(T, N, sizes, bits, cap))
    assert nws > 0
    big_ws, ws = _canary(nws)
    outs, optr = {}, (C.c_void_p * 6)()
    for i, m in enumerate(MS):
        if m in ms:
            outs[m] = (_canary(T * N * sz[8 + i]), _canary(N * sz[11]))
            optr[2 * i], optr[2 * i + 1] = outs[m][0][1].data_ptr(), outs[m][1][1].data_ptr()
    prm = (C.c_void_p * 74)(*[None if p is None else p.data_ptr() for p in model._impute_params(ms)])
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert L.mfm_impute_missing(T, N, sizes, bits, prm, C.c_void_p(x.data_ptr()), C.c_void_p(ws.data_ptr()), optr, cap, stream) == 0
    torch.cuda.synchronize()
    assert _intact(big_ws, nws)
    for i, m in enumerate(MS):
        if m in ms:
            for (big, view), ref in zip(outs[m], s["single"][m]):
                assert _intact(big, ref.numel()), m
                assert torch.equal(_bits(view), _bits(ref.reshape(-1))), m


# ----------------------------------------------------------------------------------- 12. capture
def test_each_in_a_captured_graph():
    s = _case("small")
    cfgs = s["cfgs"]
    model, _ = _pair(cfgs)
    x = s["x"]
    T, N = x.shape[:2]
    xin = x.clone()
    model.impute(xin, "each")                                # warm-up: buffers, code objects
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        g = model.impute(xin, "each")
    xn, _ = synth.make_batch(s["cfg"]["input_dims"], N, T, seed=23)
    x2 = torch.from_numpy(xn).cuda()
    xin.copy_(x2)
    graph.replay()
    torch.cuda.synchronize()
    captured = _keep(g)
    eager = _keep(model.impute(x2, "each"))
    for m in MS:
        assert _same(captured[m], eager[m]), m
        assert not _same(eager[m], s["single"][m])           # (the new input did change the result)


# ----------------------------------------------------------------------------------- 13. no allocation after the first call
def test_no_allocation_and_no_synchronisation_after_the_first_call():
    s = _case("small")
    model, x = s["model"], s["x"]
    for _ in range(2):
        model.impute(x, "each")
        model.impute(x, "a")
    torch.cuda.synchronize()
    allocated = torch.cuda.memory_allocated()
    count = torch.cuda.memory_stats()["allocation.all.allocated"]
    torch.cuda.set_sync_debug_mode("error")
    try:
        for _ in range(10):
            model.impute(x, "each")
            model.impute(x, "a")
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.cuda.memory_allocated() == allocated
    assert torch.cuda.memory_stats()["allocation.all.allocated"] == count


# ----------------------------------------------------------------------------------- 14. refusal takes the composition
def test_forced_refusal_takes_the_composition_and_agrees():
    s = _case("small")
    model, _ = _pair(s["cfgs"])
    x = s["x"]
    model._impute_refused = True
    for m in MS:
        slow = model.impute(x, m)
        _check(slow, [t.cpu() for t in s["single"][m]], "composed no%s" % m)
    each = model.impute(x, "each")
    for m in MS:
        _check(each[m], [t.cpu() for t in s["single"][m]], "composed each no%s" % m)
    assert not model.__dict__.get("_impute_bufs")            # (the fused entry was not used)
    # a parameter that is not a contiguous float32 tensor: the composition's own checks speak
    model._impute_refused = False
    model.decoder_l.fc1.weight.data = model.decoder_l.fc1.weight.data.t().contiguous().t()
    assert not model.decoder_l.fc1.weight.is_contiguous()
    with pytest.raises(_lib.MfmError, match="contiguous"):
        model.impute(x, "l")
    assert not model.__dict__.get("_impute_bufs")
    _check(model.impute(x, "a"), [t.cpu() for t in s["single"]["a"]], "fused a beside a strided decoder_l")
    assert model.__dict__.get("_impute_bufs")


def test_a_refusal_for_one_shape_is_remembered_without_buffers(monkeypatch):
    """a refusal that is no property of the model (the LDS limit depends on the tile rows, hence on N and max_rows; stood in for
    here by an entry that refuses) is remembered for that shape: later calls compose at once, nothing is allocated for them, and
    other shapes still run fused"""
    s = _case("small")
    model, _ = _pair(s["cfgs"])
    x = s["x"]
    L, calls = _lib.lib(), []
    monkeypatch.setattr(L, "mfm_impute_missing", lambda *a: (calls.append(1), _lib.MFM_ERR_UNSUPPORTED)[1], raising=True)
    _check(model.impute(x, "l"), [t.cpu() for t in s["single"]["l"]], "refused shape, composed")
    assert calls == [1] and not model._impute_refused and list(model._impute_bufs.values()) == [False]
    torch.cuda.synchronize()
    allocated = torch.cuda.memory_allocated()
    _check(model.impute(x, "l"), [t.cpu() for t in s["single"]["l"]], "refused shape, composed again")
    assert calls == [1] and list(model._impute_bufs.values()) == [False]
    monkeypatch.undo()
    x2 = x[:, :5].contiguous()
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() <= allocated + x2.numel() * 4 + 512
    model.impute(x2, "l")
    assert [v is not False for v in model._impute_bufs.values()] == [False, True]


def test_wide_sizes_are_refused_by_the_entry_and_composed():
    cfgs = configs.canonical_configs(dropout=False, zv_size=136)      # encoder_la_to_v: h = 136 > 128
    model, ref = _pair(cfgs)
    T, N = 3, 4
    xn, _ = synth.make_batch(cfgs[0]["input_dims"], N, T, seed=21)
    xc = torch.from_numpy(xn)
    x = xc.cuda()
    with pytest.raises(_lib.MfmUnsupported, match="136"):
        model._impute_fused(x, ("v",), model._impute_params(("v",)), 0)
    assert model._impute_refused and not model.__dict__.get("_impute_bufs")
    _check(model.impute(x, "v"), _oracle_impute(ref, xc, "v"), "wide nov")
    each = model.impute(x, "each")
    for m in MS:
        _check(each[m], _oracle_impute(ref, xc, m), "wide each no%s" % m)
    assert not model.__dict__.get("_impute_bufs")


# ----------------------------------------------------------------------------------- 15. errors
def test_errors_name_the_problem_and_reach_no_kernel(monkeypatch):
    s = _case("small")
    model, x = s["model"], s["x"]
    L, calls = _lib.lib(), []
    real = L.mfm_impute_missing
    monkeypatch.setattr(L, "mfm_impute_missing", lambda *a: (calls.append(1), real(*a))[1], raising=True)
    bufs = dict(model._impute_bufs)
    with pytest.raises(ValueError, match="'l', 'a', 'v' or 'each'"):
        model.impute(x, "la")
    with pytest.raises(ValueError, match="'l', 'a', 'v' or 'each'"):
        model.impute(x, 0)
    with pytest.raises(_lib.MfmError, match="features per time step"):
        model.impute(x[:, :, :-1], "l")
    with pytest.raises(_lib.MfmError, match=r"\[T, N, %d\]" % x.shape[2]):
        model.impute(x[0], "l")
    with pytest.raises(_lib.MfmError, match="input is on cpu"):
        model.impute(x.cpu(), "v")
    with pytest.raises(_lib.MfmError, match="empty split"):
        model.impute(x[:, :0], "each")
    with pytest.raises(_lib.MfmError, match="empty split"):
        model.impute(x[:0], "a")
    with pytest.raises(_lib.MfmError, match="max_rows"):
        model.impute(x, "a", max_rows=0)
    assert not calls and model._impute_bufs == bufs          # the entry was not reached, nothing was allocated
    model.impute(x, "a")                                     # (the counter does count)
    assert calls == [1]
