"""The ABI contract of the grouped GEMM (include/mfm_hip.h: MfmGemmDesc, mfm_gemm_grouped_f32 / _bf16) against the float64
descriptor reference of tests/gemm_ref.py, at the forms the other GEMM tests (test_gpu_ops.py, test_gpu_bf16.py) do not reach:
oddly strided operands (gemm_f32_kernel<FR, false>) alone and mixed into a group of unit-stride products, accumulate onto
non-zero outputs with explicit splits, alpha with both biases, batched b and bias, k = 0, K-loop ring edges, finite neighbours of
any size behind a row, base pointers off 16 bytes, stores around C, and operand spans beyond the kernels' 32-bit byte offsets.

Tolerances are the project's own (tests.cases.rel_err, as test_gpu_ops.py / test_gpu_bf16.py hold the same kernels): 2e-6 for
plain fp32 products, 5e-6 where atomics add parts; bf16 operands 1e-5 (2e-5 with atomics) against the reference with A and B
rounded to bf16.  All shapes are tiny: a tile is 32, 64 or 128 wide, a K stage 32 (fp32) or 64 (bf16) deep."""
import numpy as np
import pytest
import torch

from tests import gemm_ref as R
from tests import mfn_entries as E
from tests.cases import rel_err

pytestmark = pytest.mark.gpu

FR_ALL = ["auto", "1", "2", "4"]       # the gemm_fr fixture of test_gpu_ops.py
FR_TILES = ["1", "2", "4"]
F32, BF16 = "f32", "bf16"
TOL = {(F32, False): 2e-6, (F32, True): 5e-6, (BF16, False): 1e-5, (BF16, True): 2e-5}   # (precision, atomics)
BIG = np.float32(3e38)


@pytest.fixture(scope="module")
def eng():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from factorized_amd import engine
    return engine


def _set_fr(monkeypatch, fr):
    if fr == "auto":
        monkeypatch.delenv("MFM_GEMM_FR", raising=False)
    else:
        monkeypatch.setenv("MFM_GEMM_FR", fr)


@pytest.fixture(params=FR_ALL)
def gemm_fr(request, monkeypatch):
    """tile size of the grouped GEMM: 32x32, 64x64, 128x128 or the launcher's own choice (as in test_gpu_ops.py)"""
    _set_fr(monkeypatch, request.param)
    return request.param


@pytest.fixture(params=FR_TILES)
def gemm_tile(request, monkeypatch):
    _set_fr(monkeypatch, request.param)
    return request.param


def launch(eng, descs, prec=F32):
    if prec == F32:
        eng.gemm_grouped(descs)
    else:
        from factorized_amd import _lib
        arr = (_lib.GemmDesc * len(descs))(*descs)
        _lib.check(_lib.lib().mfm_gemm_grouped_bf16(arr, len(descs), None), "mfm_gemm_grouped_bf16")
    torch.cuda.synchronize()


def dev_at(host, r=0):
    """the flat host array on the device, starting r floats into its allocation"""
    host = np.ascontiguousarray(host, dtype=np.float32).reshape(-1)
    big = torch.zeros(host.size + r, device="cuda")
    view = big[r:]
    view.copy_(torch.from_numpy(host))
    return view


# ------------------------------------------------------------------------------------------ operand layouts
# name -> (allocation shape, row stride, column stride) of a [rows, cols] operand; rows = m (A) or n (B), cols = k
LAYOUTS = {
    "kc": lambda r, c: (r * c, c, 1),                             # k-contiguous, dense
    "kc3": lambda r, c: (r * (c + 3), c + 3, 1),                  # k-contiguous rows of a wider matrix
    "rc": lambda r, c: (c * r, 1, r),                             # m-/n-contiguous, dense
    "rc5": lambda r, c: (c * (r + 5), 1, r + 5),                  # m-/n-contiguous with a leading dimension of rows + 5
    "odd2": lambda r, c: (r * (2 * c + 1), 2 * c + 1, 2),         # every second column of a wider matrix
    "oddT": lambda r, c: (c * (2 * r + 1), 2, 2 * r + 1),         # the transposed view of such a slice
}
FORMS = {"kcontig": ("kc", "kc3"), "rcontig": ("rc", "rc5"), "odd": ("odd2", "oddT")}


class Prob:
    """one problem: host allocations, the descriptor's keywords, device copies, reference"""

    def __init__(self, rs, m, n, k, la="kc", lb="kc", n_valid=None, batch=1, shared=(), prefill=7.0, biases=0, c2=False,
                 ldc=None, a_alloc=None, b_alloc=None, **kw):
        self.m, self.n, self.k = m, n, k
        nv = n if n_valid is None else n_valid
        kk = max(k, 1)                                  # k = 0: a and b still address one element
        asz, a_sr, a_sc = LAYOUTS[la](m, kk)
        bsz, b_sr, b_sc = LAYOUTS[lb](max(nv, 1), kk)
        ldc = n if ldc is None else ldc
        self.kw = dict(a_sm=a_sr, a_sk=a_sc, b_sn=b_sr, b_sk=b_sc, ldc=ldc, n_valid=nv, batch=batch,
                       a_sz=0 if "a" in shared else (asz if batch > 1 else 0),
                       b_sz=0 if "b" in shared else (bsz if batch > 1 else 0),
                       c_sz=m * ldc if batch > 1 else 0,
                       bias_sz=0 if "bias" in shared else (nv if batch > 1 and biases else 0))
        self.kw.update(kw)
        na = asz * (1 if "a" in shared else batch)
        nb = bsz * (1 if "b" in shared else batch)
        self.h = dict(a=rs.normal(size=na).astype(np.float32) if a_alloc is None else a_alloc,
                      b=rs.normal(size=nb).astype(np.float32) if b_alloc is None else b_alloc,
                      bias=None, bias2=None, c2=None)
        nbias = nv * (1 if "bias" in shared else batch)
        if biases >= 1:
            self.h["bias"] = rs.normal(size=nbias).astype(np.float32)
        if biases >= 2:
            self.h["bias2"] = rs.normal(size=nbias).astype(np.float32)
        csz = batch * m * ldc
        if prefill == "random":
            self.h["c"] = rs.normal(size=csz).astype(np.float32)
            if c2:
                self.h["c2"] = rs.normal(size=csz).astype(np.float32)
        else:
            self.h["c"] = np.full(csz, prefill, np.float32)
            if c2:
                self.h["c2"] = np.full(csz, prefill + 1.0, np.float32)
        self.atomics = bool(self.kw.get("accumulate", 0))
        self.d = {}

    def upload(self, offs=None, c_views=None):
        offs = offs or {}
        self.d = {key: (None if v is None else dev_at(v, offs.get(key, 0))) for key, v in self.h.items()}
        for key, view in (c_views or {}).items():           # outputs placed by the caller (canary frames)
            view.copy_(torch.from_numpy(self.h[key]))
            self.d[key] = view
        return self

    def desc(self, eng, **over):
        d = self.d
        return eng.make_gemm(d["a"], d["b"], d["c"], self.m, self.n, self.k, bias=d["bias"], bias2=d["bias2"], c2=d["c2"],
                             **dict(self.kw, **over))

    def ref(self, round_bf16=False):
        h = self.h
        out = R.expected(h["a"], h["b"], h["c"], self.m, self.n, self.k, bias=h["bias"], bias2=h["bias2"], c2=h["c2"],
                         round_bf16=round_bf16, **self.kw)
        return out if h["c2"] is not None else (out, None)

    def outs(self):
        return (self.d["c"].cpu().numpy().copy(), None if self.d["c2"] is None else self.d["c2"].cpu().numpy().copy())

    def regions(self):
        return R.regions(self.h["c"].size, self.m, self.n, self.kw["n_valid"], self.kw["batch"], self.kw["c_sz"], self.kw["ldc"])

    def hold(self, prec=F32, tol=None, tag="", round_bf16=None):
        """both outputs against the reference: the valid elements to `tol`, the pad columns exact zeros (their prefill,
        bit for bit, under accumulate), everything else in the allocation bit for bit what it was -> the errors"""
        tol = TOL[(prec, self.atomics)] if tol is None else tol
        refs = self.ref(round_bf16=(prec == BF16) if round_bf16 is None else round_bf16)
        valid, pad, rest = self.regions()
        errs = []
        for key, out, ref in zip(("c", "c2"), self.outs(), refs):
            if ref is None:
                continue
            init = self.h[key]
            err = rel_err(out[valid], ref[valid])
            print("gemm-contract %s %s: rel err %.3e (bound %.1e)" % (tag, key, err, tol))
            assert err < tol, (tag, key, err)
            if self.atomics:
                assert np.array_equal(out[pad].view(np.int32), init[pad].view(np.int32)), (tag, key, "pad columns moved")
            else:
                assert np.all(out[pad] == 0.0), (tag, key, "pad columns not zero")
            assert np.array_equal(out[rest].view(np.int32), init[rest].view(np.int32)), (tag, key, "stored outside C")
            errs.append(err)
        return errs


# ------------------------------------------------------------------------------------------ layout matrix
@pytest.mark.parametrize("m,n,k", [(33, 31, 37), (65, 5, 97), (129, 33, 4)])
@pytest.mark.parametrize("fb", list(FORMS))
@pytest.mark.parametrize("fa", list(FORMS))
def test_layout_matrix(eng, gemm_tile, fa, fb, m, n, k):
    """every pairing of a k-contiguous, an m-/n-contiguous and an oddly strided operand; both variants of each form"""
    rs = np.random.RandomState(m + k)
    for v in (0, 1):
        p = Prob(rs, m, n, k, la=FORMS[fa][v], lb=FORMS[fb][v], n_valid=n - 2).upload()
        launch(eng, [p.desc(eng)])
        p.hold(tag="%s x %s" % (FORMS[fa][v], FORMS[fb][v]))


# ------------------------------------------------------------------------------------------ mixed groups
def _mixed(rs):
    fwd = Prob(rs, 37, 21, 45, la="kc3", lb="kc", n_valid=19, biases=1)                        # x W^T + b
    wg = Prob(rs, 30, 27, 140, la="rc5", lb="rc", batch=4, prefill="random", accumulate=1, split_k=0)  # dW += dA^T X per gate
    odd = Prob(rs, 19, 9, 23, la="odd2", lb="oddT")
    return fwd, wg, odd


@pytest.mark.parametrize("odd_first", [True, False])
def test_mixed_group_with_one_odd_member(eng, gemm_fr, odd_first):
    """One oddly strided operand sends the whole launch to the dword kernel: the unit-stride members beside it must come out
    as they do in a launch of their own."""
    fwd, wg, odd = [p.upload() for p in _mixed(np.random.RandomState(11))]
    group = [odd, fwd, wg] if odd_first else [fwd, wg, odd]
    launch(eng, [p.desc(eng) for p in group])
    with_odd = {}
    for name, p in (("fwd", fwd), ("wgrad", wg), ("odd", odd)):
        p.hold(tag="mixed/%s" % name)
        with_odd[name] = p.outs()[0]
    fwd2, wg2, _ = [p.upload() for p in _mixed(np.random.RandomState(11))]        # the control: the same without the odd member
    launch(eng, [fwd2.desc(eng), wg2.desc(eng)])
    for name, p in (("fwd", fwd2), ("wgrad", wg2)):
        p.hold(tag="control/%s" % name)
        valid = p.regions()[0]
        assert rel_err(with_odd[name][valid], p.outs()[0][valid].astype(np.float64)) < TOL[(F32, p.atomics)], name


# ------------------------------------------------------------------------------------------ bf16 entry, odd group
def test_bf16_entry_runs_an_odd_group_in_fp32(eng, gemm_tile):
    rs = np.random.RandomState(21)

    def members():
        rs2 = np.random.RandomState(22)
        return Prob(rs2, 37, 21, 96, la="kc3", lb="kc", biases=1), Prob(rs2, 30, 27, 70, la="rc5", lb="rc")
    odd = Prob(rs, 19, 9, 23, la="odd2", lb="kc").upload()
    fwd, wg = [p.upload() for p in members()]
    launch(eng, [fwd.desc(eng), odd.desc(eng), wg.desc(eng)], BF16)
    valid = fwd.regions()[0]
    for name, p in (("fwd", fwd), ("wgrad", wg), ("odd", odd)):
        p.hold(prec=F32, tag="bf16-entry+odd/%s" % name)                   # the fp32 result, to the fp32 bound
        v = p.regions()[0]
        away = rel_err(p.outs()[0][v], p.ref(round_bf16=True)[0][v])
        print("bf16-entry+odd/%s: distance from the bf16-rounded product %.3e" % (name, away))
        if p.k >= 64:
            assert away > 1e-4, name
    fwd2, wg2 = [p.upload() for p in members()]                              # without the odd member: bf16 operands
    launch(eng, [fwd2.desc(eng), wg2.desc(eng)], BF16)
    fwd2.hold(prec=BF16, tag="bf16-entry/fwd")
    wg2.hold(prec=BF16, tag="bf16-entry/wgrad")
    assert rel_err(fwd2.outs()[0][valid], fwd2.ref()[0][valid]) > 1e-4      # and that one really is bf16 arithmetic


def test_bf16_resident_operands_refused_in_an_odd_group(eng):
    from factorized_amd import _lib
    rs = np.random.RandomState(23)
    odd = Prob(rs, 19, 9, 23, la="odd2", lb="kc").upload()
    m, n, k = 16, 8, 64
    a16 = torch.zeros(m, k, device="cuda", dtype=torch.bfloat16)
    b = torch.zeros(n, k, device="cuda")
    c = torch.full((m, n), 7.0, device="cuda")
    c16 = torch.zeros(m, n, device="cuda", dtype=torch.bfloat16)
    a = torch.zeros(m, k, device="cuda")
    res_a = eng.make_gemm(a16, b, c, m, n, k, a_sm=k, a_sk=1, b_sk=1, b_sn=k, ldc=n, a_bf16=True)
    res_c = eng.make_gemm(a, b, c16, m, n, k, a_sm=k, a_sk=1, b_sk=1, b_sn=k, ldc=n, c_bf16=True)
    text = "bf16-resident operands need unit-stride operands in the whole group"
    for d in (res_a, res_c):
        with pytest.raises(_lib.MfmError, match=text):
            launch(eng, [d, odd.desc(eng)], BF16)
        with pytest.raises(_lib.MfmError, match=text):
            launch(eng, [odd.desc(eng), d], BF16)
    assert bool((c == 7.0).all()) and not bool(c16.float().any())           # refused before anything ran
    launch(eng, [res_a, res_c], BF16)                                        # the same descriptors are taken without the odd member


# ------------------------------------------------------------------------------------------ K edges
K_EDGES = [0, 1, 3, 4, 5, 31, 32, 33, 63, 64, 65, 97, 129]


@pytest.mark.parametrize("prec", [F32, BF16])
@pytest.mark.parametrize("la,lb", [("kc", "kc"), ("rc", "rc")])
def test_k_edges(eng, gemm_tile, la, lb, prec):
    """the register ring (3 / 2 / 1 tiles of 32 in flight, two LDS images; bf16: stages of 64) at tile counts 0..5 with last
    tiles of 1, 3, 4, 5 and 31..33 elements, with a bias, pad columns and rows that end inside a tile"""
    rs = np.random.RandomState(31)
    for k in K_EDGES:
        p = Prob(rs, 33, 17, k, la=la, lb=lb, n_valid=16, biases=1).upload()
        launch(eng, [p.desc(eng)], prec)
        p.hold(prec=prec, tag="k=%d %sx%s %s" % (k, la, lb, prec))


@pytest.mark.parametrize("prec", [F32, BF16])
@pytest.mark.parametrize("la,lb", [("kc", "kc"), ("rc", "rc")])
def test_k_zero_is_the_bias(eng, gemm_fr, la, lb, prec):
    rs = np.random.RandomState(32)
    m, n = 33, 17
    p = Prob(rs, m, n, 0, la=la, lb=lb, biases=1).upload()
    launch(eng, [p.desc(eng)], prec)
    assert np.array_equal(p.outs()[0].reshape(m, n).view(np.int32), np.broadcast_to(p.h["bias"], (m, n)).view(np.int32))
    p = Prob(rs, m, n, 0, la=la, lb=lb).upload()
    launch(eng, [p.desc(eng)], prec)
    assert np.all(p.outs()[0] == 0.0)
    # accumulate: the bias (b1 + b2 summed in fp32, then one atomic add) exactly once, whatever split is asked for
    for split in (1, 4, 0):
        p = Prob(rs, m, n, 0, la=la, lb=lb, biases=2, prefill="random", c2=True, accumulate=1, split_k=split).upload()
        launch(eng, [p.desc(eng)], prec)
        bsum = (p.h["bias"] + p.h["bias2"]).astype(np.float32)
        for key, out in zip(("c", "c2"), p.outs()):
            want = (p.h[key].reshape(m, n) + bsum[None, :]).astype(np.float32)
            assert np.array_equal(out.reshape(m, n).view(np.int32), want.view(np.int32)), (key, split)


# ------------------------------------------------------------------------------------------ accumulate, split, alpha, bias, c2
@pytest.mark.parametrize("prec", [F32, BF16])
@pytest.mark.parametrize("split", [1, 2, 5, 0])
def test_accumulate_split_alpha_biases_dual_output(eng, gemm_fr, split, prec):
    """C0 + 0.5 A B + b1 + b2 onto DIFFERENT non-zero C and C2: a store in place of an add, a bias added per split or scaled
    by alpha, or a pad column touched all show.  split 5 at k = 33 collapses to two splits (one for bf16's 64-deep stage)."""
    rs = np.random.RandomState(41)
    for (la, lb) in (("rc5", "rc"), ("kc3", "kc")):
        for k in (33, 130, 300):
            p = Prob(rs, 35, 22, k, la=la, lb=lb, n_valid=19, biases=2, prefill="random", c2=True, accumulate=1,
                     split_k=split, alpha=0.5).upload()
            launch(eng, [p.desc(eng)], prec)
            p.hold(prec=prec, tag="acc split=%d k=%d %s %s" % (split, k, la, prec))


@pytest.mark.parametrize("prec", [F32, BF16])
def test_plain_product_writes_both_outputs(eng, gemm_fr, prec):
    rs = np.random.RandomState(42)
    p = Prob(rs, 35, 22, 70, la="kc3", lb="rc5", n_valid=19, biases=2, c2=True, alpha=0.5).upload()
    launch(eng, [p.desc(eng)], prec)
    p.hold(prec=prec, tag="plain c2 %s" % prec)
    c, c2 = p.outs()
    assert np.array_equal(c.view(np.int32), c2.view(np.int32))


@pytest.mark.parametrize("prec", [F32, BF16])
def test_split_without_accumulate_is_refused(eng, prec):
    from factorized_amd import _lib
    p = Prob(np.random.RandomState(43), 35, 22, 130).upload()
    with pytest.raises(_lib.MfmError, match="split_k needs accumulate"):
        launch(eng, [p.desc(eng, split_k=2)], prec)
    assert np.all(p.outs()[0] == 7.0)


# ------------------------------------------------------------------------------------------ batch strides
@pytest.mark.parametrize("prec", [F32, BF16])
@pytest.mark.parametrize("shared", [(), ("a",), ("bias",)], ids=["all-strided", "a-shared", "bias-shared"])
def test_batch_strides(eng, gemm_fr, shared, prec):
    rs = np.random.RandomState(51)
    p = Prob(rs, 35, 22, 70, la="kc3", lb="rc5", n_valid=19, batch=3, shared=shared, biases=2).upload()
    assert all(p.kw[s] != 0 for s in ("a_sz", "b_sz", "c_sz", "bias_sz") if s[:-3] not in shared)
    assert all(p.kw[s + "_sz"] == 0 for s in shared)
    launch(eng, [p.desc(eng)], prec)
    p.hold(prec=prec, tag="batch %s %s" % (shared, prec))


# ------------------------------------------------------------------------------------------ neighbours and stores
def _slice_of(rs, lay, rows, cols, fill):
    """an operand as a slice of a larger array whose other elements are `fill` (None: +-3e38 with random signs) ->
    the allocation; the operand's own elements come from rs in either case"""
    size, sr, sc = LAYOUTS[lay](rows, cols)
    own = R.index(1, rows, cols, 0, sr, sc).reshape(-1)
    signs = np.where(rs.randint(0, 2, size) > 0, BIG, -BIG).astype(np.float32)
    alloc = signs if fill is None else np.full(size, fill, np.float32)
    alloc[own] = rs.normal(size=own.size).astype(np.float32)
    return alloc


@pytest.mark.parametrize("prec", [F32, BF16])
@pytest.mark.parametrize("form", ["plain", "accumulate", "c2"])
@pytest.mark.parametrize("la,lb", [("kc3", "kc3"), ("rc5", "rc5"), ("kc3", "rc5")])
def test_finite_neighbours_have_no_effect_and_stores_stay_inside(eng, gemm_fr, la, lb, form, prec):
    """The 16-byte fetches read up to three elements behind a row's K range (k % 4 = 1 here) and behind m / n_valid of an
    m-/n-contiguous operand (m % 4 = 1, n_valid % 4 = 3) and zero them by a multiply: +-3e38 there must give the bits that
    zeros give.  C has ldc = n + 3 and sits in a canary frame; the gap columns hold the canary too."""
    m, n, k, nv = 33, 21, 37, 19
    ldc = n + 3
    kw = dict(accumulate=1, split_k=1) if form == "accumulate" else {}
    got = {}
    for fill in (None, 0.0):
        rs = np.random.RandomState(61)                      # the same draws for the operands' own elements
        a_alloc, b_alloc = _slice_of(rs, la, m, k, fill), _slice_of(rs, lb, nv, k, fill)
        p = Prob(rs, m, n, k, la=la, lb=lb, n_valid=nv, ldc=ldc, biases=1, prefill="random", c2=(form == "c2"),
                 a_alloc=a_alloc, b_alloc=b_alloc, **kw)
        rest = p.regions()[2]
        frames, views = {}, {}
        for key in ("c", "c2") if form == "c2" else ("c",):
            p.h[key][rest] = np.array([E.CANARY], np.int32).view(np.float32)[0]      # the gap columns [n, ldc)
            frames[key], views[key] = E.canary(p.h[key].size)
        p.upload(c_views=views)
        launch(eng, [p.desc(eng)], prec)
        p.hold(prec=prec, tag="neighbours %s %sx%s fill=%s %s" % (form, la, lb, fill, prec))   # includes the gap columns, bit for bit
        for key in frames:
            assert E.intact(frames[key], p.h[key].size), (key, "canary frame")
        got[fill] = [o for o in p.outs() if o is not None]
    for big, zero in zip(got[None], got[0.0]):              # (accumulate at split 1 is one atomic add per element: deterministic too)
        assert np.array_equal(big.view(np.int32), zero.view(np.int32))


# ------------------------------------------------------------------------------------------ base pointers off 16 bytes
@pytest.mark.parametrize("prec", [F32, BF16])
@pytest.mark.parametrize("r", [1, 2, 3])
def test_base_pointers_off_16_bytes(eng, gemm_fr, r, prec):
    """a, b, c and bias each r floats into their allocation: buffer_load_dwordx4 needs 4-byte alignment only, so the result is
    the aligned run's, bit for bit"""
    outs = {}
    for off in (0, r):
        rs = np.random.RandomState(71)
        fwd = Prob(rs, 37, 21, 45, la="kc3", lb="kc", n_valid=19, biases=1)
        wg = Prob(rs, 30, 27, 70, la="rc5", lb="rc", biases=1)
        offs = dict(a=off, b=off, c=off, bias=off)
        for p in (fwd, wg):
            p.upload(offs)
            assert all(p.d[key].data_ptr() % 16 == 4 * off for key in offs)
        launch(eng, [fwd.desc(eng), wg.desc(eng)], prec)
        fwd.hold(prec=prec, tag="offset %d fwd %s" % (off, prec))
        wg.hold(prec=prec, tag="offset %d wgrad %s" % (off, prec))
        outs[off] = (fwd.outs()[0], wg.outs()[0])
    for a, b in zip(outs[0], outs[r]):
        assert np.array_equal(a.view(np.int32), b.view(np.int32))


# ------------------------------------------------------------------------------------------ large spans
@pytest.mark.parametrize("prec", [F32, BF16])
@pytest.mark.parametrize("a_sm", [2 ** 29 + 4, 2 ** 30 + 4], ids=["2^29+4", "2^30+4"])
def test_large_operand_span_is_right_or_refused(eng, a_sm, prec):
    """A 2-row operand whose rows lie a_sm elements apart (one untouched allocation, two rows written).  The kernels carry
    32-bit byte offsets: the call either returns the right product or is refused with the operand and its span in the
    message -- never a wrong C."""
    from factorized_amd import _lib
    m, n, k = 2, 8, 16
    rs = np.random.RandomState(81)
    A = rs.normal(size=(m, k)).astype(np.float32)
    W = rs.normal(size=(n, k)).astype(np.float32)
    span = (m - 1) * a_sm + k
    big = torch.empty(span, device="cuda")
    try:
        big[:k].copy_(torch.from_numpy(A[0]))
        big[a_sm:a_sm + k].copy_(torch.from_numpy(A[1]))
        w_d = dev_at(W)
        c = torch.full((m, n), 7.0, device="cuda")
        d = eng.make_gemm(big, w_d, c, m, n, k, a_sm=a_sm, a_sk=1, b_sk=1, b_sn=k, ldc=n)
        try:
            launch(eng, [d], prec)
        except _lib.MfmError as e:
            print("span %d refused: %s" % (span, e))
            assert "operand a spans %d elements" % span in str(e)
            assert bool((c == 7.0).all())
        else:
            ref = (R.bf16_round(A) @ R.bf16_round(W).T) if prec == BF16 else A.astype(np.float64) @ W.T.astype(np.float64)
            err = rel_err(c.cpu().numpy(), ref)
            print("span %d taken: rel err %.3e" % (span, err))
            assert err < TOL[(prec, False)]
    finally:
        del big
        torch.cuda.empty_cache()
