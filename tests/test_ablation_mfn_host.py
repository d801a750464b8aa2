"""Host-side checks of predict / evaluate of the ablations M_A and M_C (mfm_predict_ablation_mfn, csrc/ablation_mfn.hip): the new
symbols in the header, the library and the binding; the workspace and tile-row queries; the entry's argument checks and refusals,
which answer before anything touches a device; the modules' refusals on the CPU, their pickling and their unchanged state_dict
surface.  No GPU compute here."""
import ctypes as C
import os
import pickle
import re

import pytest
import torch

from factorized_amd import _lib, configs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["mfm_predict_ablation_mfn", "mfm_predict_ablation_mfn_tile_rows", "mfm_predict_ablation_mfn_workspace_floats"]
# d_l d_a d_v | zl za zv | zy | h_l h_a h_v | memsize windowsize | att1 att2 gamma1 gamma2 | heads | fl fa fv fy output_dim loss_kind
SIZES = [300, 5, 20, 32, 8, 80, 32, 88, 64, 48, 64, 2, 128, 128, 128, 128, 0, 88, 8, 8, 16, 1, 0]
ODD = [37, 3, 11, 20, 12, 36, 24, 40, 12, 20, 24, 2, 36, 20, 28, 44, 0, 28, 4, 20, 12, 2, 0]
CLASSES = ("M_A", "M_C")
NP = 66
ZL, HL, WIN, FL, FY = 3, 7, 11, 17, 20          # places in the size array


def _declared():
    src = open(os.path.join(ROOT, "include", "mfm_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return set(re.findall(r"\b(mfm_[a-z0-9_]+)\s*\(", src))


def test_new_symbols_are_declared_exported_and_bound():
    L = _lib.lib()
    declared, bound = _declared(), set(_lib.exported_names())
    for n in NEW:
        assert n in declared, "include/mfm_hip.h does not declare %s" % n
        assert hasattr(L, n), "libmfm_hip.so does not export %s" % n
        assert n in bound, "_lib.py does not bind %s" % n
    assert declared == bound


def test_abi_version_is_still_5():
    assert _lib.lib().mfm_abi_version() == 5 == _lib.ABI_VERSION


def test_the_header_documents_the_families_the_parameter_table_the_refusals_and_the_ticket():
    src = open(os.path.join(ROOT, "include", "mfm_hip.h")).read()
    doc = src[src.index("Prediction of the ablations M_A and M_C"):src.index("int64_t mfm_predict_ablation_mfn_workspace_floats")]
    for word in ("family 0, M_A", "family 1, M_C", "66 DEVICE pointers", "38-55", "56-65", "may be null", "enqueue nothing",
                 "MFM_ERR_UNSUPPORTED", "zl > 128", "above 128", "windowsize other than 2", "ticket word", "the embedding block"):
        assert word in doc, word


def test_workspace_query_equals_the_formula_of_the_header():
    L = _lib.lib()
    T, N = 20, 33
    hp = lambda h: (h + 15) // 16 * 16
    up4 = lambda v: (v + 3) // 4 * 4
    cdiv = lambda a, b: (a + b - 1) // b

    def want(S, family, gen, labels, rows):
        hm, w = S[7:10], (S[FY] + S[FL] if family == 0 else S[FY])
        f = rows * T * 4 * sum(hp(h) for h in hm)
        if family == 0 and gen:
            f += rows * T * 4 * hp(S[ZL])
        f += rows * T * sum(hp(h) for h in hm) + sum(up4(rows * h) for h in hm)
        f += up4(rows * T * S[10]) + up4(rows * T * S[14]) + up4(rows * T * S[15])
        f += up4(rows * w)
        if gen:
            f += 3 * rows * T * hp(w) + up4(sum(cdiv(T * rows, 64) * cdiv(d, 64) for d in S[0:3])) + 12
        if labels:
            f += up4(rows)
        return f + 4

    for S in (SIZES, ODD):
        sz = (C.c_int32 * 23)(*S)
        for family in (0, 1):
            for gen in (0, 1):
                for labels in (0, 1):
                    for cap, rows in ((0, N), (5, 5), (N + 1, N), (1000, N)):
                        got = L.mfm_predict_ablation_mfn_workspace_floats(T, N, sz, family, gen, labels, cap)
                        assert got == want(S, family, gen, labels, rows), (S, family, gen, labels, cap)
    # it does not grow with N beyond the row cap
    sz = (C.c_int32 * 23)(*SIZES)
    assert L.mfm_predict_ablation_mfn_workspace_floats(T, 33, sz, 0, 1, 1, 8) == L.mfm_predict_ablation_mfn_workspace_floats(T, 4000, sz, 0, 1, 1, 8)
    # (T, N, family, with_gen, max_rows)
    for bad in ((0, N, 0, 0, 0), (T, 0, 0, 0, 0), (T, N, 2, 0, 0), (T, N, -1, 0, 0), (T, N, 0, 0, -1), (T, N, 0, 2, 0), (T, N, 1, -1, 0)):
        assert L.mfm_predict_ablation_mfn_workspace_floats(bad[0], bad[1], sz, bad[2], bad[3], 1, bad[4]) == 0, bad
    assert L.mfm_predict_ablation_mfn_workspace_floats(T, N, None, 0, 1, 1, 0) == 0
    for i in (5, 18, 21):
        zero = (C.c_int32 * 23)(*[0 if j == i else v for j, v in enumerate(SIZES)])
        assert L.mfm_predict_ablation_mfn_workspace_floats(T, N, zero, 0, 1, 1, 0) == 0, i


def test_tile_rows_query_counts_the_three_mfn_lstms_whatever_gen():
    """one-row tiles while 3 LSTMs x rows stay below six workgroups per CU, else four-row tiles -- the recurrence launch the same
    with and without gen (encoder_l's workgroups do not count), the decoders' launch 0 without gen"""
    L = _lib.lib()
    cus = L.mfm_device_cus()
    r = (C.c_int32 * 2)()

    def q(N, family, gen, cap=0):
        assert L.mfm_predict_ablation_mfn_tile_rows(N, family, gen, cap, r) == 0
        return list(r)
    for family in (0, 1):
        assert q(2 * cus - 1, family, 1) == [1, 1] and q(2 * cus, family, 1) == [4, 4]
        assert q(2 * cus - 1, family, 0) == [1, 0] and q(2 * cus, family, 0) == [4, 0]
        assert q(6 * cus, family, 1, 2 * cus - 1) == [1, 1] and q(6 * cus, family, 0, 2 * cus) == [4, 0]      # (the row cap counts, not N)
        for N in (cus - 1, cus, 2 * cus, 3 * cus, 6 * cus):
            assert q(N, family, 1)[0] == q(N, family, 0)[0] == L.mfm_predict_mfn_tile_rows(N, 0)
    for bad in ((0, 0, 0, 0), (5, 2, 0, 0), (5, -1, 0, 0), (5, 0, 0, -1), (5, 0, 2, 0), (5, 1, -1, 0)):
        assert L.mfm_predict_ablation_mfn_tile_rows(bad[0], bad[1], bad[2], bad[3], r) == -1, bad
    assert L.mfm_predict_ablation_mfn_tile_rows(5, 0, 0, 0, None) == -1


def _call(T=4, N=6, sizes=SIZES, family=0, with_gen=1, params=None, x=0x1000, y=0x3000, ws=0x2000, y_hat=0x90000, gen=None,
          disc=0x92000, cap=0, null=()):
    """mfm_predict_ablation_mfn on made-up (aligned, never dereferenced) addresses: every call here must be refused by the checks,
    which come before any launch.  gen defaults to what with_gen asks for"""
    L = _lib.lib()
    gen = (0x91000 if with_gen else 0) if gen is None else gen
    sz = None if "sizes" in null else (C.c_int32 * 23)(*sizes)
    prm = None if "params" in null else (C.c_void_p * NP)(*(params or [0x10000 + 64 * i for i in range(NP)]))
    rc = L.mfm_predict_ablation_mfn(T, N, sz, family, with_gen, prm, C.c_void_p(x), C.c_void_p(y), C.c_void_p(ws), C.c_void_p(y_hat),
                                    C.c_void_p(gen), C.c_void_p(disc), cap, None)
    return rc, L.mfm_last_error().decode()


BIG = dict(T=4000, N=(1 << 24) - 1)       # passes every argument check and refusal and is stopped by the row check behind them


def test_argument_checks_answer_without_a_device():
    ptrs = [0x10000 + 64 * i for i in range(NP)]
    at = lambda i, v: [v if j == i else s for j, s in enumerate(SIZES)]
    for null in ("sizes", "params"):
        rc, msg = _call(null=(null,))
        assert rc == -1 and "must not be null" in msg, (null, msg)
    for kw in (dict(x=0), dict(ws=0), dict(y_hat=0)):
        rc, msg = _call(**kw)
        assert rc == -1 and "must not be null" in msg, (kw, msg)
    for kw, word in ((dict(family=2), "family = 2"), (dict(family=-1), "family = -1"), (dict(cap=-1), "row cap -1"), (dict(T=0), "T 0"),
                     (dict(N=0), "N 0"), (dict(N=1 << 24), "2^24"), (dict(sizes=at(5, 0)), "sizes must be positive"),
                     (dict(sizes=at(22, 2)), "loss kind 0 or 1"), (dict(sizes=at(16, 2)), "heads")):
        for family in ((kw["family"],) if "family" in kw else (0, 1)):
            rc, msg = _call(**dict(kw, family=family))
            assert rc == -1 and word in msg, (kw, family, msg)
    # labels and disc come together; so do with_gen and gen
    for family in (0, 1):
        for kw in (dict(y=0), dict(disc=0)):
            rc, msg = _call(family=family, **kw)
            assert rc == -1 and "labels and disc come together" in msg, (family, kw, msg)
        rc, msg = _call(family=family, with_gen=1, gen=0)
        assert rc == -1 and "with_gen and gen come together" in msg, msg
        rc, msg = _call(family=family, with_gen=0, gen=0x91000)
        assert rc == -1 and "with_gen and gen come together" in msg, msg
        rc, msg = _call(family=family, with_gen=2, gen=0x91000)
        assert rc == -1 and "with_gen = 2" in msg, msg
    # a complete call gets as far as the row check, with and without labels, with and without gen, both loss kinds
    for family in (0, 1):
        for kw in (dict(), dict(y=0, disc=0), dict(with_gen=0), dict(with_gen=0, y=0, disc=0), dict(sizes=at(22, 1))):
            rc, msg = _call(**dict(kw, family=family, **BIG))
            assert rc == -1 and "pass a row cap" in msg, (family, kw, msg)
    # a null or misaligned parameter is named; slots that are not read are not looked at
    for i in (0, 13, 29, 37, 38, 55, 56, 65):
        rc, msg = _call(params=[0 if j == i else p for j, p in enumerate(ptrs)])
        assert rc == -1 and "parameter %d is null" % i in msg, (i, msg)
    noenc = [0 if i >= 56 else p for i, p in enumerate(ptrs)]
    nodec = [0 if i >= 38 else p for i, p in enumerate(ptrs)]
    rc, msg = _call(family=1, params=noenc, **BIG)
    assert rc == -1 and "pass a row cap" in msg, msg
    rc, msg = _call(family=0, params=noenc)
    assert rc == -1 and "parameter 56 is null" in msg, msg
    for family in (0, 1):
        rc, msg = _call(family=family, with_gen=0, params=nodec, **BIG)
        assert rc == -1 and "pass a row cap" in msg, msg
        rc, msg = _call(family=family, params=nodec)
        assert rc == -1 and "parameter 38 is null" in msg, msg
    for i in (1, 8, 38, 45, 56, 57):            # LSTM weights: 16 bytes
        rc, msg = _call(params=[p + 4 if j == i else p for j, p in enumerate(ptrs)])
        assert rc == -1 and "parameter %d is misaligned" % i in msg, (i, msg)
    rc, msg = _call(params=[p + 2 if j == 30 else p for j, p in enumerate(ptrs)])
    assert rc == -1 and "parameter 30 is misaligned" in msg, msg
    rc, msg = _call(params=[p + 4 if j in (2, 3, 12, 28, 30, 40, 42, 58, 60, 62) else p for j, p in enumerate(ptrs)], **BIG)      # (4 bytes: fine but for the LSTM weights)
    assert rc == -1 and "pass a row cap" in msg, msg
    rc, msg = _call(x=0x1002)
    assert rc == -1 and "x must be 4-byte aligned" in msg, msg
    rc, msg = _call(ws=0x2004)
    assert rc == -1 and "workspace 16-byte aligned" in msg, msg
    rc, msg = _call(gen=0x91002)
    assert rc == -1 and "misaligned" in msg, msg
    rc, msg = _call(sizes=at(22, 1), y=0x3004)
    assert rc == -1 and "misaligned" in msg, msg
    rc, msg = _call(x=0x1004, y=0x3004, **BIG)      # (x and float labels on 4 bytes are fine)
    assert rc == -1 and "pass a row cap" in msg, msg


def test_sizes_the_launches_do_not_cover_are_refused_as_unsupported_without_a_device():
    """what mfm_predict_mfn refuses (an h_dims entry of 136, windowsize 3) always; with gen alone zl = 136 (M_A) and a decoder
    width of 132 (fy + fl for M_A, fy for M_C); more LDS than a CU has: MFM_ERR_UNSUPPORTED with the size named"""
    at = lambda i, v: [v if j == i else s for j, s in enumerate(SIZES)]
    UNS = _lib.MFM_ERR_UNSUPPORTED
    for family in (0, 1):
        for gen in (0, 1):
            for i in range(3):
                rc, msg = _call(family=family, with_gen=gen, sizes=at(HL + i, 136))
                assert rc == UNS and "h = 136" in msg, (family, gen, i, msg)
            rc, msg = _call(family=family, with_gen=gen, sizes=at(WIN, 3))
            assert rc == UNS and "windowsize 3" in msg, (family, gen, msg)
            rc, msg = _call(family=family, with_gen=gen, sizes=at(10, 600))
            assert rc == UNS and "memory 600" in msg, (family, gen, msg)
    # encoder_l's hidden size: M_A with gen alone
    rc, msg = _call(family=0, sizes=at(ZL, 136))
    assert rc == UNS and "h = 136" in msg, msg
    for kw in (dict(family=0, with_gen=0), dict(family=1), dict(family=1, with_gen=0)):
        rc, msg = _call(sizes=at(ZL, 136), **dict(kw, **BIG))
        assert rc == -1 and "pass a row cap" in msg, (kw, msg)
    # the decoders' width: fy + fl = 16 + 116 for M_A (for M_C fl does not count), fy = 132 for M_C; with gen alone
    rc, msg = _call(family=0, sizes=at(FL, 116))
    assert rc == UNS and "h = 132" in msg, msg
    rc, msg = _call(family=1, sizes=at(FY, 132))
    assert rc == UNS and "h = 132" in msg, msg
    rc, msg = _call(family=0, sizes=at(FL, 112), **BIG)          # (128 is covered)
    assert rc == -1 and "pass a row cap" in msg, msg
    for kw in (dict(family=0, with_gen=0, sizes=at(FL, 116)), dict(family=1, sizes=at(FL, 5000)), dict(family=1, with_gen=0, sizes=at(FY, 132))):
        rc, msg = _call(**dict(kw, **BIG))
        assert rc == -1 and "pass a row cap" in msg, (kw, msg)
    # entries a family does not have may hold anything positive: za, zv, fa, fv everywhere; heads 0 or 1
    for i, v in ((4, 5000), (5, 5000), (18, 5000), (19, 5000), (16, 1)):
        for family in (0, 1):
            rc, msg = _call(family=family, sizes=at(i, v), **BIG)
            assert rc == -1 and "pass a row cap" in msg, (i, family, msg)
    # LDS: the label tail's activations (zy = 30000 floats, twice) do not fit a CU's
    rc, msg = _call(with_gen=0, sizes=at(6, 30000))
    assert rc == UNS and "label tail" in msg and "LDS" in msg, msg


def _model(name, **sizes):
    from factorized_amd import mfm_model as M
    cfgs = configs.canonical_configs(dropout=False, **sizes)
    return getattr(M, name)(*cfgs), cfgs


@pytest.mark.parametrize("name", CLASSES)
def test_predict_and_evaluate_on_a_cpu_model_raise(name):
    model, cfgs = _model(name)
    x = torch.zeros(3, 2, sum(cfgs[0]["input_dims"]))
    y = torch.zeros(2, 1)
    for call in (lambda: model.predict(x), lambda: model.predict(x, y, gen=False), lambda: model.evaluate(x, y)):
        with pytest.raises(_lib.MfmError, match="move the model to the GPU"):
            call()
    with pytest.raises(ValueError, match="'l1' or 'ce'"):
        model.predict(x, y, loss="mse")
    with pytest.raises(ValueError, match="'l1' or 'ce'"):
        model.evaluate(x, y, loss="mse")
    with pytest.raises(_lib.MfmError, match="labels are required"):
        model.evaluate(x, None)
    assert not [k for k in model.__dict__ if k.startswith("_ablation")]      # (nothing was cached on the way to the refusal)


@pytest.mark.parametrize("name,family", zip(CLASSES, range(2)))
def test_sizes_and_parameter_tables(name, family):
    model, _ = _model(name)
    want = list(SIZES)
    want[4] = want[5] = want[18] = want[19] = 1
    if family == 1:
        want[ZL] = want[FL] = 1
    assert list(model._ablation_sizes()) == want and model._ABL_FAMILY == family
    assert model._ABL_NPARAM == NP and model._ABL_ENTRY == "mfm_predict_ablation_mfn" and want[model._ABL_OD] == 1
    nogen = model._ablation_params(False)
    assert len(nogen) == NP and [p is not None for p in nogen] == [i < 38 for i in range(NP)]
    assert tuple(nogen[0].shape) == (4 * 88, 300) and tuple(nogen[5].shape) == (4 * 64, 64) and tuple(nogen[8].shape) == (4 * 48, 20)
    assert tuple(nogen[12].shape) == (128, 400) and tuple(nogen[18].shape) == (64, 128) and tuple(nogen[20].shape) == (128, 464)
    assert tuple(nogen[22].shape) == (64, 128) and tuple(nogen[24].shape) == (128, 464)
    assert tuple(nogen[28].shape) == (32, 264) and tuple(nogen[30].shape) == (16, 32) and tuple(nogen[36].shape) == (1, 16)
    full = model._ablation_params(True)
    w = 104 if family == 0 else 16
    assert len(full) == NP and [p is not None for p in full] == [i < (66 if family == 0 else 56) for i in range(NP)]
    assert tuple(full[38].shape) == (4 * w, w) and tuple(full[42].shape) == (300, w) and tuple(full[48].shape) == (5, w)
    assert tuple(full[54].shape) == (20, w)
    if family == 0:
        assert tuple(full[56].shape) == (4 * 32, 325) and tuple(full[60].shape) == (32, 32) and tuple(full[62].shape) == (88, 32)
        assert tuple(full[64].shape) == (88, 88)
    assert all(a is b for a, b in zip(full, nogen) if b is not None)
    # what a refusal means for the model: an h_dims entry for every call, the decoders' / encoder_l's width for the calls with gen
    at = lambda i, v: [v if j == i else s for j, s in enumerate(want)]
    assert model._ablation_wide(want, True) == () and set(model._ablation_wide(at(8, 136), False)) == {False, True}
    assert model._ablation_wide(at(FY, 132), True) == (True,) and model._ablation_wide(at(FY, 132), False) == ()
    assert model._ablation_wide(at(ZL, 136), True) == ((True,) if family == 0 else ())


@pytest.mark.parametrize("name", CLASSES)
def test_the_module_pickles_and_keeps_its_state_dict_keys(name):
    from oracle import mfm_oracle_extra as X
    model, cfgs = _model(name)
    keys = list(model.state_dict().keys())
    assert keys == list(X.CLASSES[name](*cfgs).state_dict().keys())
    # a stubbed cache entry, as a call leaves it: a ctypes table cannot be pickled, so it has to be dropped
    model._ablation_bufs = {(3, 2, True, False, 1024, "cuda:0"): (torch.zeros(4), (C.c_void_p * NP)())}
    assert list(model.state_dict().keys()) == keys
    clone = pickle.loads(pickle.dumps(model))
    assert "_ablation_bufs" not in clone.__dict__ and "_ablation_bufs" in model.__dict__
    assert list(clone.state_dict().keys()) == keys
    for k, v in model.state_dict().items():
        assert torch.equal(v, clone.state_dict()[k]), k
