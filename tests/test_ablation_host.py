"""Host-side checks of predict / evaluate of the ablations M_B and M_D (mfm_predict_ablation, csrc/ablation.hip): the new symbols
in the header, the library and the binding; the workspace and tile-row queries; the entry's argument checks and refusals, which
answer before anything touches a device; the modules' refusals on the CPU, their pickling and their unchanged state_dict
surface.  No GPU compute here."""
import ctypes as C
import os
import pickle
import re

import pytest
import torch

from factorized_amd import _lib, configs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["mfm_predict_ablation", "mfm_predict_ablation_tile_rows", "mfm_predict_ablation_workspace_floats"]
SIZES = [32, 8, 80, 32, 88, 8, 8, 16, 300, 5, 20, 1]          # zl za zv zy fl fa fv fy d_l d_a d_v output_dim
ODD = [3, 5, 7, 1, 28, 1, 20, 12, 37, 3, 11, 2]
CLASSES = ("M_B", "M_D")
NP = 52


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


def test_the_header_documents_the_families_and_the_parameter_table():
    src = open(os.path.join(ROOT, "include", "mfm_hip.h")).read()
    doc = src[src.index("Prediction of the ablations M_B and M_D"):src.index("int64_t mfm_predict_ablation_workspace_floats")]
    for word in ("family 0, M_B", "family 1, M_D", "52 DEVICE pointers", "enqueue nothing", "may be null", "ticket"):
        assert word in doc, word


def test_workspace_query_equals_the_formula_of_the_header():
    L = _lib.lib()
    T, N = 20, 33
    hp = lambda h: (h + 15) // 16 * 16
    up4 = lambda v: (v + 3) // 4 * 4
    cdiv = lambda a, b: (a + b - 1) // b

    def want(S, gen, labels, rows):
        f = rows * T * 4 * sum(hp(z) for z in S[0:3]) + up4(rows * sum(S[4:7]))
        if gen:
            f += rows * T * sum(hp(v) for v in S[4:7]) + up4(sum(cdiv(T * rows, 64) * cdiv(d, 64) for d in S[8:11])) + 12
        if labels:
            f += up4(rows)
        return f + up4(rows) + 4

    for S in (SIZES, ODD):
        sz = (C.c_int32 * 12)(*S)
        for family in (0, 1):
            for gen in ((0, 1) if family == 0 else (0,)):
                for labels in (0, 1):
                    for cap, rows in ((0, N), (5, 5), (N + 1, N), (1000, N)):
                        got = L.mfm_predict_ablation_workspace_floats(T, N, sz, family, gen, labels, cap)
                        assert got == want(S, gen, labels, rows), (S, family, gen, labels, cap)
    sz = (C.c_int32 * 12)(*SIZES)
    # (T, N, family, with_gen, max_rows)
    for bad in ((0, N, 0, 0, 0), (T, 0, 0, 0, 0), (T, N, 2, 0, 0), (T, N, -1, 0, 0), (T, N, 0, 0, -1), (T, N, 1, 1, 0), (T, N, 0, 2, 0)):
        assert L.mfm_predict_ablation_workspace_floats(bad[0], bad[1], sz, bad[2], bad[3], 1, bad[4]) == 0, bad
    assert L.mfm_predict_ablation_workspace_floats(T, N, None, 0, 1, 1, 0) == 0
    zero = (C.c_int32 * 12)(*[0 if i == 5 else v for i, v in enumerate(SIZES)])
    assert L.mfm_predict_ablation_workspace_floats(T, N, zero, 0, 1, 1, 0) == 0


def test_tile_rows_query_follows_the_six_workgroups_per_cu_rule():
    """one-row tiles while 3 LSTMs x rows of a launch stay below six workgroups per CU, else four-row tiles; the decoders' launch
    is 0 without gen"""
    L = _lib.lib()
    cus = L.mfm_device_cus()
    r = (C.c_int32 * 2)()

    def q(N, family, gen, cap=0):
        assert L.mfm_predict_ablation_tile_rows(N, family, gen, cap, r) == 0
        return list(r)
    assert q(2 * cus - 1, 0, 1) == [1, 1] and q(2 * cus, 0, 1) == [4, 4]
    assert q(2 * cus - 1, 0, 0) == [1, 0] and q(2 * cus, 0, 0) == [4, 0]
    assert q(2 * cus - 1, 1, 0) == [1, 0] and q(2 * cus, 1, 0) == [4, 0]
    assert q(6 * cus, 0, 1, 2 * cus - 1) == [1, 1] and q(6 * cus, 1, 0, 2 * cus) == [4, 0]      # (the row cap counts, not N)
    # ... and agrees with the query of mfm_predict_missing where the launches count the same LSTMs (family 1, all three cases)
    rm = (C.c_int32 * 2)()
    for N in (cus - 1, cus, 2 * cus, 3 * cus, 6 * cus):
        assert L.mfm_predict_missing_tile_rows(N, 1, 7, 0, rm) == 0
        assert q(N, 0, 1) == list(rm)
    for bad in ((0, 0, 0, 0), (5, 2, 0, 0), (5, -1, 0, 0), (5, 0, 0, -1), (5, 1, 1, 0), (5, 0, 2, 0)):
        assert L.mfm_predict_ablation_tile_rows(bad[0], bad[1], bad[2], bad[3], r) == -1, bad
    assert L.mfm_predict_ablation_tile_rows(5, 0, 0, 0, None) == -1


def _call(T=4, N=6, sizes=SIZES, family=0, loss=0, with_gen=None, params=None, x=0x1000, y=0x3000, ws=0x2000, y_hat=0x90000,
          gen=None, disc=0x92000, cap=0, null=()):
    """mfm_predict_ablation on made-up (aligned, never dereferenced) addresses: every call here must be refused by the argument
    checks, which come before any launch.  with_gen / gen default to what the family has"""
    L = _lib.lib()
    with_gen = (1 if family == 0 else 0) if with_gen is None else with_gen
    gen = (0x91000 if with_gen else 0) if gen is None else gen
    sz = None if "sizes" in null else (C.c_int32 * 12)(*sizes)
    prm = None if "params" in null else (C.c_void_p * NP)(*(params or [0x10000 + 64 * i for i in range(NP)]))
    rc = L.mfm_predict_ablation(T, N, sz, family, loss, with_gen, prm, C.c_void_p(x), C.c_void_p(y), C.c_void_p(ws), C.c_void_p(y_hat),
                                C.c_void_p(gen), C.c_void_p(disc), cap, None)
    return rc, L.mfm_last_error().decode()


BIG = dict(T=4000, N=(1 << 24) - 1)       # passes every argument check and is refused by the row check behind them


def test_argument_checks_answer_without_a_device():
    ptrs = [0x10000 + 64 * i for i in range(NP)]
    for null in ("sizes", "params"):
        rc, msg = _call(null=(null,))
        assert rc == -1 and "must not be null" in msg, (null, msg)
    for kw in (dict(x=0), dict(ws=0), dict(y_hat=0)):
        rc, msg = _call(**kw)
        assert rc == -1 and "must not be null" in msg, (kw, msg)
    for kw, word in ((dict(family=2), "family = 2"), (dict(family=-1), "family = -1"), (dict(cap=-1), "row cap -1"), (dict(T=0), "T 0"),
                     (dict(N=0), "N 0"), (dict(loss=2), "loss kind 2"), (dict(N=1 << 24), "2^24"),
                     (dict(sizes=[0 if i == 2 else v for i, v in enumerate(SIZES)]), "size 2 is 0")):
        for family in ((kw["family"],) if "family" in kw else (0, 1)):
            rc, msg = _call(**dict(kw, family=family))
            assert rc == -1 and word in msg, (kw, family, msg)
    # labels and disc come together; so do with_gen and gen; M_D has neither
    for family in (0, 1):
        for kw in (dict(y=0), dict(disc=0)):
            rc, msg = _call(family=family, **kw)
            assert rc == -1 and "labels and disc come together" in msg, (family, kw, msg)
    rc, msg = _call(with_gen=1, gen=0)
    assert rc == -1 and "with_gen and gen come together" in msg, msg
    rc, msg = _call(with_gen=0, gen=0x91000)
    assert rc == -1 and "with_gen and gen come together" in msg, msg
    rc, msg = _call(with_gen=2, gen=0x91000)
    assert rc == -1 and "with_gen = 2" in msg, msg
    for kw in (dict(with_gen=1, gen=0x91000), dict(with_gen=0, gen=0x91000), dict(with_gen=1, gen=0)):
        rc, msg = _call(family=1, **kw)
        assert rc == -1 and "M_D" in msg and "no decoders" in msg, (kw, msg)
    # a complete call gets as far as the row check, with and without labels, with and without gen
    for kw in (dict(), dict(y=0, disc=0), dict(with_gen=0), dict(family=1), dict(family=1, y=0, disc=0)):
        rc, msg = _call(**dict(kw, **BIG))
        assert rc == -1 and "pass a row cap" in msg, (kw, msg)
    # a null or misaligned parameter is named; slots that are not read are not looked at
    rc, msg = _call(params=[0 if i == 24 else p for i, p in enumerate(ptrs)])
    assert rc == -1 and "parameter 8 of modality 1 is null" in msg, msg
    rc, msg = _call(params=[0 if i == 44 else p for i, p in enumerate(ptrs)])
    assert rc == -1 and "parameter 12 of modality 2 is null" in msg, msg
    rc, msg = _call(params=[0 if i == 51 else p for i, p in enumerate(ptrs)])
    assert rc == -1 and "label-head parameter 3" in msg, msg
    rc, msg = _call(family=1, params=[0 if i == 49 else p for i, p in enumerate(ptrs)])
    assert rc == -1 and "label-head parameter 1" in msg, msg
    nodec = [0 if i < 48 and i % 16 >= 10 else p for i, p in enumerate(ptrs)]
    rc, msg = _call(with_gen=0, params=nodec, **BIG)
    assert rc == -1 and "pass a row cap" in msg, msg
    rc, msg = _call(family=1, params=[0 if i >= 50 else p for i, p in enumerate(nodec)], **BIG)
    assert rc == -1 and "pass a row cap" in msg, msg
    rc, msg = _call(params=nodec)
    assert rc == -1 and "parameter 10 of modality 0 is null" in msg, msg
    rc, msg = _call(params=[p + 4 if i == 17 else p for i, p in enumerate(ptrs)])
    assert rc == -1 and "parameter 1 of modality 1 is misaligned" in msg, msg
    rc, msg = _call(params=[p + 4 if i == 10 else p for i, p in enumerate(ptrs)])
    assert rc == -1 and "parameter 10 of modality 0 is misaligned" in msg, msg
    rc, msg = _call(params=[p + 2 if i == 2 else p for i, p in enumerate(ptrs)])
    assert rc == -1 and "parameter 2 of modality 0 is misaligned" in msg, msg
    rc, msg = _call(params=[p + 4 if i in (2, 4, 6, 14, 48) else p for i, p in enumerate(ptrs)], **BIG)      # (4 bytes: fine but for the LSTM weights)
    assert rc == -1 and "pass a row cap" in msg, msg
    rc, msg = _call(x=0x1002)
    assert rc == -1 and "x must be 4-byte aligned" in msg, msg
    rc, msg = _call(ws=0x2004)
    assert rc == -1 and "workspace 16-byte aligned" in msg, msg
    rc, msg = _call(gen=0x91002)
    assert rc == -1 and "misaligned" in msg, msg
    rc, msg = _call(loss=1, y=0x3004)
    assert rc == -1 and "misaligned" in msg, msg
    rc, msg = _call(x=0x1004, y=0x3004, **BIG)      # (x and float labels on 4 bytes are fine)
    assert rc == -1 and "pass a row cap" in msg, msg


def test_sizes_the_launches_do_not_cover_are_refused_as_unsupported_without_a_device():
    """a z_m above 128 always, an f_m above 128 with gen (a decoder's hidden size) and only then; more LDS than a CU has; a label
    head whose input row does not fit: MFM_ERR_UNSUPPORTED with the size named"""
    at = lambda i, v: [v if j == i else s for j, s in enumerate(SIZES)]
    for i in range(3):
        for family in (0, 1):
            for gen in ((0, 1) if family == 0 else (0,)):
                rc, msg = _call(family=family, with_gen=gen, sizes=at(i, 136))
                assert rc == _lib.MFM_ERR_UNSUPPORTED and "136" in msg, (i, family, gen, msg)
        rc, msg = _call(sizes=at(4 + i, 136))
        assert rc == _lib.MFM_ERR_UNSUPPORTED and "h = 136" in msg, (i, msg)
        for family in (0, 1):
            rc, msg = _call(family=family, with_gen=0, sizes=at(4 + i, 136), **BIG)
            assert rc == -1 and "pass a row cap" in msg, (i, family, msg)
    # unused entries may hold anything positive: zy everywhere, fy for M_D
    rc, msg = _call(sizes=at(3, 5000), **BIG)
    assert rc == -1 and "pass a row cap" in msg, msg
    rc, msg = _call(family=1, sizes=at(7, 1 << 20), **BIG)
    assert rc == -1 and "pass a row cap" in msg, msg
    # the label head: fl + fa + fv = 3 x 4000 floats a row, four rows a workgroup (N large enough) -> beyond 160 KB
    wide = [4000 if 4 <= j < 7 else s for j, s in enumerate(SIZES)]
    cus = _lib.lib().mfm_device_cus()
    rc, msg = _call(with_gen=0, sizes=wide, N=2 * cus)
    assert rc == _lib.MFM_ERR_UNSUPPORTED and "label head" in msg and "12000" in msg, msg
    rc, msg = _call(family=1, sizes=wide, N=2 * cus)
    assert rc == _lib.MFM_ERR_UNSUPPORTED and "label head" in msg and "12000" in msg, msg
    # the MLP's activations of a one-row workgroup fit, those of a four-row one do not
    rc, msg = _call(with_gen=0, sizes=at(4, 6000), N=2 * cus)
    assert rc == _lib.MFM_ERR_UNSUPPORTED and "bytes of LDS" in msg and "6000" in msg, msg
    rc, msg = _call(with_gen=0, sizes=at(4, 6000), N=2 * cus, cap=7, T=1 << 20)
    assert rc == -1 and "pass a row cap" in msg, msg


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
    want = {0: [32, 8, 80, 1, 88, 8, 8, 16, 300, 5, 20, 1], 1: [32, 8, 80, 1, 88, 8, 8, 1, 300, 5, 20, 1]}[family]
    assert list(model._ablation_sizes()) == want and model._ABL_FAMILY == family
    nodec = model._ablation_params(False)
    assert len(nodec) == NP
    assert [p is not None for p in nodec] == [(i < 48 and i % 16 < 10) or 48 <= i < (52 if family == 0 else 50) for i in range(NP)]
    assert tuple(nodec[0].shape) == (4 * 32, 300) and tuple(nodec[16].shape) == (4 * 8, 5) and tuple(nodec[33].shape) == (4 * 80, 80)
    assert tuple(nodec[6].shape) == (88, 32) and tuple(nodec[8].shape) == (88, 88) and tuple(nodec[4].shape) == (32, 32)
    assert tuple(nodec[48].shape) == ((16, 104) if family == 0 else (1, 104))
    if family == 0:
        full = model._ablation_params(True)
        assert len(full) == NP and all(p is not None for p in full)
        assert tuple(full[10].shape) == (4 * 88, 88) and tuple(full[11].shape) == (4 * 88, 88) and tuple(full[14].shape) == (300, 88)
        assert tuple(full[50].shape) == (1, 16)
        assert all(a is b for a, b in zip(full, nodec) if b is not None)


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
