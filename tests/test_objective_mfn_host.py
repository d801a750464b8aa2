"""mfm_objective_mfn without a GPU: the symbols and their prototypes, the workspace formula of include/mfm_hip.h term by term, the
argument checks that run before anything touches a device (the Gaussian sample's among them), what engine.objective refuses on
the host, and the fixtures against the CPU oracle."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from factorized_amd import _lib, configs, engine, synth
from tests import cases
from tests.mfn_entries import CANON_SIZES as CANON, hp as _hp, odd_cfgs, ODD_SIZES as ODD, up4 as _up4

NEW = ["mfm_objective_mfn", "mfm_objective_mfn_tile_rows", "mfm_objective_mfn_workspace_floats"]
CANON_MMD = CANON[:16] + (0,) + CANON[17:]
FIELDS = ("loss", "disc", "gen_l", "gen_a", "gen_v", "reg")


def _formula(T, N, sz, max_rows):
    """the workspace of mfm_objective_mfn as include/mfm_hip.h states it, term by term"""
    rows = min(N, max_rows) if max_rows > 0 else N
    d = sz[0:3]
    z = sz[3:7]
    hl, ha, hv = sz[7:10]
    M, g1, g2, heads = sz[10], sz[14], sz[15], sz[16]
    fl, fa, fv, fy, od = sz[17:22]
    hsum = _hp(hl) + _hp(ha) + _hp(hv)
    total = (max(rows * T * 4 * (hsum + _hp(z[0]) + _hp(z[1]) + _hp(z[2])), rows * T * (_hp(fy + fl) + _hp(fy + fa) + _hp(fy + fv)))
             + rows * T * hsum
             + _up4(rows * hl) + _up4(rows * ha) + _up4(rows * hv)
             + _up4(rows * T * M) + _up4(rows * T * g1) + _up4(rows * T * g2))
    if heads:
        total += 2 * sum(_up4(rows * s) for s in z)
    else:
        total += sum(_up4(N * s) for s in z)
    total += _up4(rows * od) + _up4(sum(-(-T * rows // 64) * -(-dm // 64) for dm in d))
    if not heads:
        total += _up4(4 * -(-N // (8 if N <= 256 else 32)))
    return total + 12


def _sizes(sz):
    return (C.c_int32 * 23)(*sz)


def test_symbols_and_prototypes():
    L = _lib.lib()
    for n in NEW:
        assert hasattr(L, n), n
        assert n in _lib.exported_names(), n
        res, args = _lib._SIGS[n]
        assert getattr(L, n).restype == res and list(getattr(L, n).argtypes) == list(args)
    assert L.mfm_objective_mfn_workspace_floats.restype == C.c_int64
    assert list(L.mfm_objective_mfn_workspace_floats.argtypes) == [C.c_int32, C.c_int64, C.POINTER(C.c_int32), C.c_int64]
    assert list(L.mfm_objective_mfn_tile_rows.argtypes) == [C.c_int64, C.c_int64]
    # the arguments of mfm_objective_klef with the Gaussian sample behind the labels
    klef = list(L.mfm_objective_klef.argtypes)
    assert L.mfm_objective_mfn.restype == C.c_int and list(L.mfm_objective_mfn.argtypes) == klef[:8] + [C.c_void_p] + klef[8:]
    assert L.mfm_abi_version() == 5


@pytest.mark.parametrize("sz", [CANON, CANON_MMD, ODD])
@pytest.mark.parametrize("T,N,cap", [(20, 32, 0), (20, 1024, 1024), (7, 33, 16), (1, 1, 0), (9, 19, 4), (3, 5000, 1024), (2, 257, 0)])
def test_workspace_is_the_formula_of_the_header(sz, T, N, cap):
    assert _lib.lib().mfm_objective_mfn_workspace_floats(T, N, _sizes(sz), cap) == _formula(T, N, sz, cap)


def test_workspace_is_zero_for_bad_sizes():
    f = _lib.lib().mfm_objective_mfn_workspace_floats
    assert f(5, 5, _sizes(CANON), 0) > 0
    assert f(0, 5, _sizes(CANON), 0) == 0
    assert f(5, 0, _sizes(CANON), 0) == 0
    assert f(5, 5, _sizes(CANON), -1) == 0
    assert f(5, 5, None, 0) == 0
    for i in list(range(16)) + list(range(17, 22)):
        bad = list(CANON)
        bad[i] = 0
        assert f(5, 5, _sizes(bad), 0) == 0, i
    for i in (16, 22):              # heads and the loss kind: 0 or 1
        bad = list(CANON)
        bad[i] = 2
        assert f(5, 5, _sizes(bad), 0) == 0, i


@pytest.mark.parametrize("sz", [CANON, CANON_MMD])
def test_workspace_is_monotone_in_the_row_cap_and_survives_large_N(sz):
    f = _lib.lib().mfm_objective_mfn_workspace_floats
    N = 300
    prev = 0
    for cap in (1, 2, 7, 64, 299, 300):
        cur = f(20, N, _sizes(sz), cap)
        assert cur > prev, cap
        prev = cur
    assert f(20, N, _sizes(sz), 0) == prev and f(20, N, _sizes(sz), 5000) == prev
    big = f(20, 1 << 22, _sizes(sz), 0)                      # 4 M rows in one chunk: far beyond 32 bits
    assert big == _formula(20, 1 << 22, sz, 0) and big > (1 << 33)


def test_workspace_grows_with_N_beyond_the_row_cap_by_the_whole_split_arrays_alone():
    f = _lib.lib().mfm_objective_mfn_workspace_floats
    at_cap = f(20, 64, _sizes(CANON), 64)
    for N in (65, 1024, 1 << 20):
        assert f(20, N, _sizes(CANON), 64) == at_cap         # with heads: nothing grows
    gl = sum(CANON_MMD[3:7])
    at_cap = f(20, 64, _sizes(CANON_MMD), 64)
    for N in (256, 1024, 1 << 20):                           # (multiples of 4: no rounding of the arrays)
        tiles = -(-N // (8 if N <= 256 else 32))
        assert f(20, N, _sizes(CANON_MMD), 64) - at_cap == (N - 64) * gl + _up4(4 * tiles) - _up4(4 * 8)


def test_tile_rows_query_follows_the_six_workgroups_per_cu_rule():
    """six recurrences per row: four-row tiles from CUs rows per chunk"""
    L = _lib.lib()
    cus = L.mfm_device_cus()
    assert L.mfm_objective_mfn_tile_rows(cus - 1, 0) == 1 and L.mfm_objective_mfn_tile_rows(cus, 0) == 4
    assert L.mfm_objective_mfn_tile_rows(10 * cus, cus - 1) == 1
    assert L.mfm_objective_mfn_tile_rows(0, 0) == -1 and L.mfm_objective_mfn_tile_rows(5, -1) == -1
    assert L.mfm_objective_mfn_tile_rows(5, 0) == L.mfm_encode_mfn_tile_rows(5, 0)


def test_entry_validates_on_the_host():
    """T < 1, N < 1, a bad size, a null pointer, a Gaussian sample where there is no MMD or none where there is one, and a
    negative row cap: -1 and a message, before any pointer is followed or any GPU call is made (the device pointers here are
    made-up addresses)."""
    L = _lib.lib()
    offs = (C.c_int64 * 100)(*[64 * i for i in range(100)])
    lda = (C.c_float * 4)(1, 1, 1, 1)
    fake = [C.c_void_p(0x1000 * (i + 1)) for i in range(6)]       # params, x, y, workspace, out, gauss

    def call(T=7, N=33, sizes=_sizes(CANON), lambdas=lda, params=fake[0], offsets=offs, x=fake[1], y=fake[2], gauss=None, ws=fake[3],
             out=fake[4], max_rows=0):
        return L.mfm_objective_mfn(T, N, sizes, lambdas, params, offsets, x, y, gauss, ws, out, max_rows, None)

    zero_size = list(CANON)
    zero_size[18] = 0
    mmd = _sizes(CANON_MMD)
    for kw, text in ((dict(T=0), b"T 0"), (dict(N=0), b"N 0"), (dict(sizes=None), b"sizes must be positive"),
                     (dict(sizes=_sizes(zero_size)), b"sizes must be positive"), (dict(lambdas=None), b"must not be null"),
                     (dict(params=None), b"must not be null"), (dict(offsets=None), b"must not be null"), (dict(x=None), b"must not be null"),
                     (dict(y=None), b"must not be null"), (dict(ws=None), b"must not be null"), (dict(out=None), b"must not be null"),
                     (dict(gauss=fake[5]), b"must be null"), (dict(sizes=mmd), b"must not be null"),
                     (dict(max_rows=-1), b"row cap -1"), (dict(sizes=mmd, gauss=fake[5], max_rows=-1), b"row cap -1")):
        assert call(**kw) == -1, kw
        msg = L.mfm_last_error()
        assert b"objective mfn" in msg and text in msg, (kw, msg)


@pytest.mark.parametrize("variant,count", [("kl", 100), ("mmd", 86)])
def test_offsets_tables_name_only_tensors_of_the_layout(variant, count):
    names = engine.MFMEngine._ENCODE_MFN_TENSORS[variant] + engine.MFMEngine._DECODE_TENSORS
    shapes = engine.param_shapes(configs.canonical_configs(dropout=False), variant)
    assert len(names) == count and len(set(names)) == count
    assert all(n in shapes for n in names), [n for n in names if n not in shapes]


def test_entries_table_keeps_a_cache_of_its_own():
    from factorized_amd import _infer
    assert _infer._ENTRIES["objective_mfn"] == ("_objective_mfn_bufs", "_objective_mfn_refused", "mfm_objective_mfn")
    assert _infer._ENTRIES["objective"] == ("_objective_bufs", "_objective_refused", "mfm_objective_klef")


@pytest.mark.parametrize("cls", ["MFM_KL_EF", "MFM_KL", "MFM"])
def test_objective_on_cpu_tensors_raises(cls):
    from factorized_amd import mfm_model as M
    cfgs = configs.canonical_configs(dropout=False)
    cfg = cfgs[0]
    model = getattr(M, cls)(*cfgs)
    xn, yn = synth.make_batch(cfg["input_dims"], 5, 3, seed=1, output_dim=cfg["output_dim"])
    with pytest.raises(_lib.MfmError):
        model.objective(torch.from_numpy(xn), torch.from_numpy(yn))


@pytest.mark.parametrize("variant", ["kl", "mmd"])
def test_oracle_reproduces_the_fixture(variant):
    """pins the fixtures (the reference's own run, tests/golden/make_golden_objective_mfn.py) and the oracle to each other"""
    from oracle import mfm_oracle as O
    cfgs = odd_cfgs()
    cfg = cfgs[0]
    gold = np.load(os.path.join(cases.GOLDEN, "%s_objective_b19_t9.npz" % variant))
    B, T = [int(v) for v in gold["meta"]]
    assert (B, T) == (19, 9) and all(gold[k].dtype.kind in "fi" for k in gold.files)
    xn, yn = synth.make_batch(cfg["input_dims"], B, T, seed=7, output_dim=cfg["output_dim"])
    m = O.build(variant, cfgs)
    O.load_numpy_weights(m, synth.make_weights(O.state_shapes(m), seed=1234))
    m.eval()
    if variant == "mmd":
        zs = [cfg["zl_size"], cfg["za_size"], cfg["zv_size"], cfg["zy_size"]]
        assert gold["mmd_gauss"].shape == (B, sum(zs))
        m.mmd_gauss = list(torch.split(torch.from_numpy(np.ascontiguousarray(gold["mmd_gauss"])), zs, dim=1))
    torch.set_num_threads(1)
    with torch.no_grad():
        ref = O.loss_terms(m, torch.from_numpy(xn), torch.from_numpy(yn), cfg, "l1")
    for k in FIELDS:
        assert abs(float(ref[k]) - float(gold[k])) <= 2e-6 * abs(float(gold[k])), (k, float(ref[k]), float(gold[k]))
