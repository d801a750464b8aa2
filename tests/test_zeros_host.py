"""Host side of the zeroed-modality test protocol (engine.Zeros, mfm_predict_zeros_klef, model.predict_zeros): the namedtuple, the
ABI symbols, the argument checks that run before anything touches the GPU, the workspace size rule, and the fixture against the
CPU oracle.  No GPU compute here."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from factorized_amd import _lib, configs, engine, synth
from tests import cases, zeros_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mfm_predict_zeros_klef_workspace_floats", "mfm_predict_zeros_klef")


def _sizes(cfg=None, loss_kind=0):
    c = cfg or configs.canonical_configs()[0]
    return (C.c_int32 * 13)(c["zl_size"], c["za_size"], c["zv_size"], c["zy_size"], c["fl_size"], c["fa_size"], c["fv_size"],
                            c["fy_size"], *c["input_dims"], c["output_dim"], loss_kind)


def test_zeros_namedtuple_has_the_three_fields_in_order():
    assert engine.Zeros._fields == ("y_hat", "gen", "disc")
    z = engine.Zeros(*range(3))
    assert (z.y_hat, z.gen, z.disc) == (0, 1, 2)


def test_symbols_in_header_library_and_binding():
    src = open(os.path.join(ROOT, "include", "mfm_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(mfm_[a-z0-9_]+)\s*\(", src))
    L = _lib.lib()
    for n in NAMES:
        assert n in declared, n
        assert hasattr(L, n), n
        assert n in _lib.exported_names(), n
    assert L.mfm_abi_version() == 5


def test_entry_validates_on_the_host():
    """T < 1, N < 1, a null pointer and a negative row cap: -1 and a message, before any pointer is followed or any GPU call
    is made (the device pointers here are made-up addresses)."""
    L = _lib.lib()
    sizes = _sizes()
    offs = (C.c_int64 * 78)(*[64 * i for i in range(78)])
    fake = [C.c_void_p(0x1000 * (i + 1)) for i in range(7)]       # params, x, y, workspace, y_hat, gen, disc

    def call(T=7, N=33, params=fake[0], y=fake[2], disc=fake[6], max_rows=0):
        return L.mfm_predict_zeros_klef(T, N, sizes, params, offs, fake[1], y, fake[3], fake[4], fake[5], disc, max_rows, None)

    for kw, text in ((dict(T=0), b"T 0"), (dict(N=0), b"N 0"), (dict(params=None), b"must not be null"),
                     (dict(disc=None), b"come together"), (dict(y=None), b"come together"), (dict(max_rows=-1), b"row cap -1")):
        assert call(**kw) == -1, kw
        msg = L.mfm_last_error()
        assert b"predict zeros klef" in msg and text in msg, (kw, msg)


def test_workspace_grows_with_n_up_to_the_cap_and_not_beyond():
    L = _lib.lib()
    sizes = _sizes()
    T, cap = 20, 64
    ws = [int(L.mfm_predict_zeros_klef_workspace_floats(T, n, sizes, cap)) for n in range(1, cap + 1)]
    assert ws[0] > 0 and all(a <= b for a, b in zip(ws, ws[1:])) and ws[0] < ws[-1]
    for n in (cap + 1, 229, 4096, 1 << 20):
        assert int(L.mfm_predict_zeros_klef_workspace_floats(T, n, sizes, cap)) == ws[-1], n
    # cap 0: one chunk, so the size follows N
    assert int(L.mfm_predict_zeros_klef_workspace_floats(T, 229, sizes, 0)) > ws[-1]
    # bad sizes: 0
    assert L.mfm_predict_zeros_klef_workspace_floats(0, 33, sizes, cap) == 0
    assert L.mfm_predict_zeros_klef_workspace_floats(T, 0, sizes, cap) == 0
    assert L.mfm_predict_zeros_klef_workspace_floats(T, 33, sizes, -1) == 0
    assert L.mfm_predict_zeros_klef_workspace_floats(T, 33, None, cap) == 0
    # at least the three partial projections and the three gate sets of a chunk, or the stored h that takes their place
    c = configs.canonical_configs()[0]
    hp = (c["zl_size"] + c["za_size"] + c["zv_size"] + 15) // 16 * 16
    dec = int(L.mfm_decode_factors_workspace_floats(T, 229, c["fy_size"], c["fl_size"], c["fa_size"], c["fv_size"], cap))
    assert ws[-1] > max(6 * cap * T * 4 * hp, dec)


def test_oracle_on_zeroed_inputs_reproduces_the_fixture():
    """pins the fixture (the reference's own run, tests/golden/make_golden_zeros.py) and the oracle to each other"""
    cs = cases.load_case("klef_odd_b19_t9")
    gold = np.load(os.path.join(cases.GOLDEN, "klef_zeros_b19_t9.npz"))
    assert list(gold["meta"]) == [cs["B"], cs["T"]]
    from oracle import mfm_oracle as O
    w = synth.make_weights(O.state_shapes(O.build("kl_ef", cs["cfgs"])), seed=1234)
    ref = zeros_ref.oracle_zeros("kl_ef", cs["cfgs"], w, cs["x"], cs["y"])
    assert ref["y_hat"].shape == gold["y_hat"].shape == (3, cs["B"], cs["cfg"]["output_dim"])
    assert cases.rel_err(ref["y_hat"], gold["y_hat"]) <= 1e-6
    for k in ("gen", "disc"):
        for c in range(3):
            assert abs(ref[k][c] - gold[k][c]) <= 1e-6 * abs(gold[k][c]), (k, c, ref[k][c], gold[k][c])


def test_model_predict_zeros_on_a_cpu_model_raises():
    import torch
    from factorized_amd import mfm_model as M
    model = M.MFM_KL_EF(*configs.canonical_configs(dropout=False))
    x = torch.zeros(3, 2, sum(configs.canonical_configs()[0]["input_dims"]))
    with pytest.raises(_lib.MfmError):
        model.predict_zeros(x)
