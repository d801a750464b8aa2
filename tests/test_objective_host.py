"""Host side of the full validation objective (engine.Objective, mfm_objective_klef, model.objective): the namedtuple, the ABI
symbols, the argument checks that run before anything touches the GPU, and the workspace size rule.  No GPU compute here."""
import ctypes as C
import os
import re

import pytest

from factorized_amd import _lib, configs, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mfm_objective_klef_workspace_floats", "mfm_objective_klef")


def _sizes(cfg=None, loss_kind=0):
    c = cfg or configs.canonical_configs()[0]
    return (C.c_int32 * 13)(c["zl_size"], c["za_size"], c["zv_size"], c["zy_size"], c["fl_size"], c["fa_size"], c["fv_size"],
                            c["fy_size"], *c["input_dims"], c["output_dim"], loss_kind)


def test_objective_namedtuple_has_the_six_fields_in_order():
    assert engine.Objective._fields == ("loss", "disc", "gen_l", "gen_a", "gen_v", "reg")
    o = engine.Objective(*range(6))
    assert (o.loss, o.disc, o.gen_l, o.gen_a, o.gen_v, o.reg) == tuple(range(6))


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
    lda = (C.c_float * 4)(1.0, 1.0, 1.0, 1.0)
    offs = (C.c_int64 * 78)(*[64 * i for i in range(78)])
    fake = [C.c_void_p(0x1000 * (i + 1)) for i in range(5)]       # params, x, y, workspace, out

    def call(T=7, N=33, params=fake[0], max_rows=0):
        return L.mfm_objective_klef(T, N, sizes, lda, params, offs, fake[1], fake[2], fake[3], fake[4], max_rows, None)

    for kw, text in ((dict(T=0), b"T 0"), (dict(N=0), b"N 0"), (dict(params=None), b"must not be null"),
                     (dict(max_rows=-1), b"row cap -1")):
        assert call(**kw) == -1, kw
        msg = L.mfm_last_error()
        assert b"objective klef" in msg and text in msg, (kw, msg)


def test_workspace_grows_with_n_up_to_the_cap_and_not_beyond():
    L = _lib.lib()
    sizes = _sizes()
    T, cap = 20, 64
    ws = [int(L.mfm_objective_klef_workspace_floats(T, n, sizes, cap)) for n in range(1, cap + 1)]
    assert ws[0] > 0 and all(a <= b for a, b in zip(ws, ws[1:])) and ws[0] < ws[-1]
    for n in (cap + 1, 229, 4096, 1 << 20):
        assert int(L.mfm_objective_klef_workspace_floats(T, n, sizes, cap)) == ws[-1], n
    # cap 0: one chunk, so the size follows N
    assert int(L.mfm_objective_klef_workspace_floats(T, 229, sizes, 0)) > ws[-1]
    # bad sizes: 0
    assert L.mfm_objective_klef_workspace_floats(0, 33, sizes, cap) == 0
    assert L.mfm_objective_klef_workspace_floats(T, 0, sizes, cap) == 0
    assert L.mfm_objective_klef_workspace_floats(T, 33, sizes, -1) == 0
    # at least what the two halves need for a chunk (the stored h takes the place of the x-projections)
    c = configs.canonical_configs()[0]
    enc = int(L.mfm_encode_klef_workspace_floats(T, 229, c["zl_size"], c["za_size"], c["zv_size"], cap))
    dec = int(L.mfm_decode_factors_workspace_floats(T, 229, c["fy_size"], c["fl_size"], c["fa_size"], c["fv_size"], cap))
    assert max(enc, dec) < ws[-1] < enc + dec


def test_model_objective_on_a_cpu_model_raises():
    import torch
    from factorized_amd import mfm_model as M
    model = M.MFM_KL_EF(*configs.canonical_configs(dropout=False))
    x = torch.zeros(3, 2, sum(configs.canonical_configs()[0]["input_dims"]))
    y = torch.zeros(2, 1)
    with pytest.raises(_lib.MfmError):
        model.objective(x, y)
