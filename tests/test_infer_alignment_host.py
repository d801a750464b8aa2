"""What the no-plan inference entries of MFM_KL_EF ask of their pointers (csrc/infer_dev.h, infer_check_aligned): x on 4 bytes --
any contiguous float view, such as batch i of an [nb, T, B, D] dataset or a time crop x[k:] -- params and the workspace on 16.
The device pointers here are made-up addresses that are never followed: every call must be answered by the argument checks,
which come before any launch.  A call whose alignment is accepted is sent with N = 2^24, the next check in line, so that it is
refused as well and nothing reaches a device.  No GPU compute here."""
import ctypes as C

import pytest

from factorized_amd import _lib, configs

PARAMS, X, Y, WS, OUT = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000
T, N = 4, 6


def _sizes13():
    c = configs.canonical_configs()[0]
    return (C.c_int32 * 13)(c["zl_size"], c["za_size"], c["zv_size"], c["zy_size"], c["fl_size"], c["fa_size"], c["fv_size"],
                            c["fy_size"], *c["input_dims"], c["output_dim"], 0)


def _offs(n):
    return (C.c_int64 * n)(*[64 * i for i in range(n)])


def _predict(params, x, ws, n):
    return _lib.lib().mfm_predict_klef(T, n, 325, 120, 32, 16, 1, 0, C.c_void_p(params), _offs(16), C.c_void_p(x), C.c_void_p(Y),
                                       C.c_void_p(ws), C.c_void_p(OUT), C.c_void_p(OUT + 64), 0, None)


def _encode(params, x, ws, n):
    out = (C.c_void_p * 8)(*[OUT + 64 * i for i in range(8)])
    return _lib.lib().mfm_encode_klef(T, n, 300, 5, 20, 32, 8, 80, 32, C.c_void_p(params), _offs(40), C.c_void_p(x), C.c_void_p(ws),
                                      out, 0, None)


def _objective(params, x, ws, n):
    lda = (C.c_float * 4)(1.0, 1.0, 1.0, 1.0)
    return _lib.lib().mfm_objective_klef(T, n, _sizes13(), lda, C.c_void_p(params), _offs(78), C.c_void_p(x), C.c_void_p(Y),
                                         C.c_void_p(ws), C.c_void_p(OUT), 0, None)


def _zeros(params, x, ws, n):
    return _lib.lib().mfm_predict_zeros_klef(T, n, _sizes13(), C.c_void_p(params), _offs(78), C.c_void_p(x), C.c_void_p(Y),
                                             C.c_void_p(ws), C.c_void_p(OUT), C.c_void_p(OUT + 64), C.c_void_p(OUT + 128), 0, None)


ENTRIES = {"predict klef": _predict, "encode klef": _encode, "objective klef": _objective, "predict zeros klef": _zeros}


def _msg():
    return _lib.lib().mfm_last_error().decode()


@pytest.mark.parametrize("who", list(ENTRIES))
def test_x_two_bytes_off_is_refused_with_the_four_byte_message(who):
    for off in (1, 2, 3, 6):
        assert ENTRIES[who](PARAMS, X + off, WS, N) == -1
        assert _msg() == "%s: x must be 4-byte aligned" % who, (off, _msg())


@pytest.mark.parametrize("who", list(ENTRIES))
def test_params_or_workspace_four_bytes_off_is_still_refused(who):
    for params, ws in ((PARAMS + 4, WS), (PARAMS, WS + 4), (PARAMS + 8, WS), (PARAMS, WS + 12)):
        assert ENTRIES[who](params, X, ws, N) == -1
        assert _msg() == "%s: params and workspace must be 16-byte aligned" % who, (params, ws, _msg())
    # ... whatever x is
    assert ENTRIES[who](PARAMS + 4, X + 4, WS, N) == -1
    assert "16-byte aligned" in _msg()


@pytest.mark.parametrize("who", list(ENTRIES))
def test_x_on_any_four_byte_address_passes_the_alignment_check(who):
    """residues 4, 8 and 12 get as far as residue 0 does: to the row-count check behind the alignment check"""
    for r in (0, 4, 8, 12):
        assert ENTRIES[who](PARAMS, X + r, WS, 1 << 24) == -1
        assert "2^24" in _msg() and "aligned" not in _msg(), (r, _msg())
