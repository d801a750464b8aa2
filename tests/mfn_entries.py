"""What the tests of the four MFN entries share (mfm_encode_mfn, mfm_predict_zeros_mfn, mfm_objective_mfn, mfm_predict_mfn:
tests/test_gpu_{encode,zeros,objective,predict}_mfn.py and tests/test_{encode,zeros,objective,predict}_mfn_host.py): the odd
configuration, the seeded model, bit patterns, canary frames for the raw ABI, and the size arrays with the arithmetic of the
header's workspace formulas.  A plain module like tests/cases.py; the per-entry oracles, formulas and checks stay with their tests."""
import ctypes as C

import pytest
import torch

from factorized_amd import configs, synth

CLS = {"kl": "MFM_KL", "mmd": "MFM", "kl_ef": "MFM_KL_EF"}
# nothing a multiple of 4 or of a tile
ODD = dict(input_dims=[7, 3, 5], h_dims=[9, 6, 7], memsize=5, zy_size=5, zl_size=6, za_size=3, zv_size=7)
ODD_ATT = (10, 11, 12, 13)
# the 23 sizes of the entries (the first 17: mfm_encode_mfn's), canonical and odd with cross entropy over 3 classes:
# d_l d_a d_v | zl za zv | zy | h_l h_a h_v | memsize | windowsize | att1 att2 gamma1 gamma2 | heads | fl fa fv fy | od | loss kind
CANON_SIZES = (300, 5, 20, 32, 8, 80, 32, 88, 64, 48, 64, 2, 128, 128, 128, 128, 1, 88, 8, 8, 16, 1, 0)
ODD_SIZES = (7, 3, 5, 6, 3, 7, 5, 9, 6, 7, 5, 2, 10, 11, 12, 13, 0, 88, 8, 8, 16, 3, 1)
CANARY = 0x7FC0DEAD                   # a NaN with a payload: any store over it shows


def odd_cfgs(**over):
    cfgs = configs.canonical_configs(dropout=False, **dict(ODD, **over))
    for k, w in zip(cfgs[1:5], ODD_ATT):
        k["shapes"] = w
    return cfgs


def model(cfgs, variant):
    """the class of `variant` on the device with the seed-1234 weights -> (model, the weights as numpy arrays)"""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from factorized_amd import mfm_model as M
    m = getattr(M, CLS[variant])(*cfgs)
    shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    w = synth.make_weights(shapes, seed=1234)
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in w.items()})
    return m.to("cuda"), w


def bits(t):
    """the int32 bit patterns of a tensor on the host, a copy (the engine reuses its tensors)"""
    return t.detach().cpu().contiguous().view(torch.int32).clone()


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def canary(n, pad=256):
    """n floats framed by `pad` canary words on either side -> (the whole int32 buffer, the float32 view of the middle)"""
    big = torch.full((pad + n + pad,), CANARY, dtype=torch.int32, device="cuda")
    return big, big[pad:pad + n].view(torch.float32)


def intact(big, n, pad=256):
    return bool((big[:pad] == CANARY).all()) and bool((big[pad + n:] == CANARY).all())


def hp(h):
    return (h + 15) // 16 * 16


def up4(v):
    return (v + 3) // 4 * 4
