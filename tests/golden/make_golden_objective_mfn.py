#!/usr/bin/env python3
"""Generate tests/golden/kl_objective_b19_t9.npz and mmd_objective_b19_t9.npz by RUNNING THE REFERENCE ITSELF (build container only).

    python tests/golden/make_golden_objective_mfn.py      # needs the reference checkout make_golden.py imports

The validation objective of the reference's drivers (mfm_mosi.py:319-324, :724-726, :826-845) for the classes whose label factor
comes from the Memory Fusion Network: the REFERENCE's MFM_KL / MFM in eval mode on the odd sizes of tests/test_gpu_encode_mfn.py
(nothing a multiple of 4 or of a tile), the weights synth.make_weights(seed 1234), the batch synth.make_batch(seed 7) at B = 19,
T = 9.  The six numbers come from the model's own forward (its loss_KLD / compute_kernel) and F.mse_loss / F.l1_loss as the drivers
combine them.  For MFM the Gaussian sample loss_MMD draws is injected, seeded, and recorded, as make_golden.py records mmd_gauss.
Recorded per variant:

    loss disc gen_l gen_a gen_v reg    float64 scalars
    mmd_gauss  [19, zl + za + zv + zy] (MFM only)
    meta       [B, T]

reg is also computed in float64 (the same model converted to double): the generator asserts that it differs from the float32
value by less than 1e-5 relative, so that the tests' 1e-4 does not rest on a cancellation the reference itself does not resolve
(another batch seed would have to be picked if it did).  Only numbers are written.
"""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import make_golden as G  # noqa: E402  (imports the reference read-only; fixes the CPU thread count)
from factorized_amd import synth  # noqa: E402
from make_golden_zeros_mfn import B, T, odd_cfgs  # noqa: E402

BATCH_SEED = 7
GAUSS_SEED = 99
FIELDS = ("loss", "disc", "gen_l", "gen_a", "gen_v", "reg")


def terms_of(model, x, y, cfg, gauss):
    """ref_losses around the reference's forward with loss_MMD's samples injected (mfm_model.py:26), in x's dtype"""
    if gauss is None:
        return G.ref_losses(model, x, y, cfg, "l1")[0]
    it = iter([g.to(x.dtype) for g in gauss])
    orig = torch.randn
    torch.randn = lambda *a, **k: next(it)
    try:
        return G.ref_losses(model, x, y, cfg, "l1")[0]
    finally:
        torch.randn = orig


def run(variant):
    cfgs = odd_cfgs()
    cfg = cfgs[0]
    model = G.REF_CLASS[variant](*cfgs)
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    w = synth.make_weights(shapes, seed=1234)
    model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in w.items()})
    xn, yn = synth.make_batch(cfg["input_dims"], B, T, seed=BATCH_SEED, output_dim=cfg["output_dim"])
    x, y = torch.from_numpy(xn), torch.from_numpy(yn)
    out = dict(meta=np.array([B, T], dtype=np.int64))
    gauss = None
    if variant == "mmd":
        rs = np.random.RandomState(GAUSS_SEED)
        sizes = [cfg["zl_size"], cfg["za_size"], cfg["zv_size"], cfg["zy_size"]]
        gauss = [torch.from_numpy(rs.normal(size=(B, s)).astype(np.float32)) for s in sizes]
        out["mmd_gauss"] = np.concatenate([g.numpy() for g in gauss], axis=1)
    model.eval()
    with torch.no_grad():
        t32 = terms_of(model, x, y, cfg, gauss)
        torch.set_default_dtype(torch.float64)      # (the reference makes its initial LSTM states with torch.zeros)
        try:
            t64 = terms_of(model.double(), x.double(), y.double(), cfg, gauss)
        finally:
            torch.set_default_dtype(torch.float32)
    for k in FIELDS:
        out[k] = np.float64(float(t32[k]))
        assert np.isfinite(out[k]), k
    r32, r64 = float(t32["reg"]), float(t64["reg"])
    rel = abs(r32 - r64) / abs(r64)
    print("%s: reg float32 %.9g float64 %.9g (%.2e relative)" % (variant, r32, r64, rel))
    assert rel < 1e-5, "reg is not resolved in float32 for this batch: pick another BATCH_SEED"
    path = os.path.join(HERE, "%s_objective_b%d_t%d.npz" % (variant, B, T))
    np.savez(path, **out)
    print("%s: %s (%d bytes)" % (os.path.basename(path), " ".join("%s %.8g" % (k, out[k]) for k in FIELDS), os.path.getsize(path)))


if __name__ == "__main__":
    for v in ("kl", "mmd"):
        run(v)
