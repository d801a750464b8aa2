#!/usr/bin/env python3
"""Generate tests/golden/kl_zeros_b19_t9.npz and mmd_zeros_b19_t9.npz by RUNNING THE REFERENCE ITSELF (build container only).

    python tests/golden/make_golden_zeros_mfn.py      # needs the reference checkout make_golden.py imports

What make_golden_zeros.py records for MFM_KL_EF, for the classes whose label factor comes from the Memory Fusion Network: the
test protocol of the reference's train_mfm_test_zeros (`predict`, mfm_mosi.py:572-596, restated below because the Python-2 driver
cannot be imported) around the REFERENCE's MFM_KL / MFM in eval mode -- the batch through the model's own forward three times,
modality l, a, v zeroed in turn with the driver's own torch.cat lines.  The sizes are the odd ones of
tests/test_gpu_encode_mfn.py (nothing a multiple of 4 or of a tile), the weights synth.make_weights(seed 1234), the batch
synth.make_batch(seed 7) at B = 19, T = 9.  Recorded per variant:

    y_hat   [3, 19, output_dim]  y_hat_nol, y_hat_noa, y_hat_nov
    gen     [3]   F.mse_loss(x_l_hat_nol, x_l), F.mse_loss(x_a_hat_noa, x_a), F.mse_loss(x_v_hat_nov, x_v): what the driver prints
    disc    [3]   the L1 loss of the three y_hat against the batch's labels (the driver's evaluate(), per case)
    meta    [B, T]

Only numbers are written.
"""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import make_golden as G  # noqa: E402  (imports the reference read-only; fixes the CPU thread count)
from factorized_amd import configs, synth  # noqa: E402

B, T = 19, 9
ODD = dict(input_dims=[7, 3, 5], h_dims=[9, 6, 7], memsize=5, zy_size=5, zl_size=6, za_size=3, zv_size=7)
ODD_ATT = (10, 11, 12, 13)


def odd_cfgs():
    cfgs = configs.canonical_configs(dropout=False, **ODD)
    for k, w in zip(cfgs[1:5], ODD_ATT):
        k["shapes"] = w
    return cfgs


def run(variant):
    cfgs = odd_cfgs()
    cfg = cfgs[0]
    model = G.REF_CLASS[variant](*cfgs)
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    w = synth.make_weights(shapes, seed=1234)
    model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in w.items()})
    xn, yn = synth.make_batch(cfg["input_dims"], B, T, seed=7, output_dim=cfg["output_dim"])
    batch_X, batch_y = torch.from_numpy(xn), torch.from_numpy(yn)
    d_l, d_a, _ = cfg["input_dims"]
    model.eval()
    with torch.no_grad():
        batch_X_nol = torch.cat([torch.zeros_like(batch_X[:, :, :d_l]), batch_X[:, :, d_l:]], dim=2)
        batch_X_noa = torch.cat([batch_X[:, :, :d_l], torch.zeros_like(batch_X[:, :, d_l:d_l + d_a]), batch_X[:, :, d_l + d_a:]], dim=2)
        batch_X_nov = torch.cat([batch_X[:, :, :d_l + d_a], torch.zeros_like(batch_X[:, :, d_l + d_a:])], dim=2)
        decoded = [model.forward(b)[0] for b in (batch_X_nol, batch_X_noa, batch_X_nov)]
        real = [batch_X[:, :, :d_l], batch_X[:, :, d_l:d_l + d_a], batch_X[:, :, d_l + d_a:]]
        gen = [F.mse_loss(decoded[c][c], real[c]).item() for c in range(3)]
        y_hat = torch.stack([decoded[c][3] for c in range(3)])
        disc = [(F.l1_loss(y_hat[c].squeeze(1), batch_y) if y_hat.shape[2] == 1 else F.l1_loss(y_hat[c], batch_y)).item() for c in range(3)]
    out = dict(y_hat=y_hat.numpy().astype(np.float32), gen=np.array(gen, dtype=np.float64), disc=np.array(disc, dtype=np.float64),
               meta=np.array([B, T], dtype=np.int64))
    assert out["y_hat"].shape == (3, B, cfg["output_dim"]) and np.isfinite(out["y_hat"]).all()
    assert np.isfinite(out["gen"]).all() and np.isfinite(out["disc"]).all()
    # the three cases differ: a zeroed modality does reach the prediction
    assert not np.allclose(out["y_hat"][0], out["y_hat"][1]) and not np.allclose(out["y_hat"][1], out["y_hat"][2])
    path = os.path.join(HERE, "%s_zeros_b%d_t%d.npz" % (variant, B, T))
    np.savez(path, **out)
    print("%s: gen %s disc %s (%d bytes)" % (os.path.basename(path), out["gen"], out["disc"], os.path.getsize(path)))


if __name__ == "__main__":
    for v in ("kl", "mmd"):
        run(v)
