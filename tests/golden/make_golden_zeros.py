#!/usr/bin/env python3
"""Generate tests/golden/klef_zeros_b19_t9.npz by RUNNING THE REFERENCE ITSELF (build container only).

    python tests/golden/make_golden_zeros.py      # needs the reference checkout make_golden.py imports

The test protocol of the reference's train_mfm_test_zeros (`predict`, mfm_mosi.py:572-596, restated below because the Python-2
driver cannot be imported) around the REFERENCE's MFM_KL_EF in eval mode, on the weights and the batch of klef_odd_b19_t9: the
batch through the model three times, modality l, a, v zeroed in turn with the driver's own torch.cat lines.  Recorded:

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
from factorized_amd import synth  # noqa: E402

NAME = "klef_zeros_b19_t9"
BASE = "klef_odd_b19_t9"


def main():
    _, variant, cfg_fn, overrides, B, T, _ = [c for c in G.CASES if c[0] == BASE][0]
    assert variant == "kl_ef"
    cfgs = cfg_fn(dropout=False, **overrides)
    cfg = cfgs[0]
    model = G.REF.MFM_KL_EF(*cfgs)
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
    path = os.path.join(HERE, NAME + ".npz")
    np.savez(path, **out)
    print("%s: gen %s disc %s (%d bytes)" % (NAME, out["gen"], out["disc"], os.path.getsize(path)))


if __name__ == "__main__":
    main()
