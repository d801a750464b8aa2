#!/usr/bin/env python3
"""Generate tests/golden/klef_clip_b32_t20.npz by RUNNING THE REFERENCE ITSELF (build container only).

    python tests/golden/make_golden_clip.py       # needs the reference checkout make_golden.py imports

The run of make_golden_sgd.py -- the reference's MFM_KL_EF, the weights and batch of klef_b32_t20, the joint loss and
torch.optim.SGD(lr=0.01, momentum=0.9): with SGD a gradient scale shows linearly in the parameters -- with the usual clipping
line between backward() and step():

    loss.backward(); torch.nn.utils.clip_grad_norm_(model.parameters(), MAX_NORM); optimizer.step()

MAX_NORM = 20 is taken from the norms the reference itself produces: the unclipped SGD run's 20 gradient norms go from 65.8 down
to 10.9 with a median of 20.8, and the clipped run crosses 20 in both directions (65.8, 51.8, 30.4 | 16.4 | 22.8, 26.6, 25.1,
21.0 | 16.9 ... 7.9), so both the clipping and the non-clipping branch are in the fixture (asserted below).  Recorded:

    trace                 [20, 4]  loss, disc, gen, reg of every step of the joint loss
    total_norm            [20]     what torch.nn.utils.clip_grad_norm_ returned in every step
    param_after1 / param_after_last   summaries of every parameter after the first / the last step
    staged_trace          [n1 + n2, 4]  train_beta_vae's schedule (n1 steps of gen + reg, then n2 of disc + reg), clipped the same
                          way, zero_grad() with torch's default set_to_none=True: a parameter the stage loss does not reach has
                          no gradient -- it is not in the norm and does not move
    staged_total_norm     [n1 + n2]
    staged_param_after_stage1 / staged_param_after_stage2
    meta                  [B, T, steps, n1, n2, MAX_NORM]

Only numbers are written.
"""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import make_golden as G  # noqa: E402  (imports the reference read-only; fixes the CPU thread count)
from factorized_amd import configs as C  # noqa: E402
from factorized_amd import synth  # noqa: E402

NAME = "klef_clip_b32_t20"
B, T, STEPS, N1, N2 = 32, 20, 20, 4, 4
MAX_NORM = 20.0


def _model(cfgs):
    model = G.REF.MFM_KL_EF(*cfgs)
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    w = synth.make_weights(shapes, seed=1234)
    model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in w.items()})
    model.train()
    return model


def main():
    cfgs = C.canonical_configs(dropout=False)
    cfg = cfgs[0]
    xn, yn = synth.make_batch(cfg["input_dims"], B, T, seed=7)
    x, y = torch.from_numpy(xn), torch.from_numpy(yn)
    out = {}

    model = _model(cfgs)
    opt = torch.optim.SGD(model.parameters(), lr=cfg["lr"], momentum=cfg["momentum"])      # mfm_mosi.py:404
    trace, norms = [], []
    for s in range(STEPS):
        opt.zero_grad()
        terms, _ = G.ref_losses(model, x, y, cfg, "l1")
        terms["loss"].backward()
        norms.append(float(torch.nn.utils.clip_grad_norm_(model.parameters(), MAX_NORM)))
        opt.step()
        trace.append([terms[k].item() for k in ("loss", "disc", "gen", "reg")])
        if s == 0:
            out["param_after1"] = np.stack([G.summarize(p) for p in model.parameters()])
    out["param_after_last"] = np.stack([G.summarize(p) for p in model.parameters()])
    out["trace"] = np.array(trace, dtype=np.float64)
    out["total_norm"] = np.array(norms, dtype=np.float64)
    assert np.isfinite(out["trace"]).all() and np.isfinite(out["total_norm"]).all(), out["trace"][:, 0]
    # both branches: some steps are scaled down, some are left as they are
    assert out["total_norm"].min() < MAX_NORM < out["total_norm"].max(), out["total_norm"]

    model = _model(cfgs)
    opt = torch.optim.SGD(model.parameters(), lr=cfg["lr"], momentum=cfg["momentum"])
    trace, norms = [], []
    for s in range(N1 + N2):
        opt.zero_grad()
        terms, _ = G.ref_losses(model, x, y, cfg, "l1")
        reg = cfg["lda_mmd"] * terms["reg"]
        loss = terms["gen"] + reg if s < N1 else terms["disc"] + reg      # mfm_mosi.py:278-281
        loss.backward()
        norms.append(float(torch.nn.utils.clip_grad_norm_(model.parameters(), MAX_NORM)))
        opt.step()
        trace.append([loss.item(), terms["disc"].item(), terms["gen"].item(), terms["reg"].item()])
        if s == N1 - 1:
            out["staged_param_after_stage1"] = np.stack([G.summarize(p) for p in model.parameters()])
    out["staged_param_after_stage2"] = np.stack([G.summarize(p) for p in model.parameters()])
    out["staged_trace"] = np.array(trace, dtype=np.float64)
    out["staged_total_norm"] = np.array(norms, dtype=np.float64)
    assert np.isfinite(out["staged_trace"]).all() and np.isfinite(out["staged_total_norm"]).all()
    out["param_names"] = np.array([n for n, _ in model.named_parameters()])
    out["meta"] = np.array([B, T, STEPS, N1, N2, MAX_NORM], dtype=np.float64)
    path = os.path.join(HERE, NAME + ".npz")
    np.savez_compressed(path, **out)
    print(NAME, "loss0=%.6f lossN=%.6f" % (out["trace"][0, 0], out["trace"][-1, 0]),
          "norms", np.round(out["total_norm"], 2).tolist(), "staged norms", np.round(out["staged_total_norm"], 2).tolist(),
          "bytes=%d" % os.path.getsize(path))


if __name__ == "__main__":
    main()
