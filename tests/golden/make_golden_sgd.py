#!/usr/bin/env python3
"""Generate tests/golden/klef_sgd_b32_t20.npz by RUNNING THE REFERENCE ITSELF (build container only).

    python tests/golden/make_golden_sgd.py        # needs the reference checkout make_golden.py imports

The reference's other optimizer line (mfm_mosi.py:404, commented out under the Adam line in every driver):

    optimizer = optim.SGD(model.parameters(), lr=config["lr"], momentum=config["momentum"])

with the canonical values lr=0.01, momentum=0.9 (factorized_amd/configs.py, from mfm_mosi.py:1230), on the reference's
MFM_KL_EF with the weights and batch of klef_b32_t20 (same synth seeds, same joint loss as make_golden.py).  Recorded:

    trace                 [20, 4]  loss, disc, gen, reg of every step of the joint loss
    param_after1 / param_after_last   summaries of every parameter after the first / the last step
    staged_trace          [n1 + n2, 4]  train_beta_vae's schedule (n1 steps of gen + reg, then n2 of disc + reg), one SGD
                          optimizer, zero_grad() with torch's default set_to_none=True (a parameter the stage loss does not
                          reach is skipped, its momentum buffer included)
    staged_param_after_stage1 / staged_param_after_stage2
    meta                  [B, T, steps, n1, n2]

20 steps at this learning rate stay finite in fp32: the joint loss goes from 44.2 to 4.0, not monotonically.
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

NAME = "klef_sgd_b32_t20"
B, T, STEPS, N1, N2 = 32, 20, 20, 4, 4


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
    trace = []
    for s in range(STEPS):
        opt.zero_grad()
        terms, _ = G.ref_losses(model, x, y, cfg, "l1")
        terms["loss"].backward()
        opt.step()
        trace.append([terms[k].item() for k in ("loss", "disc", "gen", "reg")])
        if s == 0:
            out["param_after1"] = np.stack([G.summarize(p) for p in model.parameters()])
    out["param_after_last"] = np.stack([G.summarize(p) for p in model.parameters()])
    out["trace"] = np.array(trace, dtype=np.float64)
    assert np.isfinite(out["trace"]).all() and out["trace"][-1, 0] < out["trace"][0, 0], out["trace"][:, 0]

    model = _model(cfgs)
    opt = torch.optim.SGD(model.parameters(), lr=cfg["lr"], momentum=cfg["momentum"])
    trace = []
    for s in range(N1 + N2):
        opt.zero_grad()
        terms, _ = G.ref_losses(model, x, y, cfg, "l1")
        reg = cfg["lda_mmd"] * terms["reg"]
        loss = terms["gen"] + reg if s < N1 else terms["disc"] + reg      # mfm_mosi.py:278-281
        loss.backward()
        opt.step()
        trace.append([loss.item(), terms["disc"].item(), terms["gen"].item(), terms["reg"].item()])
        if s == N1 - 1:
            out["staged_param_after_stage1"] = np.stack([G.summarize(p) for p in model.parameters()])
    out["staged_param_after_stage2"] = np.stack([G.summarize(p) for p in model.parameters()])
    out["staged_trace"] = np.array(trace, dtype=np.float64)
    out["param_names"] = np.array([n for n, _ in model.named_parameters()])
    out["meta"] = np.array([B, T, STEPS, N1, N2])
    path = os.path.join(HERE, NAME + ".npz")
    np.savez_compressed(path, **out)
    print(NAME, "loss0=%.6f lossN=%.6f" % (out["trace"][0, 0], out["trace"][-1, 0]),
          "staged lossN=%.6f" % out["staged_trace"][-1, 0], "bytes=%d" % os.path.getsize(path))


if __name__ == "__main__":
    main()
