#!/usr/bin/env python3
"""Generate tests/golden/klef_adamw_b32_t20.npz by RUNNING THE REFERENCE ITSELF (build container only).

    python tests/golden/make_golden_adamw.py        # needs the reference checkout make_golden.py imports

The reference's MFM_KL_EF with the weights and batch of klef_b32_t20 (same synth seeds, same joint loss as make_golden.py),
20 steps each under the optimizer lines a user of torch.optim.Adam's other options writes:

    adamw       torch.optim.AdamW(model.parameters(), lr=1e-3, weight_decay=1e-2)
    amsgrad     torch.optim.Adam(model.parameters(), lr=1e-3, weight_decay=1e-4, amsgrad=True)
    groups      torch.optim.AdamW([{"params": the four encoders, "lr": 1e-4}, {"params": the rest}], lr=1e-3, weight_decay=1e-2)

("the four encoders": encoder_l, encoder_a, encoder_v and ef_encoder; in `groups` they keep AdamW's weight_decay default, which
is the 1e-2 given.)  Recorded per run, under the run's name as prefix:

    <run>_trace               [20, 4]  loss, disc, gen, reg of every step of the joint loss
    <run>_param_after1 / <run>_param_after_last   summaries of every parameter after the first / the last step
    param_names, meta         [B, T, steps]

All three runs stay finite in fp32 and lower the joint loss.  Only numbers and parameter names are written.
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

NAME = "klef_adamw_b32_t20"
B, T, STEPS = 32, 20, 20
ENCODERS = ("encoder_l.", "encoder_a.", "encoder_v.", "ef_encoder.")


def _model(cfgs):
    model = G.REF.MFM_KL_EF(*cfgs)
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    w = synth.make_weights(shapes, seed=1234)
    model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in w.items()})
    model.train()
    return model


def _two_groups(model):
    enc = [p for n, p in model.named_parameters() if n.startswith(ENCODERS)]
    rest = [p for n, p in model.named_parameters() if not n.startswith(ENCODERS)]
    assert enc and rest
    return [{"params": enc, "lr": 1e-4}, {"params": rest}]


RUNS = {
    "adamw": lambda m: torch.optim.AdamW(m.parameters(), lr=1e-3, weight_decay=1e-2),
    "amsgrad": lambda m: torch.optim.Adam(m.parameters(), lr=1e-3, weight_decay=1e-4, amsgrad=True),
    "groups": lambda m: torch.optim.AdamW(_two_groups(m), lr=1e-3, weight_decay=1e-2),
}


def main():
    cfgs = C.canonical_configs(dropout=False)
    cfg = cfgs[0]
    xn, yn = synth.make_batch(cfg["input_dims"], B, T, seed=7)
    x, y = torch.from_numpy(xn), torch.from_numpy(yn)
    out = {}
    for run, make in RUNS.items():
        model = _model(cfgs)
        opt = make(model)
        trace = []
        for s in range(STEPS):
            opt.zero_grad()
            terms, _ = G.ref_losses(model, x, y, cfg, "l1")
            terms["loss"].backward()
            opt.step()
            trace.append([terms[k].item() for k in ("loss", "disc", "gen", "reg")])
            if s == 0:
                out[run + "_param_after1"] = np.stack([G.summarize(p) for p in model.parameters()])
        out[run + "_param_after_last"] = np.stack([G.summarize(p) for p in model.parameters()])
        out[run + "_trace"] = tr = np.array(trace, dtype=np.float64)
        assert np.isfinite(tr).all() and np.isfinite(out[run + "_param_after_last"]).all() and tr[-1, 0] < tr[0, 0], tr[:, 0]
        out["param_names"] = np.array([n for n, _ in model.named_parameters()])
        print(run, "loss0=%.6f lossN=%.6f" % (tr[0, 0], tr[-1, 0]))
    out["meta"] = np.array([B, T, STEPS])
    path = os.path.join(HERE, NAME + ".npz")
    np.savez_compressed(path, **out)
    print(NAME, "bytes=%d" % os.path.getsize(path))


if __name__ == "__main__":
    main()
