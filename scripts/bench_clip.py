"""ms per step of the reference's UNCHANGED loop (mfm_mosi.py:427-441 incl. its per-step .item()) on MFM_KL_EF, B=32, T=20, fp32,
factorized_amd.optim.SGD(lr=0.01, momentum=0.9), in three forms (the method of scripts/bench_dropin.py):

    none    no clipping
    torch   torch.nn.utils.clip_grad_norm_(model.parameters(), MAX_NORM) between backward() and step()
    flat    factorized_amd.nn_utils.clip_grad_norm_(model.parameters(), MAX_NORM) there

    python scripts/bench_clip.py                         # the three forms, alternating, --rounds times each
    python scripts/bench_clip.py --only flat --steps 200 # one form alone, e.g. under rocprofv3 --kernel-trace --stats
"""
import argparse
import gc
import os
import sys
import time

import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from factorized_amd import configs, nn_utils, synth  # noqa: E402
from factorized_amd.mfm_model import MFM_KL_EF  # noqa: E402
import factorized_amd.optim as optim  # noqa: E402

MAX_NORM = 20.0
FORMS = {"none": None, "torch": lambda ps: torch.nn.utils.clip_grad_norm_(ps, MAX_NORM),
         "flat": lambda ps: nn_utils.clip_grad_norm_(ps, MAX_NORM)}

ap = argparse.ArgumentParser()
ap.add_argument("--only", choices=list(FORMS))
ap.add_argument("--steps", type=int, default=300)
ap.add_argument("--warmup", type=int, default=30)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--no-item", action="store_true", help="leave out the loop's per-step disc_loss.item()")
args = ap.parse_args()

cfgs = configs.canonical_configs(dropout=True)
config = cfgs[0]
B, T = 32, 20
xn, yn = synth.make_batch(config["input_dims"], B, T, seed=7)
X, y = torch.from_numpy(xn).cuda(), torch.from_numpy(yn).cuda()
d_l, d_a, d_v = config["input_dims"]


def loop(model, optimizer, steps, clip, item):
    criterion, gen_criterion = nn.L1Loss(), nn.MSELoss()
    epoch_loss = 0.0
    for _ in range(steps):
        optimizer.zero_grad()
        batch_X, batch_y = X, y
        decoded, mmd_loss, missing_loss = model.forward(batch_X)
        [x_l_hat, x_a_hat, x_v_hat, y_hat] = decoded
        gen_loss = config["lda_xl"] * gen_criterion(x_l_hat, batch_X[:, :, :d_l]) + config["lda_xa"] * gen_criterion(x_a_hat, batch_X[:, :, d_l:d_l + d_a]) \
            + config["lda_xv"] * gen_criterion(x_v_hat, batch_X[:, :, d_l + d_a:])
        disc_loss = criterion(y_hat.squeeze(1), batch_y)
        loss = disc_loss + gen_loss + config["lda_mmd"] * mmd_loss + missing_loss
        loss.backward()
        if clip is not None:
            clip(model.parameters())
        optimizer.step()
        if item:
            epoch_loss += disc_loss.item()


def run(form, item):
    gc.collect()
    torch.cuda.empty_cache()
    model = MFM_KL_EF(*cfgs)
    optimizer = optim.SGD(model.parameters(), lr=config["lr"], momentum=config["momentum"])
    model = model.to("cuda")
    model.train()
    loop(model, optimizer, args.warmup, FORMS[form], item)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    loop(model, optimizer, args.steps, FORMS[form], item)
    torch.cuda.synchronize()
    ms = 1e3 * (time.perf_counter() - t0) / args.steps
    assert model._handover_ok() and model._grad_views_attached() and optimizer._fallback is None      # the flat path all along
    return ms


items = (False,) if args.no_item else (True, False)
for item in items:
    for r in range(1 if args.only else args.rounds):
        for form in ([args.only] if args.only else list(FORMS)):
            print("%-6s %-28s round %d  %.3f ms/step" % (form, "with per-step .item()" if item else "no per-step .item()", r,
                                                         run(form, item)), flush=True)
