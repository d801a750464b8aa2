"""ms per step of the reference's UNCHANGED loop (mfm_mosi.py:427-441 incl. its per-step .item()) on MFM_KL_EF, B=32, T=20, fp32,
factorized_amd.optim.Adam, in three forms (the method of scripts/bench_clip.py):

    none    no weight averaging
    torch   torch.optim.swa_utils.AveragedModel(model, multi_avg_fn=get_ema_multi_avg_fn(0.999)), updated after every step()
    flat    factorized_amd.swa_utils.AveragedModel with this library's get_ema_multi_avg_fn(0.999), updated there

    python scripts/bench_swa.py                          # the three forms, alternating, --rounds times each
    python scripts/bench_swa.py --only flat --steps 200  # one form alone, e.g. under rocprofv3 --kernel-trace --stats
    python scripts/bench_swa.py --out profiles/swa_step_times.txt      # ... and the record

The time is a host clock around `--steps` steps that end in a device synchronise, after `--warmup` steps of the same form.
"""
import argparse
import gc
import os
import sys
import time

import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from factorized_amd import configs, swa_utils, synth  # noqa: E402
from factorized_amd.mfm_model import MFM_KL_EF  # noqa: E402
import factorized_amd.optim as optim  # noqa: E402

DECAY = 0.999
FORMS = {"none": None,
         "torch": lambda m: torch.optim.swa_utils.AveragedModel(m, multi_avg_fn=torch.optim.swa_utils.get_ema_multi_avg_fn(DECAY)),
         "flat": lambda m: swa_utils.AveragedModel(m, multi_avg_fn=swa_utils.get_ema_multi_avg_fn(DECAY))}

ap = argparse.ArgumentParser()
ap.add_argument("--only", choices=list(FORMS))
ap.add_argument("--steps", type=int, default=300)
ap.add_argument("--warmup", type=int, default=30)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--no-item", action="store_true", help="leave out the loop's per-step disc_loss.item()")
ap.add_argument("--out", help="write the record (every round, the medians, what the averaging adds) to this file")
args = ap.parse_args()

cfgs = configs.canonical_configs(dropout=True)
config = cfgs[0]
B, T = 32, 20
xn, yn = synth.make_batch(config["input_dims"], B, T, seed=7)
X, y = torch.from_numpy(xn).cuda(), torch.from_numpy(yn).cuda()
d_l, d_a, d_v = config["input_dims"]


def loop(model, optimizer, steps, averaged, item):
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
        optimizer.step()
        if averaged is not None:
            averaged.update_parameters(model)
        if item:
            epoch_loss += disc_loss.item()


def run(form, item):
    gc.collect()
    torch.cuda.empty_cache()
    model = MFM_KL_EF(*cfgs)
    optimizer = optim.Adam(model.parameters())
    model = model.to("cuda")
    model.train()
    loop(model, optimizer, 1, None, item)                # (the source is on its engine before the copy is taken)
    averaged = FORMS[form](model) if FORMS[form] else None
    loop(model, optimizer, args.warmup, averaged, item)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    loop(model, optimizer, args.steps, averaged, item)
    torch.cuda.synchronize()
    ms = 1e3 * (time.perf_counter() - t0) / args.steps
    assert model._handover_ok() and model._grad_views_attached() and optimizer._fallback is None      # the flat path all along
    if averaged is not None:
        assert int(averaged.n_averaged) == args.warmup + args.steps
        if form == "flat":
            assert averaged._mfm_ticket is not None and int(averaged._mfm_ticket) == 0                # ... of the averaging too
    return ms


lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


items = (False,) if args.no_item else (True, False)
forms = [args.only] if args.only else list(FORMS)
for item in items:
    what = "with per-step .item()" if item else "no per-step .item()"
    seen = {f: [] for f in forms}
    for r in range(1 if args.only else args.rounds):
        for form in forms:
            ms = run(form, item)
            seen[form].append(ms)
            say("%-6s %-24s round %d  %.3f ms/step" % (form, what, r, ms))
    med = {f: sorted(v)[len(v) // 2] for f, v in seen.items()}
    for f in forms:
        say("%-6s %-24s median   %.3f ms/step   (spread of the rounds %.3f)" % (f, what, med[f], max(seen[f]) - min(seen[f])))
    if "none" in med:
        for f in forms:
            if f != "none":
                say("%-6s %-24s adds     %+.3f ms/step to the loop without averaging" % (f, what, med[f] - med["none"]))
if args.out:
    with open(args.out, "w") as f:
        f.write("scripts/bench_swa.py --steps %d --warmup %d --rounds %d: MFM_KL_EF, B=%d, T=%d, fp32, optim.Adam, EMA decay %g\n"
                % (args.steps, args.warmup, args.rounds, B, T, DECAY))
        f.write("\n".join(lines) + "\n")
