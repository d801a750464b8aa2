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

import torch

from _bench_common import B, T, cfgs, loop, mosi_batch, need_gpu, report, say, timed_steps, write_out
from factorized_amd import swa_utils  # noqa: E402
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

need_gpu("bench_swa.py")
mosi_batch()


def run(form, item):
    gc.collect()
    torch.cuda.empty_cache()
    model = MFM_KL_EF(*cfgs)
    optimizer = optim.Adam(model.parameters())
    model = model.to("cuda")
    model.train()
    loop(model, optimizer, 1, item)                      # (the source is on its engine before the copy is taken)
    averaged = FORMS[form](model) if FORMS[form] else None
    update = averaged.update_parameters if averaged is not None else None
    ms = timed_steps(lambda k: loop(model, optimizer, k, item, after_step=update), args.steps, args.warmup)
    assert model._handover_ok() and model._grad_views_attached() and optimizer._fallback is None      # the flat path all along
    if averaged is not None:
        assert int(averaged.n_averaged) == args.warmup + args.steps
        if form == "flat":
            assert averaged._mfm_ticket is not None and int(averaged._mfm_ticket) == 0                # ... of the averaging too
    return ms


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
    med = report(seen, lambda f, m, spread: "%-6s %-24s median   %.3f ms/step   (spread of the rounds %.3f)" % (f, what, m, spread))
    if "none" in med:
        for f in forms:
            if f != "none":
                say("%-6s %-24s adds     %+.3f ms/step to the loop without averaging" % (f, what, med[f] - med["none"]))
write_out(args.out, "scripts/bench_swa.py --steps %d --warmup %d --rounds %d: MFM_KL_EF, B=%d, T=%d, fp32, optim.Adam, EMA decay %g"
          % (args.steps, args.warmup, args.rounds, B, T, DECAY))
