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

import torch

from _bench_common import cfgs, config, loop, mosi_batch, need_gpu, timed_steps
from factorized_amd import nn_utils  # noqa: E402
from factorized_amd.mfm_model import MFM_KL_EF  # noqa: E402
import factorized_amd.optim as optim  # noqa: E402

MAX_NORM = 20.0
FORMS = {"none": None, "torch": lambda m: torch.nn.utils.clip_grad_norm_(m.parameters(), MAX_NORM),
         "flat": lambda m: nn_utils.clip_grad_norm_(m.parameters(), MAX_NORM)}

ap = argparse.ArgumentParser()
ap.add_argument("--only", choices=list(FORMS))
ap.add_argument("--steps", type=int, default=300)
ap.add_argument("--warmup", type=int, default=30)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--no-item", action="store_true", help="leave out the loop's per-step disc_loss.item()")
args = ap.parse_args()

need_gpu("bench_clip.py")
mosi_batch()


def run(form, item):
    gc.collect()
    torch.cuda.empty_cache()
    model = MFM_KL_EF(*cfgs)
    optimizer = optim.SGD(model.parameters(), lr=config["lr"], momentum=config["momentum"])
    model = model.to("cuda")
    model.train()
    ms = timed_steps(lambda k: loop(model, optimizer, k, item, after_backward=FORMS[form]), args.steps, args.warmup)
    assert model._handover_ok() and model._grad_views_attached() and optimizer._fallback is None      # the flat path all along
    return ms


items = (False,) if args.no_item else (True, False)
for item in items:
    for r in range(1 if args.only else args.rounds):
        for form in ([args.only] if args.only else list(FORMS)):
            print("%-6s %-28s round %d  %.3f ms/step" % (form, "with per-step .item()" if item else "no per-step .item()", r,
                                                         run(form, item)), flush=True)
