"""What "keep the best model" costs at the MOSI configuration (MFM_KL_EF, B=32, T=20, fp32, factorized_amd.optim.Adam), per call,
against the epoch it sits at the end of (the reference's `if valid_loss <= best_valid: torch.save(model, path)`,
mfm_mosi.py:467-473; 1284 training samples = 40 steps per epoch):

    save      torch.save(model, file) into a temporary directory, as the reference does (whole-module pickle)
    deepcopy  copy.deepcopy(model.state_dict()): the usual in-memory replacement
    take      factorized_amd.checkpoint.KeepBest.update(metric) when it takes a snapshot      (device metric, one launch)
    skip      KeepBest.update(metric) when it does not take one                               (the same launch, no copy)
    epoch     40 steps of the reference's unchanged loop (with its per-step .item()), for scale

    python scripts/bench_keepbest.py                                     # the five, alternating, --rounds times each
    python scripts/bench_keepbest.py --out profiles/keepbest_times.txt   # ... and the record

Every time is a host clock around `--calls` calls (epoch: `--epochs` epochs) that end in a device synchronise, after `--warmup`
calls of the same form; the forms alternate within a round and the median over the rounds is reported with the spread.
"""
import argparse
import copy
import os
import tempfile

import torch

from _bench_common import B, T, cfgs, loop, mosi_batch, need_gpu, report, say, timed, write_out
from factorized_amd.checkpoint import KeepBest  # noqa: E402
from factorized_amd.mfm_model import MFM_KL_EF  # noqa: E402
import factorized_amd.optim as optim  # noqa: E402

FORMS = ["save", "deepcopy", "take", "skip", "epoch"]
STEPS_PER_EPOCH = 40

ap = argparse.ArgumentParser()
ap.add_argument("--only", choices=FORMS)
ap.add_argument("--calls", type=int, default=200)
ap.add_argument("--epochs", type=int, default=25)
ap.add_argument("--warmup", type=int, default=20)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--out", help="write the record (every round, the medians, the ratios) to this file")
args = ap.parse_args()

need_gpu("bench_keepbest.py")
mosi_batch()
model = MFM_KL_EF(*cfgs)
optimizer = optim.Adam(model.parameters())
model = model.to("cuda")
model.train()
loop(model, optimizer, STEPS_PER_EPOCH)                  # (on its engine, every code object loaded)
tmp = tempfile.mkdtemp(prefix="keepbest_")
path = os.path.join(tmp, "mfn_0.pt")
good, bad = torch.tensor(1.0, device="cuda"), torch.tensor(2.0, device="cuda")
best = KeepBest(model, initial=1.0)                      # `good` ties (takes, and keeps 1.0), `bad` never takes
best.update(good)
assert best.last_path == "flat"


RUN = {
    "save": lambda: timed(lambda: torch.save(model, path), args.calls, args.warmup),
    "deepcopy": lambda: timed(lambda: copy.deepcopy(model.state_dict()), args.calls, args.warmup),
    "take": lambda: timed(lambda: best.update(good), args.calls * 50, args.warmup),
    "skip": lambda: timed(lambda: best.update(bad), args.calls * 50, args.warmup),
    "epoch": lambda: timed(lambda: loop(model, optimizer, STEPS_PER_EPOCH), args.epochs, args.warmup),
}

forms = [args.only] if args.only else FORMS
seen = {f: [] for f in forms}
for r in range(args.rounds):
    for form in forms:
        calls0 = best.calls
        ms = RUN[form]()
        seen[form].append(ms)
        if form in ("take", "skip"):                     # the launch took / skipped every time, on the flat path
            n = best.calls - calls0
            assert best.last_path == "flat" and best.value == 1.0 and best.taken == (form == "take")
            assert best.epoch == (best.calls - 1 if form == "take" else best.epoch) and n == args.calls * 50 + min(args.warmup, args.calls * 50)
        say("%-9s round %d  %9.4f ms/%s" % (form, r, ms, "epoch" if form == "epoch" else "call"))
med = report(seen, lambda f, m, spread: "%-9s median   %9.4f ms/%s   (spread of the rounds %.4f)"
             % (f, m, "epoch" if f == "epoch" else "call", spread))
if "epoch" in med:
    step = med["epoch"] / STEPS_PER_EPOCH
    say("step      = epoch / %d = %.4f ms" % (STEPS_PER_EPOCH, step))
    for f in forms:
        if f != "epoch":
            say("%-9s = %.3f epochs = %.2f steps" % (f, med[f] / med["epoch"], med[f] / step))
say("file size of the whole-module pickle: %d bytes; snapshot range: %d floats"
    % (os.path.getsize(path) if os.path.exists(path) else -1, model.engine.layout.guard))
if os.path.exists(path):
    os.remove(path)
os.rmdir(tmp)
write_out(args.out, "scripts/bench_keepbest.py --calls %d --epochs %d --warmup %d --rounds %d: MFM_KL_EF, B=%d, T=%d, fp32, optim.Adam"
          % (args.calls, args.epochs, args.warmup, args.rounds, B, T))
