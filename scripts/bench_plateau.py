"""What `scheduler.step(valid_loss)` costs at the MOSI configuration (MFM_KL_EF, B=32, T=20, fp32, factorized_amd.optim.Adam with
capturable=True and a device lr), per call, against the epoch it sits at the end of (the reference's
`scheduler.step(valid_loss)` with ReduceLROnPlateau(optimizer, 'min'), mfm_mosi.py:470-477; 1284 training samples = 40 steps per
epoch).  valid_loss is a device scalar, as an evaluate() that does not read it back leaves it:

    torch     torch.optim.lr_scheduler.ReduceLROnPlateau.step(valid_loss.item()): the read-back, then the rule on the host
    device    factorized_amd.lr_scheduler.ReduceLROnPlateau.step(valid_loss): one launch, nothing read back
    epoch     40 steps of the reference's unchanged loop (with its per-step .item()), for scale

    python scripts/bench_plateau.py                                    # the three, alternating, --rounds times each
    python scripts/bench_plateau.py --out profiles/plateau_times.txt   # ... and the record

Every time is a host clock around `--calls` calls (epoch: `--epochs` epochs) that end in a device synchronise, after `--warmup`
calls of the same form; the forms alternate within a round and the median over the rounds is reported with the spread.  Both
schedulers see a metric that never improves with a patience that never runs out: a bad epoch, no reduction, every call.
"""
import argparse
import os
import subprocess

import torch

from _bench_common import B, T, cfgs, loop, mosi_batch, need_gpu, report, say, timed, write_out
from factorized_amd.lr_scheduler import ReduceLROnPlateau  # noqa: E402
from factorized_amd.mfm_model import MFM_KL_EF  # noqa: E402
import factorized_amd.optim as optim  # noqa: E402

FORMS = ["torch", "device", "epoch"]
STEPS_PER_EPOCH = 40

ap = argparse.ArgumentParser()
ap.add_argument("--only", choices=FORMS)
ap.add_argument("--calls", type=int, default=10000)
ap.add_argument("--epochs", type=int, default=25)
ap.add_argument("--warmup", type=int, default=20)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--commit", help="the commit the record is taken on (default: git rev-parse HEAD, if this is a checkout)")
ap.add_argument("--out", help="write the record (every round, the medians, the ratios) to this file")
args = ap.parse_args()

need_gpu("bench_plateau.py")
mosi_batch()
model = MFM_KL_EF(*cfgs).to("cuda")
lr = torch.tensor([1e-3], device="cuda")
optimizer = optim.Adam(model.parameters(), lr=lr, capturable=True)
model.train()
loop(model, optimizer, STEPS_PER_EPOCH)                  # (on its engine, every code object loaded)
NEVER = 2 ** 30                                          # a patience that never runs out
valid_loss = torch.tensor(2.0, device="cuda")
theirs = torch.optim.lr_scheduler.ReduceLROnPlateau(optimizer, "min", patience=NEVER)
ours = ReduceLROnPlateau(optimizer, "min", patience=NEVER)
theirs.step(1.0)
ours.step(1.0)
assert ours.last_path == "device"


RUN = {
    "torch": lambda: timed(lambda: theirs.step(valid_loss.item()), args.calls, args.warmup),
    "device": lambda: timed(lambda: ours.step(valid_loss), args.calls, args.warmup),
    "epoch": lambda: timed(lambda: loop(model, optimizer, STEPS_PER_EPOCH), args.epochs, args.warmup),
}

forms = [args.only] if args.only else FORMS
seen = {f: [] for f in forms}
for r in range(args.rounds):
    for form in forms:
        ms = RUN[form]()
        seen[form].append(ms)
        say("%-7s round %d  %9.4f ms/%s" % (form, r, ms, "epoch" if form == "epoch" else "call"))
# every call was a bad epoch that reduced nothing, on the device path
assert ours.last_path == "device" and ours.best == theirs.best == 1.0 and ours.reductions == 0 and float(lr) == float(torch.tensor(1e-3))
assert ours.num_bad_epochs == ours.last_epoch - 1 and theirs.num_bad_epochs == theirs.last_epoch - 1
med = report(seen, lambda f, m, spread: "%-7s median   %9.4f ms/%s   (spread of the rounds %.4f)"
             % (f, m, "epoch" if f == "epoch" else "call", spread))
if "epoch" in med:
    step = med["epoch"] / STEPS_PER_EPOCH
    say("step    = epoch / %d = %.4f ms" % (STEPS_PER_EPOCH, step))
    for f in forms:
        if f != "epoch":
            say("%-7s = %.5f epochs = %.4f steps" % (f, med[f] / med["epoch"], med[f] / step))
if args.out:
    commit = args.commit
    if commit is None:
        try:
            commit = subprocess.check_output(["git", "rev-parse", "HEAD"], cwd=os.path.dirname(os.path.abspath(__file__)),
                                             stderr=subprocess.DEVNULL).decode().strip()
        except (OSError, subprocess.CalledProcessError):
            commit = "unknown"
    write_out(args.out, "scripts/bench_plateau.py --calls %d --epochs %d --warmup %d --rounds %d: MFM_KL_EF, B=%d, T=%d, fp32, "
              "optim.Adam(capturable=True, lr=device tensor); taken on commit %s"
              % (args.calls, args.epochs, args.warmup, args.rounds, B, T, commit))
