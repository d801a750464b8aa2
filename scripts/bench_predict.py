"""What the epoch's tail costs -- validation loss, scheduler.step, keep-best -- the reference's way and on the prediction-only
path (MFM_KL_EF, fp32, factorized_amd.optim.Adam with a device lr), per call, beside one 40-step training epoch at B=32, T=20:

    ref_module  model.eval(); model(X); l1_loss(y_hat, y).item(); scheduler.step(v); KeepBest.update(v); model.train()
                (mfm_mosi.py:445-477: the whole eval forward, all four outputs, one host read)
    ref_engine  engine.forward(X, train=False, want_xhat=False); l1_loss(...).item(); scheduler.step(v); KeepBest.update(v)
                (the cheapest form the package offered before: still seven recurrences and a training workspace)
    new_eager   model.evaluate(X, y) -> scheduler.step(loss) -> KeepBest.update(loss), no host read
    new_graph   the same three calls replayed as one captured graph
    epoch       40 steps of the reference's unchanged loop, for scale

at the MOSI validation shape (N=229, T=20), at N=1024, T=20 and at N=2048, T=50.

    python scripts/bench_predict.py --out profiles/predict_times.txt

Every time is a host clock around `--calls` calls that end in a device synchronise, after `--warmup` calls of the same form; the
forms alternate within a round and the median over the rounds is reported with the spread (max - min of the rounds).
"""
import argparse

import torch
import torch.nn as nn

from _bench_common import batch, cfgs, loop, mosi_batch, need_gpu, say, timed, write_out
from factorized_amd import _lib  # noqa: E402
from factorized_amd.checkpoint import KeepBest  # noqa: E402
from factorized_amd.lr_scheduler import ReduceLROnPlateau  # noqa: E402
from factorized_amd.mfm_model import MFM_KL_EF  # noqa: E402
import factorized_amd.optim as optim  # noqa: E402

FORMS = ["ref_module", "ref_engine", "new_eager", "new_graph"]
SHAPES = [(229, 20), (1024, 20), (2048, 50)]
STEPS_PER_EPOCH = 40

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=30)
ap.add_argument("--epochs", type=int, default=5)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--out", help="write the record to this file")
args = ap.parse_args()

need_gpu("bench_predict.py")
mosi_batch()                                             # (B=32, T=20: the training epoch beside the tails)
model = MFM_KL_EF(*cfgs)
lr = torch.tensor([1e-3], device="cuda")
optimizer = optim.Adam(model.parameters(), lr=lr, capturable=True)
model = model.to("cuda")
model.train()
loop(model, optimizer, STEPS_PER_EPOCH)                  # (on its engine, every code object loaded)
eng = model.engine
# patience beyond the run: the tail must not move the lr under the timed training epoch
scheduler = ReduceLROnPlateau(optimizer, "min", patience=1 << 30)
best = KeepBest(model)
criterion = nn.L1Loss()

med_all = {}
for N, T in SHAPES:
    X, y = batch(N, T, 9)

    def ref_module():
        model.eval()
        with torch.no_grad():
            decoded, _, _ = model(X)
            v = criterion(decoded[3].squeeze(1), y).item()
        scheduler.step(v)
        best.update(v)
        model.train()

    def ref_engine():
        out = eng.forward(X, None, train=False, want_xhat=False)
        v = criterion(out["y_hat"].squeeze(1), y).item()
        scheduler.step(v)
        best.update(v)

    def new_eager():
        loss = model.evaluate(X, y)
        scheduler.step(loss)
        best.update(loss)

    new_eager()
    ref = criterion(eng.forward(X, None, train=False, want_xhat=False)["y_hat"].squeeze(1), y).item()
    got = float(model.evaluate(X, y))
    assert abs(got - ref) <= 1e-4 * max(abs(ref), 1e-3), (got, ref)
    assert scheduler.last_path == "device" and best.last_path == "flat"
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        new_eager()
    RUN = {"ref_module": ref_module, "ref_engine": ref_engine, "new_eager": new_eager, "new_graph": graph.replay}
    seen = {f: [] for f in FORMS}
    for r in range(args.rounds):
        for form in FORMS:
            seen[form].append(timed(RUN[form], args.calls, args.warmup))
    say("N=%d T=%d   (valid loss %.6f both ways)" % (N, T, got))
    for f in FORMS:
        v = sorted(seen[f])
        med_all[(N, T, f)] = (v[len(v) // 2], v[-1] - v[0])
        say("  %-10s median %9.4f ms/call   (spread of the rounds %.4f; rounds %s)"
            % (f, v[len(v) // 2], v[-1] - v[0], " ".join("%.4f" % t for t in seen[f])))
    pl = eng.plan(T, N)
    pw = int(_lib.lib().mfm_plan_workspace_bytes(pl.handle))
    nw = 4 * eng.predict_workspace_floats(T, N)
    say("  workspace: predict %d bytes (row cap %d), training plan %d bytes" % (nw, eng.PREDICT_MAX_ROWS, pw))
    del graph, pl
    eng._plans.pop((T, N, eng.reg_scale, eng.precision, eng.variant), None)
    eng.__dict__.get("_predict_bufs", {}).clear()
    torch.cuda.empty_cache()

ep = sorted(timed(lambda: loop(model, optimizer, STEPS_PER_EPOCH), args.epochs, args.warmup) for _ in range(args.rounds))
say("epoch (40 steps, B=32, T=20) median %9.4f ms   (spread of the rounds %.4f)" % (ep[len(ep) // 2], ep[-1] - ep[0]))
for N, T in SHAPES:
    base = med_all[(N, T, "ref_engine")]
    for f in ("new_eager", "new_graph"):
        m = med_all[(N, T, f)]
        say("N=%d T=%d  %s / ref_engine = %.3f   (%.4f vs %.4f ms; spreads %.4f, %.4f)   = %.4f epochs"
            % (N, T, f, m[0] / base[0], m[0], base[0], m[1], base[1], m[0] / ep[len(ep) // 2]))
write_out(args.out, "scripts/bench_predict.py --calls %d --epochs %d --warmup %d --rounds %d: MFM_KL_EF, fp32, optim.Adam"
          % (args.calls, args.epochs, args.warmup, args.rounds))
