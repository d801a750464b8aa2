"""What one training step of the ablation M_D costs (the `train` block of the reference's train_mfm_ablation: the label loss, all
gradients, Adam, zero_grad) on the one-call entry and the way the package offered before, fp32, MOSI sizes, train mode
(dropout as configured), per step:

    composed     zero_grad -> forward() -> F.l1_loss -> .backward() -> optim.Adam.step: the composed autograd path of the module's
                 granular HIP operations, as it was before loss_and_grad existed
    new_eager    zero_grad -> model.loss_and_grad(X, y) -> optim.Adam.step
    new_graph    zero_grad(set_to_none=False) -> loss_and_grad -> optim.Adam(capturable=True).step replayed as one captured graph

at T = 20 and N = 32 (the training batch), 229 (the MOSI validation split's size) and 1024, with the peak device memory of either
way (beyond the parameters and the batch, which both need).  It sets no threshold; it records.

    python scripts/bench_train_ablation.py --out profiles/train_ablation_times.txt

Every time is a host clock around `--calls` steps that end in a device synchronise, after `--warmup` steps of the same form; the
forms alternate within a round and the median over the rounds is reported with the spread (max - min of the rounds).
"""
import argparse
import copy

import torch
import torch.nn.functional as F

from _bench_common import batch, captured, cfgs, median, need_gpu, peak_of, say, timed, write_out
from factorized_amd import mfm_model as M  # noqa: E402
from factorized_amd import optim  # noqa: E402

FORMS = ["composed", "new_eager", "new_graph"]
SHAPES = [(32, 20), (229, 20), (1024, 20)]

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=30)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--out", help="write the record to this file")
args = ap.parse_args()

need_gpu("bench_train_ablation.py")
base = M.M_D(*cfgs).to("cuda")
med_all = {}
for N, T in SHAPES:
    X, y = batch(N, T, 9)
    y = y.reshape(N, 1).contiguous()
    models = {f: copy.deepcopy(base) for f in FORMS}
    opts = {f: optim.Adam(models[f].parameters(), lr=torch.tensor([1e-3], device="cuda") if f == "new_graph" else 1e-3,
                          capturable=(f == "new_graph")) for f in FORMS}

    def composed():
        model, opt = models["composed"], opts["composed"]
        opt.zero_grad()
        loss = F.l1_loss(model.forward(X)[0][3], y)
        loss.backward()
        opt.step()
        return loss

    def new_eager():
        model, opt = models["new_eager"], opts["new_eager"]
        opt.zero_grad()
        loss = model.loss_and_grad(X, y)
        opt.step()
        return loss

    def graph_step():
        model, opt = models["new_graph"], opts["new_graph"]
        opt.zero_grad(set_to_none=False)
        loss = model.loss_and_grad(X, y)
        opt.step()
        return loss

    # both ways compute the same step: in eval mode (no dropout) the first losses agree
    for m in models.values():
        m.eval()
    peak_new = peak_of(new_eager)
    peak_ref = peak_of(composed)
    l_new, l_ref = float(new_eager()), float(composed())
    assert abs(l_new - l_ref) <= 1e-4 * abs(l_ref), (N, l_new, l_ref)
    for m in models.values():
        m.train()
    graph_step()
    graph = captured(graph_step)
    RUN = {"composed": composed, "new_eager": new_eager, "new_graph": graph.replay}
    seen = {f: [] for f in FORMS}
    for r in range(args.rounds):
        for form in FORMS:
            seen[form].append(timed(RUN[form], args.calls, args.warmup))
    say("M_D N=%d T=%d   (second-step loss in eval mode: loss_and_grad %.6f, composed %.6f)" % (N, T, l_new, l_ref))
    for f in FORMS:
        med_all[(N, f)] = median(seen[f])
        say("  %-11s median %9.4f ms/step   (spread of the rounds %.4f; rounds %s)"
            % (f, med_all[(N, f)][0], med_all[(N, f)][1], " ".join("%.4f" % t for t in seen[f])))
    say("  peak device memory of a first step: loss_and_grad %d bytes (row cap %d), the composed path %d bytes"
        % (peak_new, base.TRAIN_MAX_ROWS, peak_ref))
    del graph, models, opts
    torch.cuda.empty_cache()

for N, T in SHAPES:
    ref = med_all[(N, "composed")]
    for f in ("new_eager", "new_graph"):
        m = med_all[(N, f)]
        say("M_D N=%d T=%d  %s / composed = %.3f   (%.4f vs %.4f ms; spreads %.4f, %.4f)" % (N, T, f, m[0] / ref[0], m[0], ref[0], m[1], ref[1]))
write_out(args.out, "scripts/bench_train_ablation.py --calls %d --warmup %d --rounds %d: M_D, fp32, train mode" % (args.calls, args.warmup, args.rounds))
