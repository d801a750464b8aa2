"""What the full validation objective of a split costs -- loss, disc, gen_l, gen_a, gen_v, reg -- on the plan-free path and the
way the package offered before (MFM_KL_EF, fp32), per call:

    ref_forward  engine.forward(X, y, train=False) on a training plan of the split's shape, then the six numbers from its loss
                 slots on the device (every x_hat written to HBM, the BPTT workspace allocated)
    new_eager    model.objective(X, y)
    new_graph    the same call replayed as one captured graph

at T = 20 and N = 229 (the MOSI validation split), 1024 and 4096, with the peak device memory of either way (beyond the
parameters and the split, which both need).  It sets no threshold; it records.

    python scripts/bench_objective.py --out profiles/objective_times.txt

Every time is a host clock around `--calls` calls that end in a device synchronise, after `--warmup` calls of the same form; the
forms alternate within a round and the median over the rounds is reported with the spread (max - min of the rounds).
"""
import argparse

import torch

from _bench_common import batch, captured, cfgs, need_gpu, peak_of, say, timed, write_out
from factorized_amd.mfm_model import MFM_KL_EF  # noqa: E402

FORMS = ["ref_forward", "new_eager", "new_graph"]
SHAPES = [(229, 20), (1024, 20), (4096, 20)]

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=30)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--out", help="write the record to this file")
args = ap.parse_args()

need_gpu("bench_objective.py")
model = MFM_KL_EF(*cfgs).to("cuda")
model.train()
eng = model.engine
c = eng.cfg


def six(l):
    out = torch.empty(6, dtype=torch.float32, device="cuda")
    out[1:6] = l[0:5]
    out[0] = l[0] + c["lda_xl"] * l[1] + c["lda_xa"] * l[2] + c["lda_xv"] * l[3] + c["lda_mmd"] * l[4]
    return out


med_all = {}
for N, T in SHAPES:
    X, y = batch(N, T, 9)

    def ref_forward():
        return six(eng.forward(X, y, train=False)["losses"])

    def new_eager():
        return model.objective(X, y)

    key = (T, N, eng.reg_scale, eng.precision, eng.variant)
    peak_new = peak_of(new_eager)
    peak_ref = peak_of(ref_forward)
    ref = [float(v) for v in ref_forward().cpu()]
    got = [float(v) for v in torch.stack(list(new_eager())).cpu()]
    for g, r in zip(got, ref):
        assert abs(g - r) <= 1e-4 * max(abs(r), 1e-3), (got, ref)
    graph = captured(new_eager)
    RUN = {"ref_forward": ref_forward, "new_eager": new_eager, "new_graph": graph.replay}
    seen = {f: [] for f in FORMS}
    for r in range(args.rounds):
        for form in FORMS:
            seen[form].append(timed(RUN[form], args.calls, args.warmup))
    say("N=%d T=%d   (loss %.6f disc %.6f gen_l %.6f gen_a %.6f gen_v %.6f reg %.4f both ways)" % ((N, T) + tuple(got)))
    for f in FORMS:
        v = sorted(seen[f])
        med_all[(N, f)] = (v[len(v) // 2], v[-1] - v[0])
        say("  %-11s median %9.4f ms/call   (spread of the rounds %.4f; rounds %s)"
            % (f, v[len(v) // 2], v[-1] - v[0], " ".join("%.4f" % t for t in seen[f])))
    say("  peak device memory of a first call: objective %d bytes (workspace %d, row cap %d), eval forward on a plan %d bytes"
        % (peak_new, 4 * eng.objective_workspace_floats(T, N), eng.PREDICT_MAX_ROWS, peak_ref))
    del graph
    eng._plans.pop(key, None)
    eng.__dict__.get("_objective_bufs", {}).clear()
    torch.cuda.empty_cache()

for N, T in SHAPES:
    base = med_all[(N, "ref_forward")]
    for f in ("new_eager", "new_graph"):
        m = med_all[(N, f)]
        say("N=%d T=%d  %s / ref_forward = %.3f   (%.4f vs %.4f ms; spreads %.4f, %.4f)"
            % (N, T, f, m[0] / base[0], m[0], base[0], m[1], base[1]))
write_out(args.out, "scripts/bench_objective.py --calls %d --warmup %d --rounds %d: MFM_KL_EF, fp32" % (args.calls, args.warmup, args.rounds))
