"""What model.predict_zeros of the MFN classes (MFM_KL, MFM, fp32) costs per call through the fused entry
(mfm_predict_zeros_mfn) and on the path it replaces, both in one session on one card:

    old_route    what predict_zeros of these classes did before the entry, unchanged in engine.predict_zeros as the fallback for
                 sizes the entry refuses, and taken here by a second model of the same weights whose engine is told the entry
                 refused: three x.clone() copies with a column range zeroed, three forward(train=False, handover=False) on a
                 training plan of the split's shape, three reductions
    new_eager    model.predict_zeros(X, y)
    new_graph    the same call replayed as one captured graph

at T = 20 and N = 32 (one MOSI batch), 229 (the MOSI validation split) and 1024, with the peak device memory of a first call
either way (beyond the parameters and the split, which both need).  It sets no threshold; it records.

    python scripts/bench_zeros_mfn.py --out profiles/zeros_mfn_times.txt

Every time is a host clock around `--calls` calls that end in a device synchronise, after `--warmup` calls of the same form; the
forms alternate within a round and the median over the rounds (at least five) is reported with the spread (max - min of the
rounds).  Two medians count as apart when they differ by more than the larger of the two spreads.
"""
import argparse

import torch

from _bench_common import batch, captured, cfgs, median, need_gpu, peak_of, say, timed, write_out
from factorized_amd import mfm_model as M  # noqa: E402

FORMS = ["old_route", "new_eager", "new_graph"]
SHAPES = [(32, 20), (229, 20), (1024, 20)]
CLS = (("MFM_KL", "kl"), ("MFM", "mmd"))

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=30)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--out", help="write the record to this file")
args = ap.parse_args()
if args.rounds < 5:
    ap.error("--rounds must be at least 5: the medians are compared against the spread of the rounds")

need_gpu("bench_zeros_mfn.py")


verdicts = []
for cls, variant in CLS:
    torch.manual_seed(0)
    model = getattr(M, cls)(*cfgs).to("cuda")
    torch.manual_seed(0)                             # the same initialisation: the two routes are compared below
    old = getattr(M, cls)(*cfgs).to("cuda")
    model.train()
    old.train()
    eng = model.engine
    old.engine._zeros_mfn_refused = True             # the fallback: the path before the entry
    for N, T in SHAPES:
        X, y = batch(N, T, 9)

        def old_route():
            return old.predict_zeros(X, y)

        def new_eager():
            return model.predict_zeros(X, y)

        peak_new = peak_of(new_eager)
        peak_old = peak_of(old_route)
        assert eng.__dict__.get("_zeros_mfn_bufs") and not eng._plans and not old.engine.__dict__.get("_zeros_mfn_bufs")
        ref = [t.cpu() for t in old_route()]
        got = [t.cpu() for t in new_eager()]
        for g, r in zip(got, ref):
            assert float((g - r).abs().max()) <= 1e-4 * max(float(r.abs().max()), 1e-3), (g, r)
        graph = captured(new_eager)
        RUN = {"old_route": old_route, "new_eager": new_eager, "new_graph": graph.replay}
        seen = {f: [] for f in FORMS}
        for r in range(args.rounds):
            for form in FORMS:
                seen[form].append(timed(RUN[form], args.calls, args.warmup))
        say("%s N=%d T=%d   (gen %s disc %s both ways)" % (cls, N, T, " ".join("%.6f" % v for v in got[1]), " ".join("%.6f" % v for v in got[2])))
        med = {f: median(seen[f]) for f in FORMS}
        for f in FORMS:
            say("  %-10s median %9.4f ms/call   (spread of the rounds %.4f; rounds %s)"
                % (f, med[f][0], med[f][1], " ".join("%.4f" % t for t in seen[f])))
        say("  peak device memory of a first call: predict_zeros %d bytes (workspace %d, row cap %d), the three eval forwards on a plan %d bytes"
            % (peak_new, 4 * eng.predict_zeros_workspace_floats(T, N), eng.PREDICT_MAX_ROWS, peak_old))
        for f in ("new_eager", "new_graph"):
            apart = med["old_route"][0] - med[f][0] > max(med["old_route"][1], med[f][1])
            verdicts.append("%s N=%d T=%d  %s / old_route = %.3f   (%.4f vs %.4f ms; spreads %.4f, %.4f): %s"
                            % (cls, N, T, f, med[f][0] / med["old_route"][0], med[f][0], med["old_route"][0], med[f][1], med["old_route"][1],
                               "faster" if apart else "not faster"))
        del graph
        old.engine._plans.clear()
        eng.__dict__.get("_zeros_mfn_bufs", {}).clear()
        torch.cuda.empty_cache()
    del model, old

for v in verdicts:
    say(v)
write_out(args.out, "scripts/bench_zeros_mfn.py --calls %d --warmup %d --rounds %d: MFM_KL and MFM, fp32" % (args.calls, args.warmup, args.rounds))
