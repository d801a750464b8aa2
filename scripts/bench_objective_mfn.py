"""What model.objective of the MFN classes (MFM_KL, MFM, fp32) costs per call through the fused entry (mfm_objective_mfn) and on
the path it replaces, both in one session on one card:

    old_route    what objective of these classes did before the entry, unchanged in engine.objective as the fallback for sizes
                 the entry refuses, and taken here by a second model of the same weights whose engine is told the entry refused:
                 forward(train=False, handover=False) on a training plan of the split's shape and the six numbers re-assembled
                 with torch operations
    new_eager    model.objective(X, y)
    new_graph    the same call replayed as one captured graph

at T = 20 and N = 32 (one MOSI batch), 229 (the MOSI validation split), 1024 and 4096, with the peak device memory of a first
call either way (beyond the parameters and the split, which both need).  MFM gets the same fixed Gaussian sample on both routes
(a drawn one costs the fused route one .normal_() launch more, the old route one torch.randn).  It sets no threshold; it records.

    python scripts/bench_objective_mfn.py --out profiles/objective_mfn_times.txt

Every time is a host clock around `--calls` calls that end in a device synchronise, after `--warmup` calls of the same form; the
forms alternate within a round and the median over the rounds (at least five) is reported with the spread (max - min of the
rounds).  Two medians count as apart when they differ by more than the larger of the two spreads.
"""
import argparse

import torch

from _bench_common import batch, captured, cfgs, median, need_gpu, peak_of, say, timed, write_out
from factorized_amd import mfm_model as M  # noqa: E402

FORMS = ["old_route", "new_eager", "new_graph"]
SHAPES = [(32, 20), (229, 20), (1024, 20), (4096, 20)]
CLS = (("MFM_KL", "kl"), ("MFM", "mmd"))

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=30)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--out", help="write the record to this file")
args = ap.parse_args()
if args.rounds < 5:
    ap.error("--rounds must be at least 5: the medians are compared against the spread of the rounds")

need_gpu("bench_objective_mfn.py")


verdicts = []
for cls, variant in CLS:
    torch.manual_seed(0)
    model = getattr(M, cls)(*cfgs).to("cuda")
    torch.manual_seed(0)                             # the same initialisation: the two routes are compared below
    old = getattr(M, cls)(*cfgs).to("cuda")
    model.train()
    old.train()
    eng = model.engine
    old.engine._objective_mfn_refused = True         # the fallback: the path before the entry
    for N, T in SHAPES:
        X, y = batch(N, T, 9)
        if variant == "mmd":
            c = eng.cfg
            g = torch.randn(N, c["zl_size"] + c["za_size"] + c["zv_size"] + c["zy_size"], device="cuda")
            model.mmd_gauss = old.mmd_gauss = list(torch.split(g, [c["zl_size"], c["za_size"], c["zv_size"], c["zy_size"]], dim=1))

        def old_route():
            return old.objective(X, y)

        def new_eager():
            return model.objective(X, y)

        peak_new = peak_of(new_eager)
        peak_old = peak_of(old_route)
        assert eng.__dict__.get("_objective_mfn_bufs") and not eng._plans and not old.engine.__dict__.get("_objective_mfn_bufs")
        ref = [float(t) for t in old_route()]
        got = [float(t) for t in new_eager()]
        for gv, rv in zip(got, ref):
            assert abs(gv - rv) <= 1e-4 * max(abs(rv), 1e-3), (got, ref)
        graph = captured(new_eager)
        RUN = {"old_route": old_route, "new_eager": new_eager, "new_graph": graph.replay}
        seen = {f: [] for f in FORMS}
        for r in range(args.rounds):
            for form in FORMS:
                seen[form].append(timed(RUN[form], args.calls, args.warmup))
        say("%s N=%d T=%d   (loss disc gen_l gen_a gen_v reg: new %s, old %s)" % (cls, N, T, " ".join("%.6f" % v for v in got), " ".join("%.6f" % v for v in ref)))
        med = {f: median(seen[f]) for f in FORMS}
        for f in FORMS:
            say("  %-10s median %9.4f ms/call   (spread of the rounds %.4f; rounds %s)"
                % (f, med[f][0], med[f][1], " ".join("%.4f" % t for t in seen[f])))
        say("  peak device memory of a first call: objective %d bytes (workspace %d, row cap %d), the eval forward on a plan %d bytes"
            % (peak_new, 4 * eng.objective_workspace_floats(T, N), eng.PREDICT_MAX_ROWS, peak_old))
        for f in ("new_eager", "new_graph"):
            apart = med["old_route"][0] - med[f][0] > max(med["old_route"][1], med[f][1])
            slower = med[f][0] - med["old_route"][0] > max(med["old_route"][1], med[f][1])
            verdicts.append("%s N=%d T=%d  %s / old_route = %.3f   (%.4f vs %.4f ms; spreads %.4f, %.4f): %s"
                            % (cls, N, T, f, med[f][0] / med["old_route"][0], med[f][0], med["old_route"][0], med[f][1], med["old_route"][1],
                               "faster" if apart else ("slower" if slower else "not apart")))
        del graph
        old.engine._plans.clear()
        eng.__dict__.get("_objective_mfn_bufs", {}).clear()
        torch.cuda.empty_cache()
    del model, old

for v in verdicts:
    say(v)
write_out(args.out, "scripts/bench_objective_mfn.py --calls %d --warmup %d --rounds %d: MFM_KL and MFM, fp32" % (args.calls, args.warmup, args.rounds))
