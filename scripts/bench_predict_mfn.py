"""What model.evaluate of the MFN classes (MFM_KL, MFM, fp32) costs per call on the label path alone
(label_only=True: mfm_predict_mfn) and on the default path, both in one session on one card:

    default_eager   model.evaluate(X, y): the eval forward on a training plan of the split's shape, want_xhat=False -- what
                    evaluate of these classes does without the keyword, bit for bit what it did before the keyword existed
    default_graph   the same call replayed as one captured graph
    label_eager     model.evaluate(X, y, label_only=True)
    label_graph     the same call replayed as one captured graph

at T = 20 and N = 32 (one MOSI batch), 229 (the MOSI validation split) and 1024, with the peak device memory of a first call
either way (beyond the parameters and the split, which both need).  It sets no threshold; it records.

    python scripts/bench_predict_mfn.py --out profiles/predict_mfn_times.txt

Every time is a host clock around `--calls` calls that end in a device synchronise, after `--warmup` calls of the same form; the
forms alternate within a round and the median over the rounds (at least five) is reported with the spread (max - min of the
rounds).  Two medians count as apart when they differ by more than the larger of the two spreads.
"""
import argparse

import torch

from _bench_common import batch, captured, cfgs, median, need_gpu, peak_of, say, timed, write_out
from factorized_amd import mfm_model as M  # noqa: E402

FORMS = ["default_eager", "default_graph", "label_eager", "label_graph"]
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

need_gpu("bench_predict_mfn.py")


verdicts = []
for cls, variant in CLS:
    torch.manual_seed(0)
    model = getattr(M, cls)(*cfgs).to("cuda")
    torch.manual_seed(0)                             # the same initialisation: the two paths are compared below
    dflt = getattr(M, cls)(*cfgs).to("cuda")         # (a model of its own, so that each path's first-call memory is its own)
    model.train()
    dflt.train()
    eng = model.engine
    for N, T in SHAPES:
        X, y = batch(N, T, 9)

        def default_eager():
            return dflt.evaluate(X, y)

        def label_eager():
            return model.evaluate(X, y, label_only=True)

        peak_new = peak_of(label_eager)
        peak_old = peak_of(default_eager)
        assert eng.__dict__.get("_predict_mfn_bufs") and not eng._plans and dflt.engine._plans
        assert not dflt.engine.__dict__.get("_predict_mfn_bufs")
        ref, got = float(default_eager()), float(label_eager())
        assert abs(got - ref) <= 1e-4 * max(abs(ref), 1e-3), (got, ref)
        g_old, g_new = captured(default_eager), captured(label_eager)
        RUN = {"default_eager": default_eager, "default_graph": g_old.replay, "label_eager": label_eager, "label_graph": g_new.replay}
        seen = {f: [] for f in FORMS}
        for r in range(args.rounds):
            for form in FORMS:
                seen[form].append(timed(RUN[form], args.calls, args.warmup))
        say("%s N=%d T=%d   (loss %.6f label-only, %.6f default)" % (cls, N, T, got, ref))
        med = {f: median(seen[f]) for f in FORMS}
        for f in FORMS:
            say("  %-13s median %9.4f ms/call   (spread of the rounds %.4f; rounds %s)"
                % (f, med[f][0], med[f][1], " ".join("%.4f" % t for t in seen[f])))
        say("  peak device memory of a first call: label_only %d bytes (workspace %d, row cap %d), the eval forward on a plan %d bytes"
            % (peak_new, 4 * eng.predict_workspace_floats(T, N, label_only=True), eng.PREDICT_MAX_ROWS, peak_old))
        for new, old in (("label_eager", "default_eager"), ("label_graph", "default_graph")):
            d = med[old][0] - med[new][0]
            lim = max(med[old][1], med[new][1])
            verdicts.append("%s N=%d T=%d  %s / %s = %.3f   (%.4f vs %.4f ms; spreads %.4f, %.4f): %s"
                            % (cls, N, T, new, old, med[new][0] / med[old][0], med[new][0], med[old][0], med[new][1], med[old][1],
                               "faster" if d > lim else ("slower" if -d > lim else "not apart")))
        del g_old, g_new
        dflt.engine._plans.clear()
        eng.__dict__.get("_predict_mfn_bufs", {}).clear()
        torch.cuda.empty_cache()
    del model, dflt

for v in verdicts:
    say(v)
write_out(args.out, "scripts/bench_predict_mfn.py --calls %d --warmup %d --rounds %d: MFM_KL and MFM, fp32" % (args.calls, args.warmup, args.rounds))
