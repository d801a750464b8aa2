"""What `evaluate` and `predict` of a split cost for the ablations M_A, M_B, M_C and M_D (the per-epoch validation loss and the
final prediction of the reference's train_mfm_ablation) on the plan-free entry (M_B, M_D: mfm_predict_ablation; M_A, M_C:
mfm_predict_ablation_mfn) and the way the package offered before (fp32), per call:

    ref_eval     the class's eval forward() under no_grad, then F.l1_loss on y_hat
    new_eval     model.evaluate(X, y)
    graph_eval   the same call replayed as one captured graph
    ref_pred     the eval forward(), then F.l1_loss and (the classes with decoders) the three F.mse_loss
    new_pred     model.predict(X, y)
    graph_pred   the same call replayed as one captured graph

at T = 20 and N = 32 (the training batch), 229 (the MOSI validation split) and 1024, with the peak device memory of either way
(beyond the parameters and the split, which both need).  It sets no threshold; it records.

    python scripts/bench_ablation.py --classes M_B,M_D --out profiles/ablation_times.txt
    python scripts/bench_ablation.py --classes M_A,M_C --out profiles/ablation_mfn_times.txt

Every time is a host clock around `--calls` calls that end in a device synchronise, after `--warmup` calls of the same form; the
forms alternate within a round and the median over the rounds is reported with the spread (max - min of the rounds).
"""
import argparse

import torch
import torch.nn.functional as F

from _bench_common import batch, captured, cfgs, d_a, d_l, median, need_gpu, peak_of, say, timed, write_out
from factorized_amd import mfm_model as M  # noqa: E402

FORMS = ["ref_eval", "new_eval", "graph_eval", "ref_pred", "new_pred", "graph_pred"]
BASE = {"new_eval": "ref_eval", "graph_eval": "ref_eval", "new_pred": "ref_pred", "graph_pred": "ref_pred"}
HAS_GEN = {"M_A": True, "M_B": True, "M_C": True, "M_D": False}
SHAPES = [(32, 20), (229, 20), (1024, 20)]

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=30)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--classes", default="M_A,M_B,M_C,M_D", help="comma-separated classes to time")
ap.add_argument("--out", help="write the record to this file")
args = ap.parse_args()
CLASSES = args.classes.split(",")
assert CLASSES and all(c in HAS_GEN for c in CLASSES), "--classes takes names out of %s" % sorted(HAS_GEN)

need_gpu("bench_ablation.py")
med_all = {}
for name in CLASSES:
    model = getattr(M, name)(*cfgs).to("cuda")
    model.eval()
    for N, T in SHAPES:
        X, y = batch(N, T, 9)
        y = y.reshape(N, 1).contiguous()
        real = (X[:, :, :d_l], X[:, :, d_l:d_l + d_a], X[:, :, d_l + d_a:])

        def ref_eval():
            with torch.no_grad():
                return F.l1_loss(model.forward(X)[0][3], y)

        def ref_pred():
            with torch.no_grad():
                out = model.forward(X)[0]
                gen = torch.stack([F.mse_loss(out[i], real[i]) for i in range(3)]) if HAS_GEN[name] else None
                return out[3], gen, F.l1_loss(out[3], y)

        def new_eval():
            return model.evaluate(X, y)

        def new_pred():
            return model.predict(X, y)

        peak = {f.__name__: peak_of(f) for f in (new_eval, new_pred, ref_eval, ref_pred)}
        ref, got = ref_pred(), new_pred()
        for g, r in zip(got, ref):
            assert (g is None) == (r is None)
            if g is not None:
                assert float((g - r).abs().max()) <= 1e-4 * max(float(r.abs().max()), 1e-3), (name, N, g, r)
        assert float((new_eval() - ref_eval()).abs()) <= 1e-4 * float(ref_eval().abs())
        graphs = {"graph_eval": captured(new_eval), "graph_pred": captured(new_pred)}
        RUN = {"ref_eval": ref_eval, "new_eval": new_eval, "graph_eval": graphs["graph_eval"].replay,
               "ref_pred": ref_pred, "new_pred": new_pred, "graph_pred": graphs["graph_pred"].replay}
        seen = {f: [] for f in FORMS}
        for r in range(args.rounds):
            for form in FORMS:
                seen[form].append(timed(RUN[form], args.calls, args.warmup))
        say("%s N=%d T=%d   (gen %s disc %.6f both ways)" % (name, N, T, "-" if got.gen is None else " ".join("%.6f" % v for v in got.gen.cpu()),
                                                           float(got.disc)))
        for f in FORMS:
            med_all[(name, N, f)] = median(seen[f])
            say("  %-11s median %9.4f ms/call   (spread of the rounds %.4f; rounds %s)"
                % (f, med_all[(name, N, f)][0], med_all[(name, N, f)][1], " ".join("%.4f" % t for t in seen[f])))
        say("  peak device memory of a first call (row cap %d): evaluate %d bytes, the eval forward and l1_loss %d bytes; predict %d bytes, "
            "the eval forward and its reductions %d bytes" % (model.ABLATION_MAX_ROWS, peak["new_eval"], peak["ref_eval"], peak["new_pred"],
                                                              peak["ref_pred"]))
        del graphs
        model.__dict__.get("_ablation_bufs", {}).clear()
        torch.cuda.empty_cache()
    del model

for name in CLASSES:
    for N, T in SHAPES:
        for f in ("new_eval", "graph_eval", "new_pred", "graph_pred"):
            m, base = med_all[(name, N, f)], med_all[(name, N, BASE[f])]
            say("%s N=%d T=%d  %s / %s = %.3f   (%.4f vs %.4f ms; spreads %.4f, %.4f)"
                % (name, N, T, f, BASE[f], m[0] / base[0], m[0], base[0], m[1], base[1]))
write_out(args.out, "scripts/bench_ablation.py --calls %d --warmup %d --rounds %d: %s, fp32" % (args.calls, args.warmup, args.rounds, ", ".join(CLASSES)))
