"""What the missing-modality test protocol of a split costs (the `predict` / `score` blocks of the reference's train_mfm_missing,
seq2seq and basic_missing loops: per missing case the error of the rebuilt modality, the label prediction and its label loss)
on the plan-free entry and the way the package offered before, for MFM_missing, seq2seq and basic_missing (fp32), per call:

    ref_route    the class's eval forward() under no_grad, then F.mse_loss / F.l1_loss on what the protocol reports
    new_eager    model.predict_missing(X, y, missing="each")
    new_graph    the same call replayed as one captured graph

at T = 20 and N = 32 (the training batch), 229 (the MOSI validation split) and 1024, with the peak device memory of either way
(beyond the parameters and the split, which both need).  It sets no threshold; it records.

    python scripts/bench_missing.py --out profiles/missing_times.txt

Every time is a host clock around `--calls` calls that end in a device synchronise, after `--warmup` calls of the same form; the
forms alternate within a round and the median over the rounds is reported with the spread (max - min of the rounds).
"""
import argparse

import torch
import torch.nn.functional as F

from _bench_common import batch, captured, cfgs, d_a, d_l, median, need_gpu, peak_of, say, timed, write_out
from factorized_amd import mfm_model as M  # noqa: E402

FORMS = ["ref_route", "new_eager", "new_graph"]
CLASSES = ["MFM_missing", "seq2seq", "basic_missing"]
SHAPES = [(32, 20), (229, 20), (1024, 20)]

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=30)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--out", help="write the record to this file")
args = ap.parse_args()

need_gpu("bench_missing.py")
med_all = {}
for name in CLASSES:
    model = getattr(M, name)(*cfgs).to("cuda")
    model.eval()
    for N, T in SHAPES:
        X, y = batch(N, T, 9)
        y = y.reshape(N, 1).contiguous()
        real = (X[:, :, :d_l], X[:, :, d_l:d_l + d_a], X[:, :, d_l + d_a:])

        def ref_route():
            with torch.no_grad():
                out = model.forward(X)
                if name == "MFM_missing":
                    cases = out[1:4]
                    return (torch.stack([c[3] for c in cases]), torch.stack([F.mse_loss(c[i], real[i]) for i, c in enumerate(cases)]),
                            torch.stack([F.l1_loss(c[3], y) for c in cases]))
                if name == "seq2seq":
                    return None, torch.stack([F.mse_loss(out[i][0], real[i]) for i in range(3)]), None
                return torch.stack(list(out[:3])), None, torch.stack([F.l1_loss(v, y) for v in out[:3]])

        def new_eager():
            if name == "seq2seq":
                return model.predict_missing(X, missing="each")
            return model.predict_missing(X, y, missing="each")

        peak_new = peak_of(new_eager)
        peak_ref = peak_of(ref_route)
        ref, got = ref_route(), new_eager()
        for g, r in zip(got, ref):
            assert (g is None) == (r is None)
            if g is not None:
                assert float((g - r).abs().max()) <= 1e-4 * max(float(r.abs().max()), 1e-3), (name, N, g, r)
        graph = captured(new_eager)
        RUN = {"ref_route": ref_route, "new_eager": new_eager, "new_graph": graph.replay}
        seen = {f: [] for f in FORMS}
        for r in range(args.rounds):
            for form in FORMS:
                seen[form].append(timed(RUN[form], args.calls, args.warmup))
        say("%s N=%d T=%d   (gen %s disc %s both ways)" % (name, N, T, "-" if got.gen is None else " ".join("%.6f" % v for v in got.gen.cpu()),
                                                         "-" if got.disc is None else " ".join("%.6f" % v for v in got.disc.cpu())))
        for f in FORMS:
            med_all[(name, N, f)] = median(seen[f])
            say("  %-11s median %9.4f ms/call   (spread of the rounds %.4f; rounds %s)"
                % (f, med_all[(name, N, f)][0], med_all[(name, N, f)][1], " ".join("%.4f" % t for t in seen[f])))
        say("  peak device memory of a first call: predict_missing %d bytes (row cap %d), the eval forward and its reductions %d bytes"
            % (peak_new, model.MISSING_MAX_ROWS, peak_ref))
        del graph
        model.__dict__.get("_missing_bufs", {}).clear()
        torch.cuda.empty_cache()
    del model

for name in CLASSES:
    for N, T in SHAPES:
        base = med_all[(name, N, "ref_route")]
        for f in ("new_eager", "new_graph"):
            m = med_all[(name, N, f)]
            say("%s N=%d T=%d  %s / ref_route = %.3f   (%.4f vs %.4f ms; spreads %.4f, %.4f)"
                % (name, N, T, f, m[0] / base[0], m[0], base[0], m[1], base[1]))
write_out(args.out, "scripts/bench_missing.py --calls %d --warmup %d --rounds %d: MFM_missing, seq2seq, basic_missing, fp32"
          % (args.calls, args.warmup, args.rounds))
