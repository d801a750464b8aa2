"""What surrogate inference costs (MFM_missing, fp32, canonical sizes), per call, beside the only way to obtain the
missing-modality decodings the package offered before -- the class's eval forward under no_grad:

    impute_l    model.impute(X, "l")                          (two surrogate encoders, one decoder: 5 launches)
    impute_each model.impute(X, "each")                       (six surrogate encoders, three decoders: the same 5 launches)
    forward     model.eval(); model.forward(X)                (nine encoders, the MFN, four z -> f stacks, twelve decoders)

each eager and replayed as a captured graph, at the reference's B=32, T=20 and at the MOSI validation shape (N=229, T=20).

    python scripts/bench_impute.py --commit <what is measured> --out profiles/impute_times.txt

Every time is a host clock around `--calls` calls that end in a device synchronise, after `--warmup` calls of the same form; the
forms alternate within a round and the median over the rounds is reported with the spread (max - min of the rounds).  The one
expectation -- `impute_each` is not slower than `forward`, which is unchanged code and does a strict superset of the work -- is
no threshold of the script: it prints which way the measurement came out.
"""
import argparse
import subprocess

import torch

from _bench_common import batch, cfgs, need_gpu, say, timed, write_out
from factorized_amd.mfm_model import MFM_missing  # noqa: E402

FORMS = ["impute_l", "impute_each", "forward"]
SHAPES = [(32, 20), (229, 20)]

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=30)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--commit", help="the commit measured, for the header line (default: git rev-parse HEAD; name it where there is no git checkout)")
ap.add_argument("--out", help="write the record to this file")
args = ap.parse_args()

need_gpu("bench_impute.py")
commit = args.commit
if not commit:
    try:
        commit = subprocess.check_output(["git", "rev-parse", "--short", "HEAD"], text=True, stderr=subprocess.DEVNULL).strip()
    except (OSError, subprocess.CalledProcessError):
        commit = "unknown (no git checkout here)"
model = MFM_missing(*cfgs).to("cuda")
model.eval()
c = cfgs[0]

for N, T in SHAPES:
    X, _ = batch(N, T, 9)
    # (fixed N(0,1) samples: the forward's loss_MMD would otherwise draw them with the host's generator on every call)
    model.mmd_gauss = [torch.randn(N, c[k], device="cuda") for k in ("zl_size", "za_size", "zv_size", "zy_size")]

    def impute_l():
        model.impute(X, "l")

    def impute_each():
        model.impute(X, "each")

    def forward():
        with torch.no_grad():
            model.forward(X)

    # the two paths compute the same thing
    with torch.no_grad():
        ref = model.forward(X)
    each = model.impute(X, "each")
    for i, m in enumerate("lav"):
        for got, want in ((each[m].x_hat, ref[1 + i][i]), (each[m].y_hat, ref[1 + i][3])):
            err = float((got - want).abs().max() / want.abs().max())
            assert err < 1e-4, (m, err)
    RUN = {"impute_l": impute_l, "impute_each": impute_each, "forward": forward}
    graphs = {}
    forms = list(FORMS)
    for f in FORMS:
        RUN[f]()                                             # (buffers and code objects before the capture)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        try:
            with torch.cuda.graph(g):
                RUN[f]()
        except RuntimeError as e:
            say("N=%d T=%d: %s cannot be captured (%s)" % (N, T, f, str(e).splitlines()[0][:120]))
            torch.cuda.synchronize()
            continue
        graphs[f] = g
        RUN[f + "_graph"] = g.replay
        forms.append(f + "_graph")
    seen = {f: [] for f in forms}
    for r in range(args.rounds):
        for f in forms:
            seen[f].append(timed(RUN[f], args.calls, args.warmup))
    say("N=%d T=%d" % (N, T))
    med = {}
    for f in forms:
        v = sorted(seen[f])
        med[f] = (v[len(v) // 2], v[-1] - v[0])
        say("  %-18s median %9.4f ms/call   (spread of the rounds %.4f; rounds %s)"
            % (f, med[f][0], med[f][1], " ".join("%.4f" % t for t in seen[f])))
    for a, b in (("impute_each", "forward"), ("impute_each_graph", "forward_graph"), ("impute_l", "forward")):
        if a not in med or b not in med:
            continue
        ratio = med[a][0] / med[b][0]
        say("  %s / %s = %.3f   (%.4f vs %.4f ms; spreads %.4f, %.4f): %s" % (
            a, b, ratio, med[a][0], med[b][0], med[a][1], med[b][1],
            "not slower than the eval forward" if med[a][0] <= med[b][0] + max(med[a][1], med[b][1]) else "SLOWER than the eval forward"))
    sz = model._impute_bufs
    say("  workspace and outputs kept by impute: %d bytes" % sum(
        4 * (st[0].numel() + sum(t.numel() for o in st[1].values() for t in o)) for st in sz.values()))
    del graphs
    for f in forms:
        RUN.pop(f, None)
    model._impute_bufs.clear()
    torch.cuda.empty_cache()

write_out(args.out, "commit %s; scripts/bench_impute.py --calls %d --warmup %d --rounds %d: MFM_missing, fp32, canonical sizes"
          % (commit, args.calls, args.warmup, args.rounds))
