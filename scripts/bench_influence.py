"""What the gradient-based interpretation costs (MFM_KL_EF, fp32, canonical sizes), per call:

    influence       model.influence(X)                        (encode's two launches, the weight packing, one launch per row chunk)
    factors         model.influence_factors(zl, za, zv, zy, T)   (without the encoder half)
    torch           the same recursion with torch device operations (model._influence_torch: what a refusal falls back to)

influence and factors each eager and replayed as a captured graph, at T = 20 and N = 32 / 229 / 1024, with the peak device
memory of the fused entry and of the torch recursion above what was allocated before the call.

    python scripts/bench_influence.py --out profiles/influence_times.txt

Every time is a host clock around `--calls` calls that end in a device synchronise, after `--warmup` calls of the same form; the
forms alternate within a round and the median over the rounds is reported with the spread (max - min of the rounds).  Nothing is
a threshold: the script reports the figures, the FLOP rate of the two MFMA products they amount to, and which way the
comparison came out.
"""
import argparse

import torch

from _bench_common import batch, cfgs, need_gpu, say, timed, write_out
from factorized_amd.mfm_model import MFM_KL_EF  # noqa: E402

FORMS = ["influence", "factors"]
SHAPES = [(32, 20), (229, 20), (1024, 20)]

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=10)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--out", help="write the record to this file")
args = ap.parse_args()

need_gpu("bench_influence.py")
model = MFM_KL_EF(*cfgs).to("cuda")
model.eval()
eng = model.engine
c = cfgs[0]


def product_flops(N, T):
    """FLOP of J^a = W_s J^h (steps 1 on) and J^x = W_fc1 J^h (every step) at the true sizes, the three decoders"""
    total = 0
    for fm, d in zip((c["fl_size"], c["fa_size"], c["fv_size"]), c["input_dims"]):
        h = c["fy_size"] + fm
        total += N * ((T - 1) * 2 * 4 * h * h * h + T * 2 * d * h * h)
    return total


def peak_above(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - before


for N, T in SHAPES:
    X, _ = batch(N, T, 9)
    z = [t.clone() for t in model.encode(X)[:4]]

    def influence():
        model.influence(X)

    def factors():
        model.influence_factors(z[0], z[1], z[2], z[3], T)

    def torch_form():
        with torch.no_grad():
            model._influence_torch(z[0], z[1], z[2], z[3], T)

    # the two paths compute the same thing, element by element
    eng.__dict__.get("_influence_bufs", {}).clear()
    torch.cuda.empty_cache()
    peak_fused = peak_above(factors)
    got = model.influence_factors(*z, T)
    got = torch.stack([got.fy, got.fm]).clone()
    peak_torch = peak_above(torch_form)
    with torch.no_grad():
        ref = model._influence_torch(*z, T)
    ref = torch.stack([ref.fy, ref.fm])
    err = float(((got - ref).abs() / ref.abs()).max())
    assert err < 1e-4, err
    RUN = {"influence": influence, "factors": factors, "torch": torch_form}
    graphs = {}
    for f in FORMS:
        RUN[f]()                                             # (buffers and code objects before the capture)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            RUN[f]()
        graphs[f] = g
        RUN[f + "_graph"] = g.replay
    forms = FORMS + [f + "_graph" for f in FORMS] + ["torch"]
    seen = {f: [] for f in forms}
    for r in range(args.rounds):
        for f in forms:
            seen[f].append(timed(RUN[f], args.calls, args.warmup))
    say("N=%d T=%d   (fused against the torch recursion, worst element: %.2e relative)" % (N, T, err))
    med = {}
    for f in forms:
        v = sorted(seen[f])
        med[f] = (v[len(v) // 2], v[-1] - v[0])
        say("  %-16s median %9.4f ms/call   (spread of the rounds %.4f; rounds %s)"
            % (f, med[f][0], med[f][1], " ".join("%.4f" % t for t in seen[f])))
    fl = product_flops(N, T)
    say("  the two products: %.2f GFLOP -> %.1f TFLOP/s in factors_graph (fp32 MFMA peak 157)" % (fl / 1e9, fl / med["factors_graph"][0] / 1e9))
    say("  factors / torch = %.3f   (%.4f vs %.4f ms): the fused entry is %s" % (
        med["factors"][0] / med["torch"][0], med["factors"][0], med["torch"][0],
        "faster" if med["factors"][0] < med["torch"][0] else "SLOWER than the torch recursion"))
    say("  peak device memory above the inputs: fused %d bytes (workspace %d, result %d), torch %d bytes" % (
        peak_fused, 4 * eng.influence_factors_workspace_floats(T, N), 4 * 2 * 3 * T * N, peak_torch))
    del graphs
    for f in forms:
        RUN.pop(f, None)
    eng.__dict__.get("_encode_bufs", {}).clear()
    eng.__dict__.get("_influence_bufs", {}).clear()
    torch.cuda.empty_cache()

write_out(args.out, "scripts/bench_influence.py --calls %d --warmup %d --rounds %d: MFM_KL_EF, fp32" % (args.calls, args.warmup, args.rounds))
