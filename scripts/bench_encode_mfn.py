#!/usr/bin/env python
"""model.encode of the MFN classes (MFM_KL, MFM) through the fused entry (mfm_encode_mfn) against the composition of the
granular operations (model._encode_composed: what encode ran before the entry existed) and against the eval forward on a
training plan, at T = 20 and N = 32 / 229 / 1024, eager and replayed from a captured graph, with the peak memory each takes
above the model and its input.

    python scripts/bench_encode_mfn.py [--iters 200] [--out profiles/encode_mfn_times.txt]

Every figure of one (class, N) comes from the same process and session: warm-up calls first, then `--iters` timed calls per
path with device events around each call (eager) or each replay (captured), the median and the 10th / 90th percentiles."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from factorized_amd import configs, mfm_model as M, synth      # noqa: E402

T = 20


def timed(fn, iters, warmup=20):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    ms = np.array([a.elapsed_time(b) for a, b in ev]) * 1e3
    return np.median(ms), np.percentile(ms, 10), np.percentile(ms, 90)


def peak_mb(fn):
    """peak device memory of two calls above what is allocated before them (buffers the first call keeps are counted)"""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def captured(fn):
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    return g.replay


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = ["# model.encode of the MFN classes, T = %d, fp32, median us [p10 p90] over %d calls; peak MB above model + input" % (T, args.iters),
             "# device: %s" % torch.cuda.get_device_name(0),
             "%-7s %5s  %-10s %28s %28s %9s" % ("class", "N", "path", "eager us", "captured us", "peak MB")]
    for cls in ("MFM_KL", "MFM"):
        for N in (32, 229, 1024):
            cfgs = configs.canonical_configs(dropout=False)
            peaks = {}
            # peak memory first, each path on a model of its own: nothing another path allocated is in the way
            for path in ("fused", "composed", "plan_eval"):
                model = getattr(M, cls)(*cfgs).to("cuda").eval()
                xn, _ = synth.make_batch(cfgs[0]["input_dims"], N, T, seed=3, output_dim=cfgs[0]["output_dim"])
                x = torch.from_numpy(xn).cuda()
                eng = model.engine
                fns = {"fused": lambda: model.encode(x), "composed": lambda: model._encode_composed(x),
                       "plan_eval": lambda: eng.forward(x, None, train=False, handover=False)}
                with torch.no_grad():
                    peaks[path] = peak_mb(fns[path])
                del model, eng, fns
            model = getattr(M, cls)(*cfgs).to("cuda").eval()
            eng = model.engine
            fns = {"fused": lambda: model.encode(x), "composed": lambda: model._encode_composed(x),
                   "plan_eval": lambda: eng.forward(x, None, train=False, handover=False)}
            with torch.no_grad():
                for path in ("fused", "composed", "plan_eval"):
                    e = timed(fns[path], args.iters)
                    try:
                        c = timed(captured(fns[path]), args.iters)
                        cs = "%8.1f [%7.1f %7.1f]" % c
                    except Exception as exc:          # a path that cannot be captured says so
                        torch.cuda.synchronize()
                        cs = "not capturable (%s)" % type(exc).__name__
                    lines.append("%-7s %5d  %-10s %28s %28s %9.1f" % (cls, N, path, "%8.1f [%7.1f %7.1f]" % e, cs, peaks[path]))
                    print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
