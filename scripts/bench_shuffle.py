"""ms per new sample order of a device-resident split (train.DeviceDataset), in three forms:

    host        what there was before `reshuffle`: numpy.random.permutation, X[:, p] / y[p] on the host, DeviceDataset.from_arrays
                (a new [nb, T, B, D] layout built by numpy and copied host-to-device)
    seed        data.reshuffle(seed=epoch): the permutation from numpy, N indices uploaded, one mfm_dataset_gather launch
    generator   data.reshuffle(generator=g): torch.randperm on the device, one launch

at the MOSI shape (N 1284, T 20, B 32, D 325: 33 MB) and a MOSEI-sized one (N 16265, T 20, B 32, D 409: 532 MB, past the
256 MiB Infinity Cache), fp32, float labels.  Beside them the gather launch ALONE (a fixed device permutation, device events
around `--launches` launches) as bytes moved / time, and a torch device-to-device copy of the same bytes in the same run.

    python scripts/bench_shuffle.py                                        # both shapes, the forms alternating, --rounds times each
    python scripts/bench_shuffle.py --shape mosi --only seed               # one form alone, e.g. under rocprofv3 --kernel-trace --stats
    python scripts/bench_shuffle.py --out profiles/shuffle_times.txt       # ... and the record

A form's time is a host clock around `reps` new orders that end in a device synchronise, after warm-up calls of the same form.
"""
import argparse
import ctypes as C
import itertools
import sys

import numpy as np
import torch

from _bench_common import say, timed, write_out
from factorized_amd import _lib, train  # noqa: E402

SHAPES = {"mosi": (1284, 20, 32, 325), "mosei": (16265, 20, 32, 409)}
FORMS = ("host", "seed", "generator")
# scripts/micro/hbm_read_probe.hip on this part (profiles/r05_dw_stream_study.txt, section 1)
PROBE = "global_load_dwordx4 into registers, 2+ workgroups per CU, 1 GB / 200 MB buffers: 6.9 - 7.2 TB/s READ"

ap = argparse.ArgumentParser()
ap.add_argument("--shape", choices=list(SHAPES))
ap.add_argument("--only", choices=FORMS)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--launches", type=int, default=200, help="gather launches inside one event bracket")
ap.add_argument("--out", help="write the record to this file")
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_shuffle.py measures on the GPU: no ROCm device here")


def events(fn, reps, warmup):
    """ms per call of `fn` by device events around `reps` calls"""
    for _ in range(warmup):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def bench(name):
    N, T, B, D = SHAPES[name]
    rng = np.random.default_rng(0)
    X, y = rng.standard_normal((T, N, D), dtype=np.float32), rng.standard_normal(N, dtype=np.float32)
    data = train.DeviceDataset.from_arrays(X, y, B, "cuda", pool=True)
    nb = data.nb
    moved = 2 * (nb * T * B * D * 4 + nb * B * 4) + nb * B * 8          # rows and labels read and written, indices read
    say("%s: N %d, T %d, B %d, D %d -> %d batches, %d samples left out per epoch; X %.1f MB; a gather moves %.1f MB"
        % (name, N, T, B, D, nb, N - nb * B, nb * T * B * D * 4 / 1e6, moved / 1e6))
    gen = torch.Generator(device="cuda").manual_seed(1)
    keep = []

    def host(i):
        p = np.random.RandomState(i).permutation(N)
        keep[:] = [train.DeviceDataset.from_arrays(X[:, p], y[p], B, "cuda")]

    forms = {"host": host, "seed": lambda i: data.reshuffle(seed=i), "generator": lambda i: data.reshuffle(generator=gen)}
    # enough work per window: the host form takes tens of ms (MOSI) to about a second (MOSEI) per order, the device forms well
    # under a millisecond
    reps = {"host": 20 if name == "mosi" else 3, "seed": 300, "generator": 300}
    warm = {"host": 3 if name == "mosi" else 1, "seed": 30, "generator": 30}
    which = [args.only] if args.only else list(FORMS)
    seen = {f: [] for f in which}
    for r in range(args.rounds):
        for f in which:
            ms = timed(lambda i=itertools.count(): forms[f](next(i)), reps[f], warm[f])      # (order i of this window)
            seen[f].append(ms)
            say("  %-10s round %d  %10.4f ms per order   (%d orders)" % (f, r, ms, reps[f]))
    med = {f: sorted(v)[len(v) // 2] for f, v in seen.items()}
    for f in which:
        say("  %-10s median   %10.4f ms per order   (spread of the rounds %.4f)" % (f, med[f], max(seen[f]) - min(seen[f])))
    if "host" in med:
        for f in which:
            if f != "host":
                say("  %-10s is %.0f x faster than the host form" % (f, med["host"] / med[f]))
    del keep[:]

    # the launch alone
    perm = torch.randperm(N, generator=gen, device="cuda")
    L = _lib.lib()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = [C.c_void_p(t.data_ptr()) for t in (data.X, data.y, data.X_pool, data.y_pool, perm)]

    def gather():
        _lib.check(L.mfm_dataset_gather(*ptr, N, nb, T, B, D, 4, stream), "mfm_dataset_gather")

    twin = torch.empty_like(data.X)
    k_ms = sorted(events(gather, args.launches, 20) for _ in range(args.rounds))
    c_ms = sorted(events(lambda: twin.copy_(data.X), args.launches, 20) for _ in range(args.rounds))
    g_ms, t_ms = k_ms[len(k_ms) // 2], c_ms[len(c_ms) // 2]
    say("  gather launch alone      %9.2f us  %7.0f GB/s moved (read + written)   [rounds: %s us]"
        % (1e3 * g_ms, moved / g_ms / 1e6, ", ".join("%.2f" % (1e3 * v) for v in k_ms)))
    say("  torch copy, same bytes   %9.2f us  %7.0f GB/s moved (read + written)   [rounds: %s us]"
        % (1e3 * t_ms, 2 * twin.numel() * 4 / t_ms / 1e6, ", ".join("%.2f" % (1e3 * v) for v in c_ms)))
    say()
    return g_ms, t_ms


say("scripts/bench_shuffle.py --rounds %d --launches %d: a new sample order for train.DeviceDataset, fp32, %s"
    % (args.rounds, args.launches, torch.cuda.get_device_name(0)))
say("plain read on this part, recorded by scripts/micro/hbm_read_probe.hip: %s" % PROBE)
say()
for name in ([args.shape] if args.shape else list(SHAPES)):
    bench(name)
write_out(args.out)
