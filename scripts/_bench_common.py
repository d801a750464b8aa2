"""What the feature bench scripts share (bench_dropin, bench_keepbest, bench_plateau, bench_predict, bench_swa, bench_clip,
bench_shuffle, and bench_zeros, bench_objective and their *_mfn kin): the MOSI set-up, the reference's unchanged training loop, the
host-clock timers, what the inference benches measure with (peak_of, median, captured) and the recorder of what a script prints.  Importing it puts the repository on sys.path."""
import os
import sys
import time

import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from factorized_amd import configs, synth  # noqa: E402

# the MOSI configuration: canonical configs with dropout, B=32, T=20
cfgs = configs.canonical_configs(dropout=True)
config = cfgs[0]
B, T = 32, 20
d_l, d_a, d_v = config["input_dims"]
X = y = None                    # the seed-7 batch on the device, once `mosi_batch` has run


def need_gpu(script):
    if not torch.cuda.is_available():
        sys.exit("%s needs the GPU: a time taken anywhere else says nothing" % script)


def batch(N, T, seed):
    xn, yn = synth.make_batch(config["input_dims"], N, T, seed=seed)
    return torch.from_numpy(xn).cuda(), torch.from_numpy(yn).cuda()


def mosi_batch():
    """the batch `loop` trains on: B=32, T=20, seed 7, on the device"""
    global X, y
    X, y = batch(B, T, 7)
    return X, y


def loop(model, optimizer, steps, item=True, after_backward=None, after_step=None):
    """the reference's unchanged training loop (mfm_mosi.py:427-441) on the one batch; item: its per-step .item();
    after_backward(model) / after_step(model): what a script puts between backward() and step(), or behind step()"""
    criterion, gen_criterion = nn.L1Loss(), nn.MSELoss()
    epoch_loss = 0.0
    for _ in range(steps):
        optimizer.zero_grad()
        batch_X, batch_y = X, y
        decoded, mmd_loss, missing_loss = model.forward(batch_X)
        [x_l_hat, x_a_hat, x_v_hat, y_hat] = decoded
        gen_loss = config["lda_xl"] * gen_criterion(x_l_hat, batch_X[:, :, :d_l]) + config["lda_xa"] * gen_criterion(x_a_hat, batch_X[:, :, d_l:d_l + d_a]) \
            + config["lda_xv"] * gen_criterion(x_v_hat, batch_X[:, :, d_l + d_a:])
        disc_loss = criterion(y_hat.squeeze(1), batch_y)
        loss = disc_loss + gen_loss + config["lda_mmd"] * mmd_loss + missing_loss
        loss.backward()
        if after_backward is not None:
            after_backward(model)
        optimizer.step()
        if after_step is not None:
            after_step(model)
        if item:
            epoch_loss += disc_loss.item()


def timed_steps(run, steps, warmup):
    """ms per step of `run(k)`, which takes k steps: a host clock around run(steps) that ends in a device synchronise, after
    run(warmup)"""
    run(warmup)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    run(steps)
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / steps


def timed(fn, n, warmup):
    """ms per call of `fn`: a host clock around n calls that end in a device synchronise, after min(warmup, n) calls"""
    def run(k):
        for _ in range(k):
            fn()
    return timed_steps(run, n, min(warmup, n))


def peak_of(fn):
    """peak device memory of a first call of `fn` (its buffers included) beyond what is allocated now, in bytes"""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    keep = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del keep
    return peak


def median(v):
    """(the median of the rounds, their spread max - min)"""
    v = sorted(v)
    return v[len(v) // 2], v[-1] - v[0]


def captured(fn):
    """one call of `fn` captured as a graph on the current device"""
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fn()
    return graph


# ---------------------------------------------------------------------- the record of a run
lines = []


def say(text=""):
    print(text, flush=True)
    lines.append(text)


def report(seen, text):
    """say `text(form, median, spread)` for the rounds of every form in `seen`; returns the medians"""
    med = {f: sorted(v)[len(v) // 2] for f, v in seen.items()}
    for f, v in seen.items():
        say(text(f, med[f], max(v) - min(v)))
    return med


def write_out(path, header=None):
    """the `--out` file: the header line, then everything said"""
    if path:
        with open(path, "w") as f:
            f.write((header + "\n" if header else "") + "\n".join(lines) + "\n")
