"""What the zeroed-modality test protocol of a split costs (the reference's train_mfm_test_zeros, mfm_mosi.py:572-596: y_hat with
modality l, a, v zeroed in turn, and F.mse_loss of the zeroed modality's reconstruction against the real one) on the plan-free
entry and the way the package offered before (MFM_KL_EF, fp32), per call:

    ref_route    three zeroed copies of the split with the driver's torch.cat lines, three engine.forward(train=False) on a
                 training plan of the split's shape, three F.mse_loss, the three y_hat kept
    new_eager    model.predict_zeros(X, y)
    new_graph    the same call replayed as one captured graph

at T = 20 and N = 229 (the MOSI validation split), 1024 and 4096, with the peak device memory of either way (beyond the
parameters and the split, which both need).  Then the two forms of the ef encoder's input projection for the three cases, on the
library's grouped fp32 GEMM at the shape of one row chunk (min(N, 1024) rows):

    split        ONE grouped launch of the three per-modality products P_m = x_m W_ih[:, columns of m]^T (K = 325 in all), as
                 the entry launches it; the pass that forms the three gate sets from them is timed as three torch.add -- 9 units
                 of traffic where the entry's own pass (P read once) moves 6: an upper bound of it
    k_reduced    the three cases as products of their own over the present columns, biases in the epilogue (K = 650 in all): no
                 l and no v on one column range each, no a on two -- its second range accumulates into the first's result, so
                 it is a second launch

It sets no threshold; it records.

    python scripts/bench_zeros.py --out profiles/zeros_times.txt

Every time is a host clock around `--calls` calls that end in a device synchronise, after `--warmup` calls of the same form; the
forms alternate within a round and the median over the rounds is reported with the spread (max - min of the rounds).
"""
import argparse

import torch
import torch.nn.functional as F

from _bench_common import batch, captured, cfgs, d_a, d_l, d_v, median, need_gpu, peak_of, say, timed, write_out
from factorized_amd import engine as E  # noqa: E402
from factorized_amd.mfm_model import MFM_KL_EF  # noqa: E402

FORMS = ["ref_route", "new_eager", "new_graph"]
PROJ = ["split_gemm", "split_pass_bound", "k_reduced"]
SHAPES = [(229, 20), (1024, 20), (4096, 20)]

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=30)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--out", help="write the record to this file")
args = ap.parse_args()

need_gpu("bench_zeros.py")
model = MFM_KL_EF(*cfgs).to("cuda")
model.train()
eng = model.engine
c = eng.cfg
D = d_l + d_a + d_v
he = c["zl_size"] + c["za_size"] + c["zv_size"]
Hp = (he + 15) // 16 * 16
views = eng.param_views()
W, b_ih, b_hh = views["ef_encoder.lstm.weight_ih"], views["ef_encoder.lstm.bias_ih"], views["ef_encoder.lstm.bias_hh"]


def proj_forms(X, rows, T):
    """the two forms on the first `rows` rows of X as one [T * rows, D] matrix per step range (rows == N: the whole split)"""
    Xc = X[:, :rows].contiguous()
    M = T * rows
    P = [torch.empty(M, 4, Hp, device="cuda") for _ in range(3)]
    G = [torch.empty(M, 4, Hp, device="cuda") for _ in range(3)]
    col = (0, d_l, d_l + d_a, D)

    def prob(out, c0, c1, bias, acc=0):
        return E.make_gemm(Xc.view(-1)[c0:], W.view(-1)[c0:], out, M, Hp, c1 - c0, D, 1, 1, D, 4 * Hp, bias=b_ih if bias else None,
                           bias2=b_hh if bias else None, n_valid=he, batch=4, b_sz=he * D, c_sz=Hp, bias_sz=he if bias else 0,
                           accumulate=acc)
    split = [prob(P[m], col[m], col[m + 1], False) for m in range(3)]
    first = [prob(G[0], col[1], col[3], True), prob(G[2], col[0], col[2], True), prob(G[1], col[0], col[1], True)]
    second = [prob(G[1], col[2], col[3], False, acc=1)]

    def split_gemm():
        E.gemm_grouped(split)

    def split_pass_bound():
        torch.add(P[1], P[2], out=G[0]); torch.add(P[0], P[2], out=G[1]); torch.add(P[0], P[1], out=G[2])

    def k_reduced():
        E.gemm_grouped(first)
        E.gemm_grouped(second)
    # the two forms give the same gates (the split form's biases added here)
    split_gemm(); split_pass_bound()
    bias = torch.zeros(4, Hp, device="cuda")
    bias[:, :he] = (b_ih + b_hh).view(4, he)
    a = [g + bias for g in G]
    k_reduced()
    for u, v in zip(a, G):
        assert float((u - v).abs().max()) <= 1e-4 * max(float(v.abs().max()), 1e-3)
    return {"split_gemm": split_gemm, "split_pass_bound": split_pass_bound, "k_reduced": k_reduced}


med_all = {}
for N, T in SHAPES:
    X, y = batch(N, T, 9)

    def ref_route():
        batch_X = X
        batch_X_nol = torch.cat([torch.zeros_like(batch_X[:, :, :d_l]), batch_X[:, :, d_l:]], dim=2)
        batch_X_noa = torch.cat([batch_X[:, :, :d_l], torch.zeros_like(batch_X[:, :, d_l:d_l + d_a]), batch_X[:, :, d_l + d_a:]], dim=2)
        batch_X_nov = torch.cat([batch_X[:, :, :d_l + d_a], torch.zeros_like(batch_X[:, :, d_l + d_a:])], dim=2)
        real = (batch_X[:, :, :d_l], batch_X[:, :, d_l:d_l + d_a], batch_X[:, :, d_l + d_a:])
        y_hat, gen, disc = [], [], []
        for i, (xz, key) in enumerate(((batch_X_nol, "x_l_hat"), (batch_X_noa, "x_a_hat"), (batch_X_nov, "x_v_hat"))):
            out = eng.forward(xz, y, train=False)
            y_hat.append(out["y_hat"])
            gen.append(F.mse_loss(out[key], real[i]))
            disc.append(out["losses"][0].clone())
        return torch.stack(y_hat), torch.stack(gen), torch.stack(disc)

    def new_eager():
        return model.predict_zeros(X, y)

    key = (T, N, eng.reg_scale, eng.precision, eng.variant)
    peak_new = peak_of(new_eager)
    peak_ref = peak_of(ref_route)
    ref = [t.cpu() for t in ref_route()]
    got = [t.cpu() for t in new_eager()]
    for g, r in zip(got, ref):
        assert float((g - r).abs().max()) <= 1e-4 * max(float(r.abs().max()), 1e-3), (g, r)
    graph = captured(new_eager)
    RUN = {"ref_route": ref_route, "new_eager": new_eager, "new_graph": graph.replay}
    seen = {f: [] for f in FORMS}
    for r in range(args.rounds):
        for form in FORMS:
            seen[form].append(timed(RUN[form], args.calls, args.warmup))
    say("N=%d T=%d   (gen %s disc %s both ways)" % (N, T, " ".join("%.6f" % v for v in got[1]), " ".join("%.6f" % v for v in got[2])))
    for f in FORMS:
        med_all[(N, f)] = median(seen[f])
        say("  %-11s median %9.4f ms/call   (spread of the rounds %.4f; rounds %s)"
            % (f, med_all[(N, f)][0], med_all[(N, f)][1], " ".join("%.4f" % t for t in seen[f])))
    say("  peak device memory of a first call: predict_zeros %d bytes (workspace %d, row cap %d), the three eval forwards on a plan %d bytes"
        % (peak_new, 4 * eng.predict_zeros_workspace_floats(T, N), eng.PREDICT_MAX_ROWS, peak_ref))
    del graph
    eng._plans.pop(key, None)
    eng.__dict__.get("_zeros_bufs", {}).clear()
    torch.cuda.empty_cache()

    rows = min(N, eng.PREDICT_MAX_ROWS)
    forms = proj_forms(X, rows, T)
    seen = {f: [] for f in PROJ}
    for r in range(args.rounds):
        for form in PROJ:
            seen[form].append(timed(forms[form], args.calls, args.warmup))
    m = {f: median(seen[f]) for f in PROJ}
    say("  ef projection of one chunk of %d rows, three cases: split %.4f ms (one grouped GEMM) + at most %.4f ms (the pass, as three"
        " torch.add) = at most %.4f ms; k_reduced %.4f ms (two grouped GEMMs)   (spreads %.4f, %.4f, %.4f)"
        % (rows, m["split_gemm"][0], m["split_pass_bound"][0], m["split_gemm"][0] + m["split_pass_bound"][0], m["k_reduced"][0],
           m["split_gemm"][1], m["split_pass_bound"][1], m["k_reduced"][1]))
    del forms
    torch.cuda.empty_cache()

for N, T in SHAPES:
    base = med_all[(N, "ref_route")]
    for f in ("new_eager", "new_graph"):
        m = med_all[(N, f)]
        say("N=%d T=%d  %s / ref_route = %.3f   (%.4f vs %.4f ms; spreads %.4f, %.4f)"
            % (N, T, f, m[0] / base[0], m[0], base[0], m[1], base[1]))
write_out(args.out, "scripts/bench_zeros.py --calls %d --warmup %d --rounds %d: MFM_KL_EF, fp32" % (args.calls, args.warmup, args.rounds))
