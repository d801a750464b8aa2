"""The value matrix of tests/data_regimes.py without a GPU: the two conditions under which the 1e-4 the HIP kernels are held
to against the float64 oracle (tests/test_gpu_data_regimes.py) means something.

1. Oracle headroom.  On every regime at (B, T) = (19, 5), weights make_weights(seed=1234), the fp32 oracle (kl_ef; loss_terms,
   then backward) stays within 1e-5 of the same oracle in float64 -- every loss term relative to max(|ref|, 1e-3), every
   gradient in tests.cases.rel_err.  Measured (worst loss term / worst gradient): unit noise 4.8e-8 / 3.9e-7, mixed 8.3e-8 /
   6.1e-7, saturated 5.3e-8 / 6.1e-6, small 1.1e-7 / 3.8e-7, big_all 1.1e-7 / 6.3e-6, padded 4.3e-8 / 2.8e-6, outlier 8.0e-8 /
   5.1e-6: 1.6x under the condition at the worst, and the GPU bound is at least 16x the oracle's own distance from float64.
2. Every regime does what its name says, computed from the float64 oracle's gate pre-activations (the cell restated below):
   saturated / big_all reach |a| > 88.7 in encoder_a / ef_encoder, small keeps max|x W_ih^T| < 1e-2, padded has its exact
   zeros and constants where it was built to, mixed has its three gen terms at least 10^3 apart.  A regime that misses its
   condition gets another factor (tests/data_regimes.py), never another condition."""
import numpy as np
import pytest
import torch

from factorized_amd import engine, synth
from oracle import mfm_oracle as O
from tests import data_regimes as DR
from tests.cases import rel_err

HEADROOM = 1e-5
B, T = 19, 5
ENCODERS = ("encoder_l", "encoder_a", "encoder_v", "ef_encoder")
_CACHE = {}


def _weights(cfgs):
    return synth.make_weights(engine.param_shapes(cfgs, "kl_ef"), seed=DR.WEIGHT_SEED)


def _run32(cfgs, w, x, y):
    m = O.build("kl_ef", cfgs)
    O.load_numpy_weights(m, w)
    m.train()
    terms = O.loss_terms(m, torch.from_numpy(x), torch.from_numpy(y), cfgs[0])
    terms["loss"].backward()
    return m, terms


def _case(regime):
    """both oracles on one regime, computed once and left unchanged"""
    if regime not in _CACHE:
        torch.set_num_threads(4)
        cfgs = DR.canonical()
        w = _weights(cfgs)
        x, y = DR.make(regime, B, T)
        m32, t32 = _run32(cfgs, w, x, y)
        m64, t64 = DR.oracle64("kl_ef", cfgs, w, x, y)
        _CACHE[regime] = dict(x=x, y=y, m32=m32, t32=t32, m64=m64, t64=t64)
    return _CACHE[regime]


def _slices():
    d_l, d_a, d_v = DR.DIMS
    return {"encoder_l": slice(0, d_l), "encoder_a": slice(d_l, d_l + d_a), "encoder_v": slice(d_l + d_a, d_l + d_a + d_v),
            "ef_encoder": slice(0, d_l + d_a + d_v)}


def _preactivations(m64, x):
    """encoder -> (gate pre-activations [T, B, 4h], x-projections x W_ih^T [T, B, 4h]) of the float64 oracle: the LSTM cell
    restated, a_t = x_t W_ih^T + b_ih + h_{t-1} W_hh^T + b_hh with the oracle's own hidden states"""
    xt = torch.from_numpy(x).double()
    out = {}
    with torch.no_grad():
        for name, sl in _slices().items():
            enc = getattr(m64, name)
            xs = xt[:, :, sl]
            _, hs = enc.run(xs, keep=True)
            hprev = torch.stack([torch.zeros_like(hs[0])] + hs[:-1])
            proj = xs @ enc.lstm.weight_ih.T
            a = proj + enc.lstm.bias_ih + hprev @ enc.lstm.weight_hh.T + enc.lstm.bias_hh
            out[name] = (a.numpy(), proj.numpy())
    return out


@pytest.mark.parametrize("regime", DR.REGIMES)
def test_fp32_oracle_has_headroom(regime):
    s = _case(regime)
    worst_l, worst_g = ("", 0.0), ("", 0.0)
    for k in DR.LOSS_KEYS:
        a, r = float(s["t32"][k].detach()), float(s["t64"][k].detach())
        assert np.isfinite(a) and np.isfinite(r), (k, a, r)
        d = DR.loss_rel(a, r)
        if d > worst_l[1]:
            worst_l = (k, d)
    g64 = dict(s["m64"].named_parameters())
    for n, p in s["m32"].named_parameters():
        r = g64[n].grad.numpy()
        assert np.all(np.isfinite(p.grad.numpy())) and np.all(np.isfinite(r)), n
        d = rel_err(p.grad.numpy(), r)
        if d > worst_g[1]:
            worst_g = (n, d)
    print("regime %s fp32 vs float64: worst loss term %s %.2e, worst gradient %s %.2e" % ((regime,) + worst_l + worst_g))
    assert worst_l[1] <= HEADROOM, worst_l
    assert worst_g[1] <= HEADROOM, worst_g


@pytest.mark.parametrize("regime", DR.REGIMES)
def test_regime_does_what_its_name_says(regime):
    s = _case(regime)
    x = s["x"]
    pre = _preactivations(s["m64"], x)
    amax = {n: float(np.abs(a).max()) for n, (a, _) in pre.items()}
    pmax = {n: float(np.abs(p).max()) for n, (_, p) in pre.items()}
    gen = {k: float(s["t64"][k].detach()) for k in ("gen_l", "gen_a", "gen_v")}
    print("regime %s max|a| %s max|x W_ih^T| %s gen %s" % (
        regime, " ".join("%s %.3g" % kv for kv in amax.items()), " ".join("%s %.3g" % kv for kv in pmax.items()),
        " ".join("%s %.4g" % kv for kv in gen.items())))
    if regime == "saturated":
        assert amax["encoder_a"] > DR.SAT, amax
        assert amax["ef_encoder"] > DR.SAT, amax
    elif regime == "big_all":
        assert all(amax[n] > DR.SAT for n in ENCODERS), amax          # ef_encoder, and "in all four encoders at once"
    elif regime == "small":
        assert max(pmax.values()) < 1e-2, pmax
    elif regime == "mixed":
        assert max(gen.values()) >= 1e3 * min(gen.values()), gen
    elif regime == "outlier":
        rows = np.abs(x).max(axis=(0, 2))
        others = np.delete(rows, DR.OUTLIER_ROW)
        assert rows[DR.OUTLIER_ROW] >= 5.0 * others.max(), (rows[DR.OUTLIER_ROW], others.max())
    elif regime == "padded":
        pads = DR.pad_steps(B, T)
        assert pads[0] == 0 and max(pads) == T - 1, pads
        free = np.ones(x.shape[2], dtype=bool)
        for col, val in DR.CONST_COLS:
            free[col] = False
            assert np.all(x[:, :, col] == np.float32(val)), col
        for b, n in enumerate(pads):
            assert np.all(x[:n, b][:, free] == 0.0), b
        assert np.any(x[pads[0]:, 0][:, free] != 0.0)
        # and the exact zeros reach the gradients: the zero-valued constant column of weight_ih, in both encoders that read it
        g64 = dict(s["m64"].named_parameters())
        for enc in ("encoder_l", "ef_encoder"):
            assert np.all(g64[enc + ".lstm.weight_ih"].grad.numpy()[:, 0] == 0.0), enc
        # a non-zero constant column is the bias gradient scaled
        for enc, cols in DR.CONST_BY_ENCODER.items():
            gw, gb = g64[enc + ".lstm.weight_ih"].grad.numpy(), g64[enc + ".lstm.bias_ih"].grad.numpy()
            for col, val in cols:
                if val != 0.0:
                    assert rel_err(gw[:, col], np.float64(np.float32(val)) * gb) < 1e-12, (enc, col)
