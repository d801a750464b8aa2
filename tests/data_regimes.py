"""Value matrix of the parity tests, shared by tests/test_data_regimes_host.py (the fp32 oracle against itself in float64, and
whether each regime does what its name says) and tests/test_gpu_data_regimes.py (HIP against the float64 oracle).  It plays for
the VALUES that go through the kernels the role tests/plan_forms.py plays for the sizes: every other parity test draws
synth.make_batch as it is -- unit-scale noise on every modality -- while the data the model exists for has word vectors near unit
scale, acoustic features in the tens to hundreds, visual features in the hundredths, left-padded sequences and columns that
never change.

make(regime, B, T) starts from synth.make_batch(DIMS, B, T, seed) on the canonical [300, 5, 20] input dims (which already
zeroes a random number of leading steps per sample) and returns (x [T, B, 325] float32, y [B] float32):

  regime      construction                                         what it is there for
  mixed       modality scales (1, 50, 0.02)                        MSE terms 10^4 apart; a small modality beside a large one
                                                                   in the early-fusion projection
  saturated   modality scales (1, 200, 1)                          acoustic-encoder and ef pre-activations beyond +-88.7: the
                                                                   inf / exact-0 branch of the fast activations (common.h:
                                                                   v_exp_f32 + v_rcp_f32), forward and BPTT
  big_all     modality scales (31, 100, 150)                       saturation in all four encoders at once; large dW_ih
  small       every modality x 1e-3, weights and biases unchanged  projections that vanish beside the biases
  padded      sample b has its first (s b) mod T steps set to      exact zeros through projections, dA and dW rows
              exactly 0, s = 3 (s = 2 where 3 divides T: the
              rule would pad nothing) -- sample 0 has none, one
              sample has T - 1; then columns 0 and 299 of l, 2 of
              a and 7 of v are held constant over time AND batch,
              padded steps included (values 0, 1.5, -40, 0.01)
  outlier     mixed, plus sample 3 of the batch x 30               one row dominating every max-norm; the rest of the batch
                                                                   must still be right (judged row by row)

Two factors are not the first ones tried, and both were chosen on the float64 oracle alone (tests/test_data_regimes_host.py
prints the figures).  big_all as "every modality x 30" reaches |a| = 48 in the early-fusion encoder, short of 88.7; a uniform
factor that reaches it (x 56 .. 60) costs the fp32 oracle itself 1e-5 .. 4e-5 on encoder_l's weight_ih gradient, because the
300 word-vector products of |x| ~ 20 no longer pin a gate pre-activation to 1e-5.  (31, 100, 150) are round per-modality
factors at which each of the four encoders crosses 88.7 (90.9, 198, 98.9, ef 107) with the fp32 oracle at 6.3e-6.  outlier
with sample 3 x 100 leaves the fp32 oracle at 3.4e-5 for the same reason; x 30 (5.1e-6) still has the row dominate every
max-norm thirtyfold.

The constant columns are written after the padding: a padded step is zero in every column but the three non-zero constants, and
the weight_ih gradient of a constant column is exactly value x (sum of dA over all steps and rows) = value x the bias gradient.

DELIBERATELY LEFT OUT: zero biases with vanishing inputs.  act_tanh (common.h) is 2 sigmoid(2x) - 1, which loses about 1.2e-7
ABSOLUTE to cancellation; at |x| ~ 1e-3 that is already ~1e-4 relative, the project's whole tolerance.  It does not show in
`small` because the gate biases (U(+-1/sqrt(h))) keep every pre-activation away from 0, and no initialisation or trained state of
this model puts all four gate biases at zero; a polynomial branch for small |x| would sit on the hot path of every recurrence.
DESIGN.md section 5 says the same."""
import numpy as np

from factorized_amd import configs, synth

DIMS = [300, 5, 20]
WEIGHT_SEED = 1234
BATCH_SEED = 7
SAT = 88.7                       # beyond this |a| the fp32 exponential of the fast activations is inf or 0

SCALES = {"mixed": (1.0, 50.0, 0.02), "saturated": (1.0, 200.0, 1.0), "big_all": (31.0, 100.0, 150.0),
          "small": (1e-3, 1e-3, 1e-3), "outlier": (1.0, 50.0, 0.02)}
REGIMES = ("mixed", "saturated", "big_all", "small", "padded", "outlier")
OUTLIER_ROW, OUTLIER_FACTOR = 3, 30.0
# padded: (column of the concatenated input, value); l 0, l 299, a 2, v 7
CONST_COLS = ((0, 0.0), (299, 1.5), (300 + 2, -40.0), (305 + 7, 0.01))
# the same columns inside each encoder's own input: encoder -> ((column, value), ...)
CONST_BY_ENCODER = {"encoder_l": ((0, 0.0), (299, 1.5)), "encoder_a": ((2, -40.0),), "encoder_v": ((7, 0.01),),
                    "ef_encoder": CONST_COLS}


def pad_steps(B, T):
    """padded: the number of leading zero steps of every sample"""
    s = 2 if T % 3 == 0 else 3
    return [(s * b) % T for b in range(B)]


def make(regime, B, T, seed=BATCH_SEED):
    x, y = synth.make_batch(DIMS, B, T, seed=seed)
    d_l, d_a, _ = DIMS
    if regime in SCALES:
        sl, sa, sv = SCALES[regime]
        x[:, :, :d_l] *= np.float32(sl)
        x[:, :, d_l:d_l + d_a] *= np.float32(sa)
        x[:, :, d_l + d_a:] *= np.float32(sv)
        if regime == "outlier":
            x[:, OUTLIER_ROW, :] *= np.float32(OUTLIER_FACTOR)
    elif regime == "padded":
        for b, n in enumerate(pad_steps(B, T)):
            x[:n, b, :] = 0.0
        for col, val in CONST_COLS:
            x[:, :, col] = np.float32(val)
    else:
        raise KeyError(regime)
    return x, y


def canonical():
    cfgs = configs.canonical_configs(dropout=False)
    assert cfgs[0]["input_dims"] == DIMS
    return cfgs


def oracle64(variant, cfgs, w, x, y, gauss=None):
    """the float64 oracle's train-mode step on (x, y): (model, terms); terms["loss"].backward() has run"""
    import copy

    import torch
    from oracle import mfm_oracle as O
    m = O.build(variant, cfgs)
    O.load_numpy_weights(m, w)
    m = copy.deepcopy(m).double()
    m.train()
    if gauss is not None:
        m.mmd_gauss = [g.double() for g in gauss]
    terms = O.loss_terms(m, torch.from_numpy(x).double(), torch.from_numpy(y).double(), cfgs[0])
    terms["loss"].backward()
    return m, terms


LOSS_KEYS = ("disc", "gen_l", "gen_a", "gen_v", "gen", "reg", "loss")


def loss_rel(got, ref):
    """relative distance of one loss term, against max(|ref|, 1e-3)"""
    return abs(float(got) - float(ref)) / max(abs(float(ref)), 1e-3)
