"""Size matrix of the fused plan's kernel forms, shared by tests/test_gpu_plan_forms.py (HIP against the oracle) and
tests/test_plan_forms_host.py (the fp32 oracle against itself in float64 on the same weights and batches).

Every entry is there for ONE form that the plan chooses from the sizes and the batch alone (csrc/plan_build.hip; no switch is
set), named in `want`: fields of MFMEngine.latent_form() that must hold exactly, plus `stepwise`, the hidden sizes of the LSTMs
MFMEngine.seq_form() must report on the step-by-step path (every other one on the weight-resident kernels).  The sizes assume the
256 compute units of an MI355X where a form depends on them (nch, split0); the GPU test checks that first.

What the row kernels' conditions make of the wished-for edges (plan_build.hip, the block that sets row_path):
 * K = N = 128 for the early-fusion encoder's head (zl + za + zv = 128) is out of the row kernels' reach: the stage of the
   classifier's first layer also carries the four logvar heads, so its backward has 4 * (fy + 2 * (zl + za + zv)) work items
   against 1024 threads -- zl + za + zv <= 124 with fy = 8 (the canonical sizes, 120 and fy = 16, already sit on that limit).
   "row_edge" is that largest config: 1024 backward items, K = N = 124, and decoder_l 128 wide (the resident limit);
   "row_k128" reaches K = N = 128 through fl instead (zl_to_fl_fc2), with decoder_l (136) step by step beside it.
 * zl = 40, za = 8, zv = 80 (128 wide, a first stage of exactly 1024 forward items) is therefore the first config PAST the edge:
   "past_edge_resident" (staged kernels, panel in LDS, every LSTM resident); "past_edge" adds the step-by-step encoder (132).
 * the row kernels take four workgroups per row while 4 * B <= compute units, i.e. up to B = 64: one workgroup per row is B = 65.

Group (h), sizes off the multiple of 4: ONE layer whose reduction length K is no multiple of 4 takes the whole plan off the row
kernels and off the MFMA products (plan_build.hip: the blocks that set mfma and row_path), so the staged quad kernels run their
scalar branch (latent.hip: (op.K & 3) != 0, or an odd w_off without a panel); the LSTMs with h % 4 != 0 stage their recurrent
weights through the LDS panel, take the general form of the decoder's step-0 product and get no forward weight images
(lstm_seq_small_dev.h, lstm_seq_small.hip).  OFF4's LSTMs are 18, 7, 33, 58 wide (encoders, the early-fusion one last) and
37, 15, 30 (decoders): every residue of h mod 4 in both roles.
"""
import numpy as np

from factorized_amd import configs, synth

ROW_EDGE = dict(zl_size=36, za_size=8, zv_size=80, fy_size=8, fl_size=120)
WIDE = dict(zl_size=156, fl_size=256, za_size=16, fa_size=32)          # test_wide_hidden_sizes_match_oracle's sizes
NOPANEL = dict(row_path=False, wpanel=0, mfma=False)
OFF4 = dict(input_dims=[37, 3, 11], zl_size=18, za_size=7, zv_size=33, zy_size=21, fy_size=10, fl_size=27, fa_size=5, fv_size=20)
QUAD = dict(row_path=False, mfma=False)                               # staged kernels, quad (VALU) products

# id -> (config overrides, B, T, want, stepwise hidden sizes)
KLEF = {
    # (a) the row kernels at their own upper edge
    "row_edge_b5": (ROW_EDGE, 5, 3, dict(row_path=True, nch=4, bias_tab=True, items_bwd=1024, max_k=124, max_n=124), []),
    "row_edge_b65": (ROW_EDGE, 65, 2, dict(row_path=True, nch=1, bias_tab=True, items_bwd=1024, max_k=124, max_n=124), []),
    "row_k128_b5": (dict(ROW_EDGE, fl_size=128), 5, 2, dict(row_path=True, nch=4, bias_tab=True, items_bwd=1024, max_k=128, max_n=128), [136]),
    # (b) one step past it
    "past_edge_resident_b5": (dict(zl_size=40, za_size=8, zv_size=80), 5, 3,
                              dict(row_path=False, mfma=True, items_fwd=1024, max_k=128, max_n=128, rows_per_wg=4), []),
    "past_edge_b5": (dict(zl_size=44, za_size=8, zv_size=80), 5, 3, dict(row_path=False, mfma=True, max_k=132, rows_per_wg=4), [132]),
    # (c) the panel-less staged kernels off the one tested batch
    "nopanel_b65": (WIDE, 65, 2, NOPANEL, [156, 252, 272]),
    "nopanel_b257": (WIDE, 257, 2, NOPANEL, [156, 252, 272]),
    "nopanel_split0_b1025": (WIDE, 1025, 2, dict(NOPANEL, split0=True, nstages=7), [156, 252, 272]),
    # (d) rows per workgroup halved twice (8 -> 2) under a staged panel
    "halved_panel_b65": (dict(zl_size=40, za_size=8, zv_size=80, fl_size=176), 65, 2, dict(row_path=False, mfma=True, rows_per_wg=2), [192]),
    # (e) the search fallback of the row backward's bias gradients: 1073 biases, and both directions' widest stage at 1024 items
    "bias_search_b65": (dict(fl_size=112, fa_size=64, fv_size=64), 65, 2,
                        dict(row_path=True, nch=1, bias_tab=False, n_bias=1073, items_fwd=1024, items_bwd=1024), []),
    # (f) the widest output head
    "od64_l1_b5": (dict(output_dim=64), 5, 2, dict(row_path=True, nch=4), []),
    "od64_ce_b5": (dict(output_dim=64, loss="ce"), 5, 2, dict(row_path=True, nch=4), []),
    # (h) sizes off the multiple of 4: staged quad kernels on their scalar branch, LSTMs of every residue of h mod 4
    "off4_b5": (OFF4, 5, 3, dict(QUAD, rows_per_wg=4), []),
    "off4_b65": (OFF4, 65, 2, QUAD, []),                               # past B = 64: role and fold launches out of reach
    "off4_b257": (OFF4, 257, 2, QUAD, []),                             # the first batch at which every size takes the staged kernels
    "off4_b513": (OFF4, 513, 2, QUAD, []),                             # the first on the MFMA recurrences (SEQ_MFMA): 1 to 3 pad units
    "off4_ce_b5": (dict(OFF4, output_dim=7, loss="ce"), 5, 2, dict(QUAD, rows_per_wg=4), []),
    "off4_h127_b5": (dict(zl_size=127, za_size=9, zv_size=78, zy_size=30, fy_size=10, fl_size=117, fa_size=6, fv_size=61), 5, 2,
                     NOPANEL, [214]),                                  # encoder and decoder 127 wide: the widest resident; the
                                                                       # heads on 214 columns leave no room for a panel
    "off4_nopanel_b65": (dict(zl_size=157, fl_size=255, za_size=17, fa_size=33), 65, 2, NOPANEL, [157, 254, 271]),
}
OFF4_GROUP = tuple(n for n in KLEF if n.startswith("off4_"))                 # none may take the row path or the MFMA products
PANEL = ("past_edge_resident_b5", "past_edge_b5", "halved_panel_b65",        # wpanel > 0 is asserted for these
         "off4_b5", "off4_b65", "off4_b257", "off4_b513", "off4_ce_b5")
SEQ_MFMA = ("off4_b513",)                                                    # every resident LSTM on the fp32 MFMA recurrences

# id -> (overrides of test_gpu_mfn_plan.ODD_MFN, widths of the four attention nets, B, T)
ATT = (36, 20, 28, 44)
MFN_OFF4 = dict(OFF4, h_dims=[37, 5, 18], memsize=21)
MFN = {
    # (g) MFM_KL at the resident limit of the MFN LSTMs: a cStar row of 768 columns, and one wide LSTM beside two of 4
    "mfn_h128x3_b5": (dict(h_dims=[128, 128, 128]), ATT, 5, 3),
    "mfn_h128_4_4_b5": (dict(h_dims=[128, 4, 4]), ATT, 5, 3),
    # (h) MFM_KL and MFM off the multiple of 4: MFN LSTMs, memory and attention nets of every residue too
    "mfn_off4_b5": (MFN_OFF4, (35, 19, 27, 43), 5, 3),
    "mfn_off4_b65": (MFN_OFF4, (35, 19, 27, 43), 65, 2),
}
MFN_RESIDENT = ("mfn_h128x3_b5", "mfn_h128_4_4_b5")
MFN_OFF4_GROUP = ("mfn_off4_b5", "mfn_off4_b65")

WEIGHT_SEED = 77
BATCH_SEED = 21


def klef_case(name, rates=None):
    """`rates`: dropout probabilities per site (the *_dropout keys of the config) for the train-mode dropout tests; None: none"""
    over, B, T, want, stepwise = KLEF[name]
    cfgs = configs.canonical_configs(dropout=rates is not None, **dict(over, **(rates or {})))
    cfg = cfgs[0]
    loss_kind = cfg.get("loss", "l1")
    x, y = synth.make_batch(cfg["input_dims"], B, T, seed=BATCH_SEED, output_dim=cfg["output_dim"],
                            classes=cfg["output_dim"] if loss_kind == "ce" else 0)
    return dict(name=name, cfgs=cfgs, cfg=cfg, B=B, T=T, want=want, stepwise=stepwise, loss_kind=loss_kind, x=x, y=y)


def mfn_case(name):
    from tests.test_gpu_mfn_plan import ODD_MFN
    over, att, B, T = MFN[name]
    cfgs = configs.canonical_configs(dropout=False, **dict(ODD_MFN, **over))
    cfgs[1]["shapes"], cfgs[2]["shapes"], cfgs[3]["shapes"], cfgs[4]["shapes"] = att
    x, y = synth.make_batch(cfgs[0]["input_dims"], B, T, seed=23)
    return dict(name=name, cfgs=cfgs, cfg=cfgs[0], B=B, T=T, x=x, y=y)


def expected_rows(B, rec_size, wpanel, cus, budget=150 * 1024):
    """Rows per workgroup of the staged backward and forward kernels: the rule of plan_build.hip ("rows per workgroup" and
    "the forward keeps ONE record per row") restated -- 4 / 8 / 16 by the batch, halved until two records per row and the panel
    fit the LDS budget; the forward doubles again while the launch needs more than one round of workgroups and still fits."""
    R = 4 if B <= 64 else (8 if B <= 1024 else 16)
    while R > 1 and (2 * R * rec_size + wpanel) * 4 > budget:
        R //= 2
    Rf = R
    while Rf < 16 and -(-B // Rf) > cus and (2 * Rf * rec_size + wpanel) * 4 <= budget:
        Rf *= 2
    return R, Rf


def worst_grad(named_grads, got):
    """(name, cases.grad_err) of the worst tensor; `named_grads`: (name, reference gradient or None) of EVERY parameter -- a
    parameter without a reference gradient must hold exact zeros."""
    from tests.cases import grad_err
    worst = ("", 0.0)
    for n, r in named_grads:
        g = np.asarray(got[n])
        if r is None:
            assert np.all(g == 0.0), n
            continue
        err = grad_err(g, r)
        if err > worst[1]:
            worst = (n, err)
    return worst
