"""Train-mode dropout of the latent kernels (reference mfm_model.py:599-617, 644-647, 657: nn.Dropout between fc1
and fc2 of the four z->f MLPs and of the classifier).  The GPU draws its masks from a counter-based generator,
not torch's Philox stream, so dropout cannot be compared sample by sample with a CPU run; instead the masks the
kernel actually used are read back from the plan's latent record and (tests/dropout_checks.py)

  * every mask value is 0 or 1/(1-p), the kept fraction is 1-p within 5 sigma, per site;
  * the stored post-dropout activation equals relu(fc1(input)) * mask recomputed on the host;
  * the masks are INJECTED into the CPU oracle (its nn.Dropout modules replaced by fixed multipliers): forward
    losses and all 78 gradients must then match at 1e-4 -- which pins that the backward applies the same mask
    and scale as the forward;
  * masks change from call to call and with the seed (per-rank seeds of the data-parallel step)

-- on EVERY kernel form the latent stack takes (csrc/plan_build.hip, lstm_seq_small.hip), each case asserting the form it is
there for before any number:

  (a) the form bench.py times: B = 32, the z->f chains inside the encoder launch (four chain workgroups per row), the
      classifier as tail blocks of the decoder launch, its backward as head blocks of the decoder BPTT, the rest in front of
      the encoder BPTT -- through forward + backward, grad_step and train_step, hand-overs on and off;
  (b) the batch edges of the row kernels (1, 33, 64 | 65: four workgroups per row | one);
  (c) the same batch with one form switched off at a time; the masks must not notice;
  (d) the staged kernels at the sizes tests/plan_forms.py proves with dropout off (MFMA / quad products, panel in LDS or
      not, halved rows, split first stage), the row kernels at their upper edge, the cross-entropy head;
  (e) p = 0 beside live sites, and p = 0.9;
  (f) no correlation between neighbouring rows, columns and calls of the stream.

The sizes of (b) and (d) assume the 256 compute units of an MI355X where the form depends on them (nch)."""
import os

import numpy as np
import pytest
import torch

from factorized_amd import _lib, configs, synth
from tests import plan_forms as PF
from tests.dropout_checks import P, SITES, check_dropout, read_masks

pytestmark = pytest.mark.gpu
SWITCHES = ("MFM_LATENT_PATH", "MFM_LATENT_FOLD", "MFM_LATENT_TAIL", "MFM_LATENT_BWD_HEAD", "MFM_LATENT_CHAINS", "MFM_LATENT_PRE")
ROW4 = dict(row_path=True, nch=4, split0=False)          # four chain workgroups per row
ROW1 = dict(row_path=True, nch=1, split0=False)
_first = {}


@pytest.fixture(autouse=True)
def no_latent_switches(monkeypatch):
    """a stray switch must not choose the form; a case that wants one sets it itself"""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    for k in list(os.environ):
        if k.startswith("MFM_LATENT_"):
            monkeypatch.delenv(k)


def _setup(cfgs, B, T, weight_seed=1234, batch_seed=5, handover=None):
    from factorized_amd import engine
    e = engine.MFMEngine(cfgs)
    if handover is not None:
        e.set_handover(handover)
    w = synth.make_weights(e.layout.shapes, seed=weight_seed)
    e.load_weights(w)
    xn, yn = synth.make_batch(cfgs[0]["input_dims"], B, T, seed=batch_seed)
    return e, w, xn, yn


def _default_first_masks(B):
    """masks of the FIRST training-mode call of a fresh engine in the default form (no switch set) at the rates P: the stream
    is a pure function of (seed, call number, op index, row, column), so every other form, entry and T must draw the same"""
    assert not any(k in os.environ for k in SWITCHES)
    if B not in _first:
        e, _, xn, yn = _setup(configs.canonical_configs(dropout=True, **P), B, 2)
        e.forward(torch.from_numpy(xn).cuda(), torch.from_numpy(yn).cuda(), train=True, want_xhat=False)
        _first[B] = read_masks(e, 2, B)
    return _first[B]


def _same_masks(got, want):
    for site in SITES:
        assert np.array_equal(got[site], want[site]), site


def _cus(n=256):
    assert _lib.lib().mfm_device_cus() == n, "the forms of this case are those of a device with %d compute units" % n


@pytest.mark.parametrize("B,path", [(200, "row"), (512, "staged"), (64, "forced-staged")])
def test_dropout_masks_statistics_and_gradients(B, path, monkeypatch):
    """both latent kernel families with a launch of their own: row-per-workgroup at 64 < B <= 256, staged-LDS above (or forced);
    the kept fraction is held to 5 sigma at every site, whatever its size"""
    if path == "forced-staged":
        monkeypatch.setenv("MFM_LATENT_PATH", "staged")
    T = 6
    cfgs = configs.canonical_configs(dropout=True, **P)
    e, w, xn, yn = _setup(cfgs, B, T)
    form = ROW1 if path == "row" else dict(row_path=False)
    check_dropout("b%d_%s" % (B, path), e, w, cfgs, xn, yn, "forward", form=form, own_launch=True, stats_from=0)


def test_dropout_streams_differ_between_data_parallel_ranks():
    """DataParallelStep gives every rank its own seed: two engines that differ only in the
    rank must draw different masks for the same local row numbers."""
    from factorized_amd import engine, train
    cfgs = configs.canonical_configs(dropout=True, **P)
    B, T = 32, 4
    xn, yn = synth.make_batch(cfgs[0]["input_dims"], B, T, seed=5)
    x, y = torch.from_numpy(xn).cuda(), torch.from_numpy(yn).cuda()
    got = []
    for rank in (0, 1):
        e = engine.MFMEngine(cfgs)
        e.load_weights(synth.make_weights(e.layout.shapes, seed=1234))
        train.DataParallelStep(e, world=2, allreduce=lambda t: None, rank=rank)
        assert e.reg_scale == 2.0
        e.forward(x, y, train=True, want_xhat=False)
        rec, _, lay = e.latent_record(T, B)
        o = lay["mask"]["zv_to_fv"]
        got.append(rec[:, o:o + lay["width"]["zv_to_fv"]].cpu().numpy().copy())
    assert not np.array_equal(got[0], got[1])


# ---------------------------------------------------------------------- (a) the benchmarked form
BENCH_CASES = [(3, en, ho, "P") for en in ("forward", "grad_step", "train_step") for ho in (True, False)]
BENCH_CASES += [(20, "train_step", True, "P"), (3, "train_step", True, "canonical")]


@pytest.mark.parametrize("T,entry,handover,rates", BENCH_CASES,
                         ids=["t%d-%s-%s-%s" % (t, en, "handover" if ho else "separate", r) for t, en, ho, r in BENCH_CASES])
def test_benchmarked_form(T, entry, handover, rates):
    """B = 32 at the canonical sizes: no latent launch of its own in either direction.  With the hand-overs on the projections
    are role workgroups of the encoder launch (no proj_gemm) and the decoder BPTT carries the head blocks at the first attempt
    (ONE bracket on dec_seq_bwd; a refused head launch leaves two, tests/golden/seq_launch_table.json b32_no_bwd_head).
    "canonical": the rates of canonical_configs(dropout=True) themselves -- what bench.py times; zy_to_fy and fy_to_y are 0
    there and must hold 1.0."""
    _cus()
    B = 32
    cfgs = configs.canonical_configs(dropout=True, **(P if rates == "P" else {}))
    e, w, xn, yn = _setup(cfgs, B, T, handover=handover)
    slots = dict(proj_gemm=0, dec_seq_bwd=1) if handover else None
    res = check_dropout("bench_t%d_%s_%s" % (T, "ho" if handover else "sep", rates), e, w, cfgs, xn, yn, entry, form=ROW4,
                        own_launch=False, slots=slots)
    if rates == "P":
        _same_masks(res["masks"], _default_first_masks(B))


# ---------------------------------------------------------------------- (b) batch edges of the row forms
@pytest.mark.parametrize("B,form,own_launch,slots", [
    (1, ROW4, False, dict(proj_gemm=0)),
    (33, ROW4, False, dict(proj_gemm=1)),          # past the projection roles: the chains still ride on the encoder launch
    (64, ROW4, False, None),                        # the last batch with four workgroups per row
    (65, ROW1, True, None),                         # the first with one: launches of their own
], ids=["b1", "b33", "b64", "b65"])
def test_row_form_batch_edges(B, form, own_launch, slots):
    """(B = 1: one row, so "rows do not share a mask" has nothing to compare; the sites' values, the activations, the oracle's
    gradients under the same mask and the call-to-call change are checked as everywhere)"""
    _cus()
    cfgs = configs.canonical_configs(dropout=True, **P)
    e, w, xn, yn = _setup(cfgs, B, 2)
    check_dropout("edge_b%d" % B, e, w, cfgs, xn, yn, "train_step", form=form, own_launch=own_launch, slots=slots)


# ---------------------------------------------------------------------- (c) switched forms
@pytest.mark.parametrize("switch,value,form,own_launch,slots", [
    ("MFM_LATENT_FOLD", "0", ROW4, True, None),
    ("MFM_LATENT_TAIL", "0", ROW4, False, dict(dec_seq_bwd=2)),           # whole chains in the encoder launch; no head blocks
    ("MFM_LATENT_BWD_HEAD", "0", ROW4, False, dict(dec_seq_bwd=2)),       # tails ride, the backward's head is refused
    ("MFM_LATENT_CHAINS", "0", ROW1, True, None),
    ("MFM_LATENT_PRE", "1", ROW4, False, dict(dec_seq_bwd=1)),           # refused at these sizes: the default form
], ids=["no_fold", "no_tail", "no_bwd_head", "no_chains", "pre"])
def test_switched_forms_draw_the_default_forms_masks(switch, value, form, own_launch, slots, monkeypatch):
    """One form taken away (or, PRE, opted into) at B = 32, T = 3.  FOLD, TAIL and BWD_HEAD are read at launch and cannot
    change the op table; CHAINS and PRE are read by plan_build.hip, but only AFTER every add_op: they choose how the ops of a
    stage are dealt to workgroups (the item tables carry the op's index in the ONE table, `sel[si]`), never their numbering.
    So under all five a fresh engine's first call must draw masks bit-identical to the default form's.
    PRE at the canonical sizes is not the form it names: plan_build.hip keeps it only while every stage of every chain has at
    most 512 work items, and the y chain's classifier stage (with the early-fusion logvar head) has 4 * (fy + zl + za + zv) =
    544 in the backward.  The plan then stays in the default form, which is what this case asserts;
    test_pre_chain_kernels_where_the_plan_takes_them runs the form itself."""
    _cus()
    B, T = 32, 3
    want = _default_first_masks(B)
    monkeypatch.setenv(switch, value)
    cfgs = configs.canonical_configs(dropout=True, **P)
    e, w, xn, yn = _setup(cfgs, B, T)
    res = check_dropout(switch[4:].lower() + value, e, w, cfgs, xn, yn, "train_step", form=form, own_launch=own_launch, slots=slots)
    _same_masks(res["masks"], want)


def test_pre_chain_kernels_where_the_plan_takes_them(monkeypatch):
    """MFM_LATENT_PRE=1 at the nearest sizes the plan takes it: zl = 28 and fy = 12 leave the y chain's widest stage at
    4 * (12 + 116) = 512 backward items, and every LSTM in the size class of the canonical one (hidden sizes 28, 8, 80, 116
    and 100, 20, 20 round to the same k-slices as 32, 8, 80, 120 and 104, 24, 24), so WITHOUT the switch the chains ride on the
    recurrence launches as at the canonical sizes -- asserted first.  latent_form() has no field for PRE; the fold launches do
    not take a chain kernel that requests its weights ahead (lstm_seq_small.hip chain_rows_match), so under the switch, with
    four chain workgroups per row, latent launches of their own are what shows it.  Same op table: same masks."""
    _cus()
    B, T = 32, 3
    cfgs = configs.canonical_configs(dropout=True, zl_size=28, fy_size=12, **P)
    e, w, xn, yn = _setup(cfgs, B, T)
    want = check_dropout("pre_sizes_default", e, w, cfgs, xn, yn, "train_step", form=ROW4, own_launch=False)
    monkeypatch.setenv("MFM_LATENT_PRE", "1")
    e, w, xn, yn = _setup(cfgs, B, T)
    res = check_dropout("pre_sizes_pre1", e, w, cfgs, xn, yn, "train_step", form=ROW4, own_launch=True)
    _same_masks(res["masks"], want["masks"])


# ---------------------------------------------------------------------- (d) the staged forms (and the row forms' far edge)
STAGED = ["past_edge_resident_b5", "halved_panel_b65", "nopanel_b65", "nopanel_split0_b1025", "bias_search_b65", "row_edge_b5",
          "od64_ce_b5"]


@pytest.mark.parametrize("name", STAGED)
def test_plan_form_sizes_with_dropout(name):
    """the entries of tests/plan_forms.KLEF with the rates P.  A latent launch of its own everywhere but od64_ce_b5, whose
    encoders and decoders keep the canonical sizes the fold launches are built for (row_edge_b5's do not)."""
    from factorized_amd import engine
    cs = PF.klef_case(name, rates=P)
    B, T, want = cs["B"], cs["T"], dict(cs["want"])
    cus = _lib.lib().mfm_device_cus()
    if "nch" in want:
        assert (4 * B <= cus) == (want["nch"] == 4), (B, cus)          # the sizes of the matrix assume 256 compute units
    e = engine.MFMEngine(cs["cfgs"])
    w = synth.make_weights(e.layout.shapes, seed=PF.WEIGHT_SEED)
    e.load_weights(w)
    if name in PF.PANEL:
        assert e.latent_form(T, B)["wpanel"] > 0
    check_dropout(name, e, w, cs["cfgs"], cs["x"], cs["y"], "forward", form=want, own_launch=name != "od64_ce_b5",
                  loss_kind=cs["loss_kind"])


# ---------------------------------------------------------------------- (e) rates at the edges
@pytest.mark.parametrize("B,entry,own_launch", [(32, "train_step", False), (200, "forward", True)], ids=["b32", "b200"])
@pytest.mark.parametrize("rates", [dict(P, zl_to_fl_dropout=0.0, fy_to_y_dropout=0.0), dict(P, zl_to_fl_dropout=0.9, fy_to_y_dropout=0.9)],
                         ids=["p0_mixed", "p09"])
def test_rates_at_the_edges(rates, B, entry, own_launch):
    """sites without dropout (exactly 1.0 in train mode) beside live ones -- the widest z->f MLP and the classifier -- and
    p = 0.9 (a scale of 10) at the same two"""
    _cus()
    cfgs = configs.canonical_configs(dropout=True, **rates)
    e, w, xn, yn = _setup(cfgs, B, 3)
    check_dropout("rates_b%d_%s" % (B, "p09" if rates["fy_to_y_dropout"] else "p0"), e, w, cfgs, xn, yn, entry,
                  form=ROW4 if B == 32 else ROW1, own_launch=own_launch)


# ---------------------------------------------------------------------- (f) stream independence
def _corr(a, b):
    a = a.astype(np.float64).ravel() - a.mean(dtype=np.float64)
    b = b.astype(np.float64).ravel() - b.mean(dtype=np.float64)
    return float((a * b).sum() / np.sqrt((a * a).sum() * (b * b).sum())), a.size


def test_stream_is_uncorrelated_across_rows_columns_and_calls():
    """B = 200, T = 2, pooled per site: the sample correlation of the mask with itself one row down, one column along, and
    with the next call's mask stays inside 5 / sqrt(n) (n pairs).  The masks are deterministic given the seed; a numpy
    restatement of rng_uniform stays inside this bound for every op index 0..31 and calls 1..4 at these site shapes (worst
    |r| 0.72 of the bound)."""
    B, T = 200, 2
    cfgs = configs.canonical_configs(dropout=True, **P)
    e, w, xn, yn = _setup(cfgs, B, T)
    res = check_dropout("stream_b200", e, w, cfgs, xn, yn, "forward", form=ROW1, own_launch=True)
    for site in SITES:
        m, nxt = res["masks"][site], res["next_masks"][site]
        for what, a, b in (("row", m[1:], m[:-1]), ("column", m[:, 1:], m[:, :-1]), ("call", m, nxt)):
            r, n = _corr(a, b)
            print("stream %s %s: r %.4f bound %.4f" % (site, what, r, 5 / np.sqrt(n)))
            assert abs(r) < 5 / np.sqrt(n), (site, what, r, n)
