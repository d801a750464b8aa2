"""The fused plan at the sizes where it switches kernel form (csrc/plan_build.hip): row or staged latent kernels, weight panel
in LDS or read from L2, MFMA or quad products, rows per workgroup and their LDS-driven halving, the split first stage, one or
four chain workgroups per row, tabulated or searched bias gradients, resident or step-by-step LSTMs -- each reached through the
SIZES (tests/plan_forms.py says which entry is there for which form and why), never through a switch: the latent and sequence
switches are deleted from the environment.  Every entry first asserts its form through MFMEngine.latent_form() / seq_form(),
then compares forward losses, every parameter gradient and three Adam steps with the torch-CPU oracle, which itself keeps to a
tenth of the tolerance on the same inputs (tests/test_plan_forms_host.py).  Tolerance 1e-4 relative fp32.

(d) of the matrix -- rows halved under a staged panel -- needs no exotic size: 2 * 8 records of the canonical 1180 floats plus
the 22264-float panel already exceed the 150 KB budget, so every staged plan between B = 65 and 1024 halves 8 -> 4; the entry
here grows the panel (fl = 176) until they halve twice.

(h) of the matrix -- sizes off the multiple of 4 -- holds hidden, latent and factor widths of every residue mod 4: one layer
with K % 4 != 0 turns the row kernels and the MFMA products off for the whole plan (asserted for the group), and LSTMs with
h % 4 != 0 take the panel-staged recurrent weights and the decoders' forms without forward weight images.  The same sizes run
as MFM_KL and MFM plans with MFN LSTMs, memory and attention nets off the multiple of 4 (test_mfn_off4_matches_oracle)."""
import os

import numpy as np
import pytest
import torch

from factorized_amd import _lib, configs, synth
from oracle import mfm_oracle as O
from tests import cases
from tests import plan_forms as PF

pytestmark = pytest.mark.gpu
TOL = 1e-4


@pytest.fixture(autouse=True)
def no_form_switches(monkeypatch):
    """a stray switch must not choose the form"""
    for k in list(os.environ):
        if k.startswith(("MFM_LATENT_", "MFM_SEQ_")):
            monkeypatch.delenv(k)


def _check_numbers(key, e, m, cs, loss_kind="l1"):
    """forward losses, every gradient, three Adam steps: what test_wide_hidden_sizes_match_oracle runs, with its bounds"""
    cfg, T, B = cs["cfg"], cs["T"], cs["B"]
    x, y = torch.from_numpy(cs["x"]), torch.from_numpy(cs["y"])
    torch.set_num_threads(4)
    terms = O.loss_terms(m, x, y, cfg, loss_kind)
    terms["loss"].backward()
    xd, yd = x.cuda(), y.cuda()
    out = e.forward(xd, yd, train=True, want_xhat=False)
    ld = e.loss_dict(out["losses"])
    for k in ("disc", "gen", "reg", "loss"):
        ref = float(terms[k].detach())
        print("%s %s: got %.9g ref %.9g" % (key, k, ld[k], ref))
        assert abs(ld[k] - ref) <= TOL * max(abs(ref), 1e-3), (k, ld[k], ref)
    e.backward(xd, yd, stage=0)
    got = {n: v.cpu().numpy() for n, v in e.grad_views().items()}
    named = [(n, None if p.grad is None else p.grad.numpy()) for n, p in m.named_parameters()]
    assert [n for n, _ in named] == list(got)
    worst = PF.worst_grad(named, got)
    print("%s worst gradient: %s %.3e" % (key, worst[0], worst[1]))
    cases.report("plan_form_grad_%s" % key, worst[1])
    assert worst[1] < TOL, "worst gradient mismatch %s: %.3e" % worst
    opt = torch.optim.Adam(m.parameters())
    for _ in range(3):
        opt.zero_grad()
        O.loss_terms(m, x, y, cfg, loss_kind)["loss"].backward()
        opt.step()
        e.train_step(xd, yd)
    pv = e.param_views()
    for n, p in m.named_parameters():
        # the trajectory bound of test_wide_hidden_sizes_match_oracle: a fraction of the 3 * lr the parameters can move at all
        assert np.max(np.abs(pv[n].cpu().numpy() - p.detach().numpy())) < 0.1 * 3e-3, n


def _layer_ks(cfg):
    """reduction lengths of the latent stack's layers that the sizes of group (h) move: the z -> f MLPs, the classifier, and the
    heads on the encoders' last hidden states"""
    z = [cfg["zl_size"], cfg["za_size"], cfg["zv_size"], cfg["zy_size"]]
    f = [cfg["fl_size"], cfg["fa_size"], cfg["fv_size"], cfg["fy_size"]]
    return z + f + [sum(z[:3])]


@pytest.mark.parametrize("name", list(PF.KLEF))
def test_klef_form_matches_oracle(name):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from factorized_amd import engine
    cs = PF.klef_case(name)
    B, T, want = cs["B"], cs["T"], cs["want"]
    e = engine.MFMEngine(cs["cfgs"])
    w = synth.make_weights(e.layout.shapes, seed=PF.WEIGHT_SEED)
    e.load_weights(w)
    # ---- the form, before any number
    cus = _lib.lib().mfm_device_cus()
    form, seq = e.latent_form(T, B), e.seq_form(T, B)
    print(name, form, [(s["h"], s["stepwise"]) for s in seq])
    for k, v in want.items():
        assert form[k] == v, (k, form[k], v, form)
    if name in PF.PANEL:
        assert form["wpanel"] > 0, form
    if name in PF.OFF4_GROUP:
        # what the group is there for: no row path, no MFMA products, and at least one layer the quad kernels must take scalar
        assert not form["row_path"] and not form["mfma"], form
        assert any(k % 4 for k in _layer_ks(cs["cfg"])), name
        assert any(s["h"] % 4 for s in seq if not s["stepwise"]), seq
    if name in PF.OFF4_GROUP:
        assert all(s["mfma"] == (name in PF.SEQ_MFMA) for s in seq if not s["stepwise"]), seq
    assert sorted(s["h"] for s in seq if s["stepwise"]) == sorted(cs["stepwise"]), seq
    assert len(seq) == 7 and all(s["stepwise"] == (s["h"] > 128) for s in seq)
    if "nch" in want:
        assert (4 * B <= cus) == (want["nch"] == 4), (B, cus)          # the sizes of the matrix assume 256 compute units
    if want.get("split0"):
        assert B > 1024 and B > 4 * cus, (B, cus)                      # sixteen rows nominal, split0 by the batch
    if not form["row_path"]:
        assert (form["rows_per_wg"], form["rows_fwd"]) == PF.expected_rows(B, form["rec_size"], form["wpanel"], cus), form
    assert e.latent_record(T, B)[2]["row_path"] == form["row_path"]
    # ---- the numbers
    m = O.build("kl_ef", cs["cfgs"])
    O.load_numpy_weights(m, w)
    m.train()
    _check_numbers(name, e, m, cs, cs["loss_kind"])


def test_output_dim_65_is_refused_at_plan_creation():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from factorized_amd import engine
    cfgs = configs.canonical_configs(dropout=False, output_dim=65)
    e = engine.MFMEngine(cfgs)
    w = synth.make_weights(e.layout.shapes, seed=PF.WEIGHT_SEED)
    e.load_weights(w)
    before = e.params.clone()
    xn, yn = synth.make_batch(cfgs[0]["input_dims"], 5, 2, seed=PF.BATCH_SEED, output_dim=65)
    x, y = torch.from_numpy(xn).cuda(), torch.from_numpy(yn).cuda()
    for call in (lambda: e.forward(x, y, train=True), lambda: e.train_step(x, y), lambda: e.latent_form(2, 5)):
        with pytest.raises(_lib.MfmError, match="plan: output_dim 65"):
            call()
    torch.cuda.synchronize()
    # no plan, so nothing to launch on: parameters, gradients and the step counter are untouched
    assert not e._plans and e.step_count == 0
    assert torch.equal(e.params, before) and not e.grads.any()


@pytest.mark.parametrize("name", list(PF.MFN_RESIDENT))
def test_mfn_resident_limit_matches_oracle(name):
    """MFM_KL with MFN LSTMs at the resident limit (h = 128): cStar rows of 768 columns (twelve per lane in the attention
    softmax) and one 128-wide LSTM beside two of 4, through test_gpu_mfn_plan's engine / oracle helpers."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from tests.test_gpu_mfn_plan import _engine, _oracle
    cs = PF.mfn_case(name)
    B, T, hd = cs["B"], cs["T"], cs["cfg"]["h_dims"]
    e, w = _engine(cs["cfgs"], "kl")
    form, seq = e.latent_form(T, B), e.seq_form(T, B)
    print(name, form, [(s["h"], s["stepwise"]) for s in seq])
    assert len(seq) == 9 and [s["h"] for s in seq[3:6]] == hd
    assert not any(s["stepwise"] for s in seq), seq
    assert form["row_path"] and form["nch"] == (4 if 4 * B <= _lib.lib().mfm_device_cus() else 1), form
    assert e.mfn_buffers(T, B)["cstar"].shape == (T * B, 2 * sum(hd))
    _check_numbers(name, e, _oracle("kl", cs["cfgs"], w), cs)


@pytest.mark.parametrize("variant", ["kl", "mmd"])
@pytest.mark.parametrize("name", list(PF.MFN_OFF4_GROUP))
def test_mfn_off4_matches_oracle(name, variant):
    """MFM_KL and MFM with every width off the multiple of 4: OFF4's latents and factors, MFN LSTMs of 37, 5 and 18, a memory of 21
    and attention nets of 35, 19, 27 and 43 (mfn_att.hip, mfn_mem.hip and the staged latent kernels' scalar branch in one plan).
    MFM's Gaussian sample is injected on both sides, as test_gpu_mfn_plan does."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from tests.test_gpu_mfn_plan import _engine, _oracle
    cs = PF.mfn_case(name)
    cfg, B, T = cs["cfg"], cs["B"], cs["T"]
    e, w = _engine(cs["cfgs"], variant)
    gauss = None
    if variant == "mmd":
        gl = cfg["zl_size"] + cfg["za_size"] + cfg["zv_size"] + cfg["zy_size"]
        gauss = torch.from_numpy(np.random.RandomState(5).normal(size=(B, gl)).astype(np.float32))
        e.gauss = gauss.cuda()
    form, seq = e.latent_form(T, B), e.seq_form(T, B)
    print(name, variant, form, [(s["h"], s["stepwise"]) for s in seq])
    assert not form["row_path"] and not form["mfma"] and form["wpanel"] > 0, form
    assert len(seq) == 9 and [s["h"] for s in seq] == [18, 7, 33, 37, 5, 18, 37, 15, 30], seq
    assert not any(s["stepwise"] for s in seq), seq
    bufs = e.mfn_buffers(T, B)
    assert bufs["cstar"].shape == (T * B, 2 * sum(cfg["h_dims"])) and bufs["chat"].shape == (T * B, 21)
    assert (bufs["h1"].shape[1], bufs["h2"].shape[1]) == (35, 19)
    _check_numbers("%s_%s" % (name, variant), e, _oracle(variant, cs["cfgs"], w, gauss), cs)
