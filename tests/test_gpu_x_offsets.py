"""The fused plans, the no-plan inference entries and the granular module path on tensors that start 4, 8 and 12 bytes past a
16-byte boundary (tests/offset_views.py).  The
package promises "a contiguous float32 CUDA tensor [T, B, D]" (engine._check_inputs) and nothing about where it starts:
DeviceDataset.batch(i) of an [nb, T, B, 325] dataset, a time crop x[k:] and a view of a staging buffer all start off 16 bytes,
while every other GPU test feeds freshly allocated tensors, which the allocator puts on 256.

Each case runs the same call on at_residue(x, r) for r = 4, 8, 12 and holds it to the reference and the bound that the aligned
test of that path uses: the oracle in FLOAT64 at the project's 1e-4 (tests/test_gpu_data_regimes.py), the bf16 rule of
tests/test_gpu_bf16.py for bf16 plans -- never the aligned GPU run.  The largest difference from the r = 0 run is printed and
recorded as a diagnostic only (a kernel may legitimately order its sums by address).  The sentinels around every view are
checked after the calls.  Values: the `mixed` regime of tests/data_regimes.py (modality scales 1 / 50 / 0.02; the bf16 plans
and the CE configuration: synth.make_batch as their aligned tests draw it), at the sizes
where the plan changes kernel form (tests/plan_forms.py), with T * B * D odd wherever B allows it.

Adam trajectories are held to the rule of tests/test_gpu_plan.py: Adam normalises by sqrt(v), so an element whose gradient is
~0 moves by up to lr per step whatever the rounding says; the bound is a tenth of the steps x lr a parameter can move at all.
Numbers evaluated BETWEEN training steps are compared with the float64 oracle holding the parameters the engine has at that
moment, so that 1e-4 measures the evaluation on the offset view and not the drift of the trajectory."""
import copy
import os

import numpy as np
import pytest
import torch

from factorized_amd import configs, synth
from tests import cases
from tests import data_regimes as DR
from tests import zeros_ref
from tests.cases import grad_err, rel_err
from tests.offset_views import at_residue, check_guards, forget_views, residue

pytestmark = pytest.mark.gpu
TOL = 1e-4
RES = (4, 8, 12)
REGIME = "mixed"
LR = 1e-3
# role workgroups (B <= 32), one workgroup per row, the MFMA recurrences (B > 512); T * B * 325 odd but for B = 32
FORMS = {"roles5": (5, 5), "roles32": (32, 5), "rows": (65, 3), "mfma": (513, 3)}
_REF = {}


@pytest.fixture(autouse=True)
def no_form_switches(monkeypatch):
    """a stray switch must not choose the form"""
    for k in list(os.environ):
        if k.startswith(("MFM_LATENT_", "MFM_SEQ_", "MFM_BF16_", "MFM_DW_", "MFM_GEMM_", "MFM_PROJ_")):
            monkeypatch.delenv(k)


@pytest.fixture(autouse=True)
def fresh_views():
    """a test that failed before its check_guards() must not leave its views to the next test's count"""
    forget_views()
    yield
    forget_views()


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _engine(variant="kl_ef", precision="fp32"):
    from factorized_amd import engine
    cfgs = DR.canonical()
    e = engine.MFMEngine(cfgs, variant=variant, precision=precision)
    w = synth.make_weights(e.layout.shapes, seed=DR.WEIGHT_SEED)
    e.load_weights(w)
    return e, w, cfgs


def _gauss(cfg, B):
    n = sum(cfg[k] for k in ("zl_size", "za_size", "zv_size", "zy_size"))
    return torch.from_numpy(np.random.RandomState(99).normal(size=(B, n)).astype(np.float32))


def _split_gauss(cfg, g):
    return list(torch.split(g, [cfg[k] for k in ("zl_size", "za_size", "zv_size", "zy_size")], dim=1))


def _unit_batch(B, T, w, cfgs):
    """synth.make_batch as it is, at the first seed from BATCH_SEED on where the reference has a classifier-bias gradient at
    all.  With the L1 loss that gradient is (number of positive residuals - number of negative ones) / B; at B = 160, seed 7,
    the fp32 oracle has 80 of each and the "gradient" is 2e-9 of rounding noise, against which no relative measure exists
    (tests.cases.grad_err says the same of such biases).  Decided on the oracle alone."""
    from oracle import mfm_oracle as O
    for seed in range(DR.BATCH_SEED, DR.BATCH_SEED + 8):
        x, y = synth.make_batch(DR.DIMS, B, T, seed=seed)
        m = O.build("kl_ef", cfgs)
        O.load_numpy_weights(m, w)
        m.eval()
        with torch.no_grad():
            d = m.forward(torch.from_numpy(x))[0][3].squeeze(1) - torch.from_numpy(y)
        if abs(int((d > 0).sum()) - int((d < 0).sum())) >= 2:
            return x, y
    raise AssertionError("no unit batch with an uncancelled label residual")


def _ref(variant, B, T, w, cfgs, steps=0, regime=REGIME):
    """the float64 oracle's step on (variant, B, T) and, `steps` > 0, its parameters after that many Adam steps on the same
    batch: computed once, shared, left unchanged.  regime None: synth.make_batch as it is (unit-scale noise)"""
    key = (variant, B, T, regime)
    if key not in _REF:
        torch.set_num_threads(4)
        x, y = DR.make(regime, B, T) if regime else _unit_batch(B, T, w, cfgs)
        gauss = _split_gauss(cfgs[0], _gauss(cfgs[0], B)) if variant == "mmd" else None
        m, terms = DR.oracle64(variant, cfgs, w, x, y, gauss)
        _REF[key] = dict(x=x, y=y, losses={k: float(terms[k].detach()) for k in DR.LOSS_KEYS},
                         grads=[(n, None if p.grad is None else p.grad.numpy().copy()) for n, p in m.named_parameters()])
    r = _REF[key]
    if steps and r.get("steps") != steps:
        from oracle import mfm_oracle as O
        torch.set_num_threads(4)
        m = O.build(variant, cfgs)
        O.load_numpy_weights(m, w)
        m = copy.deepcopy(m).double()
        m.train()
        opt = torch.optim.Adam(m.parameters(), lr=LR)
        x64, y64 = torch.from_numpy(r["x"]).double(), torch.from_numpy(r["y"]).double()
        for _ in range(steps):
            O.train_step(m, opt, x64, y64, cfgs[0])
        r["steps"], r["params"] = steps, {n: p.detach().numpy().copy() for n, p in m.named_parameters()}
    return r


def _step_errors(ref, ld, got):
    """(worst loss term, worst gradient) against float64, each (name, error)"""
    worst_l = max(((k, DR.loss_rel(ld[k], ref["losses"][k])) for k in DR.LOSS_KEYS), key=lambda kv: kv[1])
    assert [n for n, _ in ref["grads"]] == list(got)
    worst_g = ("", 0.0)
    for n, r in ref["grads"]:
        assert np.all(np.isfinite(got[n])), n
        if r is None:
            assert np.all(got[n] == 0.0), n
            continue
        d = grad_err(got[n], r)
        if d >= worst_g[1]:
            worst_g = (n, d)
    return worst_l, worst_g


def _grad_step(e, x, y):
    ld = e.loss_dict(e.grad_step(x, y))
    torch.cuda.synchronize()
    return ld, {n: v.cpu().numpy().copy() for n, v in e.grad_views().items()}


def _vs_aligned(got, base):
    """largest difference between two runs' gradients, relative to each tensor's own max: the diagnostic, never asserted"""
    return max(rel_err(got[n], base[n]) for n in got if np.abs(base[n]).max() > 0)


def _check_grad_steps(tag, e, ref):
    """grad_step on x at residues 0, 4, 8, 12 (labels at 0, 4, 8, 12 as well): every loss slot and every gradient against
    float64 at TOL; prints and records both figures per residue"""
    base = None
    for r in (0,) + RES:
        x, y = at_residue(ref["x"], r), at_residue(ref["y"], r)
        assert residue(x) == r and x.is_contiguous()
        ld, got = _grad_step(e, x, y)
        for k in DR.LOSS_KEYS:
            assert np.isfinite(ld[k]), (tag, r, k)
        worst_l, worst_g = _step_errors(ref, ld, got)
        base = got if r == 0 else base
        diff = _vs_aligned(got, base)
        print("%s r%-2d worst loss term: %s %.3e   worst gradient: %s %.3e   against r0: %.3e" % ((tag, r) + worst_l + worst_g + (diff,)))
        cases.report("x_offsets_loss_%s_r%d" % (tag, r), worst_l[1])
        cases.report("x_offsets_grad_%s_r%d" % (tag, r), worst_g[1])
        cases.report("x_offsets_vs_r0_%s_r%d" % (tag, r), diff)
        assert worst_l[1] <= TOL, (tag, r) + worst_l
        assert worst_g[1] < TOL, (tag, r) + worst_g
        assert e.check_status() == 0


# ----------------------------------------------------------------------------------- the fused fp32 step, MFM_KL_EF
@pytest.mark.parametrize("handover", [True, False], ids=["handover", "launches"])
@pytest.mark.parametrize("form", list(FORMS))
def test_klef_step_on_offset_batches(form, handover):
    _need_gpu()
    B, T = FORMS[form]
    e, w, cfgs = _engine()
    e.set_handover(handover)
    ref = _ref("kl_ef", B, T, w, cfgs, steps=3)
    tag = "%s_%s_b%d_t%d" % (form, "ho" if handover else "nh", B, T)
    _check_grad_steps(tag, e, ref)
    lat, seq = e.latent_form(T, B), e.seq_form(T, B)
    roles = e.plan(T, B).get_option("proj_roles_active")
    print(tag, "proj_roles_active", roles, lat, [(s["h"], s["mfma"]) for s in seq])
    if form.startswith("roles"):
        assert roles == (1 if handover else 0) and not any(s["mfma"] for s in seq)
    elif form == "rows":
        assert roles == 0 and lat["row_path"] and not any(s["mfma"] for s in seq)
    else:
        assert roles == 0 and all(s["mfma"] for s in seq)
    # three Adam steps, one on each residue, against three float64 Adam steps on the same values
    for r in RES:
        e.train_step(at_residue(ref["x"], r), at_residue(ref["y"], r), lr=LR)
    torch.cuda.synchronize()
    pv = e.param_views()
    worst = max(((n, float(np.abs(pv[n].cpu().numpy() - p).max())) for n, p in ref["params"].items()), key=lambda kv: kv[1])
    print("%s three train_steps, worst parameter: %s %.3e (bound %.1e)" % ((tag,) + worst + (0.1 * 3 * LR,)))
    cases.report("x_offsets_params_%s" % tag, worst[1])
    assert worst[1] < 0.1 * 3 * LR, worst
    assert e.check_status() == 0
    assert check_guards() == 14


@pytest.mark.parametrize("variant", ["kl", "mmd"])
def test_mfn_variants_on_offset_batches(variant):
    _need_gpu()
    B, T = 19, 5
    e, w, cfgs = _engine(variant)
    if variant == "mmd":
        e.gauss = _gauss(cfgs[0], B).cuda()
    _check_grad_steps("%s_b%d_t%d" % (variant, B, T), e, _ref(variant, B, T, w, cfgs))
    assert check_guards() == 8


def test_fp32_one_pass_weight_gradients_on_offset_batches(monkeypatch):
    """MFM_DW_F32_MINROWS=1 (the switch of tests/test_gpu_large_batch.py, variant dwf32): the LSTMs' weight gradients on
    dw_stream_kernel<true>, whose source addresses -- x itself, row stride 325 -- go into an LDS-DMA instruction"""
    _need_gpu()
    monkeypatch.setenv("MFM_DW_F32_MINROWS", "1")
    B, T = FORMS["rows"]
    e, w, cfgs = _engine()
    _check_grad_steps("dwf32_b%d_t%d" % (B, T), e, _ref("kl_ef", B, T, w, cfgs))
    # the four encoders (x is their right-hand side) and the three decoders: none fell back to the GEMMs
    assert e.plan(T, B).get_option("dw_f32_items") == 7
    assert check_guards() == 8
    monkeypatch.delenv("MFM_DW_F32_MINROWS")
    e2, _, _ = _engine()                                         # (and the option tells the two forms apart)
    ref = _ref("kl_ef", B, T, w, cfgs)
    _grad_step(e2, at_residue(ref["x"], 4), at_residue(ref["y"], 4))
    assert e2.plan(T, B).get_option("dw_f32_items") == 0
    assert check_guards() == 2


# ----------------------------------------------------------------------------------- bf16 plans
@pytest.mark.parametrize("B,T", [(32, 5), (128, 20), (160, 20)])
def test_bf16_plan_on_offset_batches(B, T):
    """B = 32: the projections stay fp32 below 128; B = 128 and 160: bf16-resident (x_to_bf16 or proj_bf16's pack of x, dw_bf16
    on the packed image).  The rule of tests/test_gpu_bf16.py: loss terms within 1e-3 of float64, every gradient within
    2 cond(n) + 1.5e-2 in relative L2 with the hard cap 0.2 -- on the batch that rule is stated for, synth.make_batch as it is:
    the 1.5e-2 beside the emulated conditioning is that test's allowance on unit-scale data (_unit_batch: seed 7 but at
    (160, 20), where seed 7 leaves the reference no classifier-bias gradient to compare with).  (On the `mixed` regime the
    ALIGNED run at (160, 20) has zy_to_fy_fc2.weight at 4.9e-2 against a bound of 4.3e-2, residue 0 included: a known limit
    of bf16 plans on mixed scales at that size, DESIGN.md section 5, not a matter of where x starts.)"""
    _need_gpu()
    from tests.test_gpu_bf16 import _check_bf16_gradients, _conditioning
    e, w, cfgs = _engine(precision="bf16")
    cfg = cfgs[0]
    ref = _ref("kl_ef", B, T, w, cfgs, regime=None)
    torch.set_num_threads(4)
    cond, g32 = _conditioning(cfgs, w, torch.from_numpy(ref["x"]), torch.from_numpy(ref["y"]), cfg, "l1")
    base = None
    for r in (0,) + RES:
        ld, got = _grad_step(e, at_residue(ref["x"], r), at_residue(ref["y"], r))
        assert e.seq_buffers(T, B, 3)["bf16_resident"] == (B >= 128)
        assert all(np.isfinite(ld[k]) for k in DR.LOSS_KEYS) and all(np.all(np.isfinite(g)) for g in got.values())
        worst_l = max((DR.loss_rel(ld[k], ref["losses"][k]), k) for k in DR.LOSS_KEYS)
        base = got if r == 0 else base
        tag = "bf16_b%d_t%d_r%d" % (B, T, r)
        print("%s worst loss term: %s %.3e   against r0: %.3e" % (tag, worst_l[1], worst_l[0], _vs_aligned(got, base)))
        cases.report("x_offsets_loss_%s" % tag, worst_l[0])
        cases.report("x_offsets_vs_r0_%s" % tag, _vs_aligned(got, base))
        assert worst_l[0] < 1e-3, (r,) + worst_l
        worst_g, _, _, worst_ratio = _check_bf16_gradients(e.grad_views(), g32, cond, "x_offsets_" + tag)
        print("%s worst gradient (relative L2): %s %.3e   against its bound: %s %.2f" % ((tag,) + worst_g + worst_ratio))
        assert e.check_status() == 0
    assert check_guards() == 8


# ----------------------------------------------------------------------------------- the no-plan inference entries
def _model(cfgs, cls="MFM_KL_EF"):
    from factorized_amd import mfm_model as M
    model = getattr(M, cls)(*cfgs)
    w = synth.make_weights({k: tuple(v.shape) for k, v in model.state_dict().items()}, seed=DR.WEIGHT_SEED)
    model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in w.items()})
    return model.to("cuda"), w


def _eval64(cfgs, w, variant="kl_ef"):
    from oracle import mfm_oracle as O
    m = O.build(variant, cfgs)
    O.load_numpy_weights(m, w)
    return copy.deepcopy(m).double().eval()


def _infer_refs(cfgs, w, x, y, T):
    """float64: the eval forward's terms, the latents, decode of the latents as fp32 holds them, the zeroed protocol"""
    from oracle import mfm_oracle as O
    from tests.test_gpu_generate import _oracle_decode, _oracle_encode
    torch.set_num_threads(4)
    m = _eval64(cfgs, w)
    x64 = torch.from_numpy(x).double()
    with torch.no_grad():
        terms = O.loss_terms(m, x64, torch.from_numpy(y).double(), cfgs[0])
    z_ref = _oracle_encode(m, x64)
    z32 = [z.float() for z in z_ref[:4]]
    dec_ref = _oracle_decode(m, *[z.double() for z in z32], T)
    zr = zeros_ref.oracle_zeros("kl_ef", cfgs, w, x, y, double=True)
    return terms, z_ref, z32, dec_ref, zr


def _infer_errors(e, xd, yd, z, T, max_rows, refs):
    """predict with and without labels, encode, decode, objective, predict_zeros on the engine's entries ->
    ({name: error against float64}, {name: the output itself as a numpy array})"""
    terms, z_ref, _, dec_ref, zr = refs
    kw = {} if max_rows is None else dict(max_rows=max_rows)
    errs, outs = {}, {}
    outs["predict.y_hat"] = e.predict(xd, **kw)["y_hat"].cpu().numpy()
    errs["predict.y_hat"] = rel_err(outs["predict.y_hat"], terms["decoded"][3].numpy())
    out = e.predict(xd, yd, **kw)
    outs["predict_y.y_hat"], outs["evaluate"] = out["y_hat"].cpu().numpy(), out["loss"].cpu().numpy().reshape(1)
    errs["predict_y.y_hat"] = rel_err(outs["predict_y.y_hat"], terms["decoded"][3].numpy())
    errs["evaluate"] = DR.loss_rel(float(out["loss"]), terms["disc"])
    enc = e.encode(xd, **kw)
    for name, g, r in zip(type(enc)._fields, enc, z_ref):
        outs["encode." + name] = g.cpu().numpy()
        errs["encode." + name] = rel_err(outs["encode." + name], r.numpy())
    for name, g, r in zip(("x_l_hat", "x_a_hat", "x_v_hat", "y_hat"), e.decode(*z, T, **kw), dec_ref):
        outs["decode." + name] = g.cpu().numpy()
        errs["decode." + name] = rel_err(outs["decode." + name], r.numpy())
    obj = e.objective(xd, yd, **kw)
    outs["objective"] = np.array([float(g) for g in obj])
    for name, g in zip(("loss", "disc", "gen_l", "gen_a", "gen_v", "reg"), obj):
        errs["objective." + name] = DR.loss_rel(float(g), terms[name])
    zs = [t.cpu().numpy() for t in e.predict_zeros(xd, yd, **kw)]
    outs["zeros.y_hat"], outs["zeros.gen"], outs["zeros.disc"] = zs
    errs["zeros.y_hat"] = max(rel_err(zs[0][c], zr["y_hat"][c]) for c in range(3))
    for c in range(3):
        errs["zeros.gen[%d]" % c] = DR.loss_rel(zs[1][c], zr["gen"][c])
        errs["zeros.disc[%d]" % c] = DR.loss_rel(zs[2][c], zr["disc"][c])
    assert all(np.isfinite(v) for v in errs.values()), errs
    return errs, outs


@pytest.mark.parametrize("max_rows", [None, 16], ids=["one_chunk", "rows16"])
def test_inference_entries_on_offset_splits(max_rows):
    """N = 37: one chunk, and chunks of 16, 16 and a 5-row tail.  x at residue r, float labels at residue 4, the four factors of
    decode each at a residue of its own"""
    _need_gpu()
    N, T = 37, 5
    model, w = _model(DR.canonical())
    cfgs = DR.canonical()
    e = model.engine
    x, y = DR.make(REGIME, N, T)
    refs = _infer_refs(cfgs, w, x, y, T)
    zres = (4, 8, 12, 4)
    base = None
    for r in (0,) + RES:
        xd, yd = at_residue(x, r), at_residue(y, 4 if r else 0)
        z = [at_residue(t, zres[(i + r // 4) % 4] if r else 0) for i, t in enumerate(refs[2])]
        assert residue(xd) == r and residue(yd) == (4 if r else 0)
        errs, outs = _infer_errors(e, xd, yd, z, T, max_rows, refs)
        base = outs if r == 0 else base
        worst = max(errs, key=errs.get)
        diff = max(rel_err(outs[k], base[k]) for k in outs)      # the outputs themselves against the r = 0 run's
        tag = "infer_rows%s_r%d" % (max_rows, r)
        print("%s worst: %s %.3e   outputs against r0: %.3e" % (tag, worst, errs[worst], diff))
        print("%s all: %s" % (tag, " ".join("%s %.2e" % kv for kv in errs.items())))
        cases.report("x_offsets_%s" % tag, errs[worst])
        cases.report("x_offsets_vs_r0_%s" % tag, diff)
        for k, v in errs.items():
            assert v <= TOL, (tag, k, v)
    assert not e._plans                                         # no plan: the entries under test, not the eval forward
    assert check_guards() == 4 * 6


@pytest.mark.parametrize("max_rows", [None, 16], ids=["one_chunk", "rows16"])
def test_predict_cross_entropy_on_offset_splits(max_rows):
    """the CE configuration (three classes): x at residue r, the int64 labels at residue 8"""
    _need_gpu()
    from oracle import mfm_oracle as O
    N, T = 37, 5
    cfgs = configs.you_configs(dropout=False)
    cfg = cfgs[0]
    assert cfg.get("loss") == "ce"
    model, w = _model(cfgs)
    e = model.engine
    x, y = synth.make_batch(cfg["input_dims"], N, T, seed=DR.BATCH_SEED, output_dim=cfg["output_dim"], classes=cfg["output_dim"])
    torch.set_num_threads(4)
    m = _eval64(cfgs, w)
    with torch.no_grad():
        terms = O.loss_terms(m, torch.from_numpy(x).double(), torch.from_numpy(y), cfg, "ce")
    kw = {} if max_rows is None else dict(max_rows=max_rows)
    for r in (0,) + RES:
        xd, yd = at_residue(x, r), at_residue(y, 8 if r else 0)
        assert yd.dtype == torch.int64 and residue(yd) == (8 if r else 0)
        plain = rel_err(e.predict(xd, **kw)["y_hat"].cpu().numpy(), terms["decoded"][3].numpy())
        out = e.predict(xd, yd, **kw)
        errs = (plain, rel_err(out["y_hat"].cpu().numpy(), terms["decoded"][3].numpy()), DR.loss_rel(float(out["loss"]), terms["disc"]))
        print("predict_ce_rows%s_r%d y_hat %.3e  with labels %.3e  loss %.3e" % ((max_rows, r) + errs))
        cases.report("x_offsets_predict_ce_rows%s_r%d" % (max_rows, r), max(errs))
        assert max(errs) <= TOL, (r, errs)
    assert not e._plans
    assert check_guards() == 8


def test_impute_each_on_offset_splits():
    """MFM_missing.impute("each"), whose entry has asked x for 4 bytes from the start (tests/test_impute_host.py)"""
    _need_gpu()
    from tests.test_gpu_impute import MS, _case, _keep, _oracle_impute
    s = _case("small")
    T, N = 4, 5
    xn, _ = synth.make_batch(s["cfg"]["input_dims"], N, T, seed=33)
    want = {m: _oracle_impute(s["ref"], torch.from_numpy(xn), m) for m in MS}
    for r in (0,) + RES:
        each = _keep(s["model"].impute(at_residue(xn, r), "each"))
        errs = {m + part: rel_err(g.cpu().numpy(), w_.numpy()) for m in MS for g, w_, part in zip(each[m], want[m], (".x_hat", ".y_hat"))}
        worst = max(errs, key=errs.get)
        print("impute_each_r%d worst: %s %.3e" % (r, worst, errs[worst]))
        cases.report("x_offsets_impute_each_r%d" % r, errs[worst])
        assert errs[worst] < TOL, (r, worst, errs[worst])
    assert check_guards() == 4


# ----------------------------------------------------------------------------------- dataset views, end to end
def _oracle_at(cfgs, state):
    """the float64 oracle in eval mode holding the parameters of `state` (a state_dict of device tensors)"""
    return _eval64(cfgs, {k: v.detach().cpu().numpy() for k, v in state.items()})


def _epoch(tag, model, cfgs, ds, m64, opt):
    """one epoch of train_step over ds.batches(); after each step evaluate and objective on the NEXT batch view, against the
    float64 oracle at the model's parameters of that moment; the oracle m64 takes the same Adam steps"""
    from oracle import mfm_oracle as O
    e, cfg = model.engine, cfgs[0]
    worst = 0.0
    for i, (xb, yb) in enumerate(ds.batches()):
        e.train_step(xb, yb, lr=LR)
        O.train_step(m64, opt, xb.cpu().double(), yb.cpu().double(), cfg)
        xn, yn = ds.batch((i + 1) % ds.nb)
        ev = float(model.evaluate(xn, yn))
        obj = [float(v) for v in model.objective(xn, yn)]
        now = _oracle_at(cfgs, model.state_dict())
        with torch.no_grad():
            terms = O.loss_terms(now, xn.cpu().double(), yn.cpu().double(), cfg)
        errs = {"evaluate": DR.loss_rel(ev, terms["disc"])}
        for name, g in zip(("loss", "disc", "gen_l", "gen_a", "gen_v", "reg"), obj):
            errs["objective." + name] = DR.loss_rel(g, terms[name])
        k = max(errs, key=errs.get)
        print("%s step %d (batch at residue %d, evaluated at %d) worst: %s %.3e" % (tag, i, residue(xb), residue(xn), k, errs[k]))
        worst = max(worst, errs[k])
        assert errs[k] <= TOL, (tag, i, k, errs[k])
    torch.cuda.synchronize()
    assert e.check_status() == 0
    return worst


def test_dataset_views_end_to_end():
    """DeviceDataset.from_arrays with T = 7, B = 33, nb = 4 on D = 325: a batch is 75075 floats, so batches 1, 2 and 3 start 12,
    8 and 4 bytes past a boundary.  One epoch, then another after reshuffle(seed=1) of the pooled dataset"""
    _need_gpu()
    from factorized_amd import train
    from oracle import mfm_oracle as O
    T, B, nb = 7, 33, 4
    cfgs = DR.canonical()
    X, y = DR.make(REGIME, B * nb, T)
    ds = train.DeviceDataset.from_arrays(X, y, B, "cuda", pool=True)
    assert ds.nb == nb and [residue(ds.batch(i)[0]) for i in range(nb)] == [0, 12, 8, 4]
    assert all(ds.batch(i)[0].is_contiguous() for i in range(nb))
    model, w = _model(cfgs)
    torch.set_num_threads(4)
    m64 = O.build("kl_ef", cfgs)
    O.load_numpy_weights(m64, w)
    m64 = copy.deepcopy(m64).double()
    m64.train()
    opt = torch.optim.Adam(m64.parameters(), lr=LR)
    steps = 0
    for tag in ("dataset_epoch0", "dataset_reshuffled"):
        if steps:
            ds.reshuffle(seed=1)
            assert [residue(ds.batch(i)[0]) for i in range(nb)] == [0, 12, 8, 4]
        worst = _epoch(tag, model, cfgs, ds, m64, opt)
        steps += nb
        sd = model.state_dict()
        wp = max(((n, float(np.abs(sd[n].cpu().numpy() - p.detach().numpy()).max())) for n, p in m64.named_parameters()),
                 key=lambda kv: kv[1])
        print("%s worst evaluated number %.3e   worst parameter after %d steps: %s %.3e (bound %.1e)" % (
            (tag, worst, steps) + wp + (0.1 * steps * LR,)))
        cases.report("x_offsets_%s_eval" % tag, worst)
        cases.report("x_offsets_%s_params" % tag, wp[1])
        assert wp[1] < 0.1 * steps * LR, wp


def test_time_crop_of_a_validation_split():
    """x[1:] of a [T + 1, 229, 325] split starts 229 x 325 floats in: residue 4"""
    _need_gpu()
    from oracle import mfm_oracle as O
    N, T = 229, 3
    cfgs = DR.canonical()
    model, w = _model(cfgs)
    x, y = DR.make(REGIME, N, T + 1)
    big, yd = at_residue(x, 0), at_residue(y, 0)
    xc = big[1:]
    assert xc.is_contiguous() and residue(xc) == 4
    torch.set_num_threads(4)
    m = _eval64(cfgs, w)
    with torch.no_grad():
        terms = O.loss_terms(m, torch.from_numpy(x[1:]).double(), torch.from_numpy(y).double(), cfgs[0])
    zr = zeros_ref.oracle_zeros("kl_ef", cfgs, w, np.ascontiguousarray(x[1:]), y, double=True)
    errs = {"evaluate": DR.loss_rel(float(model.evaluate(xc, yd)), terms["disc"])}
    zs = [t.cpu().numpy() for t in model.predict_zeros(xc, yd)]
    errs["zeros.y_hat"] = max(rel_err(zs[0][c], zr["y_hat"][c]) for c in range(3))
    for c in range(3):
        errs["zeros.gen[%d]" % c] = DR.loss_rel(zs[1][c], zr["gen"][c])
        errs["zeros.disc[%d]" % c] = DR.loss_rel(zs[2][c], zr["disc"][c])
    print("time_crop all: %s" % " ".join("%s %.2e" % kv for kv in errs.items()))
    cases.report("x_offsets_time_crop", max(errs.values()))
    for k, v in errs.items():
        assert v <= TOL, (k, v)
    assert not model.engine._plans
    assert check_guards() == 2


# ----------------------------------------------------------------------------------- the granular module path
def _grads64(out, dy, tensors):
    out.backward(torch.from_numpy(dy).double())
    return [t.grad.numpy() for t in tensors]


def _module_errors(tag, got, want, names):
    errs = {n: rel_err(g.detach().cpu().numpy(), w_) for n, g, w_ in zip(names, got, want)}
    worst = max(errs, key=errs.get)
    print("%s worst: %s %.3e   all: %s" % (tag, worst, errs[worst], " ".join("%s %.2e" % kv for kv in errs.items())))
    cases.report("x_offsets_%s" % tag, errs[worst])
    for k, v in errs.items():
        assert v < TOL, (tag, k, v)


@pytest.mark.parametrize("h,d,B,T", [(32, 37, 5, 3), (120, 325, 33, 7)])
def test_encoder_module_on_offset_input_and_gradient(h, d, B, T):
    """encoderLSTM forward and backward with x at residue 4 and the upstream gradient at residue 12: _ops.py hands both to the
    projection / weight-gradient GEMMs as they are (.contiguous() does not realign).  Reference: the float64 recurrence of
    tests/test_gpu_ops.py with fc1 behind its last hidden state"""
    _need_gpu()
    from factorized_amd import mfm_model as M
    from tests.test_gpu_ops import _cpu_lstm
    torch.manual_seed(h + B)
    mod = M.encoderLSTM(d, h)
    p = [mod.lstm.weight_ih, mod.lstm.weight_hh, mod.lstm.bias_ih, mod.lstm.bias_hh, mod.fc1.weight, mod.fc1.bias]
    pn = [t.detach().numpy().copy() for t in p]
    rs = np.random.RandomState(h + d)
    x = rs.normal(size=(T, B, d)).astype(np.float32)
    dy = rs.normal(size=(B, h)).astype(np.float32)
    # ---- float64
    x64 = torch.from_numpy(x).double().requires_grad_(True)
    cell = torch.nn.LSTMCell(d, h).double()
    fc = torch.nn.Linear(h, h).double()
    with torch.no_grad():
        for dst, src in zip(list(cell.parameters()) + list(fc.parameters()), pn):
            dst.copy_(torch.from_numpy(src).double())
    hx, cx = torch.zeros(B, h, dtype=torch.float64), torch.zeros(B, h, dtype=torch.float64)
    for t in range(T):
        hx, cx = cell(x64[t], (hx, cx))
    ref = fc(hx)
    want = [ref.detach().numpy()] + _grads64(ref, dy, [x64] + list(cell.parameters()) + list(fc.parameters()))
    # (the helper agrees with the recurrence this restates)
    assert rel_err(hx.detach().numpy(), _cpu_lstm(x, *pn[:4], double=True)[2][-1].detach().numpy()) < 1e-12
    # ---- HIP
    mod = mod.cuda()
    p = [mod.lstm.weight_ih, mod.lstm.weight_hh, mod.lstm.bias_ih, mod.lstm.bias_hh, mod.fc1.weight, mod.fc1.bias]
    xd = at_residue(x, 4).requires_grad_(True)
    gd = at_residue(dy, 12)
    assert residue(xd) == 4 and residue(gd) == 12
    out = mod(xd)
    grads = torch.autograd.grad(out, [xd] + p, grad_outputs=gd)
    _module_errors("module_encoder_h%d_d%d_b%d_t%d" % (h, d, B, T), [out] + list(grads), want,
                   ["out", "dx", "weight_ih", "weight_hh", "bias_ih", "bias_hh", "fc1.weight", "fc1.bias"])
    assert check_guards() == 2


@pytest.mark.parametrize("h,d,B,T", [(24, 5, 5, 3), (104, 300, 33, 7)])
def test_decoder_module_on_offset_input_and_gradient(h, d, B, T):
    """decoderLSTM forward and backward with the initial state at residue 4 (read by the recurrence as h_init and by the
    step-0 weight-gradient GEMM) and the upstream gradient [T, B, d] at residue 12"""
    _need_gpu()
    from factorized_amd import mfm_model as M
    torch.manual_seed(h + B)
    mod = M.decoderLSTM(h, d)
    pn = [t.detach().numpy().copy() for t in (mod.lstm.weight_ih, mod.lstm.weight_hh, mod.lstm.bias_ih, mod.lstm.bias_hh,
                                              mod.fc1.weight, mod.fc1.bias)]
    rs = np.random.RandomState(h + d)
    init = rs.normal(size=(B, h)).astype(np.float32)
    dy = rs.normal(size=(T, B, d)).astype(np.float32)
    # ---- float64 (reference semantics mfm_model.py:72-88: step 0 takes the embedding, later steps feed h back)
    i64 = torch.from_numpy(init).double().requires_grad_(True)
    cell = torch.nn.LSTMCell(h, h).double()
    fc = torch.nn.Linear(h, d).double()
    with torch.no_grad():
        for dst, src in zip(list(cell.parameters()) + list(fc.parameters()), pn):
            dst.copy_(torch.from_numpy(src).double())
    hx, cx = torch.zeros(B, h, dtype=torch.float64), torch.zeros(B, h, dtype=torch.float64)
    inp, hs = i64, []
    for t in range(T):
        hx, cx = cell(inp, (hx, cx))
        inp = hx
        hs.append(hx)
    ref = fc(torch.stack(hs))
    want = [ref.detach().numpy()] + _grads64(ref, dy, [i64] + list(cell.parameters()) + list(fc.parameters()))
    # ---- HIP
    mod = mod.cuda()
    p = [mod.lstm.weight_ih, mod.lstm.weight_hh, mod.lstm.bias_ih, mod.lstm.bias_hh, mod.fc1.weight, mod.fc1.bias]
    hd = at_residue(init, 4).requires_grad_(True)
    gd = at_residue(dy, 12)
    assert residue(hd) == 4 and residue(gd) == 12
    out = mod(hd, T)
    grads = torch.autograd.grad(out, [hd] + p, grad_outputs=gd)
    _module_errors("module_decoder_h%d_d%d_b%d_t%d" % (h, d, B, T), [out] + list(grads), want,
                   ["out", "d_init", "weight_ih", "weight_hh", "bias_ih", "bias_hh", "fc1.weight", "fc1.bias"])
    assert check_guards() == 2


@pytest.mark.parametrize("M_,K,N", [(5, 37, 11), (231, 325, 120)])
def test_linear_bridge_on_offset_input_and_gradient(M_, K, N):
    """_LinearFn (HipLinear): x at residue 4, the upstream gradient at residue 12, against float64 matrix products"""
    _need_gpu()
    from factorized_amd import _ops
    torch.manual_seed(K + N)
    lin = _ops.HipLinear(K, N)
    W, b = lin.weight.detach().numpy().astype(np.float64), lin.bias.detach().numpy().astype(np.float64)
    rs = np.random.RandomState(M_ + K)
    x = rs.normal(size=(M_, K)).astype(np.float32)
    dy = rs.normal(size=(M_, N)).astype(np.float32)
    x64, dy64 = x.astype(np.float64), dy.astype(np.float64)
    want = [x64 @ W.T + b, dy64 @ W, dy64.T @ x64, dy64.sum(0)]
    lin = lin.cuda()
    xd = at_residue(x, 4).requires_grad_(True)
    gd = at_residue(dy, 12)
    assert residue(xd) == 4 and residue(gd) == 12
    out = lin(xd)
    grads = torch.autograd.grad(out, [xd, lin.weight, lin.bias], grad_outputs=gd)
    _module_errors("module_linear_m%d_k%d_n%d" % (M_, K, N), [out] + list(grads), want, ["y", "dx", "dW", "db"])
    assert check_guards() == 2
