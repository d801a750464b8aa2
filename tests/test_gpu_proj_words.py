"""The projection hand-over of the B <= 32 step as ONE message (csrc/proj_role_dev.h): every x-projection travels as a 64-bit
word {value, epoch}, stored and loaded with one relaxed agent-scope 64-bit atomic; the consumer (small_fwd_body<.., FLG = true>)
takes a value when the epoch half of its word is this launch's epoch and loads the slice again otherwise.  No flag, no
acknowledgement wait for t >= 1.  Checked here:

  * small-shape parity -- the smallest shapes that can break the indexing of the word region and the prefetch clamps
    (T = 1, 2: min(t + 2, T - 1); T = 5: two items per role group with the default role count; B = 19: neither a tile nor a wave
    multiple; B = 1; B = 32: the full tile): the fused step on the role form against the CPU oracle at the project's 1e-4
    (fp32 plans: loss and every gradient) and against the same engine with the hand-overs off (fp32 and bf16-operand plans);
  * stale data -- three consecutive steps with three different batches on ONE plan: step k must equal the FIRST step of a fresh
    plan (zeroed workspace: nothing an earlier launch could have left) on batch k.  A consumer that accepts a word of the
    previous launch computes with the previous batch's projections and fails this;
  * the same through a captured step replayed three times, where the epoch advances by the graph's own tick node.

Bounds.  fp32, role form against separate launches: the same products summed in another order and float atomics in another
order -- 1e-5 on the losses and 2e-5 (tests.cases.grad_err) on the gradients, the bounds tests/test_gpu_role.py holds the two
forms to.  bf16-operand plans are NOT held to the fp32 oracle at 1e-4: both operands of every product are rounded to 8
mantissa bits (2^-9 = 2e-3 relative per operand), which is what tests/test_gpu_bf16.py bounds per tensor; the hand-over is
held to the separate-launch form of the same plan, whose roundings are the same and whose summation order differs: 2e-3 on the
loss, 2e-2 relative L2 per gradient (a projection that moves by one fp32 ulp can flip a later bf16 rounding), the bounds of
test_role_workgroups_bf16_plan."""
import numpy as np
import pytest
import torch

from oracle import mfm_oracle as O
from factorized_amd import configs as C
from factorized_amd import synth
from tests.cases import grad_err

pytestmark = pytest.mark.gpu
TOL = 1e-4
SHAPES = [(B, T) for T in (1, 2, 3, 5) for B in (1, 19, 32)]


def _engine(precision="fp32", handover=True):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from factorized_amd import engine
    cfgs = C.canonical_configs(dropout=False)
    e = engine.MFMEngine(cfgs, precision=precision)
    e.handover = handover
    w = synth.make_weights(e.layout.shapes, seed=1234)
    e.load_weights(w)
    return e, w, cfgs


def _batch(cfgs, B, T, seed):
    xn, yn = synth.make_batch(cfgs[0]["input_dims"], B, T, seed=seed)
    return xn, yn, torch.from_numpy(xn).cuda(), torch.from_numpy(yn).cuda()


def _step(e, x, y):
    """one fused gradient step: (loss dict, {name: gradient})"""
    l = e.grad_step(x, y)
    torch.cuda.synchronize()
    return e.loss_dict(l), {n: v.cpu().numpy().copy() for n, v in e.grad_views().items()}


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("B,T", SHAPES)
def test_small_shapes_role_form_against_oracle_and_separate_launches(B, T, precision):
    e1, w, cfgs = _engine(precision)
    xn, yn, x, y = _batch(cfgs, B, T, seed=7)
    ld1, g1 = _step(e1, x, y)
    assert e1.plan(T, B).get_option("proj_roles_active") == 1
    assert e1.check_status() == 0
    e0, _, _ = _engine(precision, handover=False)
    ld0, g0 = _step(e0, x, y)
    assert e0.plan(T, B).get_option("proj_roles_active") == 0
    if precision == "fp32":
        for k in ld1:
            d = abs(ld1[k] - ld0[k]) / max(abs(ld0[k]), 1e-3)
            print("loss term %s: role %.8g separate %.8g rel %.2e" % (k, ld1[k], ld0[k], d))
            assert d <= 1e-5, (k, ld1[k], ld0[k])
        worst = max(grad_err(g1[n], g0[n]) for n in g0)
        print("worst gradient, role vs separate: %.2e" % worst)
        assert worst < 2e-5, worst
        torch.set_num_threads(4)
        m = O.build("kl_ef", cfgs)
        O.load_numpy_weights(m, w)
        m.train()
        terms = O.loss_terms(m, torch.from_numpy(xn), torch.from_numpy(yn), cfgs[0])
        terms["loss"].backward()
        ref = terms["loss"].item()
        print("loss: role %.8g oracle %.8g" % (ld1["loss"], ref))
        assert abs(ld1["loss"] - ref) <= TOL * abs(ref), (ld1["loss"], ref)
        errs = {n: grad_err(g1[n], p.grad.numpy()) for n, p in m.named_parameters()}
        n_worst = max(errs, key=errs.get)
        print("worst gradient, role vs oracle: %s %.2e" % (n_worst, errs[n_worst]))
        assert errs[n_worst] < TOL, (n_worst, errs[n_worst])
    else:
        d = abs(ld1["loss"] - ld0["loss"]) / abs(ld0["loss"])
        print("loss: role %.8g separate %.8g rel %.2e" % (ld1["loss"], ld0["loss"], d))
        assert d <= 2e-3, (ld1["loss"], ld0["loss"])
        errs = {n: float(np.linalg.norm(g1[n] - g0[n]) / max(np.linalg.norm(g0[n]), 1e-9)) for n in g0}
        n_worst = max(errs, key=errs.get)
        print("worst gradient (relative L2), role vs separate: %s %.2e" % (n_worst, errs[n_worst]))
        assert errs[n_worst] < 2e-2, (n_worst, errs[n_worst])


STALE_B, STALE_T = 19, 5


@pytest.fixture(scope="module")
def fresh_plan_steps():
    """batch k as the FIRST step of a plan of its own (computed once, shared, left unchanged)"""
    out = []
    for k in range(3):
        e, _, cfgs = _engine()
        _, _, x, y = _batch(cfgs, STALE_B, STALE_T, seed=40 + k)
        ld, g = _step(e, x, y)
        assert e.plan(STALE_T, STALE_B).get_option("proj_roles_active") == 1
        out.append((ld, g))
    return out


def test_consecutive_steps_take_nothing_from_the_previous_launch(fresh_plan_steps):
    e, _, cfgs = _engine()
    for k in range(3):
        _, _, x, y = _batch(cfgs, STALE_B, STALE_T, seed=40 + k)
        ld, g = _step(e, x, y)
        ld0, g0 = fresh_plan_steps[k]
        for n in ld:
            d = abs(ld[n] - ld0[n]) / max(abs(ld0[n]), 1e-3)
            print("step %d loss term %s: %.8g fresh plan %.8g rel %.2e" % (k, n, ld[n], ld0[n], d))
            assert d <= 1e-5, (k, n, ld[n], ld0[n])
        worst = max(grad_err(g[n], g0[n]) for n in g0)
        print("step %d worst gradient against the fresh plan: %.2e" % (k, worst))
        assert worst < 2e-5, (k, worst)
    assert e.plan(STALE_T, STALE_B).get_option("proj_roles_active") == 1 and e.check_status() == 0


def _graphed(handover):
    from factorized_amd import mfm_model as M
    from factorized_amd import train
    cfgs = C.canonical_configs(dropout=False)
    model = M.MFM_KL_EF(*cfgs)
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    w = synth.make_weights(shapes, seed=1234)
    model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in w.items()})
    model = model.cuda().train()
    if not handover:
        model.engine.set_handover(False)
    gs = train.GraphedModuleStep(model, cfgs[0], STALE_B, STALE_T, lr=0.0)          # lr = 0: every replay starts from the same weights
    return model, gs, cfgs


def test_replays_of_a_captured_step_take_nothing_from_the_previous_replay():
    """three replays with three batches on the role form against three replays of the separate-launch form: the words of replay
    k - 1 carry another epoch (the graph's tick node advances it) and must read as "not yet" in replay k"""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    m1, g1, cfgs = _graphed(True)
    m0, g0, _ = _graphed(False)
    assert g1.fused and g0.fused
    assert m1.engine.plan(STALE_T, STALE_B).get_option("proj_roles_active") == 1
    assert m0.engine.plan(STALE_T, STALE_B).get_option("proj_roles_active") == 0
    for k in range(3):
        _, _, x, y = _batch(cfgs, STALE_B, STALE_T, seed=40 + k)
        la, da = g1.step(x, y)
        lb, db = g0.step(x, y)
        torch.cuda.synchronize()
        la, da, lb, db = float(la), float(da), float(lb), float(db)
        print("replay %d: loss %.8g / %.8g, disc %.8g / %.8g" % (k, la, lb, da, db))
        assert abs(la - lb) <= 1e-5 * abs(lb) and abs(da - db) <= 1e-5 * max(abs(db), 1e-3), (k, la, lb, da, db)
        # (the module path's gradients: what loss.backward() left on the parameters)
        ga = {n: p.grad.detach().cpu().numpy().copy() for n, p in m1.named_parameters()}
        gb = {n: p.grad.detach().cpu().numpy().copy() for n, p in m0.named_parameters()}
        assert max(float(np.abs(v).max()) for v in gb.values()) > 1e-3          # (the replay's gradients, not a cleared buffer)
        worst = max(grad_err(ga[n], gb[n]) for n in gb)
        print("replay %d worst gradient, role vs separate: %.2e" % (k, worst))
        assert worst < 2e-5, (k, worst)
    assert int(m1.engine.plan(STALE_T, STALE_B).tick.item()) == 3
    assert m1.engine.check_status() == 0
