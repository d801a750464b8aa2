"""M_D.loss_and_grad (mfm_train_ablation_d, csrc/train_ablation.hip) on the MI355X: the label loss, y_hat and all 32 gradient
tensors against oracle/mfm_oracle_extra.M_D on the CPU with torch autograd -- the weights tests/golden/extra_M_D.npz was made with
(seed 1234), loaded through tests/extra_cases.load_extra.  Bound: the project's 1e-4 relative fp32 tolerance, per tensor against
the tensor's largest magnitude (tests.cases.rel_err).  A tensor whose reference gradient is exactly zero everywhere (W_hh at
T = 1) must be exactly zero."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import mfm_oracle_extra as X
from factorized_amd import _lib, configs, synth
from tests import offset_views
from tests.cases import rel_err
from tests.extra_cases import EXTRA_SIZES, load_extra

pytestmark = pytest.mark.gpu
TOL = 1e-4
STATS_FROM = 1000          # mask elements from which a site's kept fraction is held to 5 sigma of the binomial (tests/dropout_checks.py)


class _FixedMask(torch.nn.Module):
    """the idea of tests/dropout_checks.py: the oracle's dropout module replaced by the scales the library drew"""

    def __init__(self, mask):
        super().__init__()
        self.mask = mask

    def forward(self, x):
        return x * self.mask


def _scales(seed, call, tick, site, n, f, p):
    """the dropout scales [n, f] of a site as include/mfm_hip.h states them: rng_uniform (csrc/common.h) of seed + GOLD * call + tick
    at index (site << 40) + row * f + column, kept where it is >= p"""
    u64 = np.uint64
    gold = 0x9E3779B97F4A7C15
    sd = (seed + gold * call + tick) & ((1 << 64) - 1)
    idx = u64(site << 40) + np.arange(n * f, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = u64(sd) + u64(gold) * (idx + u64(1))
        z = (z ^ (z >> u64(30))) * u64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> u64(27))) * u64(0x94D049BB133111EB)
        z = z ^ (z >> u64(31))
    u = (z >> u64(40)).astype(np.float32) * np.float32(1.0 / 16777216.0)
    scale = np.float32(1.0) / (np.float32(1.0) - np.float32(p))
    return np.where(u < np.float32(p), np.float32(0.0), scale).reshape(n, f)


def _pair(cfgs, seed=1234):
    """(M_D on the GPU, the oracle on the CPU) with the same synthetic weights"""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from factorized_amd import mfm_model as M
    ref = X.CLASSES["M_D"](*cfgs)
    w = synth.make_weights({k: tuple(v.shape) for k, v in ref.state_dict().items()}, seed=seed)
    ref.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in w.items()})
    model = M.M_D(*cfgs)
    model.load_state_dict(ref.state_dict())
    return model.cuda(), ref


def _cfgs(dropout=None, output_dim=1, **sizes):
    cfgs = configs.canonical_configs(dropout=False, output_dim=output_dim, **dict(EXTRA_SIZES, **sizes))
    for m, p in zip("lav", dropout or ()):
        cfgs[0]["z%s_to_f%s_dropout" % (m, m)] = p
    return cfgs


def _labels(N, od, loss="l1", seed=5):
    rs = np.random.RandomState(seed)
    if loss == "l1":
        return torch.from_numpy(rs.standard_normal((N, od)).astype(np.float32))
    return torch.from_numpy(rs.randint(0, od, size=N).astype(np.int64))


def _batch(cfgs, N, T, seed):
    xn, _ = synth.make_batch(cfgs[0]["input_dims"], N, T, seed=seed)
    return torch.from_numpy(xn)


def _want(ref, x, y, loss="l1"):
    """(loss, y_hat, {name: gradient}) of the oracle with torch autograd; its .grad are cleared first"""
    torch.set_num_threads(4)
    ref.zero_grad(set_to_none=True)
    y_hat = ref.forward(x)[0][3]
    out = F.l1_loss(y_hat, y) if loss == "l1" else F.cross_entropy(y_hat, y)
    out.backward()
    return float(out.detach()), y_hat.detach(), {n: p.grad.clone() for n, p in ref.named_parameters()}


def _grads(model):
    return {n: (None if p.grad is None else p.grad.detach().clone()) for n, p in model.named_parameters()}


def _check(model, got, want, what):
    wl, wy, wg = want
    assert got.dim() == 0 and got.dtype == torch.float32 and got.is_cuda and not got.requires_grad
    err = abs(float(got) - wl) / max(abs(wl), 1e-30)
    print("train %s loss %.6e want %.6e err %.3e" % (what, float(got), wl, err))
    assert err < TOL, (what, float(got), wl)
    err = rel_err(model.last_y_hat.cpu().numpy(), wy.numpy())
    print("train %s y_hat %.3e" % (what, err))
    assert err < TOL, (what, err)
    g = _grads(model)
    assert len(g) == 32 and set(g) == set(wg)
    worst = (0.0, "")
    for n, r in wg.items():
        assert g[n] is not None and tuple(g[n].shape) == tuple(r.shape), n
        if float(r.abs().max()) == 0.0:
            assert float(g[n].abs().max()) == 0.0, (what, n)
            continue
        worst = max(worst, (rel_err(g[n].cpu().numpy(), r.numpy()), n))
    print("train %s worst gradient %.3e %s" % (what, worst[0], worst[1]))
    assert worst[0] < TOL, (what, worst)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _same_grads(a, b):
    assert set(a) == set(b)
    return all((a[n] is None and b[n] is None) or torch.equal(_bits(a[n]), _bits(b[n])) for n in a)


_SHARED = {}


def _case(loss="l1"):
    """the golden shape (B = 12, T = 6): model, oracle, labels, the oracle's numbers and the one-chunk result, computed once"""
    if loss not in _SHARED:
        base, _, xn, _ = load_extra("M_D", "small")
        cfgs = base if loss == "l1" else _cfgs(output_dim=3)
        model, ref = _pair(cfgs)
        xc = torch.from_numpy(xn)
        assert tuple(xc.shape[:2]) == (6, 12)
        yc = _labels(12, cfgs[0]["output_dim"], loss)
        x, y = xc.cuda(), yc.cuda()
        want = _want(ref, xc, yc, loss)
        got = model.loss_and_grad(x, y, loss=loss).clone()
        _SHARED[loss] = dict(cfgs=cfgs, model=model, ref=ref, xc=xc, yc=yc, x=x, y=y, want=want, loss=got, y_hat=model.last_y_hat.clone(),
                             grads=_grads(model))
    return _SHARED[loss]


# ----------------------------------------------------------------------------------- 1. parity at the golden shape
@pytest.mark.parametrize("loss", ["l1", "ce"])
def test_loss_y_hat_and_all_32_gradients_match_the_oracle(loss):
    s = _case(loss)
    assert s["cfgs"][0]["output_dim"] == (1 if loss == "l1" else 3)
    model = s["model"]
    assert model._train_bufs and all(v is not False for v in model._train_bufs.values())      # (the entry took it)
    model.zero_grad(set_to_none=True)
    _check(model, model.loss_and_grad(s["x"], s["y"], loss=loss), s["want"], "golden %s" % loss)


# ----------------------------------------------------------------------------------- 2. edges of the recurrence and the row tiling
@pytest.mark.parametrize("T,N", [(1, 12), (2, 12), (6, 1)], ids=["T1", "T2", "N1"])
def test_edges_against_the_oracle(T, N):
    s = _case()
    model, _ = _pair(s["cfgs"])
    xc, yc = _batch(s["cfgs"], N, T, seed=31), _labels(N, 1, seed=32)
    want = _want(s["ref"], xc, yc)
    if T == 1:
        assert all(float(want[2]["encoder_%s.lstm.weight_hh" % m].abs().max()) == 0.0 for m in "lav")
    _check(model, model.loss_and_grad(xc.cuda(), yc.cuda()), want, "T%d N%d" % (T, N))
    if T == 1:      # ... and an exact zero is also what a second call adds
        model.loss_and_grad(xc.cuda(), yc.cuda())
        assert all(float(model._modules["encoder_" + m].lstm.weight_hh.grad.abs().max()) == 0.0 for m in "lav")


def test_ragged_tiles_on_each_side_of_the_tile_rows_switch():
    """T = 2 at an N that is no multiple of the tile rows on each side of the switch the library reports"""
    s = _case()
    L = _lib.lib()
    tr = (C.c_int32 * 1)()
    N0 = None
    for n in range(1, 4097):
        assert L.mfm_train_ablation_d_tile_rows(n, 0, tr) == 0
        if tr[0] == 4:
            N0 = n
            break
    assert N0 is not None and N0 > 4, "no N up to 4096 reaches the four-row form on %d CUs" % L.mfm_device_cus()
    for N, rows in ((N0 - 3, 1), (N0 + 3, 4)):
        assert L.mfm_train_ablation_d_tile_rows(N, N, tr) == 0 and tr[0] == rows and N % 4
        model, _ = _pair(s["cfgs"])
        xc, yc = _batch(s["cfgs"], N, 2, seed=11), _labels(N, 1, seed=12)
        _check(model, model.loss_and_grad(xc.cuda(), yc.cuda(), max_rows=N), _want(s["ref"], xc, yc), "N%d tile rows %d" % (N, rows))


def test_row_chunks_of_5_5_and_2():
    s = _case()
    model, _ = _pair(s["cfgs"])
    got = model.loss_and_grad(s["x"], s["y"], max_rows=5)
    _check(model, got, s["want"], "chunks of 5")
    assert abs(float(got) - float(s["loss"])) <= TOL * abs(float(s["loss"]))
    assert torch.equal(_bits(model.last_y_hat), _bits(s["y_hat"]))          # (a row's arithmetic does not depend on its chunk)
    for n, g in _grads(model).items():
        assert rel_err(g.cpu().numpy(), s["grads"][n].cpu().numpy()) < TOL, n


def test_widths_of_every_residue_mod_4():
    cfgs = _cfgs(zl_size=18, za_size=7, zv_size=33, fl_size=37, fa_size=15, fv_size=30)
    model, ref = _pair(cfgs, seed=77)
    xc, yc = _batch(cfgs, 9, 3, seed=41), _labels(9, 1, seed=42)
    _check(model, model.loss_and_grad(xc.cuda(), yc.cuda()), _want(ref, xc, yc), "odd widths")
    model.zero_grad(set_to_none=True)
    _check(model, model.loss_and_grad(xc.cuda(), yc.cuda(), max_rows=4), _want(ref, xc, yc), "odd widths, chunks of 4")
    assert all(v is not False for v in model._train_bufs.values())


# ----------------------------------------------------------------------------------- 3. .grad semantics, determinism
def test_a_second_call_doubles_every_gradient_exactly_and_frozen_parameters_stay_none():
    s = _case()
    model, _ = _pair(s["cfgs"])
    x, y = s["x"], s["y"]
    model.loss_and_grad(x, y)
    g1 = _grads(model)
    assert _same_grads(g1, s["grads"])                       # two fresh models: the same bits
    model.loss_and_grad(x, y)
    assert _same_grads(_grads(model), {n: 2 * g for n, g in g1.items()})
    model.zero_grad(set_to_none=False)
    frozen = ("encoder_a.lstm.weight_ih", "encoder_l.lstm.bias_hh", "zv_to_fv_fc1.weight", "fs_to_y.bias", "encoder_v.fc1.bias")
    for n, p in model.named_parameters():
        if n in frozen:
            p.requires_grad_(False)
            p.grad = None
    model.loss_and_grad(x, y)
    g3 = _grads(model)
    assert all(g3[n] is None for n in frozen)
    assert _same_grads({n: g for n, g in g3.items() if n not in frozen}, {n: g for n, g in g1.items() if n not in frozen})
    # some .grad there, some None: the missing ones are created and all of them hold one gradient more
    for n, p in model.named_parameters():
        p.requires_grad_(True)
    model.loss_and_grad(x, y)
    g4 = _grads(model)
    assert _same_grads(g4, {n: (g1[n] if n in frozen else 2 * g1[n]) for n in g1})


def test_two_fresh_calls_are_bit_identical():
    s = _case()
    model = s["model"]
    for cap in (None, 5):
        outs = []
        for _ in range(2):
            model.zero_grad(set_to_none=True)
            outs.append((model.loss_and_grad(s["x"], s["y"], max_rows=cap).clone(), _grads(model)))
        assert torch.equal(_bits(outs[0][0]), _bits(outs[1][0])) and _same_grads(outs[0][1], outs[1][1])
    key = model._train_last
    assert int(model._train_bufs[key][0].view(torch.int32)[-2]) == 0          # the ticket word is back at 0


# ----------------------------------------------------------------------------------- 4. dropout in train mode
def test_train_mode_dropout_matches_the_oracle_with_the_library_masks():
    P = (0.2, 0.5, 0.7)
    cfgs = _cfgs(dropout=P)
    model, ref = _pair(cfgs)
    twin, _ = _pair(cfgs)
    model.dropout_seed = twin.dropout_seed = 4242
    N, T = 256, 3                                            # 256 x 28 / 4 / 20 mask elements: every site reaches STATS_FROM
    xc, yc = _batch(cfgs, N, T, seed=51), _labels(N, 1, seed=52)
    x, y = xc.cuda(), yc.cuda()
    model.train()
    twin.train()
    ref.train()
    seen = []
    for call in range(2):
        model.zero_grad(set_to_none=True)
        twin.zero_grad(set_to_none=True)
        got = model.loss_and_grad(x, y)
        masks = [m.clone() for m in model.last_dropout_masks()]
        other = twin.loss_and_grad(x, y)
        assert torch.equal(_bits(got), _bits(other)) and _same_grads(_grads(model), _grads(twin))      # the same seed, call for call
        assert all(torch.equal(a, b) for a, b in zip(masks, twin.last_dropout_masks()))
        for m, p, mk in zip("lav", P, masks):
            scale = np.float32(1.0) / (np.float32(1.0) - np.float32(p))
            kept = mk != 0
            assert bool(((mk == 0) | (mk == float(scale))).all()), m
            assert mk.numel() >= STATS_FROM, (m, mk.numel())
            frac, sigma = float(kept.float().mean()), (p * (1 - p) / mk.numel()) ** 0.5
            print("train dropout site %s kept %.4f want %.4f sigma %.4f" % (m, frac, 1 - p, sigma))
            assert abs(frac - (1 - p)) < 5 * sigma, (m, frac)
            assert np.array_equal(mk.cpu().numpy(), _scales(4242, call, 0, "lav".index(m), N, mk.shape[1], p)), m      # the documented stream
            setattr(ref, "z%s_to_f%s_dropout" % (m, m), _FixedMask(mk.cpu()))
        _check(model, got, _want(ref, xc, yc), "dropout call %d" % call)
        seen.append(masks)
    assert not any(torch.equal(a, b) for a, b in zip(*seen))      # other masks on the next call


def test_replays_of_a_captured_train_mode_step_draw_new_masks_from_the_documented_stream():
    """a captured call keeps its host seed and call number; the device tick word, advanced inside the graph, moves the stream"""
    P = (0.2, 0.5, 0.7)
    cfgs = _cfgs(dropout=P)
    model, _ = _pair(cfgs)
    model.dropout_seed = 77
    model.train()
    N, T = 40, 3
    x, y = _batch(cfgs, N, T, seed=61).cuda(), _labels(N, 1, seed=62).cuda()
    model.loss_and_grad(x, y)                                # call 0, eager: buffers, code objects, the .grad tensors
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        model.zero_grad(set_to_none=False)
        gloss = model.loss_and_grad(x, y)                    # call 1, whatever the replay
    tick = model._train_bufs[model._train_last][7]
    seen, ticks, losses = [], [], []
    for _ in range(3):
        graph.replay()
        torch.cuda.synchronize()
        t = int(tick) & ((1 << 64) - 1)
        masks = [m.clone() for m in model.last_dropout_masks()]
        for site, (mk, p) in enumerate(zip(masks, P)):
            assert np.array_equal(mk.cpu().numpy(), _scales(77, 1, t, site, N, mk.shape[1], p)), site
        seen.append(masks)
        ticks.append(t)
        losses.append(float(gloss))
    assert len(set(ticks)) == 3 and 0 not in ticks and len(set(losses)) == 3
    for a, b in ((0, 1), (1, 2), (0, 2)):
        assert not any(torch.equal(p, q) for p, q in zip(seen[a], seen[b]))
    model.zero_grad(set_to_none=True)
    model.loss_and_grad(x, y)                                # eager again: call 2, no tick
    for site, (mk, p) in enumerate(zip(model.last_dropout_masks(), P)):
        assert np.array_equal(mk.cpu().numpy(), _scales(77, 2, 0, site, N, mk.shape[1], p)), site


def test_eval_mode_is_bit_identical_to_p_0():
    s = _case()
    dropped, _ = _pair(_cfgs(dropout=(0.2, 0.5, 0.7)))
    dropped.eval()
    got = dropped.loss_and_grad(s["x"], s["y"])
    assert torch.equal(_bits(got), _bits(s["loss"])) and _same_grads(_grads(dropped), s["grads"])
    assert dropped.last_dropout_masks() == [None, None, None] and not dropped.training


# ----------------------------------------------------------------------------------- 5. x as a view
def test_an_x_off_a_16_byte_boundary_and_a_batch_slice_give_the_same_bits():
    s = _case()
    model = s["model"]
    offset_views.forget_views()
    view = offset_views.at_residue(s["x"], 4)
    assert view.data_ptr() % 16 == 4
    model.zero_grad(set_to_none=True)
    got = model.loss_and_grad(view, s["y"])
    assert torch.equal(_bits(got), _bits(s["loss"])) and _same_grads(_grads(model), s["grads"])
    assert offset_views.check_guards() == 1
    # a batch slice of a larger [T, N', D] tensor (not contiguous: the call takes its contiguous copy)
    T, N, D = s["x"].shape
    big = torch.randn(T, N + 7, D, device="cuda")
    big[:, 3:3 + N] = s["x"]
    model.zero_grad(set_to_none=True)
    got = model.loss_and_grad(big[:, 3:3 + N], s["y"])
    assert torch.equal(_bits(got), _bits(s["loss"])) and _same_grads(_grads(model), s["grads"])


# ----------------------------------------------------------------------------------- 6. graph capture, a short trajectory
def test_a_captured_step_replayed_three_times_follows_three_eager_steps():
    import factorized_amd.optim as optim
    s = _case()
    x, y = s["x"], s["y"]
    captured, _ = _pair(s["cfgs"])
    eager, _ = _pair(s["cfgs"])
    opt_c = optim.Adam(captured.parameters(), lr=torch.tensor([1e-3], device="cuda"), capturable=True)
    opt_e = optim.Adam(eager.parameters(), lr=1e-3)
    for model, opt in ((captured, opt_c), (eager, opt_e)):   # one eager step each: buffers, code objects, .grad, the optimizers' state
        model.loss_and_grad(x, y)
        opt.step()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured.zero_grad(set_to_none=False)
        gloss = captured.loss_and_grad(x, y)
        opt_c.step()
    losses = []
    for _ in range(3):
        graph.replay()
        losses.append(float(gloss))
        eager.zero_grad(set_to_none=False)
        le = eager.loss_and_grad(x, y)
        opt_e.step()
        assert abs(losses[-1] - float(le)) <= TOL * abs(float(le))
    torch.cuda.synchronize()
    assert losses[0] > losses[2]
    for (n, p), (_, q) in zip(captured.named_parameters(), eager.named_parameters()):
        assert rel_err(p.detach().cpu().numpy(), q.detach().cpu().numpy()) < TOL, n


def test_a_fallback_checkpoint_of_the_plain_adam_loads_into_the_capturable_one():
    """optim.Adam(capturable=True) builds its inner torch optimizer capturable for device tensors; a "fallback" state saved by a
    plain optim.Adam still loads into it and the next step is the one the plain optimizer takes"""
    import factorized_amd.optim as optim
    s = _case()
    x, y = s["x"], s["y"]
    plain, _ = _pair(s["cfgs"])
    opt_p = optim.Adam(plain.parameters(), lr=1e-3)
    for _ in range(2):
        opt_p.zero_grad()
        plain.loss_and_grad(x, y)
        opt_p.step()
    saved = copy.deepcopy(opt_p.state_dict())
    assert "fallback" in saved
    other, _ = _pair(s["cfgs"])
    other.load_state_dict(plain.state_dict())
    opt_c = optim.Adam(other.parameters(), lr=1e-3, capturable=True)
    opt_c.load_state_dict(saved)
    for model, opt in ((plain, opt_p), (other, opt_c)):
        opt.zero_grad()
        model.loss_and_grad(x, y)
        opt.step()
    for (n, p), (_, q) in zip(plain.named_parameters(), other.named_parameters()):
        assert rel_err(q.detach().cpu().numpy(), p.detach().cpu().numpy()) < 1e-6, n


def test_five_adam_steps_follow_the_oracle():
    """five steps with torch.optim.Adam on the device against five oracle steps with torch.optim.Adam on the CPU; the parameters
    are compared (the float32 oracle stays within 1.5e-6 of the float64 oracle over these five steps, so Adam's division does not
    ask for the per-step losses instead)"""
    s = _case()
    model, ref = _pair(s["cfgs"])
    ref = copy.deepcopy(ref)
    om, orf = torch.optim.Adam(model.parameters(), lr=1e-3), torch.optim.Adam(ref.parameters(), lr=1e-3)
    torch.set_num_threads(4)
    for step in range(5):
        om.zero_grad()
        got = model.loss_and_grad(s["x"], s["y"])
        om.step()
        orf.zero_grad()
        want = F.l1_loss(ref.forward(s["xc"])[0][3], s["yc"])
        want.backward()
        orf.step()
        assert abs(float(got) - float(want.detach())) <= TOL * abs(float(want.detach())), step
    worst = max((rel_err(p.detach().cpu().numpy(), q.detach().numpy()), n) for (n, p), (_, q) in zip(model.named_parameters(), ref.named_parameters()))
    print("train trajectory worst parameter %.3e %s" % worst)
    assert worst[0] < TOL, worst


# ----------------------------------------------------------------------------------- 7. refusal
def test_a_z_of_132_takes_the_composed_path_with_the_same_numbers(monkeypatch):
    cfgs = _cfgs(zl_size=132)
    model, ref = _pair(cfgs)
    xc, yc = _batch(cfgs, 5, 3, seed=21), _labels(5, 1, seed=22)
    L, calls = _lib.lib(), []
    real = L.mfm_train_ablation_d
    monkeypatch.setattr(L, "mfm_train_ablation_d", lambda *a: (calls.append(1), real(*a))[1], raising=True)
    want = _want(ref, xc, yc)
    _check(model, model.loss_and_grad(xc.cuda(), yc.cuda()), want, "zl 132")
    assert calls == [1] and model._train_refused and not model.__dict__.get("_train_bufs")
    model.zero_grad(set_to_none=True)
    _check(model, model.loss_and_grad(xc.cuda(), yc.cuda()), want, "zl 132 again")
    assert calls == [1]                                      # (remembered: no second call into the entry)
    x, y = xc.cuda(), yc.cuda()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with pytest.raises(_lib.MfmError, match="stream capture"):
        with torch.cuda.graph(graph):
            model.loss_and_grad(x, y)


def test_the_entry_refuses_a_z_of_132_and_writes_nothing():
    s = _case()
    model = s["model"]
    L = _lib.lib()
    T, N = s["x"].shape[:2]
    sz = list(model._ablation_sizes())
    sz[0] = 132
    sizes = (C.c_int32 * 12)(*sz)
    params = model._train_params()
    sent = [torch.full((p.numel() + 132 * 4 * 200,), 7.25, device="cuda") for p in params]
    y_hat, out, ws = (torch.full((n,), 7.25, device="cuda") for n in (N, 1, 1 << 16))
    prm = (C.c_void_p * 32)(*[p.data_ptr() for p in params])
    grd = (C.c_void_p * 32)(*[g.data_ptr() for g in sent])
    rc = L.mfm_train_ablation_d(T, N, sizes, 0, 0, (C.c_float * 3)(0, 0, 0), 1, 0, None, prm, grd, 0, C.c_void_p(s["x"].data_ptr()),
                                C.c_void_p(s["y"].data_ptr()), C.c_void_p(ws.data_ptr()), C.c_void_p(y_hat.data_ptr()), C.c_void_p(out.data_ptr()),
                                0, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == _lib.MFM_ERR_UNSUPPORTED and "132" in L.mfm_last_error().decode()
    torch.cuda.synchronize()
    for t in sent + [y_hat, out, ws]:
        assert bool((t == 7.25).all())
