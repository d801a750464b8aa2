"""The autograd contract of the granular HIP ops (factorized_amd/_ops.py): what the composed module path is built from,
outside its happy path -- a second backward, partly used groups, upstream-gradient and input layouts, parameters of the
wrong dtype / layout, hidden sizes above the resident kernels' limit, one module used twice in a graph.

Reference of every numeric check: the same operation in plain torch on the CPU in float64 (oracle.mfm_oracle.SeqEncoder /
SeqDecoder / MemFusion after .double(), nn.Linear / nn.LSTMCell .double(), the reference's MMD formula), loaded with the same
weights.  Errors: tests.cases.rel_err (outputs) / grad_err (gradients) against TOL = 1e-4, the project's fp32 bound
(BASELINE.json north_star).  The worst value of each group goes to cases.report("autograd_contract_worst_<group>")."""
import pytest
import torch
import torch.nn as nn

from oracle import mfm_oracle as O
from tests import cases
from tests.cases import grad_err, rel_err

pytestmark = pytest.mark.gpu
TOL = 1e-4
RECURRENT = ("encoder", "decoder", "decoder_group", "seq_group")

_WORST = {}


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.fixture(scope="module", autouse=True)
def _report_worst():
    yield
    for g, v in sorted(_WORST.items()):
        cases.report("autograd_contract_worst_%s" % g, v)


def _chk(group, err, what, tol=TOL):
    print("%s %s: %.3e" % (group, what, err))
    _WORST[group] = max(_WORST.get(group, 0.0), err)
    assert err < tol, (group, what, err)


def _np(t):
    return t.detach().cpu().double().numpy()


def _chk_out(group, got, ref, what):
    assert got.dtype == torch.float32 and got.is_cuda and tuple(got.shape) == tuple(ref.shape), what
    _chk(group, rel_err(_np(got), _np(ref)), what)


def _chk_grad(group, got, ref, what, scale=1.0, tol=TOL):
    """gradient `got` of a GPU leaf against `scale` x the float64 reference's; a reference without gradient (the leaf is
    not reached by the loss) asks for None or exact zeros"""
    if ref is None:
        assert got is None or not bool(got.any()), "%s: gradient of an unused tensor is neither None nor zero" % what
        return
    assert got is not None, "%s: no gradient" % what
    assert tuple(got.shape) == tuple(ref.shape), what
    _chk(group, grad_err(_np(got), scale * _np(ref)), what, tol)


def _chk_params(group, m, ref, what, scale=1.0, used=True):
    for (n, p), (_, q) in zip(m.named_parameters(), ref.named_parameters()):
        _chk_grad(group, p.grad, q.grad if used else None, "%s.%s" % (what, n), scale)


def _zero(*mods_or_tensors):
    for o in mods_or_tensors:
        for t in (o.parameters() if isinstance(o, nn.Module) else [o]):
            t.grad = None


# ---------------------------------------------------------------------------------- module pairs (GPU fp32, CPU fp64)
def _pair(make_gpu, make_ref, seed):
    torch.manual_seed(seed)
    ref = make_ref()
    m = make_gpu()
    m.load_state_dict(ref.state_dict())
    return m.cuda(), ref.double()


def _enc(d, h, seed=0):
    from factorized_amd import mfm_model as M
    return _pair(lambda: M.encoderLSTM(d, h), lambda: O.SeqEncoder(d, h), 100 + seed)


def _dec(h, d, seed=0):
    from factorized_amd import mfm_model as M
    return _pair(lambda: M.decoderLSTM(h, d), lambda: O.SeqDecoder(h, d), 200 + seed)


def _cell(d, h, seed=0):
    return _pair(lambda: nn.LSTMCell(d, h), lambda: nn.LSTMCell(d, h), 300 + seed)


def _lin(i, o, seed=0):
    from factorized_amd import mfm_model as M
    return _pair(lambda: M.HipLinear(i, o), lambda: nn.Linear(i, o), 400 + seed)


def _states_ref(cell, x):
    """the contract of a "states" member of seq_group, x [T,B,d] -> (h_T, c_all [T,B,h]), as the reference's loop"""
    hx = x.new_zeros(x.shape[1], cell.hidden_size)
    cx = x.new_zeros(x.shape[1], cell.hidden_size)
    cs = []
    for t in range(x.shape[0]):
        hx, cx = cell(x[t], (hx, cx))
        cs.append(cx)
    return hx, torch.stack(cs, 0)


def _leaves(x):
    """CPU fp32 values -> (GPU fp32 leaf, CPU fp64 leaf)"""
    return x.cuda().requires_grad_(True), x.double().requires_grad_(True)


def _randn(seed, *shape):
    return torch.randn(tuple(shape), generator=torch.Generator().manual_seed(seed))


def _wsum(outs, ws):
    return sum((o * w.to(device=o.device, dtype=o.dtype)).sum() for o, w in zip(outs, ws))


def _mmd_ref(z, g):
    def ck(x, y):
        d = x.shape[1]
        return torch.exp(-((x.unsqueeze(1) - y.unsqueeze(0)) ** 2).mean(2) / float(d))
    return ck(g, g).mean() + ck(z, z).mean() - 2.0 * ck(g, z).mean()


def _mem_ref(g1, g2, chat, w1m, w2m, w1b, b1b, w2b, b2b):
    """MFN memory recurrence (reference mfm_model.py:177-181) with the attended part of gamma_n_fc1 already applied"""
    mem = chat.new_zeros(chat.shape[1], chat.shape[2])
    for t in range(chat.shape[0]):
        a1 = torch.relu(g1[t] + mem @ w1m.t())
        a2 = torch.relu(g2[t] + mem @ w2m.t())
        mem = torch.sigmoid(a1 @ w1b.t() + b1b) * mem + torch.sigmoid(a2 @ w2b.t() + b2b) * chat[t]
    return mem


class _Graph(object):
    """one small graph through one Function, built on both sides: outputs, and every leaf (inputs, parameters) in the
    same order"""

    def __init__(self, kind, T=3, B=5):
        from factorized_amd import mfm_model as M
        from factorized_amd import _ops
        self.kind = kind
        self.mods = []
        if kind == "encoder":
            m, r = _enc(11, 20)
            xg, xr = _leaves(_randn(1, 6, B, 11))
            self.mods, self.inputs = [(m, r)], [(xg, xr)]
            self.outs, self.refs = [m.forward(xg)], [r(xr)]
        elif kind == "decoder":
            m, r = _dec(20, 11)
            hg, hr = _leaves(_randn(2, B, 20))
            self.mods, self.inputs = [(m, r)], [(hg, hr)]
            self.outs, self.refs = [m.forward(hg, T)], [r(hr, T)]
        elif kind == "decoder_group":
            self.mods = [_dec(20, 11, 1), _dec(33, 1, 2), _dec(1, 11, 3)]
            self.inputs = [_leaves(_randn(3, B, 20)), _leaves(_randn(4, B, 33)), _leaves(_randn(5, B, 1))]
            self.outs = M.decoder_group([(i[0], m[0]) for i, m in zip(self.inputs, self.mods)], T)
            self.refs = [m[1](i[1], T) for i, m in zip(self.inputs, self.mods)]
        elif kind == "seq_group":
            e, c = _enc(11, 20, 4), _cell(11, 33, 5)
            xg, xr = _leaves(_randn(6, T, B, 11))
            self.mods, self.inputs = [e, c], [(xg, xr)]
            enc_out, states = M.seq_group([(xg, e[0])], [(xg, c[0])])
            self.outs = [enc_out[0], states[0][0], states[0][1]]
            self.refs = [e[1](xr)] + list(_states_ref(c[1], xr))
        elif kind == "linear":
            m, r = _lin(11, 20)
            xg, xr = _leaves(_randn(7, T, 9, 11))
            self.mods, self.inputs = [(m, r)], [(xg, xr)]
            self.outs, self.refs = [m(xg)], [r(xr)]
        elif kind == "group_linear":
            self.mods = [_lin(11, 20, 1), _lin(1, 33, 2), _lin(20, 1, 3)]
            self.inputs = [_leaves(_randn(8, 9, 11)), _leaves(_randn(9, T, B, 1)), _leaves(_randn(10, 1, 20))]
            self.outs = M.linear_group([(i[0], m[0]) for i, m in zip(self.inputs, self.mods)])
            self.refs = [m[1](i[1]) for i, m in zip(self.inputs, self.mods)]
        elif kind == "mmd":
            zg, zr = _leaves(_randn(11, 9, 11) * 1.3)
            g = _randn(12, 9, 11)
            self.inputs = [(zg, zr)]
            self.outs, self.refs = [M.loss_MMD(zg, g.cuda())], [_mmd_ref(zr, g.double())]
        elif kind == "mem":
            Mm, H1, H2 = 24, 40, 72
            shapes = [(T, B, H1), (T, B, H2), (T, B, Mm), (H1, Mm), (H2, Mm), (Mm, H1), (Mm,), (Mm, H2), (Mm,)]
            self.inputs = [_leaves(_randn(20 + i, *s) * (0.3 if len(s) == 2 else 1.0)) for i, s in enumerate(shapes)]
            self.outs = [_ops._MemFn.apply(*([i[0] for i in self.inputs] + [0.0, 0.0, False]))]
            self.refs = [_mem_ref(*[i[1] for i in self.inputs])]
        else:
            raise ValueError(kind)
        self.outs, self.refs = list(self.outs), list(self.refs)
        self.weights = [_randn(50 + i, *o.shape) for i, o in enumerate(self.refs)]

    def gpu_leaves(self):
        return [i[0] for i in self.inputs] + [p for m, _ in self.mods for p in m.parameters()]

    def zero(self):
        for g, r in self.inputs:
            g.grad = r.grad = None
        for m, r in self.mods:
            _zero(m, r)

    def check_forward(self, group):
        for i, (o, r) in enumerate(zip(self.outs, self.refs)):
            _chk_out(group, o, r, "%s out[%d]" % (self.kind, i))

    def check_grads(self, group, scale=1.0):
        for i, (g, r) in enumerate(self.inputs):
            _chk_grad(group, g.grad, r.grad, "%s input[%d]" % (self.kind, i), scale)
        for i, (m, r) in enumerate(self.mods):
            _chk_params(group, m, r, "%s member[%d]" % (self.kind, i), scale)


# ---------------------------------------------------------------------------------- 1. second backward
@pytest.mark.parametrize("kind", ["encoder", "decoder", "decoder_group", "seq_group", "linear", "group_linear", "mmd", "mem"])
def test_second_backward(kind):
    """backward(retain_graph=True) works once everywhere.  A second backward through a recurrent Function would run the BPTT
    on dA as if it were the gates (mfm_lstm_seq_bwd overwrites the saved gates in place): it raises and writes no .grad.  The
    Functions that do not overwrite what they save give the second backward's gradients (scaled by 2: a stale result fails)."""
    _need_gpu()
    G = "g1_second_backward"
    g = _Graph(kind)
    g.check_forward(G)
    loss, rloss = _wsum(g.outs, g.weights), _wsum(g.refs, g.weights)
    loss.backward(retain_graph=True)
    rloss.backward(retain_graph=True)
    g.check_grads(G)
    g.zero()
    if kind in RECURRENT:
        with pytest.raises(RuntimeError, match="already back-propagated"):
            (2.0 * loss).backward()
        torch.cuda.synchronize()
        assert all(t.grad is None for t in g.gpu_leaves())
    else:
        (2.0 * loss).backward(retain_graph=True)
        (2.0 * rloss).backward(retain_graph=True)
        g.check_grads(G)          # (both sides carry the factor 2)
        g.zero()
        loss.backward()
        rloss.backward()
        g.check_grads(G)


def test_autograd_grad_of_two_functions_of_one_encoder_output():
    """torch.autograd.grad(a, params, retain_graph=True) then torch.autograd.grad(b, params), a and b two scalars of ONE
    encoder output: the first is right, the second is refused; the supported forms -- a fresh forward, or one backward of the
    sum -- give the reference's gradients."""
    _need_gpu()
    G = "g1_second_backward"
    m, r = _enc(11, 20, 7)
    xg, xr = _leaves(_randn(60, 6, 5, 11))
    w = _randn(61, 5, 20)
    ps, qs = list(m.parameters()) + [xg], list(r.parameters()) + [xr]
    out, ref = m.forward(xg), r(xr)
    a, b = (out * w.cuda()).sum(), (out * out).sum()
    ra, rb = (ref * w.double()).sum(), (ref * ref).sum()
    ga = torch.autograd.grad(a, ps, retain_graph=True)
    for i, (u, v) in enumerate(zip(ga, torch.autograd.grad(ra, qs, retain_graph=True))):
        _chk_grad(G, u, v, "grad(a)[%d]" % i)
    with pytest.raises(RuntimeError, match="already back-propagated"):
        torch.autograd.grad(b, ps)
    want_b = torch.autograd.grad(rb, qs, retain_graph=True)
    out2 = m.forward(xg)
    for i, (u, v) in enumerate(zip(torch.autograd.grad((out2 * out2).sum(), ps), want_b)):
        _chk_grad(G, u, v, "grad(b) on a fresh forward [%d]" % i)
    out3 = m.forward(xg)
    gab = torch.autograd.grad((out3 * w.cuda()).sum() + (out3 * out3).sum(), ps)
    for i, (u, v) in enumerate(zip(gab, torch.autograd.grad(ra + rb, qs))):
        _chk_grad(G, u, v, "grad(a + b)[%d]" % i)


# ---------------------------------------------------------------------------------- 2. partly used groups
def _masked_loss(outs, ws, mask):
    return _wsum([o for o, k in zip(outs, mask) if k], [w for w, k in zip(ws, mask) if k])


# outputs of the 5-member seq_group below: enc0, enc1, enc2, (st0 h_T, st0 c_all), (st1 h_T, st1 c_all)
SEQ_MASKS = {
    "enc0_only": (1, 0, 0, 0, 0, 0, 0),
    "enc2_only": (0, 0, 1, 0, 0, 0, 0),               # (alone on its input: the shared input gets no gradient)
    "st1_only": (0, 0, 0, 0, 0, 1, 1),                # (the member behind the 4-per-launch split)
    "all_but_enc1": (1, 0, 1, 1, 1, 1, 1),
    "all_but_st1": (1, 1, 1, 1, 1, 0, 0),
    "st0_hT_only": (0, 0, 0, 1, 0, 0, 0),
    "st0_call_only": (0, 0, 0, 0, 1, 0, 0),
    "st1_call_and_enc1": (0, 1, 0, 0, 0, 0, 1),
}


@pytest.mark.parametrize("case", sorted(SEQ_MASKS))
def test_seq_group_partly_used(case):
    """3 encoders + 2 state LSTMs in one seq_group call (5 members: two recurrence launches).  enc0, enc1 and st0 read one
    shared input, enc2 and st1 another; the loss reaches only the outputs of `mask`."""
    _need_gpu()
    from factorized_amd import mfm_model as M
    G = "g2_partly_used"
    T, B = 3, 5
    mask = SEQ_MASKS[case]
    encs = [_enc(11, 20, 1), _enc(11, 33, 2), _enc(1, 1, 3)]
    sts = [_cell(11, 20, 1), _cell(1, 33, 2)]
    xg, xr = _leaves(_randn(70, T, B, 11))
    yg, yr = _leaves(_randn(71, T, B, 1))
    eo, so = M.seq_group([(xg, encs[0][0]), (xg, encs[1][0]), (yg, encs[2][0])], [(xg, sts[0][0]), (yg, sts[1][0])])
    outs = list(eo) + [so[0][0], so[0][1], so[1][0], so[1][1]]
    refs = [encs[0][1](xr), encs[1][1](xr), encs[2][1](yr)] + list(_states_ref(sts[0][1], xr)) + list(_states_ref(sts[1][1], yr))
    for i, (o, r) in enumerate(zip(outs, refs)):
        _chk_out(G, o, r, "%s out[%d]" % (case, i))
    ws = [_randn(80 + i, *r.shape) for i, r in enumerate(refs)]
    _masked_loss(outs, ws, mask).backward()
    _masked_loss(refs, ws, mask).backward()
    used = [mask[0], mask[1], mask[2], mask[3] or mask[4], mask[5] or mask[6]]
    for i, ((m, r), u) in enumerate(zip(encs + sts, used)):
        _chk_params(G, m, r, "%s member[%d]" % (case, i), used=bool(u))
    _chk_grad(G, xg.grad, xr.grad, "%s shared input" % case)        # (the reference's autograd sums over the users)
    _chk_grad(G, yg.grad, yr.grad, "%s second input" % case)


@pytest.mark.parametrize("mask", [(1, 0, 0), (0, 0, 1), (1, 0, 1), (0, 1, 1)], ids=lambda m: "".join(map(str, m)))
def test_decoder_group_partly_used(mask):
    """3 decoders; decoder 0 and 1 start from one shared embedding."""
    _need_gpu()
    from factorized_amd import mfm_model as M
    G = "g2_partly_used"
    T, B = 3, 5
    decs = [_dec(20, 11, 4), _dec(20, 1, 5), _dec(33, 7, 6)]
    hg, hr = _leaves(_randn(90, B, 20))
    kg, kr = _leaves(_randn(91, B, 33))
    outs = M.decoder_group([(hg, decs[0][0]), (hg, decs[1][0]), (kg, decs[2][0])], T)
    refs = [decs[0][1](hr, T), decs[1][1](hr, T), decs[2][1](kr, T)]
    for i, (o, r) in enumerate(zip(outs, refs)):
        _chk_out(G, o, r, "decoder_group out[%d]" % i)
    ws = [_randn(95 + i, *r.shape) for i, r in enumerate(refs)]
    _masked_loss(outs, ws, mask).backward()
    _masked_loss(refs, ws, mask).backward()
    for i, ((m, r), u) in enumerate(zip(decs, mask)):
        _chk_params(G, m, r, "decoder_group %s member[%d]" % (mask, i), used=bool(u))
    _chk_grad(G, hg.grad, hr.grad, "decoder_group %s shared embedding" % (mask,))
    _chk_grad(G, kg.grad, kr.grad, "decoder_group %s second embedding" % (mask,))


@pytest.mark.parametrize("mask", [(0, 0, 1, 0), (1, 0, 0, 0), (0, 1, 1, 1), (1, 1, 1, 0)], ids=lambda m: "".join(map(str, m)))
def test_linear_group_partly_used(mask):
    """4 Linears; layer 0 and 1 read one shared input."""
    _need_gpu()
    from factorized_amd import mfm_model as M
    G = "g2_partly_used"
    lins = [_lin(11, 20, 4), _lin(11, 1, 5), _lin(1, 33, 6), _lin(20, 11, 7)]
    xg, xr = _leaves(_randn(100, 9, 11))
    yg, yr = _leaves(_randn(101, 3, 5, 1))
    zg, zr = _leaves(_randn(102, 1, 20))
    outs = M.linear_group([(xg, lins[0][0]), (xg, lins[1][0]), (yg, lins[2][0]), (zg, lins[3][0])])
    refs = [lins[0][1](xr), lins[1][1](xr), lins[2][1](yr), lins[3][1](zr)]
    for i, (o, r) in enumerate(zip(outs, refs)):
        _chk_out(G, o, r, "linear_group out[%d]" % i)
    ws = [_randn(105 + i, *r.shape) for i, r in enumerate(refs)]
    _masked_loss(outs, ws, mask).backward()
    _masked_loss(refs, ws, mask).backward()
    for i, ((m, r), u) in enumerate(zip(lins, mask)):
        _chk_params(G, m, r, "linear_group %s member[%d]" % (mask, i), used=bool(u))
    for n, (a, b) in (("shared", (xg, xr)), ("second", (yg, yr)), ("third", (zg, zr))):
        _chk_grad(G, a.grad, b.grad, "linear_group %s %s input" % (mask, n))


# ---------------------------------------------------------------------------------- 3. upstream gradient layouts
def _through(layout, outs, ws):
    """the loss reaches every output through `layout`: what arrives at the Function's backward is an expanded stride-0
    tensor / a transposed view / the scatter of a stepped slice / a gradient cast down from float64"""
    if layout == "sum":
        return sum(o.sum() for o in outs)
    if layout == "transpose":
        return sum((o.transpose(0, 1) * w.to(o.device, o.dtype).transpose(0, 1).contiguous()).sum() for o, w in zip(outs, ws))
    if layout == "step2":
        return sum((o[..., ::2] * w.to(o.device, o.dtype)[..., ::2]).sum() for o, w in zip(outs, ws))
    if layout == "double":
        return sum((o.double() * w.to(o.device).double()).sum() for o, w in zip(outs, ws))
    raise ValueError(layout)


@pytest.mark.parametrize("layout", ["sum", "transpose", "step2", "double"])
@pytest.mark.parametrize("kind", ["encoder", "decoder", "linear", "seq_group", "decoder_group", "group_linear"])
def test_upstream_gradient_layouts(kind, layout):
    _need_gpu()
    G = "g3_upstream_layouts"
    g = _Graph(kind)
    _through(layout, g.outs, g.weights).backward()
    _through(layout, g.refs, g.weights).backward()
    g.check_grads(G)


# ---------------------------------------------------------------------------------- 4. input layouts through _rows
T4, B4, D4, H4 = 3, 5, 11, 20


def _view(name, seed):
    """-> (base CPU tensor, view function, (T, B, d)): the op's input is view(base)"""
    T, B, d = T4, B4, D4
    r = lambda *s: _randn(seed, *s)
    if name == "col1":                      # base only 4-byte aligned
        return r(T, B, d + 5), (lambda b: b[:, :, 1:1 + d]), (T, B, d)
    if name == "col1_odd_stride":           # ... and an odd row stride: no row but the first of the buffer is 8-byte aligned
        return r(T, B, d + 4), (lambda b: b[:, :, 1:1 + d]), (T, B, d)
    if name == "col1_d1":
        return r(T, B, 6), (lambda b: b[:, :, 1:2]), (T, B, 1)
    if name == "batch_first":
        return r(B, T, d), (lambda b: b.transpose(0, 1)), (T, B, d)
    if name == "time_slice":
        return r(T + 4, B, d), (lambda b: b[2:2 + T]), (T, B, d)
    if name == "batch_slice":
        return r(T, B + 6, d), (lambda b: b[:, 3:3 + B]), (T, B, d)
    if name == "step_cols":
        return r(T, B, 2 * d), (lambda b: b[:, :, ::2]), (T, B, d)
    if name == "expand":                    # strides (0, 0, 1): passed through with a row stride of 0
        return r(1, 1, d), (lambda b: b.expand(T, B, d)), (T, B, d)
    if name == "B1_of_larger":
        return r(T, B, d), (lambda b: b[:, 2:3]), (T, 1, d)
    if name == "T1_of_larger":
        return r(T, B, d), (lambda b: b[1:2]), (1, B, d)
    if name == "B1_T1_col":
        return r(T, B, d + 5), (lambda b: b[2:3, 1:2, 1:1 + d]), (1, 1, d)
    if name == "float64":
        return r(T, B, d).double(), (lambda b: b), (T, B, d)
    if name == "float16":
        return r(T, B, d).half(), (lambda b: b), (T, B, d)
    raise ValueError(name)


VIEWS = ["col1", "col1_odd_stride", "col1_d1", "batch_first", "time_slice", "batch_slice", "step_cols", "expand",
         "B1_of_larger", "T1_of_larger", "B1_T1_col", "float64", "float16"]


@pytest.mark.parametrize("through", ["encoderLSTM", "seq_group"])
@pytest.mark.parametrize("name", VIEWS)
def test_input_layouts(name, through):
    """every view goes in as it is (`_rows` passes it as a strided operand or copies it), requires grad, and is left
    bit-unchanged; outputs, parameter gradients and x.grad against the reference on the same values"""
    _need_gpu()
    from factorized_amd import mfm_model as M
    G = "g4_input_layouts"
    base, view, (T, B, d) = _view(name, 120)
    base_g = base.cuda()
    before = base_g.clone()
    xg = view(base_g).requires_grad_(True)
    xr = view(base).double().clone().requires_grad_(True)
    assert tuple(xg.shape) == (T, B, d)
    e, c = _enc(d, H4, 8), _cell(d, 33, 9)
    if through == "encoderLSTM":
        outs, refs, mods = [e[0].forward(xg)], [e[1](xr)], [e]
    else:
        eo, so = M.seq_group([(xg, e[0])], [(xg, c[0])])
        outs, refs, mods = [eo[0], so[0][0], so[0][1]], [e[1](xr)] + list(_states_ref(c[1], xr)), [e, c]
    for i, (o, r) in enumerate(zip(outs, refs)):
        _chk_out(G, o, r, "%s/%s out[%d]" % (name, through, i))
    ws = [_randn(130 + i, *r.shape) for i, r in enumerate(refs)]
    _wsum(outs, ws).backward()
    _wsum(refs, ws).backward()
    for i, (m, r) in enumerate(mods):
        _chk_params(G, m, r, "%s/%s member[%d]" % (name, through, i))
    assert xg.grad is not None and xg.grad.dtype == xg.dtype
    # x.grad has the input's dtype: a float16 gradient is the fp32 one rounded to 11 significant bits, at most 2^-11 of the
    # largest element away from it in the measure of grad_err -- that rounding is the format's, added to the fp32 bound
    tol = TOL + 2.0 ** -11 if xg.dtype == torch.float16 else TOL
    _chk_grad(G if xg.dtype != torch.float16 else G + "_f16_dx", xg.grad, xr.grad, "%s/%s x.grad" % (name, through), tol=tol)
    torch.cuda.synchronize()
    assert torch.equal(base_g, before), "the input buffer was written to"


# ---------------------------------------------------------------------------------- 5. parameter guard
def _guard_case(kind):
    """-> (GPU module, run(module) -> [outputs], make_ref() -> fp64 reference with the module's CURRENT weights and its run,
    name of the first parameter the forward hands to the library, (parameter to make non-contiguous, what the error names))"""
    from factorized_amd import configs, mfm_model as M
    from factorized_amd import mfm_extra as X
    B, T = 3, 2
    cfgs = configs.canonical_configs(dropout=False)
    d_l = cfgs[0]["input_dims"][0]
    torch.manual_seed(500)

    def sync(ref, m):
        ref.load_state_dict({k: v.detach().cpu() for k, v in m.state_dict().items()})
        return ref.double()
    if kind == "encoderLSTM":
        m = M.encoderLSTM(d_l, cfgs[0]["zl_size"])
        x = _randn(140, T, B, d_l)
        return (m.cuda(), lambda mm: [mm.forward(x.cuda())],
                lambda mm: [sync(O.SeqEncoder(d_l, mm.h), mm)(x.double())], "lstm.weight_ih", ("lstm.weight_hh", "lstm.weight_hh"))
    if kind == "decoderLSTM":
        h = cfgs[0]["fy_size"] + cfgs[0]["fl_size"]
        m = M.decoderLSTM(h, d_l)
        x = _randn(141, B, h)
        return (m.cuda(), lambda mm: [mm.forward(x.cuda(), T)],
                lambda mm: [sync(O.SeqDecoder(h, d_l), mm)(x.double(), T)], "lstm.weight_ih", ("fc1.weight", "fc1.weight"))
    if kind == "HipLinear":
        m = M.HipLinear(cfgs[0]["zy_size"], cfgs[0]["fy_size"])
        x = _randn(142, B, cfgs[0]["zy_size"])
        return (m.cuda(), lambda mm: [mm(x.cuda())],
                lambda mm: [sync(nn.Linear(mm.in_features, mm.out_features), mm)(x.double())], "weight", ("weight", "weight"))
    if kind == "MFN":
        m = M.MFN(*cfgs)
        x = _randn(143, T, B, sum(cfgs[0]["input_dims"]))
        return (m.cuda().eval(), lambda mm: [mm.forward(x.cuda())],
                lambda mm: [sync(O.MemFusion(*cfgs), mm).eval()(x.double())], "weight_ih", ("lstm_a.weight_ih", "LSTM[1]: weight_ih"))
    if kind == "M_A":
        from oracle import mfm_oracle_extra as OX
        from tests.extra_cases import extra_configs
        ecfgs = extra_configs()
        m = X.M_A(*ecfgs)
        x = _randn(144, T, B, sum(ecfgs[0]["input_dims"]))
        gs = [_randn(145, B, ecfgs[0]["zl_size"]), _randn(146, B, ecfgs[0]["zy_size"])]

        def run(mm):
            mm.mmd_gauss = [g.cuda() for g in gs]
            dec, reg, _ = mm.forward(x.cuda())
            return list(dec) + [reg]

        def ref(mm):
            r = sync(OX.CLASSES["M_A"](*ecfgs), mm).eval()
            r.mmd_gauss = [g.double() for g in gs]
            dec, reg, _ = r(x.double())
            return list(dec) + [reg]
        return m.cuda().eval(), run, ref, "lstm.weight_ih", ("decoder_a.lstm.weight_ih", "decoder_group[1]: lstm.weight_ih")
    raise ValueError(kind)


@pytest.mark.parametrize("how", ["double", "half", "bfloat16", "non_contiguous"])
@pytest.mark.parametrize("kind", ["encoderLSTM", "decoderLSTM", "HipLinear", "MFN", "M_A"])
def test_parameter_guard(kind, how, monkeypatch):
    """a module whose parameters are not contiguous fp32 is refused by name before anything is allocated or launched (the
    kernels would read another element size through the raw pointers); put right again, the same module computes the
    reference's result"""
    _need_gpu()
    from factorized_amd import _lib
    G = "g5_parameter_guard"
    m, run, ref, first, (victim, victim_msg) = _guard_case(kind)
    if how == "non_contiguous":
        p = dict(m.named_parameters())[victim]
        good = p.data
        p.data = good.t().contiguous().t()             # same values and shape, transposed storage
        assert not p.data.is_contiguous() and torch.equal(p.data, good)
        want = (victim_msg, "torch.float32", str(tuple(p.data.stride())))
    else:
        getattr(m, how)()
        want = (first, str(getattr(torch, {"double": "float64", "half": "float16"}.get(how, how))))
    launches = []
    with monkeypatch.context() as mp:
        if kind in ("encoderLSTM", "decoderLSTM", "HipLinear"):       # one Function: refused before its first launch
            from factorized_amd import engine as E
            mp.setattr(E, "gemm_grouped", lambda *a, **k: launches.append("gemm_grouped"))
            mp.setattr(E, "lstm_seq", lambda *a, **k: launches.append("lstm_seq"))
        with torch.no_grad():
            with pytest.raises(_lib.MfmError) as ei:
                run(m)
    assert launches == []
    for s in want:
        assert s in str(ei.value), (s, str(ei.value))
    if how == "non_contiguous":
        p.data = good
    else:
        m.float()
    with torch.no_grad():
        outs, refs = run(m), ref(m)
    for i, (o, r) in enumerate(zip(outs, refs)):
        _chk_out(G, o, r, "%s after %s out[%d]" % (kind, how, i))


# ---------------------------------------------------------------------------------- 6. wide hidden sizes through the ops
WIDE = [128, 129, 144, 200]            # 128: the last resident size; above it the step-wise recurrence (no switch set)
TW, BW, DW = 3, 5, 7


@pytest.mark.parametrize("h", WIDE)
def test_wide_encoder(h):
    _need_gpu()
    G = "g6_wide_hidden"
    m, r = _enc(DW, h, h)
    xg, xr = _leaves(_randn(150, TW, BW, DW))
    out, ref = m.forward(xg), r(xr)
    _chk_out(G, out, ref, "encoder h=%d" % h)
    w = _randn(151, BW, h)
    (out * w.cuda()).sum().backward()
    (ref * w.double()).sum().backward()
    _chk_params(G, m, r, "encoder h=%d" % h)
    _chk_grad(G, xg.grad, xr.grad, "encoder h=%d dx" % h)


@pytest.mark.parametrize("h", WIDE)
def test_wide_decoder(h):
    _need_gpu()
    G = "g6_wide_hidden"
    m, r = _dec(h, DW, h)
    hg, hr = _leaves(_randn(152, BW, h))
    out, ref = m.forward(hg, TW), r(hr, TW)
    _chk_out(G, out, ref, "decoder h=%d" % h)
    w = _randn(153, TW, BW, DW)
    (out * w.cuda()).sum().backward()
    (ref * w.double()).sum().backward()
    _chk_params(G, m, r, "decoder h=%d" % h)
    _chk_grad(G, hg.grad, hr.grad, "decoder h=%d d_hT" % h)


@pytest.mark.parametrize("h", WIDE)
def test_wide_state_lstm_in_seq_group(h):
    """a wide state LSTM next to a narrow encoder in one call (the launch is split between the two recurrences), with
    gradients on both h_T and c_all"""
    _need_gpu()
    from factorized_amd import mfm_model as M
    G = "g6_wide_hidden"
    c, e = _cell(DW, h, h), _enc(DW, 20, h)
    xg, xr = _leaves(_randn(154, TW, BW, DW))
    eo, so = M.seq_group([(xg, e[0])], [(xg, c[0])])
    outs, refs = [eo[0], so[0][0], so[0][1]], [e[1](xr)] + list(_states_ref(c[1], xr))
    for i, (o, r) in enumerate(zip(outs, refs)):
        _chk_out(G, o, r, "seq_group h=%d out[%d]" % (h, i))
    ws = [_randn(155 + i, *r.shape) for i, r in enumerate(refs)]
    _wsum(outs, ws).backward()
    _wsum(refs, ws).backward()
    _chk_params(G, c[0], c[1], "state LSTM h=%d" % h)
    _chk_params(G, e[0], e[1], "encoder next to state LSTM h=%d" % h)
    _chk_grad(G, xg.grad, xr.grad, "seq_group h=%d dx" % h)


# ---------------------------------------------------------------------------------- 7. one module twice in one graph
def test_same_encoder_on_two_inputs():
    """enc(x1) + enc(x2), and the same encoderLSTM listed twice in one seq_group call: parameter gradients are the sum of
    both uses"""
    _need_gpu()
    from factorized_amd import mfm_model as M
    G = "g7_module_twice"
    T, B = 6, 5
    m, r = _enc(11, 20, 10)
    ag, ar = _leaves(_randn(160, T, B, 11))
    bg, br = _leaves(_randn(161, T, B, 11))
    w1, w2 = _randn(162, B, 20), _randn(163, B, 20)
    want = _wsum([r(ar), r(br)], [w1, w2])
    want.backward()
    _wsum([m.forward(ag), m.forward(bg)], [w1, w2]).backward()
    _chk_params(G, m, r, "enc(x1) + enc(x2)")
    _chk_grad(G, ag.grad, ar.grad, "enc(x1) + enc(x2) dx1")
    _chk_grad(G, bg.grad, br.grad, "enc(x1) + enc(x2) dx2")
    _zero(m, ag, bg)
    eo, _ = M.seq_group([(ag, m), (bg, m)], [])
    _wsum(eo, [w1, w2]).backward()
    _chk_params(G, m, r, "seq_group([enc, enc])")
    _chk_grad(G, ag.grad, ar.grad, "seq_group([enc, enc]) dx1")
    _chk_grad(G, bg.grad, br.grad, "seq_group([enc, enc]) dx2")


def test_same_decoder_twice_in_one_group():
    _need_gpu()
    from factorized_amd import mfm_model as M
    G = "g7_module_twice"
    T, B = 3, 5
    m, r = _dec(20, 11, 11)
    ag, ar = _leaves(_randn(164, B, 20))
    bg, br = _leaves(_randn(165, B, 20))
    ws = [_randn(166, T, B, 11), _randn(167, T, B, 11)]
    _wsum([r(ar, T), r(br, T)], ws).backward()
    _wsum(M.decoder_group([(ag, m), (bg, m)], T), ws).backward()
    _chk_params(G, m, r, "decoder_group([dec, dec])")
    _chk_grad(G, ag.grad, ar.grad, "decoder_group([dec, dec]) d_hT1")
    _chk_grad(G, bg.grad, br.grad, "decoder_group([dec, dec]) d_hT2")


def test_two_micro_batches_accumulate_per_tensor():
    """two micro-batches back-propagated without zero_grad in between: the first backward's .grads are views carved from one
    allocation (`_zeros_many`), the second accumulates into them -- each tensor's own sum, no neighbour touched"""
    _need_gpu()
    G = "g7_module_twice"
    T = 3
    (e, re_), (d, rd), (l, rl) = _enc(11, 20, 12), _dec(20, 7, 13), _lin(7, 4, 14)
    xs = [_randn(168, T, 5, 11), _randn(169, T, 9, 11)]            # (another batch size the second time)
    ws = [_randn(170, T, 5, 4), _randn(171, T, 9, 4)]
    for k, (x, w) in enumerate(zip(xs, ws)):
        (l(d.forward(e.forward(x.cuda()), T)) * w.cuda()).sum().backward()
        (rl(rd(re_(x.double()), T)) * w.double()).sum().backward()
        for m, r, n in ((e, re_, "encoder"), (d, rd, "decoder"), (l, rl, "linear")):
            _chk_params(G, m, r, "%s after micro-batch %d" % (n, k))
