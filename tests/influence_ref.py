"""Expected values of the gradient-based interpretation (model.influence / engine.influence_factors) from the CPU oracle, shared
by test_influence_host.py and test_gpu_influence.py: the forward-mode recursion in float64 on the oracle's decoder modules,
    fy[m, t, n] = sum_i sum_{j < fy_size}      (d x_m_hat[t, n, i] / d e[n, j])^2
    fm[m, t, n] = sum_i sum_{fy_size <= j < h} (d x_m_hat[t, n, i] / d e[n, j])^2,      e = [fy | f_m],
and the oracle's f computation from the four factors.  The values fall by orders of magnitude over the steps, so comparisons
are element by element (pointwise_err), never relative to a tensor's maximum."""
import copy

import numpy as np
import torch

DECODERS = ("decoder_l", "decoder_a", "decoder_v")


def oracle_model(variant, cfgs, weights):
    from oracle import mfm_oracle as O
    m = O.build(variant, cfgs)
    O.load_numpy_weights(m, weights)
    m.eval()
    return m


def oracle_z(m, x):
    """the means zl, za, zv, zy of a kl_ef / kl oracle model for x [T, N, D], as _Factorized.forward composes them"""
    with torch.no_grad():
        y_last = m.ef_encoder(x) if m.variant == "kl_ef" else m.mfn_encoder(x)
        return [m.last_to_zl_fc1(m.encoder_l(x[:, :, :m.d_l])), m.last_to_za_fc1(m.encoder_a(x[:, :, m.d_l:m.d_l + m.d_a])),
                m.last_to_zv_fc1(m.encoder_v(x[:, :, m.d_l + m.d_a:])), m.last_to_zy_fc1(y_last)]


def oracle_f(m, zl, za, zv, zy):
    """the oracle's factors fy, (fl, fa, fv) from z, as _Factorized.forward composes them (eval: dropout off), in z's dtype"""
    with torch.no_grad():
        return m._z_to_f("zy_to_fy", zy), [m._z_to_f("zl_to_fl", zl), m._z_to_f("za_to_fa", za), m._z_to_f("zv_to_fv", zv)]


def decoder_influence(dec, e, T, nfy):
    """one oracle SeqDecoder `dec`, embedding e [N, h] -> [2, T, N] float64: the recursion
        t = 0: a = W_ih e + b, J^a = W_ih;   t >= 1: a = (W_ih + W_hh) h_{t-1} + b, J^a = (W_ih + W_hh) J^h_{t-1}
        J^c_t = diag(f(1-f) c_{t-1}) J^a_f + diag(f) J^c_{t-1} + diag(i(1-i) g) J^a_i + diag(i(1-g^2)) J^a_g
        J^h_t = diag(o(1-o) tanh c_t) J^a_o + diag(o(1-tanh^2 c_t)) J^c_t;   J^x_t = W_fc1 J^h_t"""
    w_ih, w_hh = dec.lstm.weight_ih.detach().double(), dec.lstm.weight_hh.detach().double()
    b = dec.lstm.bias_ih.detach().double() + dec.lstm.bias_hh.detach().double()
    w_fc = dec.fc1.weight.detach().double()
    e = e.detach().double()
    N, h = e.shape
    out = torch.zeros(2, T, N, dtype=torch.float64)
    hx = torch.zeros(N, h, dtype=torch.float64)
    cx = torch.zeros(N, h, dtype=torch.float64)
    jh = jc = torch.zeros(N, h, h, dtype=torch.float64)
    for t in range(T):
        if t == 0:
            a = e @ w_ih.t() + b
            ja = w_ih.unsqueeze(0).expand(N, 4 * h, h)
        else:
            a = hx @ (w_ih + w_hh).t() + b
            ja = torch.einsum("gk,nkj->ngj", w_ih + w_hh, jh)
        i, f, g, o = [a[:, k * h:(k + 1) * h] for k in range(4)]
        i, f, g, o = torch.sigmoid(i), torch.sigmoid(f), torch.tanh(g), torch.sigmoid(o)
        ja_i, ja_f, ja_g, ja_o = [ja[:, k * h:(k + 1) * h] for k in range(4)]
        jc = ((f * (1 - f) * cx)[:, :, None] * ja_f + f[:, :, None] * jc
              + (i * (1 - i) * g)[:, :, None] * ja_i + (i * (1 - g * g))[:, :, None] * ja_g)
        cx = f * cx + i * g
        tc = torch.tanh(cx)
        hx = o * tc
        jh = (o * (1 - o) * tc)[:, :, None] * ja_o + (o * (1 - tc * tc))[:, :, None] * jc
        sq = torch.einsum("ik,nkj->nij", w_fc, jh).square().sum(dim=1)
        out[0, t] = sq[:, :nfy].sum(dim=1)
        out[1, t] = sq[:, nfy:].sum(dim=1)
    return out


def oracle_influence(m, zl, za, zv, zy, T):
    """oracle model `m` (eval; left as it is), the four factors z (CPU tensors) -> [2, 3, T, N] float64 ndarray"""
    md = copy.deepcopy(m).double()
    fy, fms = oracle_f(md, zl.double(), za.double(), zv.double(), zy.double())
    nfy = fy.shape[1]
    out = torch.stack([decoder_influence(getattr(md, name), torch.cat([fy, fm], dim=1), T, nfy)
                       for name, fm in zip(DECODERS, fms)], dim=1)
    return out.numpy()


def autograd_influence(dec, e, T, nfy):
    """the same [2, T, N] from torch.autograd.functional.jacobian of the oracle decoder's own forward (float64), row by row"""
    dec = copy.deepcopy(dec).double()
    e = e.detach().double()
    N = e.shape[0]
    out = np.zeros((2, T, N))
    for n in range(N):
        jac = torch.autograd.functional.jacobian(lambda v: dec(v[None], T)[:, 0], e[n])       # [T, d, h]
        sq = jac.square().sum(dim=1)
        out[0, :, n] = sq[:, :nfy].sum(dim=1).numpy()
        out[1, :, n] = sq[:, nfy:].sum(dim=1).numpy()
    return out


def pointwise_err(got, ref):
    """max over ALL elements of |got - ref| / |ref| (no reference value is zero: each is a positive sum of squares)"""
    got = np.asarray(got, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert np.all(np.abs(ref) > 0)
    return float((np.abs(got - ref) / np.abs(ref)).max())
