"""Drop-in mirror of the reference's `mfm_model.py` class surface on the MI355X HIP library.

    from factorized_amd.mfm_model import MFM_KL_EF, encoderLSTM, decoderLSTM, loss_KLD, loss_MMD

Same constructor signatures (six positional dicts, reference mfm_model.py:470/558/663), same
sub-module / parameter names (so `state_dict()` keys equal the reference's and reference
checkpoints `load_state_dict` cleanly), same `forward` contracts:

    encoderLSTM(d, h).forward(x[T,B,d])            -> [B,h]                (mfm_model.py:40-62)
    decoderLSTM(h, d).forward(hT[B,h], t)          -> [t,B,d]              (mfm_model.py:64-91)
    MFM_KL_EF(...).forward(x[T,B,D])               -> ([x_l_hat,x_a_hat,x_v_hat,y_hat], kld, 0.0)
                                                                           (mfm_model.py:619-660)
    MFM_KL(...) / MFM(...).forward(x)              -> same contract, zy from the MFN encoder
                                                                           (mfm_model.py:723-764 / 522-555)
    MFN(...).forward(x[T,B,D])                     -> [B, sum(h_dims)+memsize] (mfm_model.py:140-199)

Modules are ordinary `nn.Module`s: `.train()/.eval()/.parameters()`, `optim.Adam(model.parameters())`
and `loss.backward()` of a reference-style driver work unchanged.  Underneath, every forward and
backward runs on libmfm_hip.so (autograd.Function wrappers); there is NO PyTorch fallback -- CPU
tensors or a missing library raise.  `.cuda()` calls inside the reference's forwards
(mfm_model.py:51-52,76-77) are replaced by "allocate on x.device".

The fastest way to train is not this autograd path but `factorized_amd.engine.MFMEngine.train_step`
(one C call per step); `MFM_KL_EF.engine` exposes it on the same parameter storage.
"""
import torch
import torch.nn as nn

from . import _lib
from . import engine as E
from ._ops import (_MMDFn, _require_cuda, _hp, _ones, _zeros_many, _rows, _EncoderSeqFn, _DecoderSeqFn, _DecoderGroupFn,      # noqa: F401
                   decoder_group, _LinearFn, _MemFn, _GroupLinearFn, linear_group, HipLinear, _SeqGroupFn, seq_group)
from ._fused import (_PARAM_OWNERS, _owner_of, _FusedEngineMixin, _KLEFFn, _KLEFFastFn, _LazyRealFn, _lazy_forward,           # noqa: F401
                     _lazy_backward, _into_flat, _flat_backward_ext, _check_plan_live)


# ----------------------------------------------------------------------------------- losses
def loss_KLD(mu, logvar):
    """Sum (not mean) KL divergence to N(0,1) -- reference mfm_model.py:36-38."""
    return -0.5 * torch.sum(1 + logvar - mu.pow(2) - logvar.exp())


def compute_kernel(x, y):
    """Gaussian kernel with the reference's double division by dim -- mfm_model.py:14-23."""
    dim = x.size(1)
    diff = x.unsqueeze(1) - y.unsqueeze(0)
    return torch.exp(-(diff.pow(2).mean(2) / float(dim)))


def loss_MMD(zy, gauss=None):
    """MMD between zy and a N(0,1) sample of the same shape -- mfm_model.py:25-34.  The reference
    draws the sample on the host; pass `gauss` to inject it (parity tests)."""
    _require_cuda(zy, "loss_MMD")          # like every op of this package: no CPU path
    if gauss is None:
        gauss = torch.randn(zy.size(), device=zy.device, dtype=zy.dtype)
    if zy.dim() == 2 and zy.shape[1] <= 256:
        return _MMDFn.apply(zy, gauss)
    # feature dimensions above the kernel's register budget (256; the reference's z sizes are 8..80) and inputs that are not
    # [B, dim]: the reference's own composition of device ops (tests/test_gpu_ops.py::test_mmd_wide_features_device_ops)
    return compute_kernel(gauss, gauss).mean() + compute_kernel(zy, zy).mean() \
        - 2.0 * compute_kernel(gauss, zy).mean()


class encoderLSTM(nn.Module):
    def __init__(self, d, h):
        super(encoderLSTM, self).__init__()
        self.lstm = nn.LSTMCell(d, h)     # parameter container: weight_ih/hh, bias_ih/hh (torch init)
        self.fc1 = nn.Linear(h, h)
        self.h = h

    def forward(self, x):
        _require_cuda(x, "encoderLSTM.forward")
        return _EncoderSeqFn.apply(x, self.lstm.weight_ih, self.lstm.weight_hh, self.lstm.bias_ih,
                                   self.lstm.bias_hh, self.fc1.weight, self.fc1.bias)


class decoderLSTM(nn.Module):
    def __init__(self, h, d):
        super(decoderLSTM, self).__init__()
        self.lstm = nn.LSTMCell(h, h)
        self.fc1 = nn.Linear(h, d)
        self.d = d
        self.h = h

    def forward(self, hT, t):
        _require_cuda(hT, "decoderLSTM.forward")
        return _DecoderSeqFn.apply(hT, t, self.lstm.weight_ih, self.lstm.weight_hh, self.lstm.bias_ih,
                                   self.lstm.bias_hh, self.fc1.weight, self.fc1.bias)


class MFM_KL_EF(_FusedEngineMixin, nn.Module):
    def __init__(self, config, NN1Config, NN2Config, gamma1Config, gamma2Config, outConfig):
        super(MFM_KL_EF, self).__init__()
        self._configs = [config, NN1Config, NN2Config, gamma1Config, gamma2Config, outConfig]
        [self.d_l, self.d_a, self.d_v] = config["input_dims"]
        zy, zl, za, zv = config['zy_size'], config['zl_size'], config['za_size'], config['zv_size']
        fy, fl, fa, fv = config['fy_size'], config['fl_size'], config['fa_size'], config['fv_size']
        output_dim = config['output_dim']
        self.encoder_l = encoderLSTM(self.d_l, zl)
        self.encoder_a = encoderLSTM(self.d_a, za)
        self.encoder_v = encoderLSTM(self.d_v, zv)
        self.decoder_l = decoderLSTM(fy + fl, self.d_l)
        self.decoder_a = decoderLSTM(fy + fa, self.d_a)
        self.decoder_v = decoderLSTM(fy + fv, self.d_v)
        last_ef_size = zl + za + zv
        self.ef_encoder = encoderLSTM(self.d_l + self.d_a + self.d_v, last_ef_size)
        self.last_to_zy_fc1 = nn.Linear(last_ef_size, zy)
        self.last_to_logvarzy_fc1 = nn.Linear(last_ef_size, zy)
        self.last_to_zl_fc1 = nn.Linear(zl, zl)
        self.last_to_za_fc1 = nn.Linear(za, za)
        self.last_to_zv_fc1 = nn.Linear(zv, zv)
        self.last_to_logvarzl_fc1 = nn.Linear(zl, zl)
        self.last_to_logvarza_fc1 = nn.Linear(za, za)
        self.last_to_logvarzv_fc1 = nn.Linear(zv, zv)
        self.zy_to_fy_fc1 = nn.Linear(zy, fy)
        self.zy_to_fy_fc2 = nn.Linear(fy, fy)
        self.zy_to_fy_dropout = nn.Dropout(config['zy_to_fy_dropout'])
        self.zl_to_fl_fc1 = nn.Linear(zl, fl)
        self.zl_to_fl_fc2 = nn.Linear(fl, fl)
        self.zl_to_fl_dropout = nn.Dropout(config['zl_to_fl_dropout'])
        self.za_to_fa_fc1 = nn.Linear(za, fa)
        self.za_to_fa_fc2 = nn.Linear(fa, fa)
        self.za_to_fa_dropout = nn.Dropout(config['za_to_fa_dropout'])
        self.zv_to_fv_fc1 = nn.Linear(zv, fv)
        self.zv_to_fv_fc2 = nn.Linear(fv, fv)
        self.zv_to_fv_dropout = nn.Dropout(config['zv_to_fv_dropout'])
        self.fy_to_y_fc1 = nn.Linear(fy, fy)
        self.fy_to_y_fc2 = nn.Linear(fy, output_dim)
        self.fy_to_y_dropout = nn.Dropout(config['fy_to_y_dropout'])
        self._init_engine_slots()

    def forward(self, x):
        _require_cuda(x, "MFM_KL_EF.forward")
        if not (x.dtype == torch.float32 and x.is_contiguous()):
            x = x.contiguous().float()
        _ = self.engine
        if self._fast_ok():
            if self.lazy_losses and self.training and torch.is_grad_enabled() and not x.requires_grad:
                res = _lazy_forward(self, x)
                if res is not None:
                    return res
            if self._flat_leaf is None or self._flat_leaf.device != x.device:
                self._flat_leaf = torch.zeros((), device=x.device, requires_grad=True)
            x_l_hat, x_a_hat, x_v_hat, y_hat, kld = _KLEFFastFn.apply(x, self, self._flat_leaf)
        else:
            self._detach_grad_views()          # (a frozen parameter / a hook: per-tensor autograd owns the gradients from here)
            x_l_hat, x_a_hat, x_v_hat, y_hat, kld = _KLEFFn.apply(x, self, *self._plist)
        decoded = [x_l_hat, x_a_hat, x_v_hat, y_hat]
        missing_loss = 0.0
        return decoded, kld, missing_loss


class MFN(nn.Module):
    """Memory Fusion Network encoder, reference mfm_model.py:93-199 (same attribute names; `out_fc1/
    out_fc2/out_dropout` exist but are unused in forward, as in the reference).

    MI355X restructuring: the three LSTMs do NOT depend on the memory, so they run as whole-sequence
    HIP recurrences first (one launch); the attention and the c-hat proposal depend only on the cell
    states, so they are evaluated for ALL timesteps at once as [T*B, .] GEMMs; only the two gamma gates
    and the memory update are sequential in t (20 tiny steps).  Matmuls run on the HIP GEMM
    (`HipLinear`) and the sequential part is ONE persistent HIP kernel per direction (`_MemFn`,
    csrc/mfn_mem.hip); the batched elementwise glue (softmax/relu/tanh/concat) uses torch device ops."""

    def __init__(self, config, NN1Config, NN2Config, gamma1Config, gamma2Config, outConfig):
        super(MFN, self).__init__()
        [self.d_l, self.d_a, self.d_v] = config["input_dims"]
        [self.dh_l, self.dh_a, self.dh_v] = config["h_dims"]
        total_h_dim = self.dh_l + self.dh_a + self.dh_v
        self.mem_dim = config["memsize"]
        window_dim = config["windowsize"]
        output_dim = config['output_dim']
        attInShape = total_h_dim * window_dim
        gammaInShape = attInShape + self.mem_dim
        final_out = total_h_dim + self.mem_dim
        self.lstm_l = nn.LSTMCell(self.d_l, self.dh_l)
        self.lstm_a = nn.LSTMCell(self.d_a, self.dh_a)
        self.lstm_v = nn.LSTMCell(self.d_v, self.dh_v)
        self.att1_fc1 = HipLinear(attInShape, NN1Config["shapes"])
        self.att1_fc2 = HipLinear(NN1Config["shapes"], attInShape)
        self.att1_dropout = nn.Dropout(NN1Config["drop"])
        self.att2_fc1 = HipLinear(attInShape, NN2Config["shapes"])
        self.att2_fc2 = HipLinear(NN2Config["shapes"], self.mem_dim)
        self.att2_dropout = nn.Dropout(NN2Config["drop"])
        self.gamma1_fc1 = HipLinear(gammaInShape, gamma1Config["shapes"])
        self.gamma1_fc2 = HipLinear(gamma1Config["shapes"], self.mem_dim)
        self.gamma1_dropout = nn.Dropout(gamma1Config["drop"])
        self.gamma2_fc1 = HipLinear(gammaInShape, gamma2Config["shapes"])
        self.gamma2_fc2 = HipLinear(gamma2Config["shapes"], self.mem_dim)
        self.gamma2_dropout = nn.Dropout(gamma2Config["drop"])
        self.out_fc1 = HipLinear(final_out, outConfig["shapes"])
        self.out_fc2 = HipLinear(outConfig["shapes"], output_dim)
        self.out_dropout = nn.Dropout(outConfig["drop"])

    def forward(self, x, states=None):
        """`states` = [(h_T, c_all)] * 3 when the caller already ran the three LSTMs (MFM / MFM_KL group them
        with their own encoders into the same launches)."""
        _require_cuda(x, "MFN.forward")
        T, B = x.shape[0], x.shape[1]
        if states is None:
            x_l = x[:, :, :self.d_l]
            x_a = x[:, :, self.d_l:self.d_l + self.d_a]
            x_v = x[:, :, self.d_l + self.d_a:]
            _, states = seq_group([], [(x_l, self.lstm_l), (x_a, self.lstm_a), (x_v, self.lstm_v)])
        (hl, cl), (ha, ca), (hv, cv) = states
        new_cs = torch.cat([cl, ca, cv], dim=2)                                   # [T,B,tot]
        prev_cs = torch.cat([torch.zeros_like(new_cs[:1]), new_cs[:-1]], dim=0)   # c_{t-1}, zeros at t=0
        cStar = torch.cat([prev_cs, new_cs], dim=2)                               # mfm_model.py:171-173
        attention = torch.softmax(self.att1_fc2(self.att1_dropout(torch.relu(self.att1_fc1(cStar)))), dim=2)
        attended = attention * cStar                                              # :174-175, all t at once
        cHat = torch.tanh(self.att2_fc2(self.att2_dropout(torch.relu(self.att2_fc1(attended)))))   # :176
        # gamma gates: split W = [W_att | W_mem]; the attended part is batched over T, only the memory
        # part is sequential (:177-180)
        na = attended.shape[2]
        g1_att = _LinearFn.apply(attended, self.gamma1_fc1.weight[:, :na].contiguous(), self.gamma1_fc1.bias)
        g2_att = _LinearFn.apply(attended, self.gamma2_fc1.weight[:, :na].contiguous(), self.gamma2_fc1.bias)
        w1m = self.gamma1_fc1.weight[:, na:].contiguous()
        w2m = self.gamma2_fc1.weight[:, na:].contiguous()
        H1, H2 = w1m.shape[0], w2m.shape[0]
        if _MemFn.supported(self.mem_dim, H1, H2):
            # the sequential part (:177-181) as one persistent HIP kernel per direction
            mem = _MemFn.apply(g1_att, g2_att, cHat, w1m, w2m, self.gamma1_fc2.weight, self.gamma1_fc2.bias,
                               self.gamma2_fc2.weight, self.gamma2_fc2.bias,
                               self.gamma1_dropout.p, self.gamma2_dropout.p, self.training)
        else:
            # sizes beyond the register-resident kernel: same math step by step on the HIP GEMM
            zb1 = torch.zeros(H1, device=x.device)
            zb2 = torch.zeros(H2, device=x.device)
            mem = torch.zeros(B, self.mem_dim, device=x.device)
            for t in range(T):
                a1 = torch.relu(g1_att[t] + _LinearFn.apply(mem, w1m, zb1))
                a2 = torch.relu(g2_att[t] + _LinearFn.apply(mem, w2m, zb2))
                gamma1 = torch.sigmoid(self.gamma1_fc2(self.gamma1_dropout(a1)))
                gamma2 = torch.sigmoid(self.gamma2_fc2(self.gamma2_dropout(a2)))
                mem = gamma1 * mem + gamma2 * cHat[t]
        return torch.cat([hl, ha, hv, mem], dim=1)


class _FactorizedMFN(_FusedEngineMixin, nn.Module):
    """Shared body of MFM (MMD regulariser, mfm_model.py:469-555) and MFM_KL (KLD, :662-764): the
    three HIP sequence encoders/decoders around the MFN fusion encoder.

    `MFM_KL.forward` is ONE call of the fused plan (variant "kl", like MFM_KL_EF) since round 3 -- its backward takes
    arbitrary upstream gradients (mfm_plan_backward_ext), so the reference's unchanged loop runs on it: `fused_forward =
    False` or an input that requires grad select the composed autograd path below.  Round 4: `MFM.forward` is the fused plan
    too (variant "mmd"): the forward leaves d MMD / d z unscaled in the plan's seed record and the backward weighs it with
    whatever upstream gradient the caller's loss puts on the regulariser (`lda_mmd * mmd_loss` in the reference's loops), so the
    reference's unchanged loop runs on one plan call per direction for all three classes.  The N(0,1) samples loss_MMD draws
    per forward (reference mfm_model.py:26) come from torch's device generator ([B, zl+za+zv+zy] in one draw), or from
    `model.mmd_gauss` (four tensors, parity tests)."""
    fused_forward = True

    def __init__(self, use_kl, config, NN1Config, NN2Config, gamma1Config, gamma2Config, outConfig):
        super(_FactorizedMFN, self).__init__()
        self._use_kl = use_kl
        self._engine_variant = "kl" if use_kl else "mmd"
        self._configs = [config, NN1Config, NN2Config, gamma1Config, gamma2Config, outConfig]
        [self.d_l, self.d_a, self.d_v] = config["input_dims"]
        [self.dh_l, self.dh_a, self.dh_v] = config["h_dims"]
        zy, zl, za, zv = config['zy_size'], config['zl_size'], config['za_size'], config['zv_size']
        fy, fl, fa, fv = config['fy_size'], config['fl_size'], config['fa_size'], config['fv_size']
        last_mfn_size = self.dh_l + self.dh_a + self.dh_v + config["memsize"]
        output_dim = config['output_dim']
        self.encoder_l = encoderLSTM(self.d_l, zl)
        self.encoder_a = encoderLSTM(self.d_a, za)
        self.encoder_v = encoderLSTM(self.d_v, zv)
        self.decoder_l = decoderLSTM(fy + fl, self.d_l)
        self.decoder_a = decoderLSTM(fy + fa, self.d_a)
        self.decoder_v = decoderLSTM(fy + fv, self.d_v)
        self.mfn_encoder = MFN(config, NN1Config, NN2Config, gamma1Config, gamma2Config, outConfig)
        self.last_to_zy_fc1 = HipLinear(last_mfn_size, zy)
        if use_kl:
            self.last_to_logvarzy_fc1 = HipLinear(last_mfn_size, zy)
            self.last_to_zl_fc1 = HipLinear(zl, zl)
            self.last_to_za_fc1 = HipLinear(za, za)
            self.last_to_zv_fc1 = HipLinear(zv, zv)
            self.last_to_logvarzl_fc1 = HipLinear(zl, zl)
            self.last_to_logvarza_fc1 = HipLinear(za, za)
            self.last_to_logvarzv_fc1 = HipLinear(zv, zv)
        self.zy_to_fy_fc1 = HipLinear(zy, fy)
        self.zy_to_fy_fc2 = HipLinear(fy, fy)
        self.zy_to_fy_dropout = nn.Dropout(config['zy_to_fy_dropout'])
        self.zl_to_fl_fc1 = HipLinear(zl, fl)
        self.zl_to_fl_fc2 = HipLinear(fl, fl)
        self.zl_to_fl_dropout = nn.Dropout(config['zl_to_fl_dropout'])
        self.za_to_fa_fc1 = HipLinear(za, fa)
        self.za_to_fa_fc2 = HipLinear(fa, fa)
        self.za_to_fa_dropout = nn.Dropout(config['za_to_fa_dropout'])
        self.zv_to_fv_fc1 = HipLinear(zv, fv)
        self.zv_to_fv_fc2 = HipLinear(fv, fv)
        self.zv_to_fv_dropout = nn.Dropout(config['zv_to_fv_dropout'])
        self.fy_to_y_fc1 = HipLinear(fy, fy)
        self.fy_to_y_fc2 = HipLinear(fy, output_dim)
        self.fy_to_y_dropout = nn.Dropout(config['fy_to_y_dropout'])
        self.mmd_gauss = None      # optional injected N(0,1) samples [zl, za, zv, zy] (parity tests)
        self._init_engine_slots()

    def forward(self, x):
        _require_cuda(x, "%s.forward" % type(self).__name__)
        # (capturable since ABI 3: the plan's dropout streams and hand-over epochs add device words a captured step advances)
        if self.fused_forward and self._fast_ok() and not x.requires_grad:
            if not (x.dtype == torch.float32 and x.is_contiguous()):
                x = x.contiguous().float()
            eng = self.engine
            if not self._use_kl:
                g = self.mmd_gauss
                eng.gauss = None if g is None else torch.cat([t.to(x.device).float() for t in g], dim=1).contiguous()
            if self.lazy_losses and self.training and torch.is_grad_enabled():
                res = _lazy_forward(self, x)
                if res is not None:
                    return res
            if self._flat_leaf is None or self._flat_leaf.device != x.device:
                self._flat_leaf = torch.zeros((), device=x.device, requires_grad=True)
            x_l_hat, x_a_hat, x_v_hat, y_hat, kld = _KLEFFastFn.apply(x, self, self._flat_leaf)
            return [x_l_hat, x_a_hat, x_v_hat, y_hat], kld, 0.0
        self._detach_grad_views()              # composed autograd path: per-tensor gradients
        x_l = x[:, :, :self.d_l]
        x_a = x[:, :, self.d_l:self.d_l + self.d_a]
        x_v = x[:, :, self.d_l + self.d_a:]
        t = x.shape[0]
        mfn = self.mfn_encoder
        (zl_last, za_last, zv_last), states = seq_group(
            [(x_l, self.encoder_l), (x_a, self.encoder_a), (x_v, self.encoder_v)],
            [(x_l, mfn.lstm_l), (x_a, mfn.lstm_a), (x_v, mfn.lstm_v)])
        mfn_last = mfn.forward(x, states)
        if self._use_kl:
            zy, zl, za, zv, lvy, lvl, lva, lvv = linear_group([
                (mfn_last, self.last_to_zy_fc1), (zl_last, self.last_to_zl_fc1), (za_last, self.last_to_za_fc1),
                (zv_last, self.last_to_zv_fc1), (mfn_last, self.last_to_logvarzy_fc1),
                (zl_last, self.last_to_logvarzl_fc1), (za_last, self.last_to_logvarza_fc1),
                (zv_last, self.last_to_logvarzv_fc1)])
            reg = loss_KLD(zl, lvl) + loss_KLD(za, lva) + loss_KLD(zv, lvv) + loss_KLD(zy, lvy)
        else:
            zy = self.last_to_zy_fc1(mfn_last)
            zl, za, zv = zl_last, za_last, zv_last
            g = self.mmd_gauss if self.mmd_gauss is not None else [None] * 4
            reg = loss_MMD(zl, g[0]) + loss_MMD(za, g[1]) + loss_MMD(zv, g[2]) + loss_MMD(zy, g[3])
        missing_loss = 0.0
        relu = torch.relu
        h1 = linear_group([(zy, self.zy_to_fy_fc1), (zl, self.zl_to_fl_fc1), (za, self.za_to_fa_fc1),
                           (zv, self.zv_to_fv_fc1)])
        drops = (self.zy_to_fy_dropout, self.zl_to_fl_dropout, self.za_to_fa_dropout, self.zv_to_fv_dropout)
        h1 = [dr(relu(v)) for v, dr in zip(h1, drops)]
        fy, fl, fa, fv = [relu(v) for v in linear_group([(h1[0], self.zy_to_fy_fc2), (h1[1], self.zl_to_fl_fc2),
                                                          (h1[2], self.za_to_fa_fc2), (h1[3], self.zv_to_fv_fc2)])]
        x_l_hat, x_a_hat, x_v_hat = decoder_group([(torch.cat([fy, fl], dim=1), self.decoder_l),
                                                   (torch.cat([fy, fa], dim=1), self.decoder_a),
                                                   (torch.cat([fy, fv], dim=1), self.decoder_v)], t)
        y_hat = self.fy_to_y_fc2(self.fy_to_y_dropout(relu(self.fy_to_y_fc1(fy))))
        return [x_l_hat, x_a_hat, x_v_hat, y_hat], reg, missing_loss


class MFM(_FactorizedMFN):
    """reference mfm_model.py:469-555 (MMD-regularised, no logvar heads)."""

    def __init__(self, config, NN1Config, NN2Config, gamma1Config, gamma2Config, outConfig):
        super(MFM, self).__init__(False, config, NN1Config, NN2Config, gamma1Config, gamma2Config, outConfig)


class MFM_KL(_FactorizedMFN):
    """reference mfm_model.py:662-764 (KLD-regularised, zy from the MFN encoder)."""

    def __init__(self, config, NN1Config, NN2Config, gamma1Config, gamma2Config, outConfig):
        super(MFM_KL, self).__init__(True, config, NN1Config, NN2Config, gamma1Config, gamma2Config, outConfig)


# the reference keeps every model class in mfm_model.py: `from mfm_model import M_A, MFM_missing, ...` keeps working
def __getattr__(name):
    if name in ("M_A", "M_B", "M_C", "M_D", "MFM_missing", "seq2seq", "basic_missing"):
        from . import mfm_extra
        return getattr(mfm_extra, name)
    raise AttributeError("module %r has no attribute %r" % (__name__, name))
