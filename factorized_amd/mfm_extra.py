"""The reference's ablation and missing-modality model classes on the MI355X HIP ops (drop-in mirror of the rest of
`mfm_model.py`'s class surface):

    M_A, M_B, M_C, M_D             reference mfm_model.py:201-467   ablations of the factorization
    MFM_missing                    reference mfm_model.py:766-898   surrogate encoders for a missing modality
    seq2seq, basic_missing         reference mfm_model.py:900-1017  baselines of the missing-modality study

Same constructors (six dicts), sub-module / parameter names (`state_dict()` keys equal the reference's, checked in
tests/test_module_surface.py) and forward contracts.  They are re-wirings of the blocks `mfm_model.py` already runs on
libmfm_hip.so -- `encoderLSTM`, `decoderLSTM`, `MFN`, `HipLinear`, `loss_MMD` -- so they are COMPOSED from those
autograd ops here, with independent LSTMs / Linears sharing launches (`seq_group`, `decoder_group`, `linear_group`).
There is no fused one-call plan for these classes ("pure re-wiring of existing ops").

`MFM_missing.impute` is the exception: surrogate inference (a missing modality and the label from the other two) as one call
of the library, `mfm_impute_missing` (csrc/impute.hip).
"""
import collections
import ctypes as C

import torch
import torch.nn as nn

from . import _lib
from . import mfm_model as M
from .mfm_model import HipLinear, MFN, decoderLSTM, encoderLSTM, loss_MMD


class _Base(nn.Module):
    def __init__(self, config):
        super().__init__()
        [self.d_l, self.d_a, self.d_v] = config["input_dims"]
        self.mmd_gauss = None       # optional injected N(0,1) samples, in loss_MMD call order (parity tests)
        self._gi = 0

    def _split(self, x):
        return x[:, :, :self.d_l], x[:, :, self.d_l:self.d_l + self.d_a], x[:, :, self.d_l + self.d_a:]

    def _mmd(self, z):
        g = self.mmd_gauss[self._gi] if self.mmd_gauss is not None else None
        self._gi += 1
        return loss_MMD(z, g)

    def _zf(self, tag, cfg, zin, fout):
        setattr(self, tag + "_fc1", HipLinear(zin, fout))
        setattr(self, tag + "_fc2", HipLinear(fout, fout))
        setattr(self, tag + "_dropout", nn.Dropout(cfg[tag + "_dropout"]))

    def _z_to_f_many(self, pairs):
        """[(tag, z)] -> [relu(fc2(drop(relu(fc1(z)))))], the fc1s in one launch and the fc2s in one launch"""
        h1 = M.linear_group([(z, getattr(self, tag + "_fc1")) for tag, z in pairs])
        h1 = [getattr(self, tag + "_dropout")(torch.relu(v)) for (tag, _), v in zip(pairs, h1)]
        out = M.linear_group([(v, getattr(self, tag + "_fc2")) for (tag, _), v in zip(pairs, h1)])
        return [torch.relu(v) for v in out]

    def _classify(self, f):
        return self.fy_to_y_fc2(self.fy_to_y_dropout(torch.relu(self.fy_to_y_fc1(f))))

    def _classifier(self, cfg, fin, fy):
        self.fy_to_y_fc1 = HipLinear(fin, fy)
        self.fy_to_y_fc2 = HipLinear(fy, cfg["output_dim"])
        self.fy_to_y_dropout = nn.Dropout(cfg["fy_to_y_dropout"])


def _sizes(c):
    return (c["zy_size"], c["zl_size"], c["za_size"], c["zv_size"], c["fy_size"], c["fl_size"], c["fa_size"], c["fv_size"])


def _encode(pairs):
    """[(x, encoderLSTM)] -> [fc1(h_T)] in shared launches"""
    out, _ = M.seq_group(pairs, [])
    return out


class M_A(_Base):
    """reference mfm_model.py:201-266: one early-fusion encoder for z_l, MFN for z_y, all decoders fed [f_y, f_l]."""

    def __init__(self, config, NN1Config, NN2Config, gamma1Config, gamma2Config, outConfig):
        super(M_A, self).__init__(config)
        zy, zl, za, zv, fy, fl, fa, fv = _sizes(config)
        last = sum(config["h_dims"]) + config["memsize"]
        self.encoder_l = encoderLSTM(self.d_l + self.d_a + self.d_v, zl)
        self.decoder_l = decoderLSTM(fy + fl, self.d_l)
        self.decoder_a = decoderLSTM(fy + fl, self.d_a)
        self.decoder_v = decoderLSTM(fy + fl, self.d_v)
        self.mfn_encoder = MFN(config, NN1Config, NN2Config, gamma1Config, gamma2Config, outConfig)
        self.last_to_zy_fc1 = HipLinear(last, zy)
        self._zf("zy_to_fy", config, zy, fy)
        self._zf("zl_to_fl", config, zl, fl)
        self._classifier(config, fy, fy)

    def forward(self, x):
        M._require_cuda(x, "M_A.forward")
        self._gi = 0
        t = x.shape[0]
        zl = self.encoder_l.forward(x)
        zy = self.last_to_zy_fc1(self.mfn_encoder.forward(x))
        mmd_loss = self._mmd(zl) + self._mmd(zy)
        fy, fl = self._z_to_f_many([("zy_to_fy", zy), ("zl_to_fl", zl)])
        fyfl = torch.cat([fy, fl], dim=1)
        x_l_hat, x_a_hat, x_v_hat = M.decoder_group([(fyfl, self.decoder_l), (fyfl, self.decoder_a), (fyfl, self.decoder_v)], t)
        return [x_l_hat, x_a_hat, x_v_hat, self._classify(fy)], mmd_loss, 0.0


class M_B(_Base):
    """reference mfm_model.py:268-335: modality-specific factors only; the classifier reads [f_l, f_a, f_v]."""

    def __init__(self, config, NN1Config, NN2Config, gamma1Config, gamma2Config, outConfig):
        super(M_B, self).__init__(config)
        zy, zl, za, zv, fy, fl, fa, fv = _sizes(config)
        self.encoder_l = encoderLSTM(self.d_l, zl)
        self.encoder_a = encoderLSTM(self.d_a, za)
        self.encoder_v = encoderLSTM(self.d_v, zv)
        self.decoder_l = decoderLSTM(fl, self.d_l)
        self.decoder_a = decoderLSTM(fa, self.d_a)
        self.decoder_v = decoderLSTM(fv, self.d_v)
        self._zf("zl_to_fl", config, zl, fl)
        self._zf("za_to_fa", config, za, fa)
        self._zf("zv_to_fv", config, zv, fv)
        self._classifier(config, fl + fa + fv, fy)

    def forward(self, x):
        M._require_cuda(x, "M_B.forward")
        self._gi = 0
        t = x.shape[0]
        x_l, x_a, x_v = self._split(x)
        zl, za, zv = _encode([(x_l, self.encoder_l), (x_a, self.encoder_a), (x_v, self.encoder_v)])
        mmd_loss = self._mmd(zl) + self._mmd(za) + self._mmd(zv)
        fl, fa, fv = self._z_to_f_many([("zl_to_fl", zl), ("za_to_fa", za), ("zv_to_fv", zv)])
        x_l_hat, x_a_hat, x_v_hat = M.decoder_group([(fl, self.decoder_l), (fa, self.decoder_a), (fv, self.decoder_v)], t)
        y_hat = self._classify(torch.cat([fl, fa, fv], dim=1))
        return [x_l_hat, x_a_hat, x_v_hat, y_hat], mmd_loss, 0.0


class M_C(_Base):
    """reference mfm_model.py:337-387: the multimodal factor only (MFN -> z_y -> f_y feeds every decoder)."""

    def __init__(self, config, NN1Config, NN2Config, gamma1Config, gamma2Config, outConfig):
        super(M_C, self).__init__(config)
        zy, zl, za, zv, fy, fl, fa, fv = _sizes(config)
        last = sum(config["h_dims"]) + config["memsize"]
        self.decoder_l = decoderLSTM(fy, self.d_l)
        self.decoder_a = decoderLSTM(fy, self.d_a)
        self.decoder_v = decoderLSTM(fy, self.d_v)
        self.mfn_encoder = MFN(config, NN1Config, NN2Config, gamma1Config, gamma2Config, outConfig)
        self.last_to_zy_fc1 = HipLinear(last, zy)
        self._zf("zy_to_fy", config, zy, fy)
        self._classifier(config, fy, fy)

    def forward(self, x):
        M._require_cuda(x, "M_C.forward")
        self._gi = 0
        t = x.shape[0]
        zy = self.last_to_zy_fc1(self.mfn_encoder.forward(x))
        mmd_loss = self._mmd(zy)
        (fy,) = self._z_to_f_many([("zy_to_fy", zy)])
        x_l_hat, x_a_hat, x_v_hat = M.decoder_group([(fy, self.decoder_l), (fy, self.decoder_a), (fy, self.decoder_v)], t)
        return [x_l_hat, x_a_hat, x_v_hat, self._classify(fy)], mmd_loss, 0.0


class M_D(_Base):
    """reference mfm_model.py:389-467: purely discriminative (no decoders; `decoded` carries the inputs back)."""

    def __init__(self, config, NN1Config, NN2Config, gamma1Config, gamma2Config, outConfig):
        super(M_D, self).__init__(config)
        zy, zl, za, zv, fy, fl, fa, fv = _sizes(config)
        self.encoder_l = encoderLSTM(self.d_l, zl)
        self.encoder_a = encoderLSTM(self.d_a, za)
        self.encoder_v = encoderLSTM(self.d_v, zv)
        self._zf("zl_to_fl", config, zl, fl)
        self._zf("za_to_fa", config, za, fa)
        self._zf("zv_to_fv", config, zv, fv)
        self.fs_to_y = HipLinear(fl + fa + fv, config["output_dim"])

    def forward(self, x):
        M._require_cuda(x, "M_D.forward")
        x_l, x_a, x_v = self._split(x)
        zl, za, zv = _encode([(x_l, self.encoder_l), (x_a, self.encoder_a), (x_v, self.encoder_v)])
        fl, fa, fv = self._z_to_f_many([("zl_to_fl", zl), ("za_to_fa", za), ("zv_to_fv", zv)])
        y_hat = self.fs_to_y(torch.cat([fl, fa, fv], dim=1))
        return [x_l, x_a, x_v, y_hat], 0.0, 0.0


Imputed = collections.namedtuple("Imputed", ["x_hat", "y_hat"])


def _lstm_fc(mod):
    """the six tensors of an encoderLSTM / decoderLSTM in the order of the C ABI (plain dict look-ups: always the current ones)"""
    lp, fp = mod._modules["lstm"]._parameters, mod._modules["fc1"]._parameters
    return [lp["weight_ih"], lp["weight_hh"], lp["bias_ih"], lp["bias_hh"], fp["weight"], fp["bias"]]


def _wb(lin):
    return [lin._parameters["weight"], lin._parameters["bias"]]


class MFM_missing(_Base):
    """reference mfm_model.py:766-898: MFM plus six surrogate encoders that predict a modality's (and z_y's) code
    from the other two modalities; forward returns the four decodings (all present / no l / no a / no v).
    `impute(x, missing)`: the no-<missing> decoding's reconstruction of that modality and its label from the other two
    modalities alone, as one call of the library."""

    IMPUTE_MAX_ROWS = 1024       # default row cap of impute(): the x-projections of at most this many rows are alive at once
    MAX_RESIDENT_H = 128         # widest LSTM of the on-chip recurrences (csrc/lstm_seq_dev.h, MFM_SEQ_MAX_RESIDENT_H)
    _CASES = ("l", "a", "v")
    _PAIR = {"l": "av", "a": "lv", "v": "la"}       # the observed pair of each case

    def __init__(self, config, NN1Config, NN2Config, gamma1Config, gamma2Config, outConfig):
        super(MFM_missing, self).__init__(config)
        zy, zl, za, zv, fy, fl, fa, fv = _sizes(config)
        d_l, d_a, d_v = self.d_l, self.d_a, self.d_v
        last = sum(config["h_dims"]) + config["memsize"]
        self.encoder_l = encoderLSTM(d_l, zl)
        self.encoder_a = encoderLSTM(d_a, za)
        self.encoder_v = encoderLSTM(d_v, zv)
        self.encoder_la_to_v = encoderLSTM(d_l + d_a, zv)
        self.encoder_lv_to_a = encoderLSTM(d_l + d_v, za)
        self.encoder_av_to_l = encoderLSTM(d_a + d_v, zl)
        self.encoder_la_to_y = encoderLSTM(d_l + d_a, zy)
        self.encoder_lv_to_y = encoderLSTM(d_l + d_v, zy)
        self.encoder_av_to_y = encoderLSTM(d_a + d_v, zy)
        self.decoder_l = decoderLSTM(fy + fl, d_l)
        self.decoder_a = decoderLSTM(fy + fa, d_a)
        self.decoder_v = decoderLSTM(fy + fv, d_v)
        self.mfn_encoder = MFN(config, NN1Config, NN2Config, gamma1Config, gamma2Config, outConfig)
        self.last_to_zy_fc1 = HipLinear(last, zy)
        self._zf("zy_to_fy", config, zy, fy)
        self._zf("zl_to_fl", config, zl, fl)
        self._zf("za_to_fa", config, za, fa)
        self._zf("zv_to_fv", config, zv, fv)
        self._classifier(config, fy, fy)

    def forward(self, x):
        M._require_cuda(x, "MFM_missing.forward")
        self._gi = 0
        t = x.shape[0]
        x_l, x_a, x_v = self._split(x)
        la = x[:, :, :self.d_l + self.d_a]                       # cat([x_l, x_a]) is a contiguous column range
        av = x[:, :, self.d_l:]
        lv = torch.cat([x_l, x_v], dim=2)
        mfn = self.mfn_encoder
        # nine sequence encoders + the MFN's three LSTMs: shared projection / recurrence / head launches
        encs, states = M.seq_group(
            [(x_l, self.encoder_l), (x_a, self.encoder_a), (x_v, self.encoder_v),
             (la, self.encoder_la_to_v), (lv, self.encoder_lv_to_a), (av, self.encoder_av_to_l),
             (la, self.encoder_la_to_y), (lv, self.encoder_lv_to_y), (av, self.encoder_av_to_y)],
            [(x_l, mfn.lstm_l), (x_a, mfn.lstm_a), (x_v, mfn.lstm_v)])
        zl, za, zv, zv_nov, za_noa, zl_nol, zy_nov, zy_noa, zy_nol = encs
        zy = self.last_to_zy_fc1(mfn.forward(x, states))
        mmd_loss = self._mmd(zl) + self._mmd(za) + self._mmd(zv) + self._mmd(zy)
        mse = torch.nn.functional.mse_loss
        missing_loss = mse(zv_nov, zv) + mse(za_noa, za) + mse(zl_nol, zl) + mse(zy_nov, zy) + mse(zy_noa, zy) + mse(zy_nol, zy)

        def decode(zl, za, zv, zy):
            fy, fl, fa, fv = self._z_to_f_many([("zy_to_fy", zy), ("zl_to_fl", zl), ("za_to_fa", za), ("zv_to_fv", zv)])
            x_l_hat, x_a_hat, x_v_hat = M.decoder_group([(torch.cat([fy, fl], dim=1), self.decoder_l),
                                                         (torch.cat([fy, fa], dim=1), self.decoder_a),
                                                         (torch.cat([fy, fv], dim=1), self.decoder_v)], t)
            return [x_l_hat, x_a_hat, x_v_hat, self._classify(fy)]
        decoded = decode(zl, za, zv, zy)
        decoded_nol = decode(zl_nol, za, zv, zy_nol)
        decoded_noa = decode(zl, za_noa, zv, zy_noa)
        decoded_nov = decode(zl, za, zv_nov, zy_nov)
        return decoded, decoded_nol, decoded_noa, decoded_nov, mmd_loss, missing_loss

    # ------------------------------------------------------------------ surrogate inference
    def __getstate__(self):
        state = dict(self.__dict__)
        state.pop("_impute_bufs", None)          # (device workspaces and native pointer tables: rebuilt on the next call)
        return state

    def _impute_params(self, cases):
        """the 74 tensors of mfm_impute_missing's parameter table (include/mfm_hip.h); None for the cases not asked for"""
        mods = self._modules
        out = []
        for m in self._CASES:
            if m not in cases:
                out += [None] * 22
                continue
            pair = self._PAIR[m]
            out += _lstm_fc(mods["encoder_%s_to_%s" % (pair, m)]) + _lstm_fc(mods["encoder_%s_to_y" % pair])
            out += _wb(mods["z%s_to_f%s_fc1" % (m, m)]) + _wb(mods["z%s_to_f%s_fc2" % (m, m)]) + _lstm_fc(mods["decoder_" + m])
        for name in ("zy_to_fy_fc1", "zy_to_fy_fc2", "fy_to_y_fc1", "fy_to_y_fc2"):
            out += _wb(mods[name])
        return out

    def _impute_sizes(self):
        """zl, za, zv, zy, fl, fa, fv, fy, d_l, d_a, d_v, output_dim, read off the parameters"""
        shp = [tuple(self._modules[n]._parameters["weight"].shape) for n in ("zl_to_fl_fc1", "za_to_fa_fc1", "zv_to_fv_fc1", "zy_to_fy_fc1")]
        return tuple(s[1] for s in shp) + tuple(s[0] for s in shp) + (self.d_l, self.d_a, self.d_v, self.fy_to_y_fc2.weight.shape[0])

    def _impute_composed(self, x, missing):
        """impute() for ONE case as the composition of this module's own sub-modules (the granular HIP operations); the dropout
        modules are left out (eval)"""
        relu = torch.relu
        d_l, d_a = self.d_l, self.d_a
        # a COPY of the observed pair, never a column slice of x: the projection GEMM masks the 16-byte fetches that pass a row's
        # K range by multiplying with zero, and on a slice those fetches meet the missing modality's columns (csrc/impute.hip)
        pair = {"l": lambda: x[:, :, d_l:].contiguous(), "v": lambda: x[:, :, :d_l + d_a].contiguous(),
                "a": lambda: torch.cat([x[:, :, :d_l], x[:, :, d_l + d_a:]], dim=2)}[missing]()
        name = self._PAIR[missing]
        zm, zy = _encode([(pair, getattr(self, "encoder_%s_to_%s" % (name, missing))), (pair, getattr(self, "encoder_%s_to_y" % name))])
        tag = "z%s_to_f%s" % (missing, missing)
        h1 = M.linear_group([(zy, self.zy_to_fy_fc1), (zm, getattr(self, tag + "_fc1"))])
        fy, fm = [relu(v) for v in M.linear_group([(relu(h1[0]), self.zy_to_fy_fc2), (relu(h1[1]), getattr(self, tag + "_fc2"))])]
        x_hat, = M.decoder_group([(torch.cat([fy, fm], dim=1), getattr(self, "decoder_" + missing))], x.shape[0])
        y1, = M.linear_group([(fy, self.fy_to_y_fc1)])
        y_hat, = M.linear_group([(relu(y1), self.fy_to_y_fc2)])
        return Imputed(x_hat, y_hat)

    def _impute_fused(self, x, cases, params, cap):
        """mfm_impute_missing on the module's own tensors; MfmUnsupported when the entry refuses the sizes"""
        T, N, _ = x.shape
        L = _lib.lib()
        bits = sum(1 << self._CASES.index(m) for m in cases)
        cache = self.__dict__.setdefault("_impute_bufs", {})
        key = (T, N, bits, cap, x.device)
        st = cache.get(key)
        if st is False:
            raise _lib.MfmUnsupported("MFM_missing.impute: mfm_impute_missing refused this shape")
        if st is None:
            sz = self._impute_sizes()
            sizes = (C.c_int32 * 12)(*sz)
            nws = int(L.mfm_impute_missing_workspace_floats(T, N, sizes, bits, cap))
            outs, optr = {}, (C.c_void_p * 6)()
            for i, m in enumerate(self._CASES):
                if m in cases:
                    outs[m] = Imputed(torch.empty(T, N, sz[8 + i], dtype=torch.float32, device=x.device),
                                      torch.empty(N, sz[11], dtype=torch.float32, device=x.device))
                    optr[2 * i], optr[2 * i + 1] = outs[m].x_hat.data_ptr(), outs[m].y_hat.data_ptr()
            st = (torch.empty(max(nws, 4), dtype=torch.float32, device=x.device), outs, sizes, optr, (C.c_void_p * 74)())
        ws, outs, sizes, optr, pptr = st
        for i, p in enumerate(params):
            pptr[i] = None if p is None else p.data_ptr()
        rc = L.mfm_impute_missing(T, N, sizes, bits, pptr, C.c_void_p(x.data_ptr()), C.c_void_p(ws.data_ptr()), optr, cap,
                                  C.c_void_p(torch._C._cuda_getCurrentRawStream(x.device.index)))
        if rc == _lib.MFM_ERR_UNSUPPORTED:
            # a hidden size beyond the on-chip recurrence is a property of the model: remembered.  The LDS limit also depends on the
            # tile rows, hence on N and max_rows: that refusal is remembered for this shape alone (no buffers are kept for it)
            sz = self._impute_sizes()
            self._impute_refused = max(max(sz[0:4]), sz[7] + max(sz[4:7])) > self.MAX_RESIDENT_H
            if not self._impute_refused:
                cache[key] = False
            raise _lib.MfmUnsupported("MFM_missing.impute: %s" % L.mfm_last_error().decode())
        _lib.check(rc, "mfm_impute_missing")
        cache[key] = st
        return outs

    def impute(self, x, missing, *, max_rows=None):
        """x [T, N, D] (columns d_l | d_a | d_v), missing in "l" / "a" / "v" -> Imputed(x_hat [T, N, d_missing], y_hat [N, output_dim]):
        the missing modality and the label from the other two modalities -- decoded_no<missing>[index of missing] and
        decoded_no<missing>[3] of forward() (reference mfm_model.py:860-885; evaluated in mfm_mosi.py:572-596, :1023-1062).  THE
        COLUMNS OF THE MISSING MODALITY ARE NEVER READ: they may hold anything, NaN included.  missing="each": all three cases
        from a complete x in shared launches, as {"l": Imputed, "a": Imputed, "v": Imputed}.

        Always the deterministic eval computation (dropout off), `self.training` left as found, without autograd; T of x is the
        decoding length.  One call of mfm_impute_missing (csrc/impute.hip): the two surrogate encoders of a case, its z -> f
        MLPs, decoder and the classifier -- no MFN, no own-modality encoder, no other decoder; the split is walked in chunks of
        at most `max_rows` rows (default IMPUTE_MAX_ROWS).  Workspace and outputs are kept on the module (outside state_dict())
        per (T, N, missing, max_rows) and REUSED: after the first call for a shape nothing is allocated and nothing synchronises
        (legal inside a stream capture), and the returned tensors are overwritten by the next call for the same shape -- clone
        what must survive it.  "each" gives the bits of the three single calls as long as both run on the same tile rows: the
        rule counts the workgroups of a launch, so "each" turns to four-row tiles at a third of the rows per chunk at which a
        single call does (in between -- about CUs to 3 CUs rows per chunk -- the two agree to rounding, not bit for bit;
        include/mfm_hip.h, mfm_impute_missing_tile_rows).  A device x that is not contiguous float32 is converted.  Sizes the
        entry refuses (a hidden size above 128, LDS beyond a CU's) take `_impute_composed`, the composition of the module's own
        operations, which reads a copy of the observed columns.  So does a model with a parameter that is not a contiguous
        float32 tensor on x's device, and there the operations' own check raises MfmError naming the tensor (convert the module
        back first).  A CPU model or input raises MfmError: there is no CPU fallback."""
        if missing not in ("l", "a", "v", "each"):
            raise ValueError("MFM_missing.impute: missing must be 'l', 'a', 'v' or 'each', not %r" % (missing,))
        dev = self.fy_to_y_fc1.weight.device
        if dev.type != "cuda":
            raise _lib.MfmError("MFM_missing.impute: parameters are on %s; move the model to the GPU first (no CPU fallback)" % dev)
        D = self.d_l + self.d_a + self.d_v
        if not torch.is_tensor(x) or x.dim() != 3:
            raise _lib.MfmError("MFM_missing.impute: x must be a CUDA tensor [T, N, %d]; got %s" % (
                D, tuple(x.shape) if torch.is_tensor(x) else type(x)))
        M._require_cuda(x, "MFM_missing.impute")
        if x.device != dev:
            raise _lib.MfmError("MFM_missing.impute: x lives on %s, the model on %s" % (x.device, dev))
        if x.shape[2] != D:
            raise _lib.MfmError("MFM_missing.impute: x has %d features per time step, the model's input_dims sum to %d" % (x.shape[2], D))
        if x.shape[0] < 1 or x.shape[1] < 1:
            raise _lib.MfmError("MFM_missing.impute: empty split %s" % (tuple(x.shape),))
        if max_rows is not None and int(max_rows) < 1:
            raise _lib.MfmError("MFM_missing.impute: max_rows must be at least 1, not %r" % (max_rows,))
        cap = self.IMPUTE_MAX_ROWS if max_rows is None else int(max_rows)
        if not (x.dtype == torch.float32 and x.is_contiguous()):
            x = x.contiguous().float()
        cases = self._CASES if missing == "each" else (missing,)
        with torch.no_grad():
            if not getattr(self, "_impute_refused", False):
                params = self._impute_params(cases)
                if all(p is None or (p.dtype == torch.float32 and p.device == dev and p.is_contiguous()) for p in params):
                    try:
                        outs = self._impute_fused(x, cases, params, cap)
                        return dict(outs) if missing == "each" else outs[missing]
                    except _lib.MfmUnsupported:
                        pass
            if missing == "each":
                return {m: self._impute_composed(x, m) for m in cases}
            return self._impute_composed(x, missing)


class seq2seq(_Base):
    """reference mfm_model.py:900-960: reconstruct each modality from the other two (no multimodal factor)."""

    def __init__(self, config, NN1Config, NN2Config, gamma1Config, gamma2Config, outConfig):
        super(seq2seq, self).__init__(config)
        zy, zl, za, zv, fy, fl, fa, fv = _sizes(config)
        d_l, d_a, d_v = self.d_l, self.d_a, self.d_v
        self.encoder_la_to_v = encoderLSTM(d_l + d_a, zv)
        self.encoder_lv_to_a = encoderLSTM(d_l + d_v, za)
        self.encoder_av_to_l = encoderLSTM(d_a + d_v, zl)
        self.decoder_l = decoderLSTM(fl, d_l)
        self.decoder_a = decoderLSTM(fa, d_a)
        self.decoder_v = decoderLSTM(fv, d_v)
        self._zf("zl_to_fl", config, zl, fl)
        self._zf("za_to_fa", config, za, fa)
        self._zf("zv_to_fv", config, zv, fv)

    def forward(self, x):
        M._require_cuda(x, "seq2seq.forward")
        self._gi = 0
        t = x.shape[0]
        x_l, x_a, x_v = self._split(x)
        la, av, lv = x[:, :, :self.d_l + self.d_a], x[:, :, self.d_l:], torch.cat([x_l, x_v], dim=2)
        zv_nov, za_noa, zl_nol = _encode([(la, self.encoder_la_to_v), (lv, self.encoder_lv_to_a), (av, self.encoder_av_to_l)])
        mmd_loss = self._mmd(zv_nov) + self._mmd(za_noa) + self._mmd(zl_nol)
        fl, fa, fv = self._z_to_f_many([("zl_to_fl", zl_nol), ("za_to_fa", za_noa), ("zv_to_fv", zv_nov)])
        x_l_hat, x_a_hat, x_v_hat = M.decoder_group([(fl, self.decoder_l), (fa, self.decoder_a), (fv, self.decoder_v)], t)
        return [x_l_hat], [x_a_hat], [x_v_hat], mmd_loss


class basic_missing(_Base):
    """reference mfm_model.py:962-1017: predict the label from two modalities, one small head per missing modality."""

    def __init__(self, config, NN1Config, NN2Config, gamma1Config, gamma2Config, outConfig):
        super(basic_missing, self).__init__(config)
        zy, zl, za, zv, fy, fl, fa, fv = _sizes(config)
        d_l, d_a, d_v = self.d_l, self.d_a, self.d_v
        self.encoder_la_to_y = encoderLSTM(d_l + d_a, zy)
        self.encoder_lv_to_y = encoderLSTM(d_l + d_v, zy)
        self.encoder_av_to_y = encoderLSTM(d_a + d_v, zy)
        for tag in ("zy_nol_to_y", "zy_noa_to_y", "zy_nov_to_y"):
            setattr(self, tag + "_fc1", HipLinear(zy, fy))
            setattr(self, tag + "_fc2", HipLinear(fy, config["output_dim"]))
            setattr(self, tag + "_dropout", nn.Dropout(config["zy_to_fy_dropout"]))

    def forward(self, x):
        M._require_cuda(x, "basic_missing.forward")
        self._gi = 0
        x_l, x_a, x_v = self._split(x)
        la, av, lv = x[:, :, :self.d_l + self.d_a], x[:, :, self.d_l:], torch.cat([x_l, x_v], dim=2)
        zy_nov, zy_noa, zy_nol = _encode([(la, self.encoder_la_to_y), (lv, self.encoder_lv_to_y), (av, self.encoder_av_to_y)])
        mmd_loss = self._mmd(zy_nov) + self._mmd(zy_noa) + self._mmd(zy_nol)
        tags, zs = ("zy_nol_to_y", "zy_noa_to_y", "zy_nov_to_y"), (zy_nol, zy_noa, zy_nov)
        h = M.linear_group([(z, getattr(self, t_ + "_fc1")) for t_, z in zip(tags, zs)])
        h = [getattr(self, t_ + "_dropout")(torch.relu(v)) for t_, v in zip(tags, h)]
        y_hat_nol, y_hat_noa, y_hat_nov = M.linear_group([(v, getattr(self, t_ + "_fc2")) for t_, v in zip(tags, h)])
        return y_hat_nol, y_hat_noa, y_hat_nov, mmd_loss
