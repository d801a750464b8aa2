"""The reference's ablation and missing-modality model classes on the MI355X HIP ops (drop-in mirror of the rest of
`mfm_model.py`'s class surface):

    M_A, M_B, M_C, M_D             reference mfm_model.py:201-467   ablations of the factorization
    MFM_missing                    reference mfm_model.py:766-898   surrogate encoders for a missing modality
    seq2seq, basic_missing         reference mfm_model.py:900-1017  baselines of the missing-modality study

Same constructors (six dicts), sub-module / parameter names (`state_dict()` keys equal the reference's, checked in
tests/test_module_surface.py) and forward contracts.  They are re-wirings of the blocks `mfm_model.py` already runs on
libmfm_hip.so -- `encoderLSTM`, `decoderLSTM`, `MFN`, `HipLinear`, `loss_MMD` -- so they are COMPOSED from those
autograd ops here, with independent LSTMs / Linears sharing launches (`seq_group`, `decoder_group`, `linear_group`).
There is no fused one-call plan for these classes ("pure re-wiring of existing ops"); the one training
entry so far is `M_D.loss_and_grad`: the label loss and every parameter's gradient as one call of `mfm_train_ablation_d`
(csrc/train_ablation.hip), without autograd.

`MFM_missing.impute` is the exception: surrogate inference (a missing modality and the label from the other two) as one call
of the library, `mfm_impute_missing` (csrc/impute.hip).  So is `predict_missing` of MFM_missing, seq2seq and basic_missing: the
missing-modality test protocol (per missing case the label, the error of the rebuilt modality and the label loss) as one call,
`mfm_predict_missing` (csrc/missing.hip); and `predict` / `evaluate` of the four ablations -- what the `evaluate` / `predict` blocks
of the reference's train_mfm_ablation report --: M_B and M_D through `mfm_predict_ablation` (csrc/ablation.hip), M_A and M_C, whose
label factor comes from the Memory Fusion Network, through `mfm_predict_ablation_mfn` (csrc/ablation_mfn.hip).  One mixin,
`_AblationProtocol`, carries the protocol; `_AblationMfnProtocol` gives the MFN pair its parameter table, sizes, entry call and
composed fallback.
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


Ablation = collections.namedtuple("Ablation", ["y_hat", "gen", "disc"])


class _AblationProtocol:
    """`predict` / `evaluate` of the ablations: argument checks, the buffer cache, the remembered refusals and the composed
    fallback around one call of the class's library entry.  As it stands it serves the ablations whose three own-modality
    encoders meet at the label head, mfm_predict_ablation (csrc/ablation.hip): a class names its family (`_ABL_FAMILY`: 0 M_B,
    1 M_D) and gives `_ablation_head()`, the tensors of its label head.  `_AblationMfnProtocol` replaces what is the entry's own:
    `_ablation_sizes`, `_ablation_params`, `_ablation_composed`, `_ablation_ws_floats`, `_ablation_entry`, `_ablation_wide`."""

    ABLATION_MAX_ROWS = 1024     # default row cap: the x-projections of at most this many rows are alive at once
    MAX_RESIDENT_H = 128         # widest LSTM of the on-chip recurrences (csrc/lstm_seq_dev.h, MFM_SEQ_MAX_RESIDENT_H)
    _MODS = ("l", "a", "v")
    _LOSS = {"l1": 0, "ce": 1}
    _ABL_ENTRY = "mfm_predict_ablation"
    _ABL_NPARAM = 52             # pointers of the entry's parameter table
    _ABL_OD = 11                 # where output_dim stands among the entry's sizes
    _ABL_HAS_GEN = True          # the class has decoders

    def __getstate__(self):
        state = dict(self.__dict__)
        state.pop("_ablation_bufs", None)        # (device workspaces and native pointer tables: rebuilt on the next call)
        state.pop("_train_bufs", None)           # (those of M_D.loss_and_grad, and which of them the latest call used)
        state.pop("_train_last", None)
        return state

    def _ablation_check_x(self, name, x, dev, max_rows, cuda):
        """the checks of a split x [T, N, D] and a row cap against a model on `dev`; cuda: x must be a device tensor"""
        D = self.d_l + self.d_a + self.d_v
        if not torch.is_tensor(x) or x.dim() != 3:
            raise _lib.MfmError("%s: x must be a %stensor [T, N, %d]; got %s" % (name, "CUDA " if cuda else "", D, tuple(x.shape) if torch.is_tensor(x) else type(x)))
        if cuda:
            M._require_cuda(x, name)
        if x.device != dev:
            raise _lib.MfmError("%s: x lives on %s, the model on %s" % (name, x.device, dev))
        if x.shape[2] != D:
            raise _lib.MfmError("%s: x has %d features per time step, the model's input_dims sum to %d" % (name, x.shape[2], D))
        if x.shape[0] < 1 or x.shape[1] < 1:
            raise _lib.MfmError("%s: empty split %s" % (name, tuple(x.shape)))
        if max_rows is not None and int(max_rows) < 1:
            raise _lib.MfmError("%s: max_rows must be at least 1, not %r" % (name, max_rows))

    def _entry_cache(self, attr, key, who):
        """(the buffer cache `attr` of an entry, its state for `key` or None); MfmUnsupported where a refusal is remembered for it"""
        cache = self.__dict__.setdefault(attr, {})
        st = cache.get(key)
        if st is False:
            raise _lib.MfmUnsupported("%s refused this shape" % who)
        return cache, st

    def _entry_refused(self, cache, key, attr, wide):
        """remember a refusal: `wide` (what a property of the model refuses, not empty) joins the set `attr` on the model; else the
        refusal belongs to this shape alone and no buffers are kept for it"""
        if wide:
            self.__dict__.setdefault(attr, set()).update(wide)
        else:
            cache[key] = False

    def _ablation_labels(self, name, y, N, loss, dev):
        """the labels of a split of N rows as the entries take them (float32 [N, output_dim] or int64 [N], contiguous on dev)"""
        od = self._ablation_sizes()[self._ABL_OD]
        if not torch.is_tensor(y) or y.device != dev:
            raise _lib.MfmError("%s: labels must be a tensor on %s; got %s" % (name, dev, y.device if torch.is_tensor(y) else type(y)))
        if loss == "l1":
            if not y.is_floating_point() or tuple(y.shape) != (N, od):
                raise _lib.MfmError("%s: loss 'l1' takes float labels [%d, %d]; got %s %s" % (name, N, od, y.dtype, tuple(y.shape)))
            if not (y.dtype == torch.float32 and y.is_contiguous()):
                y = y.contiguous().float()
            return y
        if y.dtype != torch.int64 or tuple(y.shape) != (N,):
            raise _lib.MfmError("%s: loss 'ce' takes int64 class indices [%d]; got %s %s" % (name, N, y.dtype, tuple(y.shape)))
        return y.contiguous()

    def _ablation_sizes(self):
        """zl, za, zv, zy, fl, fa, fv, fy, d_l, d_a, d_v, output_dim, read off the parameters; 1 for what the class does not have"""
        shp = [tuple(self._modules["z%s_to_f%s_fc1" % (m, m)]._parameters["weight"].shape) for m in self._MODS]
        head = self._ablation_head()
        fy = head[0].shape[0] if len(head) == 4 else 1
        return tuple(s[1] for s in shp) + (1,) + tuple(s[0] for s in shp) + (fy, self.d_l, self.d_a, self.d_v, head[-2].shape[0])

    def _ablation_params(self, gen):
        """the 52 tensors of mfm_predict_ablation's parameter table (include/mfm_hip.h); None where nothing is read"""
        mods = self._modules
        out = []
        for m in self._MODS:
            out += _lstm_fc(mods["encoder_" + m]) + _wb(mods["z%s_to_f%s_fc1" % (m, m)]) + _wb(mods["z%s_to_f%s_fc2" % (m, m)])
            out += _lstm_fc(mods["decoder_" + m]) if gen else [None] * 6
        head = self._ablation_head()
        return out + head + [None] * (4 - len(head))

    def _ablation_composed(self, x, gen):
        """(y_hat, [x_hat_l, x_hat_a, x_hat_v] or None) as the composition of this module's own sub-modules (the granular HIP
        operations); the dropout modules are left out (eval)"""
        relu = torch.relu
        mods = self._modules
        zs = _encode([(xm, mods["encoder_" + m]) for m, xm in zip(self._MODS, self._split(x))])
        h1 = M.linear_group([(z, mods["z%s_to_f%s_fc1" % (m, m)]) for m, z in zip(self._MODS, zs)])
        fs = [relu(v) for v in M.linear_group([(relu(v), mods["z%s_to_f%s_fc2" % (m, m)]) for m, v in zip(self._MODS, h1)])]
        cat = torch.cat(fs, dim=1)
        if self._ABL_FAMILY == 0:
            y1, = M.linear_group([(cat, self.fy_to_y_fc1)])
            y_hat, = M.linear_group([(relu(y1), self.fy_to_y_fc2)])
        else:
            y_hat, = M.linear_group([(cat, self.fs_to_y)])
        x_hat = M.decoder_group([(f, mods["decoder_" + m]) for m, f in zip(self._MODS, fs)], x.shape[0]) if gen else None
        return y_hat, x_hat

    def _ablation_ws_floats(self, L, T, N, sizes, gen, labels, cap):
        return L.mfm_predict_ablation_workspace_floats(T, N, sizes, self._ABL_FAMILY, int(gen), int(labels), cap)

    def _ablation_entry(self, L, T, N, sizes, loss_kind, gen, pptr, x, y, ws, ptrs, cap, stream):
        return L.mfm_predict_ablation(T, N, sizes, self._ABL_FAMILY, loss_kind, int(gen), pptr, x, y, ws, ptrs[0], ptrs[1], ptrs[2], cap, stream)

    def _ablation_wide(self, sz, gen):
        """the values of `gen` for which a refusal is a property of the model (a hidden size beyond the on-chip recurrence: an
        encoder's for every call, a decoder's for the calls with gen); empty: of this shape alone"""
        if max(sz[0:3]) > self.MAX_RESIDENT_H:
            return (False, True)
        return (True,) if gen and max(sz[4:7]) > self.MAX_RESIDENT_H else ()

    def _ablation_fused(self, x, y, gen, params, loss_kind, cap):
        """the class's entry on the module's own tensors; MfmUnsupported when the entry refuses the sizes"""
        T, N, _ = x.shape
        L = _lib.lib()
        name = type(self).__name__
        key = (T, N, gen, y is not None, cap, x.device)
        cache, st = self._entry_cache("_ablation_bufs", key, "%s.predict: %s" % (name, self._ABL_ENTRY))
        if st is None:
            sz = self._ablation_sizes()
            sizes = (C.c_int32 * len(sz))(*sz)
            nws = int(self._ablation_ws_floats(L, T, N, sizes, gen, y is not None, cap))
            f32 = dict(dtype=torch.float32, device=x.device)
            out = Ablation(torch.empty((N, sz[self._ABL_OD]), **f32), torch.empty(3, **f32) if gen else None,
                           torch.empty((), **f32) if y is not None else None)
            ptrs = [None if t is None else t.data_ptr() for t in out]
            st = (torch.empty(max(nws, 4), **f32), out, sizes, ptrs, (C.c_void_p * self._ABL_NPARAM)())
        ws, out, sizes, ptrs, pptr = st
        for i, p in enumerate(params):
            pptr[i] = None if p is None else p.data_ptr()
        rc = self._ablation_entry(L, T, N, sizes, loss_kind, gen, pptr, C.c_void_p(x.data_ptr()),
                                  None if y is None else C.c_void_p(y.data_ptr()), C.c_void_p(ws.data_ptr()), ptrs, cap,
                                  C.c_void_p(torch._C._cuda_getCurrentRawStream(x.device.index)))
        if rc == _lib.MFM_ERR_UNSUPPORTED:
            # a hidden size beyond the on-chip recurrence is a property of the model: remembered (`_ablation_wide`).  The LDS
            # limit also depends on the tile rows, hence on N and max_rows: that refusal is remembered for this shape alone (no
            # buffers are kept for it)
            self._entry_refused(cache, key, "_ablation_refused", self._ablation_wide(self._ablation_sizes(), gen))
            raise _lib.MfmUnsupported("%s.predict: %s" % (name, L.mfm_last_error().decode()))
        _lib.check(rc, self._ABL_ENTRY)
        cache[key] = st
        return out

    def _ablation_call(self, what, x, y, loss, gen, max_rows):
        name = "%s.%s" % (type(self).__name__, what)
        if loss not in self._LOSS:
            raise ValueError("%s: loss must be 'l1' or 'ce', not %r" % (name, loss))
        dev = next(self.parameters()).device
        if dev.type != "cuda":
            raise _lib.MfmError("%s: parameters are on %s; move the model to the GPU first (no CPU fallback)" % (name, dev))
        self._ablation_check_x(name, x, dev, max_rows, cuda=True)
        N = x.shape[1]
        if y is not None:
            y = self._ablation_labels(name, y, N, loss, dev)
        cap = self.ABLATION_MAX_ROWS if max_rows is None else int(max_rows)
        if not (x.dtype == torch.float32 and x.is_contiguous()):
            x = x.contiguous().float()
        gen = bool(gen) and self._ABL_HAS_GEN
        with torch.no_grad():
            if gen not in self.__dict__.get("_ablation_refused", ()):
                params = self._ablation_params(gen)
                if all(p is None or (p.dtype == torch.float32 and p.device == dev and p.is_contiguous()) for p in params):
                    try:
                        return self._ablation_fused(x, y, gen, params, self._LOSS[loss], cap)
                    except _lib.MfmUnsupported:
                        pass
            # the composition of the module's own granular operations, then torch reductions
            F = torch.nn.functional
            y_hat, x_hat = self._ablation_composed(x, gen)
            gens = torch.stack([F.mse_loss(xh, xm) for xh, xm in zip(x_hat, self._split(x))]) if gen else None
            disc = None if y is None else (F.l1_loss(y_hat, y) if loss == "l1" else F.cross_entropy(y_hat, y))
            return Ablation(y_hat, gens, disc)

    def predict(self, x, y=None, *, loss="l1", gen=True, max_rows=None):
        """x [T, N, D] (columns d_l | d_a | d_v) -> Ablation(y_hat [N, output_dim], gen, disc): what the `predict` block of the
        reference's train_mfm_ablation reports, in one call of the library (M_B, M_D: mfm_predict_ablation, csrc/ablation.hip;
        M_A, M_C: mfm_predict_ablation_mfn, csrc/ablation_mfn.hip).  gen: [3] device floats,
        F.mse_loss(x_m_hat, x_m) in the order l, a, v -- None with gen=False and for a class without decoders (M_D accepts
        gen=True and returns None); disc: the mean label loss of y_hat as a 0-dim device tensor, None without y.  y_hat and disc
        have the same bits with and without gen.

        Always the deterministic eval computation (dropout the identity), `self.training` left as found, without autograd.
        loss="l1" takes float labels [N, output_dim], loss="ce" int64 class indices [N].  The split is walked in chunks of at most
        `max_rows` rows (default ABLATION_MAX_ROWS).  Workspace and outputs are kept on the module (outside state_dict(), dropped
        when pickled) per (T, N, gen, labels or not, max_rows, device) and REUSED: after the first call for a shape nothing is
        allocated and nothing synchronises (legal inside a stream capture), and the returned tensors are overwritten by the next
        call for the same shape -- clone what must survive it.  A device x that is not contiguous float32 is converted.  Sizes
        the entry refuses (a hidden size above 128 -- for M_A / M_C an `h_dims` entry or, with gen, the decoders' fy + fl / fy --,
        LDS beyond a CU's) take the composition of the module's own granular operations in eval mode without the MMD, followed
        by torch reductions; the refusal is remembered (per model for a hidden size above 128, per shape otherwise).  So does a model with a parameter that is not a contiguous float32 tensor on x's device.  Argument errors
        (shape, device, labels, an empty split, max_rows < 1: MfmError; unknown `loss`: ValueError) are raised before anything is
        launched.  A CPU model or input raises MfmError: there is no CPU fallback."""
        return self._ablation_call("predict", x, y, loss, gen, max_rows)

    def evaluate(self, x, y, *, loss="l1", max_rows=None):
        """the mean label loss of the split as a 0-dim device float -- the label path only, `predict(x, y, gen=False).disc` bit for
        bit: no decoder runs, nothing comes back to the host, so `evaluate -> lr_scheduler.ReduceLROnPlateau.step ->
        checkpoint.KeepBest.update` can be one captured graph.  The contract of predict()."""
        if y is None:
            raise _lib.MfmError("%s.evaluate: labels are required" % type(self).__name__)
        return self._ablation_call("evaluate", x, y, loss, False, max_rows).disc


class _AblationMfnProtocol(_AblationProtocol):
    """the protocol for the ablations whose label factor comes from the Memory Fusion Network: one call of
    mfm_predict_ablation_mfn (csrc/ablation_mfn.hip).  `_ABL_FAMILY`: 0 M_A (encoder_l over all of x, decoders on [fy | fl]),
    1 M_C (decoders on fy)."""

    _ABL_ENTRY = "mfm_predict_ablation_mfn"
    _ABL_NPARAM = 66
    _ABL_OD = 21
    _MFN_LINEARS = ("att1_fc1", "att1_fc2", "att2_fc1", "att2_fc2", "gamma1_fc1", "gamma1_fc2", "gamma2_fc1", "gamma2_fc2")
    _TAIL_LINEARS = ("last_to_zy_fc1", "zy_to_fy_fc1", "zy_to_fy_fc2", "fy_to_y_fc1", "fy_to_y_fc2")

    def _ablation_sizes(self):
        """the 23 sizes of mfm_predict_zeros_mfn's layout, read off the parameters; 1 for what the class does not have (za, zv,
        fa, fv; M_C: zl, fl too), heads 0.  Entry 22, the loss kind, is set per call"""
        mods = self._modules
        mfn = mods["mfn_encoder"]._modules
        w = lambda mod: tuple(mod._parameters["weight"].shape)
        hm = [mfn["lstm_" + m]._parameters["weight_hh"].shape[1] for m in self._MODS]
        fl, zl = w(mods["zl_to_fl_fc1"]) if self._ABL_FAMILY == 0 else (1, 1)
        fy, zy = w(mods["zy_to_fy_fc1"])
        return (self.d_l, self.d_a, self.d_v, zl, 1, 1, zy, hm[0], hm[1], hm[2], w(mfn["att2_fc2"])[0], w(mfn["att1_fc1"])[1] // sum(hm),
                w(mfn["att1_fc1"])[0], w(mfn["att2_fc1"])[0], w(mfn["gamma1_fc1"])[0], w(mfn["gamma2_fc1"])[0], 0,
                fl, 1, 1, fy, w(mods["fy_to_y_fc2"])[0], 0)

    def _ablation_params(self, gen):
        """the 66 tensors of mfm_predict_ablation_mfn's parameter table (include/mfm_hip.h); None where nothing is read"""
        mods = self._modules
        mfn = mods["mfn_encoder"]._modules
        out = []
        for m in self._MODS:
            lp = mfn["lstm_" + m]._parameters
            out += [lp["weight_ih"], lp["weight_hh"], lp["bias_ih"], lp["bias_hh"]]
        for n in self._MFN_LINEARS:
            out += _wb(mfn[n])
        for n in self._TAIL_LINEARS:
            out += _wb(mods[n])
        for m in self._MODS:
            out += _lstm_fc(mods["decoder_" + m]) if gen else [None] * 6
        if gen and self._ABL_FAMILY == 0:
            return out + _lstm_fc(mods["encoder_l"]) + _wb(mods["zl_to_fl_fc1"]) + _wb(mods["zl_to_fl_fc2"])
        return out + [None] * 10

    def _ablation_composed(self, x, gen):
        """(y_hat, [x_hat_l, x_hat_a, x_hat_v] or None) as the composition of this module's own sub-modules (the granular HIP
        operations) in eval mode: the dropout modules and the MMD are left out; the MFN, whose forward applies its own dropout
        modules, runs in eval mode and is put back as found"""
        relu = torch.relu
        mods = self._modules
        mfn = mods["mfn_encoder"]
        was = [mod.training for mod in mfn.modules()]
        mfn.eval()
        try:
            last = mfn.forward(x)
        finally:
            for mod, t in zip(mfn.modules(), was):
                mod.training = t
        zy, = M.linear_group([(last, mods["last_to_zy_fc1"])])
        h1, = M.linear_group([(zy, mods["zy_to_fy_fc1"])])
        fy, = M.linear_group([(relu(h1), mods["zy_to_fy_fc2"])])
        fy = relu(fy)
        y1, = M.linear_group([(fy, mods["fy_to_y_fc1"])])
        y_hat, = M.linear_group([(relu(y1), mods["fy_to_y_fc2"])])
        if not gen:
            return y_hat, None
        emb = fy
        if self._ABL_FAMILY == 0:
            zl, = _encode([(x, mods["encoder_l"])])
            h1, = M.linear_group([(zl, mods["zl_to_fl_fc1"])])
            fl, = M.linear_group([(relu(h1), mods["zl_to_fl_fc2"])])
            emb = torch.cat([fy, relu(fl)], dim=1)
        return y_hat, M.decoder_group([(emb, mods["decoder_" + m]) for m in self._MODS], x.shape[0])

    def _ablation_ws_floats(self, L, T, N, sizes, gen, labels, cap):
        return L.mfm_predict_ablation_mfn_workspace_floats(T, N, sizes, self._ABL_FAMILY, int(gen), int(labels), cap)

    def _ablation_entry(self, L, T, N, sizes, loss_kind, gen, pptr, x, y, ws, ptrs, cap, stream):
        sizes[22] = loss_kind
        return L.mfm_predict_ablation_mfn(T, N, sizes, self._ABL_FAMILY, int(gen), pptr, x, y, ws, ptrs[0], ptrs[1], ptrs[2], cap, stream)

    def _ablation_wide(self, sz, gen):
        """an `h_dims` entry above 128 refuses every call; encoder_l's zl (M_A) or the decoders' fy + fl / fy the calls with gen"""
        if max(sz[7:10]) > self.MAX_RESIDENT_H:
            return (False, True)
        wdec = sz[20] + sz[17] if self._ABL_FAMILY == 0 else sz[20]
        wenc = sz[3] if self._ABL_FAMILY == 0 else 1
        return (True,) if gen and max(wdec, wenc) > self.MAX_RESIDENT_H else ()


class M_A(_AblationMfnProtocol, _Base):
    """reference mfm_model.py:201-266: one early-fusion encoder for z_l, MFN for z_y, all decoders fed [f_y, f_l].
    `predict(x, y)` / `evaluate(x, y)`: y_hat, the reconstruction errors and the label loss as one call of the library."""

    _ABL_FAMILY = 0

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


class M_B(_AblationProtocol, _Base):
    """reference mfm_model.py:268-335: modality-specific factors only; the classifier reads [f_l, f_a, f_v].
    `predict(x, y)` / `evaluate(x, y)`: y_hat, the reconstruction errors and the label loss as one call of the library."""

    _ABL_FAMILY = 0

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

    def _ablation_head(self):
        return _wb(self._modules["fy_to_y_fc1"]) + _wb(self._modules["fy_to_y_fc2"])


class M_C(_AblationMfnProtocol, _Base):
    """reference mfm_model.py:337-387: the multimodal factor only (MFN -> z_y -> f_y feeds every decoder).
    `predict(x, y)` / `evaluate(x, y)`: y_hat, the reconstruction errors and the label loss as one call of the library."""

    _ABL_FAMILY = 1

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


class M_D(_AblationProtocol, _Base):
    """reference mfm_model.py:389-467: purely discriminative (no decoders; `decoded` carries the inputs back).
    `predict(x, y)` / `evaluate(x, y)`: y_hat and the label loss as one call of the library; gen is None."""

    _ABL_FAMILY = 1
    _ABL_HAS_GEN = False

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

    def _ablation_head(self):
        return _wb(self._modules["fs_to_y"])

    # ------------------------------------------------------------------ one training step without the optimizer
    TRAIN_MAX_ROWS = 1024        # default row cap of loss_and_grad(): the BPTT record of at most this many rows is alive at once
    dropout_seed = None          # seed of loss_and_grad()'s dropout masks; None: torch.initial_seed() at the first call
    last_y_hat = None            # y_hat [N, output_dim] of the latest loss_and_grad() (the call's own buffer on the one-call path)

    def _train_params(self):
        """the 32 tensors of mfm_train_ablation_d's parameter table (include/mfm_hip.h)"""
        mods = self._modules
        out = []
        for m in self._MODS:
            out += _lstm_fc(mods["encoder_" + m]) + _wb(mods["z%s_to_f%s_fc1" % (m, m)]) + _wb(mods["z%s_to_f%s_fc2" % (m, m)])
        return out + _wb(mods["fs_to_y"])

    def _train_drop(self):
        """the dropout probability of the three z -> f sites as the modules stand (0: eval mode, or p = 0)"""
        drops = [self._modules["z%s_to_f%s_dropout" % (m, m)] for m in self._MODS]
        return [float(d.p) if d.training else 0.0 for d in drops]

    def _forward_torch(self, x):
        """y_hat of forward() in plain torch operations on the module's own parameters: the path of a model that is not on the GPU"""
        F = torch.nn.functional
        mods = self._modules
        fs = []
        for m, xm in zip(self._MODS, self._split(x.float())):
            enc = mods["encoder_" + m]
            cell = enc._modules["lstm"]
            h = c = xm.new_zeros(xm.shape[1], cell.hidden_size)
            for t in range(xm.shape[0]):
                h, c = cell(xm[t], (h, c))
            z = F.linear(h, enc.fc1.weight, enc.fc1.bias)
            tag = "z%s_to_f%s" % (m, m)
            fc1, fc2 = mods[tag + "_fc1"], mods[tag + "_fc2"]
            h1 = mods[tag + "_dropout"](torch.relu(F.linear(z, fc1.weight, fc1.bias)))
            fs.append(torch.relu(F.linear(h1, fc2.weight, fc2.bias)))
        return F.linear(torch.cat(fs, dim=1), self.fs_to_y.weight, self.fs_to_y.bias)

    def _train_composed(self, x, y, loss):
        F = torch.nn.functional
        with torch.enable_grad():
            y_hat = self.forward(x)[0][3] if x.is_cuda else self._forward_torch(x)
            out = F.l1_loss(y_hat, y) if loss == "l1" else F.cross_entropy(y_hat, y)
            out.backward()
        self.last_y_hat = y_hat.detach()
        self._train_last = None
        return out.detach()

    def _train_fused(self, x, y, params, loss_kind, cap):
        """mfm_train_ablation_d on the module's own tensors and their .grad; MfmUnsupported when the entry refuses the sizes, or
        a gradient that is there already is not a contiguous float32 tensor on x's device"""
        T, N, _ = x.shape
        L = _lib.lib()
        dev = x.device
        key = (T, N, cap, dev)
        cache, st = self._entry_cache("_train_bufs", key, "M_D.loss_and_grad: mfm_train_ablation_d")
        sz = self._ablation_sizes()
        if st is None:
            sizes = (C.c_int32 * 12)(*sz)
            nws = int(L.mfm_train_ablation_d_workspace_floats(T, N, sizes, cap))
            f32 = dict(dtype=torch.float32, device=dev)
            st = (torch.empty(max(nws, 4), **f32), torch.empty((N, sz[11]), **f32), torch.empty((), **f32), sizes,
                  (C.c_void_p * 32)(), (C.c_void_p * 32)(), (C.c_float * 3)(), torch.zeros(1, dtype=torch.int64, device=dev))
        ws, y_hat, out, sizes, pptr, gptr, pdrop, tick = st
        # .grad as torch keeps it: left alone where requires_grad is false, created where it is None, added to where it exists
        live = [p for p in params if p.requires_grad]
        have = [p.grad is not None for p in live]
        if not all(g is None or (g.dtype == torch.float32 and g.device == dev and g.is_contiguous() and g.shape == p.shape)
                   for p, g in ((p, p.grad) for p in live)):
            raise _lib.MfmUnsupported("M_D.loss_and_grad: a .grad is not a contiguous float32 tensor on %s" % dev)
        accumulate = any(have)
        made = []
        for p in live:
            if p.grad is None:
                p.grad = torch.zeros_like(p) if accumulate else torch.empty_like(p)
                made.append(p)
        for i, p in enumerate(params):
            pptr[i] = p.data_ptr()
            gptr[i] = p.grad.data_ptr() if p.requires_grad else None
        drop = self._train_drop()
        pdrop[:] = drop
        train = any(p > 0.0 for p in drop)
        if self.dropout_seed is None:
            self.dropout_seed = torch.initial_seed() & 0xFFFFFFFFFFFF
        call = self.__dict__.get("_train_calls", 0)
        tickp = None
        if train and torch.cuda.is_current_stream_capturing():
            # a replayed graph re-runs this call with the same host seed and call number: add a device word that the graph
            # itself advances, so every replay draws new masks
            tick.add_(0x1E3779B97F4A7C15)
            tickp = C.c_void_p(tick.data_ptr())
        rc = L.mfm_train_ablation_d(T, N, sizes, loss_kind, int(train), pdrop, int(self.dropout_seed), call, tickp, pptr, gptr,
                                    int(accumulate), C.c_void_p(x.data_ptr()), C.c_void_p(y.data_ptr()), C.c_void_p(ws.data_ptr()),
                                    C.c_void_p(y_hat.data_ptr()), C.c_void_p(out.data_ptr()), cap,
                                    C.c_void_p(torch._C._cuda_getCurrentRawStream(dev.index)))
        if rc != 0:
            for p in made:
                p.grad = None
        if rc == _lib.MFM_ERR_UNSUPPORTED:
            # a z or f size beyond the on-chip bound is a property of the model: remembered for every call; else for this shape
            self._entry_refused(cache, key, "_train_refused", ("sizes",) if max(sz[0:3] + sz[4:7]) > self.MAX_RESIDENT_H else ())
            raise _lib.MfmUnsupported("M_D.loss_and_grad: %s" % L.mfm_last_error().decode())
        _lib.check(rc, "mfm_train_ablation_d")
        self._train_calls = call + 1
        cache[key] = st
        self._train_last = key
        self.last_y_hat = y_hat
        return out

    def last_dropout_masks(self):
        """the dropout scales of the latest loss_and_grad(), read out of its workspace at the offset the library names
        (mfm_train_ablation_d_mask_offset): per site l, a, v a view [n, f_m] of 0 / 1 / (1 - p), n the rows of the call's last
        chunk -- None for a site that drew nothing (eval mode or p = 0).  None altogether when there is nothing to read: before
        the first call, after a call that took the composed path, or once the buffers were dropped (a pickled copy)"""
        key = self.__dict__.get("_train_last")
        st = self.__dict__.get("_train_bufs", {}).get(key) if key is not None else None
        if not st:
            return None
        T, N, cap, _ = key
        ws, sizes, pdrop = st[0], st[3], st[6]
        rows = min(N, cap) if cap > 0 else N
        off = int(_lib.lib().mfm_train_ablation_d_mask_offset(T, N, sizes, cap))
        n = N - (N - 1) // rows * rows
        out = []
        for f, p in zip(sizes[4:7], pdrop):
            out.append(ws[off:off + n * f].view(n, f) if p > 0.0 else None)
            off += rows * f
        return out

    def loss_and_grad(self, x, y, *, loss="l1", max_rows=None):
        """x [T, N, D] (columns d_l | d_a | d_v), labels y -> the mean label loss of y_hat = forward(x)[0][3] as a 0-dim float
        tensor on the model's device, with the gradient of that loss left in every parameter's .grad: the `train` block of the
        reference's train_mfm_ablation minus the optimizer, in one call of the library (mfm_train_ablation_d,
        csrc/train_ablation.hip: five launches per row chunk, no autograd graph).  loss="l1" takes float labels
        [N, output_dim], loss="ce" int64 class indices [N].  .grad as torch keeps it: created where it is None, added to where it
        exists (zero_grad(set_to_none=...) and accumulation over several calls both work), left alone where requires_grad is
        false.  Any optimizer then steps.  `self.training` is honoured: in train mode the three dropout sites draw the library's
        counter-based masks from `dropout_seed` (per model; None: torch.initial_seed() at the first call) and the number of
        calls so far -- `last_dropout_masks()` reads them back --, in eval mode dropout is the identity.  `last_y_hat` holds y_hat.

        The split is walked in chunks of at most `max_rows` rows (default TRAIN_MAX_ROWS) whose gradients add up in chunk order.
        Workspace, y_hat and the loss are kept on the module (outside state_dict(), dropped when pickled) per (T, N, max_rows,
        device) and REUSED: after the first call for a shape nothing is allocated (but a .grad that is None) and nothing
        synchronises -- legal inside a stream capture --, and the returned tensor is overwritten by the next call for the same
        shape.  Loss and gradients are bit-identical from call to call.  Sizes the entry refuses (a z or f size above 128), a
        model, input or .grad that is not contiguous float32 on the GPU (a CPU model among them) take the composed path
        instead -- forward() (plain torch on the CPU), the torch loss, .backward() -- with the same result; inside a stream
        capture that raises MfmError.  Argument errors (shapes, devices, labels, max_rows < 1: MfmError; unknown `loss`:
        ValueError) are raised before anything is launched."""
        name = "M_D.loss_and_grad"
        if loss not in self._LOSS:
            raise ValueError("%s: loss must be 'l1' or 'ce', not %r" % (name, loss))
        dev = next(self.parameters()).device
        self._ablation_check_x(name, x, dev, max_rows, cuda=False)
        y = self._ablation_labels(name, y, x.shape[1], loss, dev)
        cap = self.TRAIN_MAX_ROWS if max_rows is None else int(max_rows)
        if dev.type == "cuda" and x.dtype == torch.float32 and not self.__dict__.get("_train_refused", False):
            params = self._train_params()
            if all(p.dtype == torch.float32 and p.device == dev and p.is_contiguous() for p in params):
                try:
                    return self._train_fused(x.contiguous(), y, params, self._LOSS[loss], cap)
                except _lib.MfmUnsupported:
                    pass
        if dev.type == "cuda" and torch.cuda.is_current_stream_capturing():
            raise _lib.MfmError("%s: this model, input or shape takes the composed autograd path, which cannot run inside a stream capture" % name)
        return self._train_composed(x, y, loss)


Imputed = collections.namedtuple("Imputed", ["x_hat", "y_hat"])


def _lstm_fc(mod):
    """the six tensors of an encoderLSTM / decoderLSTM in the order of the C ABI (plain dict look-ups: always the current ones)"""
    lp, fp = mod._modules["lstm"]._parameters, mod._modules["fc1"]._parameters
    return [lp["weight_ih"], lp["weight_hh"], lp["bias_ih"], lp["bias_hh"], fp["weight"], fp["bias"]]


def _wb(lin):
    return [lin._parameters["weight"], lin._parameters["bias"]]


Missing = collections.namedtuple("Missing", ["y_hat", "gen", "disc"])


class _MissingProtocol:
    """`predict_missing` of the three classes of the missing-modality family: one call of mfm_predict_missing (csrc/missing.hip).
    A class names its family (`_MIS_FAMILY`: 0 MFM_missing, 1 seq2seq, 2 basic_missing) and gives `_missing_sizes()`,
    `_missing_params(cases)` and `_missing_composed(x, m)`."""

    MISSING_MAX_ROWS = 1024      # default row cap of predict_missing(): the x-projections of at most this many rows are alive at once
    MAX_RESIDENT_H = 128         # widest LSTM of the on-chip recurrences (csrc/lstm_seq_dev.h, MFM_SEQ_MAX_RESIDENT_H)
    _CASES = ("l", "a", "v")
    _PAIR = {"l": "av", "a": "lv", "v": "la"}       # the observed pair of each case
    _LOSS = {"l1": 0, "ce": 1}

    def __getstate__(self):
        state = dict(self.__dict__)
        state.pop("_impute_bufs", None)          # (device workspaces and native pointer tables: rebuilt on the next call)
        state.pop("_missing_bufs", None)
        return state

    def _pair_copy(self, x, missing):
        """a COPY of the observed pair, never a column slice of x: the projection GEMM masks the 16-byte fetches that pass a row's
        K range by multiplying with zero, and on a slice those fetches meet the missing modality's columns (csrc/impute.hip)"""
        d_l, d_a = self.d_l, self.d_a
        if missing == "l":
            return x[:, :, d_l:].contiguous()
        if missing == "v":
            return x[:, :, :d_l + d_a].contiguous()
        return torch.cat([x[:, :, :d_l], x[:, :, d_l + d_a:]], dim=2)

    def _missing_columns(self, x, missing):
        lo = {"l": 0, "a": self.d_l, "v": self.d_l + self.d_a}[missing]
        return x[:, :, lo:lo + {"l": self.d_l, "a": self.d_a, "v": self.d_v}[missing]]

    def _missing_hidden(self, sz):
        """the widest hidden size the family's recurrences run, from the 12 sizes"""
        fam = self._MIS_FAMILY
        if fam == 0:
            return max(max(sz[0:4]), sz[7] + max(sz[4:7]))
        return max(max(sz[0:3]), max(sz[4:7])) if fam == 1 else sz[3]

    def _missing_fused(self, x, y, cases, params, loss_kind, cap):
        """mfm_predict_missing on the module's own tensors; MfmUnsupported when the entry refuses the sizes"""
        T, N, _ = x.shape
        L = _lib.lib()
        fam = self._MIS_FAMILY
        name = type(self).__name__
        bits = sum(1 << self._CASES.index(m) for m in cases)
        cache = self.__dict__.setdefault("_missing_bufs", {})
        key = (T, N, bits, y is not None, cap, x.device)
        st = cache.get(key)
        if st is False:
            raise _lib.MfmUnsupported("%s.predict_missing: mfm_predict_missing refused this shape" % name)
        if st is None:
            sz = self._missing_sizes()
            sizes = (C.c_int32 * 12)(*sz)
            nws = int(L.mfm_predict_missing_workspace_floats(T, N, sizes, fam, bits, int(y is not None), cap))
            f32 = dict(dtype=torch.float32, device=x.device)
            each = len(cases) == 3
            i0 = self._CASES.index(cases[0])
            y_hat = gen = disc = None
            if fam != 1:
                y_hat = torch.empty((3, N, sz[11]) if each else (N, sz[11]), **f32)
                disc = torch.empty(3, **f32) if y is not None else None
            if fam != 2:
                gen = torch.empty(3, **f32)
            ptrs = [None if t is None else t.data_ptr() for t in (y_hat, gen, disc)]
            out = Missing(y_hat, gen if gen is None or each else gen[i0], disc if disc is None or each else disc[i0])
            st = (torch.empty(max(nws, 4), **f32), (y_hat, gen, disc), out, sizes, ptrs, (C.c_void_p * 74)())
        ws, _, out, sizes, ptrs, pptr = st
        for i, p in enumerate(params):
            pptr[i] = None if p is None else p.data_ptr()
        rc = L.mfm_predict_missing(T, N, sizes, fam, bits, loss_kind, pptr, C.c_void_p(x.data_ptr()),
                                   None if y is None else C.c_void_p(y.data_ptr()), C.c_void_p(ws.data_ptr()), ptrs[0], ptrs[1], ptrs[2],
                                   cap, C.c_void_p(torch._C._cuda_getCurrentRawStream(x.device.index)))
        if rc == _lib.MFM_ERR_UNSUPPORTED:
            # a hidden size beyond the on-chip recurrence is a property of the model: remembered.  The LDS limit also depends on the
            # tile rows, hence on N and max_rows: that refusal is remembered for this shape alone (no buffers are kept for it)
            self._missing_refused = self._missing_hidden(self._missing_sizes()) > self.MAX_RESIDENT_H
            if not self._missing_refused:
                cache[key] = False
            raise _lib.MfmUnsupported("%s.predict_missing: %s" % (name, L.mfm_last_error().decode()))
        _lib.check(rc, "mfm_predict_missing")
        cache[key] = st
        return out

    def _missing_call(self, x, y, missing, loss, max_rows):
        name = type(self).__name__ + ".predict_missing"
        fam = self._MIS_FAMILY
        if missing not in ("l", "a", "v", "each"):
            raise ValueError("%s: missing must be 'l', 'a', 'v' or 'each', not %r" % (name, missing))
        if loss not in self._LOSS:
            raise ValueError("%s: loss must be 'l1' or 'ce', not %r" % (name, loss))
        dev = next(self.parameters()).device
        if dev.type != "cuda":
            raise _lib.MfmError("%s: parameters are on %s; move the model to the GPU first (no CPU fallback)" % (name, dev))
        D = self.d_l + self.d_a + self.d_v
        if not torch.is_tensor(x) or x.dim() != 3:
            raise _lib.MfmError("%s: x must be a CUDA tensor [T, N, %d]; got %s" % (name, D, tuple(x.shape) if torch.is_tensor(x) else type(x)))
        M._require_cuda(x, name)
        if x.device != dev:
            raise _lib.MfmError("%s: x lives on %s, the model on %s" % (name, x.device, dev))
        if x.shape[2] != D:
            raise _lib.MfmError("%s: x has %d features per time step, the model's input_dims sum to %d" % (name, x.shape[2], D))
        if x.shape[0] < 1 or x.shape[1] < 1:
            raise _lib.MfmError("%s: empty split %s" % (name, tuple(x.shape)))
        if max_rows is not None and int(max_rows) < 1:
            raise _lib.MfmError("%s: max_rows must be at least 1, not %r" % (name, max_rows))
        N = x.shape[1]
        if y is not None:
            od = self._missing_sizes()[11]
            if not torch.is_tensor(y) or y.device != dev:
                raise _lib.MfmError("%s: labels must be a tensor on %s; got %s" % (name, dev, y.device if torch.is_tensor(y) else type(y)))
            if loss == "l1":
                if not y.is_floating_point() or tuple(y.shape) != (N, od):
                    raise _lib.MfmError("%s: loss 'l1' takes float labels [%d, %d]; got %s %s" % (name, N, od, y.dtype, tuple(y.shape)))
                if not (y.dtype == torch.float32 and y.is_contiguous()):
                    y = y.contiguous().float()
            else:
                if y.dtype != torch.int64 or tuple(y.shape) != (N,):
                    raise _lib.MfmError("%s: loss 'ce' takes int64 class indices [%d]; got %s %s" % (name, N, y.dtype, tuple(y.shape)))
                y = y.contiguous()
        cap = self.MISSING_MAX_ROWS if max_rows is None else int(max_rows)
        if not (x.dtype == torch.float32 and x.is_contiguous()):
            x = x.contiguous().float()
        cases = self._CASES if missing == "each" else (missing,)
        with torch.no_grad():
            if not getattr(self, "_missing_refused", False):
                params = self._missing_params(cases)
                if all(p is None or (p.dtype == torch.float32 and p.device == dev and p.is_contiguous()) for p in params):
                    try:
                        return self._missing_fused(x, y, cases, params, self._LOSS[loss], cap)
                    except _lib.MfmUnsupported:
                        pass
            # the composition of the module's own granular operations on a copy of the observed pair, then torch reductions
            F = torch.nn.functional
            y_hats, gens, discs = [], [], []
            for m in cases:
                x_hat, y_hat = self._missing_composed(x, m)
                if fam != 2:
                    gens.append(F.mse_loss(x_hat, self._missing_columns(x, m)))
                if fam != 1:
                    y_hats.append(y_hat)
                    if y is not None:
                        discs.append(F.l1_loss(y_hat, y) if loss == "l1" else F.cross_entropy(y_hat, y))
            pick = (lambda v: torch.stack(v) if v else None) if missing == "each" else (lambda v: v[0] if v else None)
            return Missing(pick(y_hats), pick(gens), pick(discs))


_MISSING_DOC = """x [T, N, D] (columns d_l | d_a | d_v), missing in "l" / "a" / "v" / "each" -> Missing(y_hat, gen, disc): the
        missing-modality test protocol of this class in one call of mfm_predict_missing (csrc/missing.hip) -- per missing case
        the label predicted from the other two modalities, the error of the rebuilt modality and the label loss; what the class
        does not have is None.  missing="each": the three cases in the order l, a, v in shared launches, y_hat [3, N, output_dim],
        gen and disc [3] device floats; one case: y_hat [N, output_dim], gen and disc 0-dim device tensors.

        Always the deterministic eval computation (dropout the identity), `self.training` left as found, without autograd.  THE
        COLUMNS OF THE MISSING MODALITY ARE NEVER READ by an encoder: they reach the squared error of `gen` alone, as its target.
        y_hat and disc of a case do not depend on them (NaN there is legal and leaves their bits alone); gen does, by definition.
        loss="l1" takes float labels [N, output_dim], loss="ce" int64 class indices [N]; disc is their mean label loss, None without
        y.  The split is walked in chunks of at most `max_rows` rows (default MISSING_MAX_ROWS).  Workspace and outputs are kept on
        the module (outside state_dict(), dropped when pickled) per (T, N, case set, labels or not, max_rows) and REUSED: after the
        first call for a shape nothing is allocated and nothing synchronises (legal inside a stream capture), and the returned
        tensors are overwritten by the next call for the same shape -- clone what must survive it.  "each" gives the bits of the
        three single calls as long as both run on the same tile rows (include/mfm_hip.h, mfm_predict_missing_tile_rows).  A device x
        that is not contiguous float32 is converted.  Sizes the entry refuses (a hidden size above 128, LDS beyond a CU's) take the
        composition of the module's own granular operations on a COPY of the observed pair, followed by torch reductions; the
        refusal is remembered.  So does a model with a parameter that is not a contiguous float32 tensor on x's device.  Argument
        errors (shape, device, labels, max_rows < 1: MfmError; unknown `missing` / `loss`: ValueError) are raised before anything is
        launched.  A CPU model or input raises MfmError: there is no CPU fallback."""


class MFM_missing(_MissingProtocol, _Base):
    """reference mfm_model.py:766-898: MFM plus six surrogate encoders that predict a modality's (and z_y's) code
    from the other two modalities; forward returns the four decodings (all present / no l / no a / no v).
    `impute(x, missing)`: the no-<missing> decoding's reconstruction of that modality and its label from the other two
    modalities alone, as one call of the library."""

    IMPUTE_MAX_ROWS = 1024       # default row cap of impute(): the x-projections of at most this many rows are alive at once
    _MIS_FAMILY = 0

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

    # ------------------------------------------------------------------ surrogate inference (__getstate__: _MissingProtocol)
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

    # ------------------------------------------------------------------ the missing-modality test protocol
    _missing_params = _impute_params       # (the 74 pointers of mfm_impute_missing unchanged)
    _missing_sizes = _impute_sizes
    _missing_composed = _impute_composed

    def predict_missing(self, x, y=None, *, missing="each", loss="l1", max_rows=None):
        return self._missing_call(x, y, missing, loss, max_rows)
    predict_missing.__doc__ = """y_hat = decoded_no<m>[3] of forward(), gen = F.mse_loss(decoded_no<m>[index of m], x_m), disc the label loss of
        y_hat -- the pipeline of impute() with the decoder's fc1 fused into the squared error: no x_hat is written.

        """ + _MISSING_DOC


class seq2seq(_MissingProtocol, _Base):
    """reference mfm_model.py:900-960: reconstruct each modality from the other two (no multimodal factor)."""

    _MIS_FAMILY = 1

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

    # ------------------------------------------------------------------ the missing-modality test protocol
    def _missing_params(self, cases):
        """the table of mfm_predict_missing for family 1 (include/mfm_hip.h); None where the family or the case set has nothing"""
        mods = self._modules
        out = []
        for m in self._CASES:
            if m not in cases:
                out += [None] * 22
                continue
            out += _lstm_fc(mods["encoder_%s_to_%s" % (self._PAIR[m], m)]) + [None] * 6
            out += _wb(mods["z%s_to_f%s_fc1" % (m, m)]) + _wb(mods["z%s_to_f%s_fc2" % (m, m)]) + _lstm_fc(mods["decoder_" + m])
        return out + [None] * 8

    def _missing_sizes(self):
        """zl, za, zv, zy, fl, fa, fv, fy, d_l, d_a, d_v, output_dim; 1 for what the class does not have"""
        shp = [tuple(self._modules[n]._parameters["weight"].shape) for n in ("zl_to_fl_fc1", "za_to_fa_fc1", "zv_to_fv_fc1")]
        return tuple(s[1] for s in shp) + (1,) + tuple(s[0] for s in shp) + (1, self.d_l, self.d_a, self.d_v, 1)

    def _missing_composed(self, x, missing):
        """(x_hat, None) of ONE case as the composition of this module's own sub-modules; the dropout modules are left out (eval)"""
        relu = torch.relu
        zm, = _encode([(self._pair_copy(x, missing), getattr(self, "encoder_%s_to_%s" % (self._PAIR[missing], missing)))])
        tag = "z%s_to_f%s" % (missing, missing)
        h1, = M.linear_group([(zm, getattr(self, tag + "_fc1"))])
        fm, = M.linear_group([(relu(h1), getattr(self, tag + "_fc2"))])
        x_hat, = M.decoder_group([(relu(fm), getattr(self, "decoder_" + missing))], x.shape[0])
        return x_hat, None

    def predict_missing(self, x, *, missing="each", max_rows=None):
        return self._missing_call(x, None, missing, "l1", max_rows)
    predict_missing.__doc__ = """gen = F.mse_loss(x_m_hat, x_m), x_m_hat = decoder_m(relu(fc2(relu(fc1(encoder_<pair>_to_<m>(pair))))), T); the class has
        no label path: y_hat and disc are None.

        """ + _MISSING_DOC


class basic_missing(_MissingProtocol, _Base):
    """reference mfm_model.py:962-1017: predict the label from two modalities, one small head per missing modality."""

    _MIS_FAMILY = 2

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

    # ------------------------------------------------------------------ the missing-modality test protocol
    def _missing_params(self, cases):
        """the table of mfm_predict_missing for family 2 (include/mfm_hip.h); None where the family or the case set has nothing"""
        mods = self._modules
        out = []
        for m in self._CASES:
            if m not in cases:
                out += [None] * 22
                continue
            tag = "zy_no%s_to_y" % m
            out += [None] * 6 + _lstm_fc(mods["encoder_%s_to_y" % self._PAIR[m]]) + _wb(mods[tag + "_fc1"]) + _wb(mods[tag + "_fc2"]) + [None] * 6
        return out + [None] * 8

    def _missing_sizes(self):
        """zl, za, zv, zy, fl, fa, fv, fy, d_l, d_a, d_v, output_dim; 1 for what the class does not have"""
        fy, zy = self._modules["zy_nol_to_y_fc1"]._parameters["weight"].shape
        return (1, 1, 1, zy, 1, 1, 1, fy, self.d_l, self.d_a, self.d_v, self._modules["zy_nol_to_y_fc2"]._parameters["weight"].shape[0])

    def _missing_composed(self, x, missing):
        """(None, y_hat) of ONE case as the composition of this module's own sub-modules; the dropout modules are left out (eval)"""
        zy, = _encode([(self._pair_copy(x, missing), getattr(self, "encoder_%s_to_y" % self._PAIR[missing]))])
        tag = "zy_no%s_to_y" % missing
        h1, = M.linear_group([(zy, getattr(self, tag + "_fc1"))])
        y_hat, = M.linear_group([(torch.relu(h1), getattr(self, tag + "_fc2"))])
        return None, y_hat

    def predict_missing(self, x, y=None, *, missing="each", loss="l1", max_rows=None):
        return self._missing_call(x, y, missing, loss, max_rows)
    predict_missing.__doc__ = """y_hat = zy_no<m>_to_y_fc2(relu(zy_no<m>_to_y_fc1(encoder_<pair>_to_y(pair)))) and disc, its label loss; the class has no decoder:
        gen is None.

        """ + _MISSING_DOC
