"""The engine's no-plan inference entries: predict, encode, decode, objective, predict_zeros and influence_factors
(`InferMixin`, a base of engine.MFMEngine).  Each is one C call of libmfm_hip.so on the current HIP stream -- no plan, no
training workspace, the split walked in chunks of at most `max_rows` rows (default PREDICT_MAX_ROWS) -- and all go through one
host path: the split validation (`_check_split`), the parameter offsets table (`_offsets`) and the fused-entry runner
(`_run_fused`).  The variants "kl" and "mmd", whose label factor comes from the Memory Fusion Network, have library functions and
state caches of their own:

    entry               "kl_ef"                    "kl", "mmd"                cache ("kl_ef" / "kl", "mmd")            refused
    predict             mfm_predict_klef           the eval forward on a plan _predict_bufs / (the plan)               falls back
      label_only=True   mfm_predict_klef           mfm_predict_mfn            _predict_bufs / _predict_mfn_bufs        falls back
    encode              mfm_encode_klef            mfm_encode_mfn             _encode_bufs / _encode_mfn_bufs          raises
    decode              mfm_decode_factors         mfm_decode_factors         _decode_bufs                             raises
    objective           mfm_objective_klef         mfm_objective_mfn          _objective_bufs / _objective_mfn_bufs    falls back
    predict_zeros       mfm_predict_zeros_klef     mfm_predict_zeros_mfn      _zeros_bufs / _zeros_mfn_bufs            falls back
    influence_factors   mfm_influence_factors      mfm_influence_factors      _influence_bufs                          raises

A cache `_<name>_bufs` remembers its refusal in `_<name>_refused` (`_ENTRIES` below).

THE REUSE CONTRACT, the same for every entry: workspace and result tensors are kept per (T, N, max_rows) in
`engine._<entry>_bufs` and REUSED.  After the first call for a shape nothing is allocated and nothing synchronises, and the
returned tensors are overwritten by the next call for the same shape: clone what must survive it.

REFUSALS, likewise: an entry answers MFM_ERR_UNSUPPORTED for sizes its kernels do not cover and enqueues nothing.  A refusal
for a hidden size above MAX_RESIDENT_H is a property of the configuration and is remembered in `engine._<entry>_refused` (the
entry is not asked again); one for the LDS a workgroup would need (very wide layers on four-row tiles) depends on N and
max_rows too and holds for that call alone.  predict, objective and predict_zeros then compute the same result from
forward(train=False, handover=False); encode, decode and influence_factors raise MfmUnsupported and the model composes its
granular operations (influence: the same recursion with torch device operations, influence_factors_torch below).

INPUTS: x is any contiguous float32 CUDA tensor [T, N, D] -- a batch view of a resident dataset, a time crop x[k:] -- at any
4-byte address; the labels and the four factors of decode() likewise (int64 class labels on 8 bytes, as torch places them).
The entries check x for 4 bytes and the parameter buffer and workspace, which the engine allocates, for 16: the kernels read x
with dword loads and with the grouped GEMM's 16-byte buffer loads, which take dword addresses (tests/test_gpu_x_offsets.py).
"""
import ctypes as C
from collections import namedtuple

import numpy as np
import torch

from . import _lib

# what encode() returns: the means and log-variances of the four latent factors, [N, size] each (logvars None for variant "mmd")
Factors = namedtuple("Factors", ["zl", "za", "zv", "zy", "logvar_zl", "logvar_za", "logvar_zv", "logvar_zy"])

# what objective() returns: the validation objective and its five terms, 0-d float32 device tensors (views of one [6] tensor)
Objective = namedtuple("Objective", ["loss", "disc", "gen_l", "gen_a", "gen_v", "reg"])

# what predict_zeros() returns, the cases in the reference's order (no l, no a, no v): y_hat [3, N, output_dim], gen [3] (the
# zeroed modality's reconstruction against the real one), disc [3] or None without labels -- float32 device tensors
Zeros = namedtuple("Zeros", ["y_hat", "gen", "disc"])

# what influence_factors() returns: fy[m, t, n] / fm[m, t, n] = the squared Frobenius norm of d x_m_hat[t, n, :] / d fy[n, :] and
# / d f_m[n, :], decoders m in the order l, a, v -- float32 device tensors [3, T, N], views of one [2, 3, T, N] tensor
Influence = namedtuple("Influence", ["fy", "fm"])


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _stream():
    # raw handle of the current stream of the current device: torch.cuda.current_stream() builds a Stream object through
    # three layers of device-index helpers (~10-20 us of host time per call; measured in the unchanged-loop profile)
    return C.c_void_p(torch._C._cuda_getCurrentRawStream(torch._C._cuda_getDevice()))


def _lstm(pre):
    return tuple(pre + suf for suf in (".lstm.weight_ih", ".lstm.weight_hh", ".lstm.bias_ih", ".lstm.bias_hh", ".fc1.weight", ".fc1.bias"))


def _lin(*names):
    return tuple(n + suf for n in names for suf in (".weight", ".bias"))


# short name of an entry -> (its state cache, its remembered refusal, the library function)
_ENTRIES = {n: ("_%s_bufs" % n, "_%s_refused" % n, f) for n, f in (
    ("predict", "mfm_predict_klef"), ("encode", "mfm_encode_klef"), ("decode", "mfm_decode_factors"),
    ("objective", "mfm_objective_klef"), ("zeros", "mfm_predict_zeros_klef"), ("influence", "mfm_influence_factors"),
    ("encode_mfn", "mfm_encode_mfn"), ("zeros_mfn", "mfm_predict_zeros_mfn"), ("objective_mfn", "mfm_objective_mfn"),
    ("predict_mfn", "mfm_predict_mfn"))}


def influence_factors_torch(decoders, fy, fms, T):
    """The forward-mode recursion of influence_factors() with torch operations, on tensors of any device and float dtype:
    `decoders` three (weight_ih, weight_hh, bias_ih, bias_hh, fc1 weight) of the decoders l, a, v, `fy` [N, fy_size], `fms` the
    three f_m [N, f_m_size] -> [2, 3, T, N] (block fy / fm, decoder, step, row).  Per decoder with e = [fy | f_m], h columns of
    tangents J^h, J^c [N, h, h] beside h_t, c_t: J^a = W_ih (step 0) or (W_ih + W_hh) J^h, the gate derivatives as row scalings,
    J^x = W_fc1 J^h_t, and the sums of its squares over the two column blocks.  What the model runs where the fused entry
    refuses (a decoder wider than MAX_RESIDENT_H), and an independent implementation to test the kernel against."""
    nfy = fy.shape[1]
    out = fy.new_empty(2, 3, T, fy.shape[0])
    for m, ((w_ih, w_hh, b_ih, b_hh, w_fc), fm) in enumerate(zip(decoders, fms)):
        e = torch.cat([fy, fm], dim=1)
        N, h = e.shape
        w_s, b = w_ih + w_hh, b_ih + b_hh
        hx = cx = jc = None
        for t in range(T):
            if t == 0:
                a = e @ w_ih.t() + b
                ja = w_ih.unsqueeze(0).expand(N, 4 * h, h)
            else:
                a = hx @ w_s.t() + b
                ja = torch.matmul(w_s, jh)                      # [4h, h] x [N, h, h] -> [N, 4h, h]
            i, f, g, o = torch.sigmoid(a[:, :h]), torch.sigmoid(a[:, h:2 * h]), torch.tanh(a[:, 2 * h:3 * h]), torch.sigmoid(a[:, 3 * h:])
            ja_i, ja_f, ja_g, ja_o = ja[:, :h], ja[:, h:2 * h], ja[:, 2 * h:3 * h], ja[:, 3 * h:]
            jc_new = (i * (1 - i) * g).unsqueeze(2) * ja_i + (i * (1 - g * g)).unsqueeze(2) * ja_g
            if t > 0:
                jc_new = jc_new + (f * (1 - f) * cx).unsqueeze(2) * ja_f + f.unsqueeze(2) * jc
                cx = f * cx + i * g
            else:
                cx = i * g
            tc = torch.tanh(cx)
            hx = o * tc
            jc = jc_new
            jh = (o * (1 - o) * tc).unsqueeze(2) * ja_o + (o * (1 - tc * tc)).unsqueeze(2) * jc
            sq = torch.matmul(w_fc, jh).square().sum(dim=1)     # [N, d, h] -> [N, h]
            out[0, m, t] = sq[:, :nfy].sum(dim=1)
            out[1, m, t] = sq[:, nfy:].sum(dim=1)
    return out


class InferMixin:
    """predict / encode / decode / objective / predict_zeros / influence_factors of MFMEngine.  Uses the engine's cfg, variant, layout, params,
    device, _check_inputs and forward."""

    PREDICT_MAX_ROWS = 1024      # default row cap: the x-projections of at most this many rows are alive at once
    MAX_RESIDENT_H = 128         # widest LSTM of the on-chip recurrences (csrc/lstm_seq_dev.h, MFM_SEQ_MAX_RESIDENT_H)

    # the parameter tensors of each entry, in the order its offsets table lists them (include/mfm_hip.h)
    _PREDICT_TENSORS = _lstm("ef_encoder") + _lin("last_to_zy_fc1", "zy_to_fy_fc1", "zy_to_fy_fc2", "fy_to_y_fc1", "fy_to_y_fc2")
    _ENCODE_TENSORS = tuple(n for enc, z in (("encoder_l", "zl"), ("encoder_a", "za"), ("encoder_v", "zv"), ("ef_encoder", "zy"))
                            for n in _lstm(enc) + _lin("last_to_%s_fc1" % z, "last_to_logvar%s_fc1" % z))
    # mfm_encode_mfn, per variant: the encoders (with their heads for "kl"), the MFN's LSTM cells, its attention and gamma
    # networks, the label head(s)
    _MFN_TENSORS = (tuple("mfn_encoder.lstm_%s.%s" % (m, n) for m in "lav" for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"))
                    + _lin(*["mfn_encoder." + n for n in ("att1_fc1", "att1_fc2", "att2_fc1", "att2_fc2", "gamma1_fc1", "gamma1_fc2",
                                                          "gamma2_fc1", "gamma2_fc2")]))
    _ENCODE_MFN_TENSORS = {
        "kl": (tuple(n for m in "lav" for n in _lstm("encoder_" + m) + _lin("last_to_z%s_fc1" % m, "last_to_logvarz%s_fc1" % m))
               + _MFN_TENSORS + _lin("last_to_zy_fc1", "last_to_logvarzy_fc1")),
        "mmd": tuple(n for m in "lav" for n in _lstm("encoder_" + m)) + _MFN_TENSORS + _lin("last_to_zy_fc1"),
    }
    # mfm_predict_mfn: the MFN, the label head and the four layers behind it -- the same 38 for both variants
    _PREDICT_MFN_TENSORS = _MFN_TENSORS + _lin("last_to_zy_fc1", "zy_to_fy_fc1", "zy_to_fy_fc2", "fy_to_y_fc1", "fy_to_y_fc2")
    _DECODE_TENSORS = (_lin(*[mlp + fc for mlp in ("zy_to_fy", "zl_to_fl", "za_to_fa", "zv_to_fv") for fc in ("_fc1", "_fc2")])
                       + _lstm("decoder_l") + _lstm("decoder_a") + _lstm("decoder_v") + _lin("fy_to_y_fc1", "fy_to_y_fc2"))

    # ------------------------------------------------------------------ the shared host path
    def _check_split(self, x, y=None, need_labels=None):
        """x [T, N, D] (, labels) -> (T, N, D), or MfmError: _check_inputs, no empty split, one label (row) per sample;
        `need_labels`: the name of an entry that cannot do without them"""
        self._check_inputs(x, y)
        if need_labels and y is None:
            raise _lib.MfmError("%s needs the labels" % need_labels)
        T, N, D = x.shape
        if T < 1 or N < 1:
            raise _lib.MfmError("empty split %s" % (tuple(x.shape),))
        if y is not None:
            ce = self.cfg.get("loss", "l1") == "ce"
            want = N if ce else N * self.cfg["output_dim"]
            if y.numel() != want:
                raise _lib.MfmError("labels must hold %d elements (%s); got shape %s" % (
                    want, "one class index per row" if ce else "[N, output_dim]", tuple(y.shape)))
        return T, N, D

    def _row_cap(self, max_rows):
        if max_rows is not None and int(max_rows) < 1:
            raise _lib.MfmError("max_rows must be at least 1, not %r" % (max_rows,))
        return self.PREDICT_MAX_ROWS if max_rows is None else int(max_rows)

    def _offsets(self, names):
        """the offsets table of an entry: where each of `names` starts in the flat parameter buffer, in floats"""
        return (C.c_int64 * len(names))(*[self.layout.offsets[n] for n in names])

    def _empty(self, *shape):
        return torch.empty(*shape, dtype=torch.float32, device=self.device)

    def _hidden_sizes(self):
        """hidden sizes of the recurrences: the ef encoder (the widest encoder), then the three decoders"""
        c = self.cfg
        return (c["zl_size"] + c["za_size"] + c["zv_size"],) + tuple(c["fy_size"] + c[k] for k in ("fl_size", "fa_size", "fv_size"))

    def _objective_sizes(self):
        c = self.cfg
        return (C.c_int32 * 13)(c["zl_size"], c["za_size"], c["zv_size"], c["zy_size"], c["fl_size"], c["fa_size"], c["fv_size"],
                                c["fy_size"], *c["input_dims"], c["output_dim"], 1 if c.get("loss", "l1") == "ce" else 0)

    def _mfn_hidden(self, encoders, decoders):
        """the recurrences of an MFN entry (variants "kl", "mmd"): the MFN's LSTMs, then the encoders and / or the decoders"""
        c = self.cfg
        return (tuple(c["h_dims"]) + ((c["zl_size"], c["za_size"], c["zv_size"]) if encoders else ())
                + (self._hidden_sizes()[1:] if decoders else ()))

    def _lambdas(self):
        c = self.cfg
        return (C.c_float * 4)(c["lda_xl"], c["lda_xa"], c["lda_xv"], c["lda_mmd"])

    def _run_fused(self, name, key, build, call, hidden):
        """One call of the fused entry `name` (a key of _ENTRIES) -> its state, or None: refused, now or remembered.  The state
        (workspace, result tensors, native tables) lives in `self._<name>_bufs[key]`: `build()` allocates it on a miss and it is
        stored once `call(fn, state)` -- fn the library function, looked up per call -- returned 0.  MFM_ERR_UNSUPPORTED sets
        `self._<name>_refused` when one of the `hidden` sizes is above MAX_RESIDENT_H (see the module docstring); any other
        code raises through _lib.check."""
        bufs, refused, entry = _ENTRIES[name]
        if getattr(self, refused, False):
            return None
        cache = self.__dict__.setdefault(bufs, {})
        st = cache.get(key)
        if st is None:
            st = build()
        rc = call(getattr(_lib.lib(), entry), st)
        if rc == 0:
            cache[key] = st
            return st
        if rc != _lib.MFM_ERR_UNSUPPORTED:
            _lib.check(rc, entry)
        setattr(self, refused, max(hidden) > self.MAX_RESIDENT_H)
        return None

    def _run_fused_or_raise(self, name, key, build, call, hidden):
        """_run_fused for the entries without a fallback of their own: a refusal raises MfmUnsupported with the library's reason"""
        _, refused, entry = _ENTRIES[name]
        remembered = getattr(self, refused, False)
        st = self._run_fused(name, key, build, call, hidden)
        if st is None:
            raise _lib.MfmUnsupported("MFMEngine.%s: %s" % (
                name, "%s refused this configuration" % entry if remembered else _lib.lib().mfm_last_error().decode()))
        return st

    # ------------------------------------------------------------------ prediction only
    def predict_workspace_floats(self, T, N, max_rows=None, label_only=False):
        """floats of workspace predict() keeps for a [T, N, D] split (mfm_predict_klef_workspace_floats; variants "kl" and "mmd"
        with label_only=True: mfm_predict_mfn_workspace_floats)"""
        if label_only and self.variant != "kl_ef":
            return int(_lib.lib().mfm_predict_mfn_workspace_floats(int(T), int(N), self._mfn_sizes(), self._row_cap(max_rows)))
        return int(_lib.lib().mfm_predict_klef_workspace_floats(int(T), int(N), self._hidden_sizes()[0], self._row_cap(max_rows)))

    def predict(self, x, y=None, *, max_rows=None, label_only=False):
        """x [T, N, D] (, labels) -> {"y_hat": [N, output_dim], "loss": 0-d device tensor or None}: the deterministic eval
        computation of y_hat and, with labels, the mean L1 / cross-entropy loss, left on the device.

        Variant "kl_ef": mfm_predict_klef -- the ef encoder's recurrence and the six layers behind it, nothing of the
        generative half.  Workspace, y_hat and the loss word are reused and a refusal falls back as the module docstring says.
        `label_only` changes nothing here: this path already is label-only.
        Variants "kl" and "mmd": by default the same dictionary from forward(train=False, want_xhat=False), bit for bit the
        eval forward on a plan.  With label_only=True: mfm_predict_mfn -- the Memory Fusion Network's three recurrences, its
        attention chain and memory recurrence on chip, the label head and the classifier in the memory recurrence's workgroup,
        the loss reduced behind it; no plan, none of the encoders, decoders or regularisers.  Its state is a cache of its own,
        `_predict_mfn_bufs`; workspace, y_hat and the loss word are reused and a refusal (remembered for an h_dims entry above
        128) falls back to the default path, as the module docstring says.  The results agree with the default's to fp32
        rounding, not bit for bit."""
        T, N, D = self._check_split(x, y)
        cap = self._row_cap(max_rows)
        c = self.cfg
        od, h = c["output_dim"], self._hidden_sizes()[0]
        if label_only and self.variant != "kl_ef":
            st = self._predict_mfn(x, y, T, N, cap)
            if st is not None:
                return {"y_hat": st[1], "loss": st[2] if y is not None else None}

        def build():
            nws = int(_lib.lib().mfm_predict_klef_workspace_floats(T, N, h, cap))
            return (self._empty(nws), self._empty(N, od), torch.zeros((), dtype=torch.float32, device=self.device),
                    self._offsets(self._PREDICT_TENSORS))

        def call(fn, st):
            ws, y_hat, loss, offs = st
            return fn(T, N, D, h, c["zy_size"], c["fy_size"], od, 1 if c.get("loss", "l1") == "ce" else 0, _ptr(self.params), offs,
                      _ptr(x), _ptr(y), _ptr(ws), _ptr(y_hat), _ptr(loss) if y is not None else None, cap, _stream())

        st = self._run_fused("predict", (T, N, cap), build, call, (h,)) if self.variant == "kl_ef" else None
        if st is not None:
            return {"y_hat": st[1], "loss": st[2] if y is not None else None}
        # (separate launches, as the eval-mode forward of the module path: inference has no optimizer guard to lean on)
        out = self.forward(x, y, train=False, want_xhat=False, handover=False)
        return {"y_hat": out["y_hat"], "loss": out["losses"][0].clone() if y is not None else None}

    def _predict_mfn(self, x, y, T, N, cap):
        """predict(label_only=True) of the variants "kl" and "mmd" through mfm_predict_mfn -> the entry's state (workspace,
        y_hat, the loss word, sizes, offsets), or None: refused"""
        def build():
            sizes = self._mfn_sizes()
            nws = int(_lib.lib().mfm_predict_mfn_workspace_floats(T, N, sizes, cap))
            return (self._empty(nws), self._empty(N, self.cfg["output_dim"]), torch.zeros((), dtype=torch.float32, device=self.device),
                    sizes, self._offsets(self._PREDICT_MFN_TENSORS))

        def call(fn, st):
            ws, y_hat, loss, sizes, offs = st
            return fn(T, N, sizes, _ptr(self.params), offs, _ptr(x), _ptr(y), _ptr(ws), _ptr(y_hat),
                      _ptr(loss) if y is not None else None, cap, _stream())

        return self._run_fused("predict_mfn", (T, N, cap), build, call, self._mfn_hidden(False, False))

    # ------------------------------------------------------------------ the factorized latents and generation from them
    def _encode_mfn_sizes(self):
        """the 17 sizes of mfm_encode_mfn (include/mfm_hip.h)"""
        c = self.cfg
        return (C.c_int32 * 17)(*c["input_dims"], c["zl_size"], c["za_size"], c["zv_size"], c["zy_size"], *c["h_dims"], c["memsize"],
                                c.get("windowsize", 2), *[k["shapes"] for k in self.configs[1:5]], 1 if self.variant == "kl" else 0)

    def encode_workspace_floats(self, T, N, max_rows=None):
        """floats of workspace encode() keeps for a [T, N, D] split (mfm_encode_klef_workspace_floats; variants "kl" and "mmd":
        mfm_encode_mfn_workspace_floats)"""
        c = self.cfg
        if self.variant != "kl_ef":
            return int(_lib.lib().mfm_encode_mfn_workspace_floats(int(T), int(N), self._encode_mfn_sizes(), self._row_cap(max_rows)))
        return int(_lib.lib().mfm_encode_klef_workspace_floats(int(T), int(N), c["zl_size"], c["za_size"], c["zv_size"],
                                                               self._row_cap(max_rows)))

    def decode_workspace_floats(self, T, N, max_rows=None):
        """floats of workspace decode() keeps for N rows and T steps (mfm_decode_factors_workspace_floats)"""
        c = self.cfg
        return int(_lib.lib().mfm_decode_factors_workspace_floats(int(T), int(N), c["fy_size"], c["fl_size"], c["fa_size"],
                                                                  c["fv_size"], self._row_cap(max_rows)))

    def encode(self, x, *, max_rows=None):
        """x [T, N, D] -> Factors(zl, za, zv, zy, logvar_zl, logvar_za, logvar_zv, logvar_zy), float32 device tensors [N, size]:
        the means and log-variances of the four latent factors (reference mfm_model.py:627-639, :723-743), the deterministic eval
        computation.  Variant "kl_ef": mfm_encode_klef (the four encoders' recurrences and their heads).  Variants "kl" and
        "mmd": mfm_encode_mfn (the three encoders and the Memory Fusion Network -- its LSTMs, the attention chain with cStar,
        attention and attended on chip, the memory recurrence and the label head); "mmd" has no heads on the encoders and no
        log-variances: zl, za, zv are the encoders' outputs and the four logvars None.  Workspace and outputs are reused as the
        module docstring says.  Raises MfmUnsupported for sizes the entry refuses (an h_dims entry or encoder size above 128 is
        remembered): the model's encode() then composes the granular operations."""
        T, N, D = self._check_split(x)
        cap = self._row_cap(max_rows)
        if self.variant != "kl_ef":
            return self._encode_mfn(x, T, N, cap)
        c = self.cfg
        zsz = (c["zl_size"], c["za_size"], c["zv_size"], c["zy_size"])

        def build():
            nws = int(_lib.lib().mfm_encode_klef_workspace_floats(T, N, zsz[0], zsz[1], zsz[2], cap))
            outs = tuple(self._empty(N, s) for s in zsz + zsz)
            return self._empty(nws), outs, self._offsets(self._ENCODE_TENSORS), (C.c_void_p * 8)(*[t.data_ptr() for t in outs])

        def call(fn, st):
            ws, _, offs, optr = st
            return fn(T, N, *c["input_dims"], *zsz, _ptr(self.params), offs, _ptr(x), _ptr(ws), optr, cap, _stream())

        return Factors(*self._run_fused_or_raise("encode", (T, N, cap), build, call, self._hidden_sizes()[:1])[1])

    def _encode_mfn(self, x, T, N, cap):
        c = self.cfg
        kl = self.variant == "kl"
        zsz = (c["zl_size"], c["za_size"], c["zv_size"], c["zy_size"])

        def build():
            sizes = self._encode_mfn_sizes()
            nws = int(_lib.lib().mfm_encode_mfn_workspace_floats(T, N, sizes, cap))
            outs = tuple(self._empty(N, s) for s in (zsz + zsz if kl else zsz))
            optr = (C.c_void_p * 8)(*[t.data_ptr() for t in outs])
            return self._empty(nws), outs + (None,) * (8 - len(outs)), self._offsets(self._ENCODE_MFN_TENSORS[self.variant]), optr, sizes

        def call(fn, st):
            ws, _, offs, optr, sizes = st
            return fn(T, N, sizes, _ptr(self.params), offs, _ptr(x), _ptr(ws), optr, cap, _stream())

        return Factors(*self._run_fused_or_raise("encode_mfn", (T, N, cap), build, call, self._mfn_hidden(True, False))[1])

    def _check_factors(self, zl, za, zv, zy, T):
        c = self.cfg
        if isinstance(T, bool) or not isinstance(T, (int, np.integer)) or T < 1:
            raise _lib.MfmError("decode: T must be an integer >= 1, not %r" % (T,))
        N = None
        for name, z, size in (("zl", zl, c["zl_size"]), ("za", za, c["za_size"]), ("zv", zv, c["zv_size"]), ("zy", zy, c["zy_size"])):
            if not (torch.is_tensor(z) and z.is_cuda and z.dtype == torch.float32 and z.dim() == 2 and z.is_contiguous()):
                raise _lib.MfmError("decode: %s must be a contiguous float32 CUDA tensor [N, %d]; got %s" % (
                    name, size, "%s %s %s" % (tuple(z.shape), z.dtype, z.device) if torch.is_tensor(z) else type(z)))
            if z.shape[1] != size:
                raise _lib.MfmError("decode: %s has %d columns, the model's %s_size is %d" % (name, z.shape[1], name, size))
            if self.device.index is not None and z.device != self.device:
                raise _lib.MfmError("decode: %s lives on %s, the engine on %s" % (name, z.device, self.device))
            if N is None:
                N = z.shape[0]
            if z.shape[0] != N or z.device != zl.device:
                raise _lib.MfmError("decode: the four factors must have the same number of rows on one device; zl has %d on %s, "
                                    "%s has %d on %s" % (N, zl.device, name, z.shape[0], z.device))
        if N < 1:
            raise _lib.MfmError("decode: no rows")
        return int(N)

    def decode(self, zl, za, zv, zy, T, *, max_rows=None):
        """four factors [N, size] (independent arguments: any rows, from encode() or not), T -> [x_l_hat, x_a_hat, x_v_hat,
        y_hat], x_m_hat [T, N, d_m], y_hat [N, output_dim]: the generative half (reference mfm_model.py:644-657), the
        deterministic eval computation, for every variant (mfm_decode_factors: the z -> f MLPs, the three decoders' recurrences
        from [fy | f_m], their fc1 and the classifier).  Workspace and outputs are reused as the module docstring says.  Raises
        MfmUnsupported for sizes the entry refuses (a decoder with fy + f_m > 128 is remembered): the model's decode() then
        composes the granular operations."""
        N = self._check_factors(zl, za, zv, zy, T)
        T = int(T)
        cap = self._row_cap(max_rows)
        c = self.cfg

        def build():
            nws = int(_lib.lib().mfm_decode_factors_workspace_floats(T, N, c["fy_size"], c["fl_size"], c["fa_size"], c["fv_size"], cap))
            outs = [self._empty(T, N, d) for d in c["input_dims"]] + [self._empty(N, c["output_dim"])]
            return (self._empty(nws), outs, self._offsets(self._DECODE_TENSORS), (C.c_int32 * 12)(*self._objective_sizes()[:12]),
                    (C.c_void_p * 4)(*[t.data_ptr() for t in outs]))

        def call(fn, st):
            ws, _, offs, sizes, optr = st
            zptr = (C.c_void_p * 4)(zl.data_ptr(), za.data_ptr(), zv.data_ptr(), zy.data_ptr())
            return fn(T, N, sizes, _ptr(self.params), offs, zptr, _ptr(ws), optr, cap, _stream())

        return list(self._run_fused_or_raise("decode", (T, N, cap), build, call, self._hidden_sizes()[1:])[1])

    # ------------------------------------------------------------------ the gradient-based interpretation
    def influence_factors_workspace_floats(self, T, N, max_rows=None):
        """floats of workspace influence_factors() keeps for N rows and T steps (mfm_influence_factors_workspace_floats: the
        decoders' packed weights)"""
        sizes = (C.c_int32 * 12)(*self._objective_sizes()[:12])
        return int(_lib.lib().mfm_influence_factors_workspace_floats(int(T), int(N), sizes, self._row_cap(max_rows)))

    def influence_factors(self, zl, za, zv, zy, T, *, max_rows=None):
        """four factors [N, size] (independent arguments, as for decode()), T -> Influence(fy, fm), float32 device tensors
        [3, T, N] (views of one [2, 3, T, N] tensor): how strongly the factors drive the generation of modality m = l, a, v at
        step t of row n -- fy[m, t, n] = || d x_m_hat[t, n, :] / d fy[n, :] ||_F^2 and fm[m, t, n] the same for the modality's own
        f_m, the derivative taken with respect to the factors behind the z -> f MLPs -- from the deterministic eval
        computation, for every variant (mfm_influence_factors: forward mode, the tangents of a row resident in LDS along the
        decoder's recurrence, the products on the fp32 MFMA; no Jacobian and no x_hat is written).  Workspace and result are
        reused as the module docstring says; results are bit-identical from run to run and for every max_rows.  Raises
        MfmUnsupported for sizes the entry refuses (a decoder with fy + f_m > 128 is remembered): the model's
        influence_factors() then runs influence_factors_torch."""
        N = self._check_factors(zl, za, zv, zy, T)
        T = int(T)
        cap = self._row_cap(max_rows)

        def build():
            sizes = (C.c_int32 * 12)(*self._objective_sizes()[:12])
            nws = int(_lib.lib().mfm_influence_factors_workspace_floats(T, N, sizes, cap))
            out = self._empty(2, 3, T, N)
            return self._empty(nws), out, Influence(out[0], out[1]), self._offsets(self._DECODE_TENSORS), sizes

        def call(fn, st):
            ws, out, _, offs, sizes = st
            zptr = (C.c_void_p * 4)(zl.data_ptr(), za.data_ptr(), zv.data_ptr(), zy.data_ptr())
            return fn(T, N, sizes, _ptr(self.params), offs, zptr, _ptr(ws), _ptr(out), cap, _stream())

        return self._run_fused_or_raise("influence", (T, N, cap), build, call, self._hidden_sizes()[1:])[2]

    # ------------------------------------------------------------------ the full validation objective
    def objective_workspace_floats(self, T, N, max_rows=None):
        """floats of workspace objective() keeps for a [T, N, D] split (mfm_objective_klef_workspace_floats; variants "kl" and
        "mmd": mfm_objective_mfn_workspace_floats)"""
        if self.variant != "kl_ef":
            return int(_lib.lib().mfm_objective_mfn_workspace_floats(int(T), int(N), self._mfn_sizes(), self._row_cap(max_rows)))
        return int(_lib.lib().mfm_objective_klef_workspace_floats(int(T), int(N), self._objective_sizes(), self._row_cap(max_rows)))

    def objective(self, x, y, *, max_rows=None):
        """x [T, N, D], labels -> Objective(loss, disc, gen_l, gen_a, gen_v, reg), 0-d float32 device tensors (views of one [6]
        tensor): what the reference's drivers validate and report (mfm_mosi.py:319-324, :724-726, :826-845) -- disc the mean L1 /
        cross entropy as evaluate() defines it, gen_m = F.mse_loss(x_m_hat, x_m), reg the sum of the four loss_KLD(mu, logvar),
        loss = disc + lda_xl gen_l + lda_xa gen_a + lda_xv gen_v + lda_mmd reg -- from the deterministic eval computation, left
        on the device.

        Variant "kl_ef": mfm_objective_klef -- the launches of encode(), the recurrence launch of decode(), then the decoders'
        fc1 fused with the squared error (x_hat is never written) and one small finishing launch.  Variants "kl" and "mmd":
        mfm_objective_mfn -- the launches of encode() for these classes (the Memory Fusion Network on chip), then the same
        decoder, squared-error and finishing launches; its state is a cache of its own, `_objective_mfn_bufs`.  For "mmd" reg
        is the sum of the four maximum mean discrepancies over all N^2 pairs of the split against a Gaussian sample [N, zl + za
        + zv + zy]: `self.gauss` when set, else a buffer of the entry's state refilled with .normal_() on every call; the
        value-only MMD launch writes one partial per workgroup and a last launch adds them in fp64 (no float atomics: reg is
        bit-identical from run to run for a given sample).  Workspace and the [6] result are reused and a refusal falls back as
        the module docstring says (remembered for an h_dims entry, an encoder or a decoder above 128): the same namedtuple
        from forward(train=False, handover=False), the total formed on the device."""
        T, N, D = self._check_split(x, y, need_labels="objective")
        cap = self._row_cap(max_rows)
        c = self.cfg
        if self.variant != "kl_ef":
            st = self._objective_mfn(x, y, T, N, cap)
            if st is not None:
                return st[2]

        def build():
            sizes = self._objective_sizes()
            nws = int(_lib.lib().mfm_objective_klef_workspace_floats(T, N, sizes, cap))
            out = torch.zeros(6, dtype=torch.float32, device=self.device)
            return (self._empty(nws), out, Objective(*out.unbind(0)), sizes, self._offsets(self._ENCODE_TENSORS + self._DECODE_TENSORS),
                    self._lambdas())

        def call(fn, st):
            ws, out, _, sizes, offs, lda = st
            return fn(T, N, sizes, lda, _ptr(self.params), offs, _ptr(x), _ptr(y), _ptr(ws), _ptr(out), cap, _stream())

        st = self._run_fused("objective", (T, N, cap), build, call, self._hidden_sizes()) if self.variant == "kl_ef" else None
        if st is not None:
            return st[2]
        # (separate launches, as the eval-mode forward of the module path: inference has no optimizer guard to lean on)
        l = self.forward(x, y, train=False, handover=False)["losses"]
        out = self._empty(6)
        out[1:6] = l[0:5]
        out[0] = l[0] + c["lda_xl"] * l[1] + c["lda_xa"] * l[2] + c["lda_xv"] * l[3] + c["lda_mmd"] * l[4]
        return Objective(*out.unbind(0))

    def _objective_mfn(self, x, y, T, N, cap):
        """objective() of the variants "kl" and "mmd" through mfm_objective_mfn -> the entry's state, or None: refused.  A given
        `self.gauss` is checked here in front of the entry, so also when the entry is remembered as refused: a sample of the
        wrong shape, dtype or device raises MfmError before the fallback's plan would trip over it with an assert"""
        c = self.cfg
        mmd = self.variant == "mmd"
        gl = c["zl_size"] + c["za_size"] + c["zv_size"] + c["zy_size"]
        given = self.gauss if mmd else None
        if given is not None and not (torch.is_tensor(given) and given.is_cuda and given.dtype == torch.float32 and given.is_contiguous()
                                      and tuple(given.shape) == (N, gl) and given.device == x.device):
            raise _lib.MfmError("objective: gauss must be a contiguous float32 CUDA tensor [%d, %d] on %s; got %s" % (
                N, gl, x.device, "%s %s %s" % (tuple(given.shape), given.dtype, given.device) if torch.is_tensor(given) else type(given)))

        def build():
            sizes = self._mfn_sizes()
            nws = int(_lib.lib().mfm_objective_mfn_workspace_floats(T, N, sizes, cap))
            out = torch.zeros(6, dtype=torch.float32, device=self.device)
            return (self._empty(nws), out, Objective(*out.unbind(0)), sizes,
                    self._offsets(self._ENCODE_MFN_TENSORS[self.variant] + self._DECODE_TENSORS), self._lambdas(),
                    self._empty(N, gl) if mmd else None)

        def call(fn, st):
            ws, out, _, sizes, offs, lda, drawn = st
            g = given
            if mmd and g is None:
                g = drawn.normal_()
            return fn(T, N, sizes, lda, _ptr(self.params), offs, _ptr(x), _ptr(y), _ptr(g), _ptr(ws), _ptr(out), cap, _stream())

        return self._run_fused("objective_mfn", (T, N, cap), build, call, self._mfn_hidden(True, True))

    # ------------------------------------------------------------------ the zeroed-modality test protocol
    def _mfn_sizes(self):
        """the 23 sizes of mfm_predict_zeros_mfn, mfm_objective_mfn and mfm_predict_mfn (include/mfm_hip.h): the 17 of
        mfm_encode_mfn, the f sizes, output_dim, loss kind"""
        c = self.cfg
        return (C.c_int32 * 23)(*self._encode_mfn_sizes(), c["fl_size"], c["fa_size"], c["fv_size"], c["fy_size"], c["output_dim"],
                                1 if c.get("loss", "l1") == "ce" else 0)

    _zeros_mfn_sizes = _mfn_sizes      # the name from when predict_zeros alone used it: callers outside this file keep working

    def predict_zeros_workspace_floats(self, T, N, max_rows=None):
        """floats of workspace predict_zeros() keeps for a [T, N, D] split (mfm_predict_zeros_klef_workspace_floats; variants
        "kl" and "mmd": mfm_predict_zeros_mfn_workspace_floats)"""
        if self.variant != "kl_ef":
            return int(_lib.lib().mfm_predict_zeros_mfn_workspace_floats(int(T), int(N), self._mfn_sizes(), self._row_cap(max_rows)))
        return int(_lib.lib().mfm_predict_zeros_klef_workspace_floats(int(T), int(N), self._objective_sizes(), self._row_cap(max_rows)))

    def predict_zeros(self, x, y=None, *, max_rows=None):
        """x [T, N, D] (, labels) -> Zeros(y_hat [3, N, output_dim], gen [3], disc [3] or None), float32 device tensors: the test
        protocol of the reference's train_mfm_test_zeros (mfm_mosi.py:572-596) -- the split through the deterministic eval forward
        with modality l, a, v zeroed in turn (the cases in that order); gen[c] = F.mse_loss(x_c_hat of case c, the REAL x_c),
        unweighted, disc[c] the mean L1 / cross entropy of y_hat[c] as evaluate() defines it (None without labels).  Every mean is
        over the whole split.

        Variant "kl_ef": mfm_predict_zeros_klef -- no zeroed copy of x, the ef encoder's projection computed once for the three
        cases, the zeroed encoder one row of work, one decoder per case with its fc1 fused into the squared error (x_hat is
        never written).  Variants "kl" and "mmd": mfm_predict_zeros_mfn -- the MFN's three LSTMs on the real columns once for
        the three cases, the zeroed modality's MFN LSTM and encoder one row of work each, the attention chain and the memory
        recurrence of encode() over the (case, row) pairs, then the same decoders' launches; its state is a cache of its own,
        `_zeros_mfn_bufs`.  Workspace and the three result tensors are reused and a refusal falls back as the module docstring
        says (remembered for an h_dims entry, an encoder or a decoder above 128): the same namedtuple from three
        forward(train=False, handover=False) calls on zeroed copies, the means formed on the device."""
        T, N, D = self._check_split(x, y)
        cap = self._row_cap(max_rows)
        c = self.cfg
        od = c["output_dim"]
        klef = self.variant == "kl_ef"

        def build():
            if klef:
                sizes = self._objective_sizes()
                nws = int(_lib.lib().mfm_predict_zeros_klef_workspace_floats(T, N, sizes, cap))
                offs = self._offsets(self._ENCODE_TENSORS + self._DECODE_TENSORS)
            else:
                sizes = self._mfn_sizes()
                nws = int(_lib.lib().mfm_predict_zeros_mfn_workspace_floats(T, N, sizes, cap))
                offs = self._offsets(self._ENCODE_MFN_TENSORS[self.variant] + self._DECODE_TENSORS)
            return (self._empty(nws), self._empty(3, N, od), torch.zeros(3, dtype=torch.float32, device=self.device),
                    torch.zeros(3, dtype=torch.float32, device=self.device), sizes, offs)

        def call(fn, st):
            ws, y_hat, gen, disc, sizes, offs = st
            return fn(T, N, sizes, _ptr(self.params), offs, _ptr(x), _ptr(y), _ptr(ws), _ptr(y_hat), _ptr(gen),
                      _ptr(disc) if y is not None else None, cap, _stream())

        if klef:
            st = self._run_fused("zeros", (T, N, cap), build, call, self._hidden_sizes())
        else:
            st = self._run_fused("zeros_mfn", (T, N, cap), build, call, self._mfn_hidden(True, True))
        if st is not None:
            return Zeros(st[1], st[2], st[3] if y is not None else None)
        # (separate launches, as the eval-mode forward of the module path: inference has no optimizer guard to lean on)
        y_hat, gen = self._empty(3, N, od), self._empty(3)
        disc = self._empty(3) if y is not None else None
        d_l, d_a, d_v = c["input_dims"]
        for i, (a, b, key) in enumerate(((0, d_l, "x_l_hat"), (d_l, d_l + d_a, "x_a_hat"), (d_l + d_a, D, "x_v_hat"))):
            xz = x.clone()
            xz[:, :, a:b] = 0
            out = self.forward(xz, y, train=False, handover=False)
            y_hat[i].copy_(out["y_hat"])
            # (the forward's own loss slot is the error against the zeroed columns: the protocol asks for the real ones)
            gen[i] = (out[key] - x[:, :, a:b]).square().mean()
            if y is not None:
                disc[i] = out["losses"][0]
        return Zeros(y_hat, gen, disc)
