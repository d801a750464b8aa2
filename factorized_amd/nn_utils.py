"""Drop-in `clip_grad_norm_` / `clip_grad_value_` for the reference-style training step:

    from factorized_amd.nn_utils import clip_grad_norm_         # instead of: from torch.nn.utils import clip_grad_norm_
    ...
    loss.backward(); clip_grad_norm_(model.parameters(), max_norm); optimizer.step()

Same signatures, return value (a 0-dim tensor on the gradients' device) and error texts as torch's.  When every listed parameter
belongs to ONE fused model (`MFM_KL_EF`, `MFM_KL`, `MFM`) whose `.grad`s are the views of its flat gradient buffer, the call is
two launches (`mfm_clip_grad_norm_flat_spans`) or one (`mfm_clip_grad_value_flat_spans`) over that buffer on the current stream,
with no host synchronisation and no per-tensor device work:

  * the spans of the launch are the exact extents of the listed tensors that received a gradient since `zero_grad()` (a tensor
    without one is skipped, as torch skips `.grad is None` -- the stale values its view may still hold stay out of the norm);
    the padding between tensors is neither read into the norm nor written;
  * the launches honour the guard word of the flat gradient buffer: after a hand-over of the step gave up, the gradients are left
    alone (the guarded optimizer is going to skip them anyway) and the returned norm is NaN;
  * `norm_type` 2, inf and 1 are built.

Everything else -- other modules, the composed models of mfm_extra.py, frozen or hooked parameters, `fast_grads = False`,
parameters of two fused models in one call, any other `norm_type`, CPU tensors -- goes, whole, to torch's function with the
caller's arguments: the gradient views are ordinary tensors, so that is always correct.

Neither function touches the model's gradient bookkeeping or any optimizer state.  `error_if_nonfinite=True` reads the norm back
(one synchronisation, as in torch) and raises torch's error; unlike torch the gradients have then already been multiplied by the
non-finite coefficient."""
import math
import weakref

import numpy as np
import torch

from . import _flat, _lib
from ._fused import _owner_of

_KINDS = {2.0: _lib.MFM_NORM_L2, math.inf: _lib.MFM_NORM_INF, 1.0: _lib.MFM_NORM_L1}

# model -> its clip state: the partials workspace of the norm launches, index of every Parameter, span tables by selection
# (weak keys, and not on the module: its __getstate__ would pickle them)
_STATE = weakref.WeakKeyDictionary()


def _state_of(m, eng):
    st = _STATE.get(m)
    if st is None or st["total"] != eng.layout.total or st["ws"].device != eng.params.device:
        order, extents = _flat.extents(eng.layout, padded=False)
        st = dict(total=eng.layout.total, ws=torch.empty(int(_lib.lib().mfm_clip_workspace_floats()), dtype=torch.float32,
                                                         device=eng.params.device),
                  index={id(p): i for i, p in enumerate(m._plist)}, order=order, extents=extents, tables={})
        _STATE[m] = st
    return st


def _flat_selection(params):
    """(model, engine, flat gradient buffer, bool mask of the listed tensors) when the call can take the flat path, else None"""
    m = _owner_of(params[0])
    if m is None:
        return None
    plist = m._plist
    if not plist[0].is_cuda:
        return None
    eng = m.engine
    gflat = getattr(m, "_grad_flat", None)
    if gflat is None or gflat.dtype != torch.float32 or not m._fast_last or not m._grad_views_attached():
        return None
    slots = eng.layout.slots
    if len(params) == len(plist) and all(a is b for a, b in zip(params, plist)):      # model.parameters(): the usual call
        listed, mask = range(len(plist)), np.ones(len(plist), dtype=bool)
    else:
        index = _state_of(m, eng)["index"]
        listed = []
        for p in params:
            i = index.get(id(p))
            if i is None or plist[i] is not p:
                return None                         # a parameter of another model / module
            listed.append(i)
        mask = np.zeros(len(plist), dtype=bool)
        mask[listed] = True
        if int(mask.sum()) != len(listed):
            return None                             # listed twice: torch counts and scales it twice
    base = gflat.data_ptr()
    for i in listed:
        g = plist[i].grad
        if g is None or g.data_ptr() != base + 4 * slots[i][0]:
            return None                             # somebody replaced this .grad: an ordinary tensor
    return m, eng, gflat, mask


def _table(m, eng, mask):
    """(ctypes span array, length) for the listed tensors that have a gradient: exact extents in address order, two tensors
    merged only where one ends exactly where the next begins; None: more spans than one launch takes; length 0: nothing"""
    st = _state_of(m, eng)
    sel = mask & m._grad_present
    key = sel.tobytes()
    hit = st["tables"].get(key)
    if hit is None:
        spans = _flat.merge_spans(st["order"], st["extents"], sel)
        if len(spans) > _lib.MFM_CLIP_MAX_SPANS:
            hit = (None, -1)
        else:
            arr = (_lib.ClipSpan * max(len(spans), 1))()
            for a, (b, e, _) in zip(arr, spans):
                a.begin, a.end = b, e
            hit = (arr, len(spans))
        if len(st["tables"]) > 32:
            st["tables"].clear()
        st["tables"][key] = hit
    return st, hit


def _as_list(parameters):
    return [parameters] if isinstance(parameters, torch.Tensor) else list(parameters)


def clip_grad_norm_(parameters, max_norm, norm_type=2.0, error_if_nonfinite=False, foreach=None):
    """torch.nn.utils.clip_grad_norm_; on a fused model two launches over its flat gradient buffer (see the module doc)"""
    params = _as_list(parameters)
    kind = _KINDS.get(float(norm_type))
    hit = _flat_selection(params) if params and kind is not None and float(max_norm) >= 0.0 else None
    if hit is not None:
        m, eng, gflat, mask = hit
        st, (arr, n) = _table(m, eng, mask)
        if n == 0:
            return torch.tensor(0.0)                 # no listed tensor has a gradient (torch: every .grad is None)
        if arr is not None:
            total = torch.empty((), dtype=torch.float32, device=gflat.device)
            stream, guard = _flat.stream_and_guard(eng, gflat)
            _lib.check(_lib.lib().mfm_clip_grad_norm_flat_spans(_flat.ptr(gflat), arr, n, kind, float(max_norm),
                                                                _flat.ptr(st["ws"]), _flat.ptr(total), guard, stream),
                       "mfm_clip_grad_norm_flat_spans")
            if error_if_nonfinite and not math.isfinite(float(total)):
                raise RuntimeError(
                    f"The total norm of order {float(norm_type)} for gradients from "
                    "`parameters` is non-finite, so it cannot be clipped. To disable "
                    "this error and scale the gradients by the non-finite norm anyway, "
                    "set `error_if_nonfinite=False`")
            return total
    return torch.nn.utils.clip_grad_norm_(params if params else parameters, max_norm, norm_type, error_if_nonfinite, foreach)


def clip_grad_value_(parameters, clip_value, foreach=None):
    """torch.nn.utils.clip_grad_value_; on a fused model one launch over its flat gradient buffer (see the module doc)"""
    params = _as_list(parameters)
    hit = _flat_selection(params) if params and float(clip_value) >= 0.0 else None
    if hit is not None:
        m, eng, gflat, mask = hit
        _, (arr, n) = _table(m, eng, mask)
        if n == 0:
            return None
        if arr is not None:
            stream, guard = _flat.stream_and_guard(eng, gflat)
            _lib.check(_lib.lib().mfm_clip_grad_value_flat_spans(_flat.ptr(gflat), arr, n, float(clip_value), guard,
                                                                 stream), "mfm_clip_grad_value_flat_spans")
            return None
    return torch.nn.utils.clip_grad_value_(params if params else parameters, clip_value, foreach)
