"""What the drop-in utilities on the engine's flat fp32 buffers share (optim, nn_utils, swa_utils, checkpoint, lr_scheduler,
train.DeviceDataset): the capture check, the raw stream handle and the guard word, the buffer walk, the metric argument of a
one-launch epoch utility, the walk over a layout's tensors in address order, and the int32 state block of the two-form state.
Plain functions, private to the package; the first offset of a layout is `engine.FlatLayout.begin`."""
import ctypes as C

import numpy as np
import torch

from . import _lib


def capturing():
    """CUDA is available and the current stream is capturing"""
    return torch.cuda.is_available() and torch.cuda.is_current_stream_capturing()


def ptr(t):
    return C.c_void_p(t.data_ptr())


def stream_ptr(device):
    """raw handle of the current stream of `device` (torch.cuda.current_stream() builds a Stream object: 10-20 us of host time)"""
    return C.c_void_p(torch._C._cuda_getCurrentRawStream(device.index))


def stream_and_guard(eng, gflat):
    """the current stream, and the guard word of the flat gradient buffer: the plan's backward stores a NaN there when a
    hand-over inside one of its launches gave up -- a guarded update then leaves parameters and optimizer state alone
    (engine.check_status() reports it)"""
    return (C.c_void_p(torch._C._cuda_getCurrentRawStream(eng.params.device.index)),          # (once per step: no nested call)
            C.c_void_p(gflat.data_ptr() + 4 * eng.layout.guard))


def has_buffers(module):
    """its state_dict is more than the flat range covers (the walk costs half a training step of host time: callers cache it)"""
    return any(sub._buffers for sub in module.modules())


def metric_arg(metric, dev, who, where):
    """The metric of a one-launch epoch utility as (tensor, host value), one of them None.  A `lazy.LossExpr` is evaluated and
    a device tensor detached, then brought to fp32 on `dev` (a 0-d or 1-element fp32 tensor already there is returned itself:
    the launch reads it by pointer, the caller keeps it alive); a python number or a CPU tensor comes back as `float(metric)`
    for the launch's scalar argument, and is refused inside a stream capture."""
    from . import lazy
    if isinstance(metric, lazy.LossExpr):
        keep = metric._value()
    elif isinstance(metric, torch.Tensor) and metric.is_cuda:
        if metric.numel() != 1:
            raise ValueError("%s: the metric must have one element, not shape %s" % (who, tuple(metric.shape)))
        keep = metric.detach()
    else:
        if capturing():
            raise _lib.MfmError("%s: a host metric (python float or CPU tensor) inside a stream capture would be baked into the "
                                "graph -- every replay would compare the same number.  Pass the metric as a 0-d fp32 tensor on %s"
                                % (who, where))
        return None, float(metric)
    if keep.device != dev or keep.dtype != torch.float32:
        keep = keep.to(device=dev, dtype=torch.float32)
    return keep, None


# ---------------------------------------------------------------------- spans of a flat buffer
def extents(layout, padded):
    """the tensors of a flat layout in address order, and (begin, end) of each: padded -- from its start to the next start, the
    last one to the guard (tensor starts are 64-float aligned: span bounds are multiples of 4) -- or exact, empty tensors skipped"""
    order = np.argsort([o for o, _, _ in layout.slots], kind="stable").tolist()
    if not padded:
        order = [i for i in order if layout.slots[i][1]]          # (an empty tensor has no exact extent: it is left out)
    starts = [layout.slots[i][0] for i in order]
    ends = starts[1:] + [layout.guard] if padded else [layout.slots[i][0] + layout.slots[i][1] for i in order]
    return order, list(zip(starts, ends))


def merge_spans(order, extents, present, keys=None):
    """[(begin, end, key)]: walk the tensors in address order (`extents[k]` belongs to tensor `order[k]`), skip tensor i unless
    present[i], merge two where one ends exactly where the next begins and their keys[i] agree (no keys: key None)"""
    spans = []
    for (b, e), i in zip(extents, order):
        if not present[i]:
            continue
        h = keys[i] if keys is not None else None
        if spans and spans[-1][1] == b and spans[-1][2] == h:
            spans[-1] = (spans[-1][0], e, h)
        else:
            spans.append((b, e, h))
    return spans


def span_tables(spans, span_cls, max_spans, fields):
    """[(ctypes array, length)]: the spans cut into chunks of at most max_spans (one launch each); a span's key is the tuple of
    its `fields`"""
    tables = []
    for k in range(0, len(spans), max_spans):
        part = spans[k:k + max_spans]
        arr = (span_cls * len(part))()
        for a, (b, e, key) in zip(arr, part):
            a.begin, a.end = b, e
            for name, val in zip(fields, key):
                setattr(a, name, val)
        tables.append((arr, len(part)))
    return tables


def launch_tables(fn, name, head, tables, tail):
    """one launch of the span entry point `fn(*head, spans, nspans, *tail)` per table"""
    for arr, n in tables:
        _lib.check(fn(*head, arr, n, *tail), name)


# ---------------------------------------------------------------------- the int32 state block of a two-form state
_KINDS = {"int32": (torch.int32, 1), "float32": (torch.float32, 1), "float64": (torch.float64, 2)}      # kind: dtype, words


def pack_words(n, fields):
    """a CPU int32 tensor of `n` words, zero but for `fields`: (word index, kind, value) with kind "int32", "float32" (one
    word) or "float64" (two words, from an even index)"""
    host = torch.zeros(n, dtype=torch.int32)
    for w, kind, value in fields:
        dtype, k = _KINDS[kind]
        host[w:w + k].view(dtype)[0] = value
    return host


def unpack_words(host, fields):
    """the python values of `fields`, (word index, kind), of a CPU int32 tensor that `pack_words` or a kernel filled"""
    return [host[w:w + _KINDS[kind][1]].view(_KINDS[kind][0])[0].item() for w, kind in fields]
