"""Drop-in `torch.optim.swa_utils` for the reference-style training loop (also reachable as `factorized_amd.optim.swa_utils`,
so a loop written against `import torch.optim as optim` switches with the same one import line as the optimizers):

    from factorized_amd.swa_utils import AveragedModel, get_ema_multi_avg_fn     # instead of: from torch.optim.swa_utils import ...
    ema = AveragedModel(model, multi_avg_fn=get_ema_multi_avg_fn(0.999))
    ...
    loss.backward(); optimizer.step(); ema.update_parameters(model)

`AveragedModel` is a subclass of torch's with the same constructor, `forward`, `state_dict()` keys (`n_averaged`, `module.*`)
and semantics.  When `model` and the averaged copy are fused models (`MFM_KL_EF`, `MFM_KL`, `MFM`) of the same class on the same
CUDA device whose parameters are the views of their engines' flat fp32 buffers, `update_parameters(model)` is ONE launch of
`mfm_avg_flat` on the current stream over [offset of the first tensor, layout.guard) of the two flat parameter buffers:

  * the update count is read from `n_averaged` ON THE DEVICE and advanced by the launch itself: no host read, no
    synchronisation (torch's method reads `n_averaged` twice per call), and the call is legal inside a stream capture -- a
    replayed graph keeps counting;
  * the first update copies the parameters bit for bit, every later one is torch's lerp with weight 1 / (n + 1) (SWA) or
    1 - decay (EMA);
  * the gradient guard plays no part: a guard-skipped optimizer step leaves the parameters unchanged, and averaging unchanged
    parameters is what torch does too.

`n_averaged` must be on the parameters' device for that: the constructor puts it there when the copy is a fused model on the
GPU (torch creates it on the CPU unless `device` is given), and `.to()` / `.cuda()` move it with the module.  The averaged copy's engine is adopted lazily on the first update (`copy.deepcopy` drops it); the source model must already be
on its engine (it is after its first forward).  The averaging rule must be one this library can name: none given (SWA, as in
torch), or a function made by THIS module's `get_ema_multi_avg_fn` / `get_swa_multi_avg_fn` / `get_ema_avg_fn` /
`get_swa_avg_fn`, which validate as torch's do and return torch's own function with two attributes that name the rule.  A
function made by torch's own factories is an opaque closure here: it is NOT recognised and takes torch's path.  On the flat
path all four rules are computed as the lerp of the `multi` forms (`get_ema_avg_fn` / `get_swa_avg_fn` differ from it by a
rounding or two on torch's path).

Everything else -- CPU models, the composed models of mfm_extra.py, any other nn.Module, a custom `avg_fn`, modules with
buffers, a model on another device or with another layout, a source model whose parameters left the flat buffer -- goes, whole,
to torch's `update_parameters`: the parameters are ordinary tensors, so that is always correct.  Both paths use the one
`n_averaged` buffer and may alternate freely.

The launch needs one int32 "ticket" word per AveragedModel (csrc/avg.hip): allocated on first use (outside a stream capture),
kept off `state_dict()`, dropped by pickling and `copy.deepcopy`, reallocated when the device changes, never shared between
instances -- two instances may update on two streams.

`SWALR` and `update_bn` are torch's objects (`SWALR` works on the flat optimizers: schedulers act on `param_groups`)."""
import torch
from torch.optim import swa_utils as _T

from . import _flat, _lib
from ._fused import _FusedEngineMixin

__all__ = list(_T.__all__)

SWALR = _T.SWALR
update_bn = _T.update_bn

_KIND_ATTR, _DECAY_ATTR = "_mfm_avg_kind", "_mfm_avg_decay"


def _named(fn, kind, decay):
    setattr(fn, _KIND_ATTR, kind)
    setattr(fn, _DECAY_ATTR, decay)
    return fn


def get_ema_multi_avg_fn(decay=0.999):
    """torch.optim.swa_utils.get_ema_multi_avg_fn, named so that AveragedModel can take the flat path"""
    return _named(_T.get_ema_multi_avg_fn(decay), _lib.MFM_AVG_EMA, float(decay))


def get_swa_multi_avg_fn():
    """torch.optim.swa_utils.get_swa_multi_avg_fn, named so that AveragedModel can take the flat path"""
    return _named(_T.get_swa_multi_avg_fn(), _lib.MFM_AVG_SWA, None)


def get_ema_avg_fn(decay=0.999):
    """torch.optim.swa_utils.get_ema_avg_fn, named so that AveragedModel can take the flat path"""
    return _named(_T.get_ema_avg_fn(decay), _lib.MFM_AVG_EMA, float(decay))


def get_swa_avg_fn():
    """torch.optim.swa_utils.get_swa_avg_fn, named so that AveragedModel can take the flat path"""
    return _named(_T.get_swa_avg_fn(), _lib.MFM_AVG_SWA, None)


class AveragedModel(_T.AveragedModel):
    """torch.optim.swa_utils.AveragedModel; between two fused models one launch over their flat buffers (see the module doc)"""

    def __init__(self, model, device=None, avg_fn=None, multi_avg_fn=None, use_buffers=False):
        super().__init__(model, device=device, avg_fn=avg_fn, multi_avg_fn=multi_avg_fn, use_buffers=use_buffers)
        # torch leaves n_averaged on the CPU unless `device` is given; the flat path reads and advances it on the GPU, so beside a
        # fused model on the GPU it starts there (where `.to(device)` / `.cuda()` would put it too; torch's path takes either)
        if isinstance(self.module, _FusedEngineMixin):
            p = self.module._plist[0]
            if p.is_cuda and self.n_averaged.device != p.device:
                self.n_averaged = self.n_averaged.to(p.device)
        self._mfm_ticket = None
        self._mfm_range = None          # (source layout, own layout) of the pair last checked for the flat path

    def __getstate__(self):
        state = dict(self.__dict__)
        state["_mfm_ticket"] = None          # (never shared with a copy: each instance draws its own tickets)
        state["_mfm_range"] = None
        return state

    def _rule(self):
        """(kind, w) of an averaging rule this library can name, else None"""
        fn = self.multi_avg_fn if self.multi_avg_fn is not None else self.avg_fn
        if fn is None:
            return _lib.MFM_AVG_SWA, 0.0
        kind = getattr(fn, _KIND_ATTR, None)
        if kind == _lib.MFM_AVG_SWA:
            return kind, 0.0
        if kind == _lib.MFM_AVG_EMA:
            return kind, 1.0 - getattr(fn, _DECAY_ATTR)          # in double; rounded once to fp32 at the call, as torch's scalar
        return None

    def _flat_args(self, model):
        """(avg engine, model engine, begin, kind, w) when this update can take the flat path, else None"""
        rule = self._rule()
        mine = self.module
        if rule is None or not isinstance(model, _FusedEngineMixin) or type(model) is not type(mine) or model is mine:
            return None
        p, q = model._plist[0], mine._plist[0]
        n = self.n_averaged
        if not (p.is_cuda and q.device == p.device and n.device == p.device and n.dtype == torch.int64):
            return None
        if not model._flat_ok():
            return None
        src, dst = model._engine, mine.engine          # (the copy is adopted here on first use)
        ls, ld = src.layout, dst.layout
        hit = self.__dict__.get("_mfm_range")
        if hit is None or hit[0] is not ls or hit[1] is not ld:
            # (once per pair of engines: walking the sub-modules for buffers costs as much host time as half a training step)
            if (ls.total != ld.total or ls.guard != ld.guard or ls.slots != ld.slots or _flat.has_buffers(model)
                    or _flat.has_buffers(mine)):
                return None
            self._mfm_range = (ls, ld)
        return dst, src, ld.begin, rule[0], rule[1]

    def update_parameters(self, model):
        hit = self._flat_args(model)
        if hit is None:
            return super().update_parameters(model)
        dst, src, begin, kind, w = hit
        dev = dst.params.device
        ticket = self.__dict__.get("_mfm_ticket")
        if ticket is None or ticket.device != dev:
            ticket = self._mfm_ticket = torch.zeros(1, dtype=torch.int32, device=dev)
        _lib.check(_lib.lib().mfm_avg_flat(_flat.ptr(dst.params), _flat.ptr(src.params), begin, dst.layout.guard, kind, w,
                                           _flat.ptr(self.n_averaged), _flat.ptr(ticket), _flat.stream_ptr(dev)), "mfm_avg_flat")
