"""Contiguous CUDA tensors that do not start on a 16-byte boundary (tests/test_gpu_x_offsets.py).  Every other GPU test hands the
kernels a freshly allocated tensor, which the allocator places on 256 bytes; the package promises its users no such thing --
batch i of an [nb, T, B, D] dataset, a time crop x[k:] and any view of a flat staging buffer are contiguous and start 4, 8 or
12 bytes past a boundary.

at_residue(t, r) returns the values and shape of `t` as a contiguous view into a flat buffer of its own,

    [ GUARD + r / itemsize sentinels | t.numel() values | GUARD sentinels ]

whose data_ptr() % 16 == r (asserted here).  The sentinels are 7: outputs are never views of the inputs, so all they can catch
is a stray write around an input; check_guards() compares them after the calls under test and is cheap."""
import torch

RESIDUES = (0, 4, 8, 12)
GUARD = 64                 # elements in front of the view and behind it
SENTINEL = 7

_LIVE = []                 # (view, flat buffer, first element of the view) of every at_residue since the last check_guards
                           # or forget_views


def at_residue(t, r, device="cuda"):
    """`t` (a torch tensor or a numpy array; float32 or int64) -> a contiguous tensor on `device` with t's values and shape whose
    data_ptr() % 16 == r"""
    t = torch.as_tensor(t)
    item = t.element_size()
    assert r in RESIDUES and r % item == 0, (r, item)
    n = t.numel()
    flat = torch.full((GUARD + r // item + n + GUARD,), SENTINEL, dtype=t.dtype, device=device)
    assert flat.data_ptr() % 16 == 0 and (GUARD * item) % 16 == 0
    first = GUARD + r // item
    view = flat[first:first + n].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and view.data_ptr() % 16 == r, (view.data_ptr() % 16, r)
    assert view.data_ptr() == flat.data_ptr() + first * item
    _LIVE.append((view, flat, first))
    return view


def forget_views():
    """drop the views handed out so far, unchecked (a fixture calls this around every test)"""
    del _LIVE[:]


def residue(t):
    return t.data_ptr() % 16


def check_guards():
    """every sentinel around every view handed out since the last call is unchanged; forgets the views and returns how many"""
    n = len(_LIVE)
    while _LIVE:
        view, flat, first = _LIVE.pop()
        head, tail = flat[:first], flat[first + view.numel():]
        assert tail.numel() == GUARD
        assert bool((head == SENTINEL).all()), "sentinels in front of a view at residue %d were overwritten" % residue(view)
        assert bool((tail == SENTINEL).all()), "sentinels behind a view at residue %d were overwritten" % residue(view)
    return n
