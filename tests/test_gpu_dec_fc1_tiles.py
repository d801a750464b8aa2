"""The decoder fc1 launch (csrc/dec_fc1.hip) through the C ABI, on the smallest shapes that reach each of its paths, against a
float64 numpy evaluation of the formulas in the file's header:

    x_hat = H Wfc^T + b,  diff = x_hat - x,  loss += sum diff^2 * inv_count,  dx_hat = grad_scale * diff,  dH = dx_hat Wfc

  * rows 1, 16, 17, 33: partial row tiles, more than one row tile
  * d 5, 20: one column group with a partly filled fragment; d 129, 300: 2 and 3 column groups, the last with fewer fragments
    and a masked tail column
  * h 24 (Hp 32), 104 (Hp 112) and 128 (Hp 128, the kernel's limit); three decoders of different Hp in one launch, as the plan runs
  * forward only and forward + dH; the bf16-operand flag

One column group STORES dH: the buffer is filled with NaN first and must come back finite (it needs no zero span), and two
runs give the same bits.  Several column groups add into a cleared buffer.  Every output buffer carries guard rows behind
`rows` that must keep their bits.  Tolerance: the project's fp32 contract, 1e-4 of the tensor's largest magnitude (what
tests/test_gpu_plan.py asks of x_hat and of the gradients); the reductions here are at most 300 terms long."""
import ctypes as C

import numpy as np
import pytest
import torch

from factorized_amd import _lib
from tests.cases import rel_err

pytestmark = pytest.mark.gpu
TOL = 1e-4
GUARD = 3                      # rows behind the last valid one in every output buffer
SENTINEL = -7.25


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _bf16(a):
    return torch.from_numpy(np.asarray(a, dtype=np.float32)).bfloat16().float().numpy().astype(np.float64)


class _Item:
    """one decoder's operands on the device, its float64 reference on the host"""

    def __init__(self, rows, d, h, Hp, seed):
        g = torch.Generator().manual_seed(seed)
        self.rows, self.d, self.h, self.Hp = rows, d, h, Hp
        H = torch.zeros(rows, Hp)
        H[:, :h] = torch.tanh(torch.randn(rows, h, generator=g))          # hidden states; pad units are zeros
        self.ldx = d + 7                                                   # the targets are columns [3, 3 + d) of a wider matrix
        X = torch.randn(rows, self.ldx, generator=g)
        self.H, self.X = H.cuda(), X.cuda()
        self.W = (torch.randn(d, h, generator=g) / h ** 0.5).cuda()
        self.b = (0.1 * torch.randn(d, generator=g)).cuda()
        self.inv_count = 1.0 / (rows * d)
        self.grad_scale = 2.0 * 0.5 / (rows * d)
        self.loss0 = 0.5
        self.fresh()

    def fresh(self, dh_fill=float("nan")):
        r = self.rows + GUARD
        self.xhat = torch.full((r, self.d), SENTINEL, device="cuda")
        self.dxhat = torch.full((r, self.d), SENTINEL, device="cuda")
        self.dH = torch.full((r, self.Hp), dh_fill, device="cuda")
        self.dH[self.rows:] = SENTINEL
        self.loss = torch.full((1,), self.loss0, device="cuda")

    def fill(self, it):
        it.hs, it.w, it.bias = self.H.data_ptr(), self.W.data_ptr(), self.b.data_ptr()
        it.x, it.ldx = self.X.data_ptr() + 3 * 4, self.ldx
        it.xhat, it.dxhat, it.dhs, it.loss = self.xhat.data_ptr(), self.dxhat.data_ptr(), self.dH.data_ptr(), self.loss.data_ptr()
        it.d, it.h, it.Hp = self.d, self.h, self.Hp
        it.inv_count, it.grad_scale = self.inv_count, self.grad_scale

    def reference(self, bf16):
        H = self.H.cpu().numpy().astype(np.float64)[:, :self.h]
        W = self.W.cpu().numpy().astype(np.float64)
        if bf16:
            H, W = _bf16(H), _bf16(W)
        x = self.X.cpu().numpy().astype(np.float64)[:, 3:3 + self.d]
        xhat = H @ W.T + self.b.cpu().numpy().astype(np.float64)
        diff = xhat - x
        return xhat, float((diff ** 2).sum() * self.inv_count), self.grad_scale * diff, W


def _launch(items, rows, with_bwd, bf16, zeroed):
    arr = (_lib.DecFc1Item * len(items))()
    for i, it in enumerate(items):
        it.fill(arr[i])
    rc = _lib.lib().mfm_dec_fc1_f32(arr, len(items), rows, with_bwd, bf16, zeroed, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc


def _run_and_check(shapes, rows, with_bwd, bf16):
    items = [_Item(rows, d, h, Hp, seed=100 + 7 * i + rows) for i, (d, h, Hp) in enumerate(shapes)]
    for it in items:                                  # stored form: NaN in, finite out; added form: the caller's cleared buffer
        it.fresh(dh_fill=float("nan") if it.d <= 128 else 0.0)
    assert _launch(items, rows, with_bwd, bf16, 1) == 0, _lib.lib().mfm_last_error()
    for it in items:
        xhat_ref, loss_ref, dx_ref, W = it.reference(bf16)
        xhat, dxhat, dH = it.xhat.cpu().numpy(), it.dxhat.cpu().numpy(), it.dH.cpu().numpy()
        tag = (rows, it.d, it.h, it.Hp, with_bwd, bf16)
        e_x, e_dx = rel_err(xhat[:rows], xhat_ref), rel_err(dxhat[:rows], dx_ref)
        loss = float(it.loss.item()) - it.loss0
        print("dec fc1 %s: x_hat %.2e  dx_hat %.2e  loss %.6g (ref %.6g)" % (tag, e_x, e_dx, loss, loss_ref))
        assert e_x < TOL and e_dx < TOL, tag
        # (the slot is added to: the sum carries the rounding of loss0 + loss, half an ulp of 0.5 .. 4)
        assert abs(loss - loss_ref) <= TOL * max(abs(loss_ref), 1e-3) + 2.5e-7, tag
        assert np.all(xhat[rows:] == SENTINEL) and np.all(dxhat[rows:] == SENTINEL), tag
        assert np.all(dH[rows:] == SENTINEL), tag
        if not with_bwd:
            continue
        assert np.all(np.isfinite(dH[:rows])), tag
        assert np.all(dH[:rows, it.h:] == 0.0), tag    # pad units leave as exact zeros
        # bf16 operands: the kernel rounds ITS d x_hat (checked above) on the way into the product; a float64 d x_hat one
        # fp32 rounding away can land on the other side of a bf16 rounding boundary, so the reference rounds the same values
        dx_in = _bf16(dxhat[:rows]) if bf16 else dx_ref
        dH_ref = dx_in @ W
        e_h = rel_err(dH[:rows, :it.h], dH_ref)
        print("dec fc1 %s: dH %.2e" % (tag, e_h))
        assert e_h < TOL, tag
    return items


CASES = [
    # (decoders' (d, h, Hp), rows, with_bwd, bf16)
    ([(5, 24, 32)], 1, 1, 0),
    ([(20, 24, 32)], 16, 1, 0),
    ([(129, 104, 112)], 17, 1, 0),
    ([(300, 104, 112)], 33, 1, 0),
    ([(300, 128, 128)], 33, 1, 0),
    ([(20, 128, 128)], 17, 1, 0),
    ([(300, 104, 112), (5, 24, 32), (20, 24, 32)], 33, 1, 0),       # the plan's launch: three decoders, mixed Hp
    ([(300, 104, 112), (5, 24, 32)], 33, 0, 0),
    ([(129, 128, 128)], 16, 0, 0),
    ([(129, 24, 32), (20, 104, 112)], 33, 1, 1),
]


@pytest.mark.parametrize("shapes,rows,with_bwd,bf16", CASES)
def test_fc1_launch_matches_float64(shapes, rows, with_bwd, bf16):
    _need_gpu()
    _run_and_check(shapes, rows, with_bwd, bf16)


def test_stored_dh_is_reproducible_bit_for_bit():
    _need_gpu()
    bits = []
    for _ in range(2):
        items = _run_and_check([(20, 104, 112), (128, 24, 32)], 33, 1, 0)
        bits.append([it.dH.cpu().numpy().view(np.uint32).copy() for it in items])
    for a, b in zip(*bits):
        assert np.array_equal(a, b)


def test_shapes_the_kernel_does_not_take_are_declined_without_a_launch():
    _need_gpu()
    wide = _Item(16, 129, 24, 32, seed=5)
    wide.fresh(dh_fill=1.0)
    assert _launch([wide], 16, 1, 0, 0) == -3          # several column groups add into dH: it has to be cleared
    big = _Item(16, 20, 140, 144, seed=6)
    big.fresh(dh_fill=1.0)
    assert _launch([big], 16, 1, 0, 1) == -3           # Hp > 128
    for it in (wide, big):
        assert bool((it.dH[:16] == 1.0).all()) and bool((it.xhat == SENTINEL).all())
