"""Host half of the granular ops' parameter guard (`_ops._require_f32`): dtype, contiguity and device equality are checked
on CPU tensors here, so the guard is known to hold before tests/test_gpu_autograd_contract.py hands a converted module to
the GPU path.  No launch, no library."""
import pytest
import torch

from factorized_amd import _lib, _ops

CPU = torch.device("cpu")
NAMES = ("lstm.weight_ih", "lstm.weight_hh", "lstm.bias_ih", "lstm.bias_hh", "fc1.weight", "fc1.bias")


def _params(h=4, d=3):
    return [torch.zeros(4 * h, d), torch.zeros(4 * h, h), torch.zeros(4 * h), torch.zeros(4 * h), torch.zeros(h, h),
            torch.zeros(h)]


def test_accepts_contiguous_float32_and_skips_none():
    _ops._require_f32("encoderLSTM", CPU, NAMES, _params())
    _ops._require_f32("Linear", CPU, ("weight", "bias"), (torch.zeros(5, 3), None))       # nn.Linear(bias=False)
    # a contiguous slice of a flat buffer (how the fused engine's parameters are stored) is fine
    flat = torch.zeros(256)
    _ops._require_f32("Linear", CPU, ("weight", "bias"), (flat[64:64 + 15].view(5, 3), flat[128:133]))


@pytest.mark.parametrize("dtype", [torch.float64, torch.float16, torch.bfloat16, torch.int32])
@pytest.mark.parametrize("which", range(6))
def test_refuses_other_dtypes_naming_the_tensor(dtype, which):
    p = _params()
    p[which] = p[which].to(dtype)
    with pytest.raises(_lib.MfmError) as ei:
        _ops._require_f32("encoderLSTM", CPU, NAMES, p)
    msg = str(ei.value)
    assert "encoderLSTM" in msg and NAMES[which] in msg and str(dtype) in msg
    assert str(tuple(p[which].stride())) in msg


def test_refuses_non_contiguous_naming_tensor_and_strides():
    p = _params()
    w = torch.arange(64.0).view(16, 4)
    p[1] = w.t().contiguous().t()                  # same values and shape, strides (1, 16)
    assert torch.equal(p[1], w) and not p[1].is_contiguous()
    with pytest.raises(_lib.MfmError) as ei:
        _ops._require_f32("decoderLSTM", CPU, NAMES, p)
    msg = str(ei.value)
    assert "lstm.weight_hh" in msg and "(1, 16)" in msg and "torch.float32" in msg
    p[1] = torch.zeros(16, 8)[:, ::2]              # a stepped column view
    with pytest.raises(_lib.MfmError, match=r"lstm\.weight_hh"):
        _ops._require_f32("decoderLSTM", CPU, NAMES, p)
    p[1] = torch.zeros(1, 4).expand(16, 4)         # stride 0
    with pytest.raises(_lib.MfmError, match=r"lstm\.weight_hh"):
        _ops._require_f32("decoderLSTM", CPU, NAMES, p)


def test_refuses_a_tensor_on_another_device_than_the_input():
    p = _params()
    p[4] = torch.zeros(4, 4, device="meta")
    with pytest.raises(_lib.MfmError) as ei:
        _ops._require_f32("encoderLSTM", CPU, NAMES, p)
    assert "fc1.weight" in str(ei.value) and "meta" in str(ei.value)
    with pytest.raises(_lib.MfmError, match=r"lstm\.weight_ih"):
        _ops._require_f32("encoderLSTM", torch.device("meta"), NAMES, _params())


def test_is_a_runtime_error_like_every_error_of_the_package():
    assert issubclass(_lib.MfmError, RuntimeError)
    with pytest.raises(RuntimeError):
        _ops._require_f32("Linear", CPU, ("weight", "bias"), (torch.zeros(2, 2).double(), None))


def test_consumed_graph_flag_raises_once_set():
    """`_consume` is what the four recurrent Functions call first in backward: silent until their BPTT launch set the flag."""
    class Ctx(object):
        pass
    ctx = Ctx()
    _ops._consume(ctx, "encoderLSTM")
    ctx.consumed = True
    with pytest.raises(RuntimeError, match="already back-propagated"):
        _ops._consume(ctx, "encoderLSTM")
