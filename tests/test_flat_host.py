"""factorized_amd._flat without a GPU: what the drop-in utilities on the flat buffers share -- the host side of the metric
argument, the span walk in both extent forms on a hand-made layout, the int32 state block, the capture check."""
import struct
from types import SimpleNamespace

import pytest
import torch

from factorized_amd import _flat, _lib


def _double_bits(v):
    return struct.pack("<d", v)


@pytest.mark.parametrize("metric", [0.1, float("inf"), float("nan"), torch.tensor(0.1, dtype=torch.float64),
                                    torch.tensor([1.0 + 2.0 ** -20], dtype=torch.float32)],
                         ids=["float", "inf", "nan", "cpu-0d", "cpu-1-element"])
def test_metric_arg_passes_a_host_metric_on_as_its_double(metric):
    keep, host = _flat.metric_arg(metric, torch.device("cuda", 0), "KeepBest.update", "the model's device")
    assert keep is None and type(host) is float
    assert _double_bits(host) == _double_bits(float(metric))


# five tensors in state_dict order as (offset, numel, shape): starts 64-float aligned, padding behind each; tensor 3 is empty;
# in address order they are 2, 0, 1, 3, 4, and tensor 0 ends exactly where tensor 1 begins
LAYOUT = SimpleNamespace(slots=[(128, 64, (64,)), (192, 10, (10,)), (0, 100, (100,)), (256, 0, (0,)), (320, 30, (30,))], guard=384)
ALL = [True] * 5
WITHOUT_1 = [True, False, True, True, True]
KEYS = ["a", "a", "b", "a", "a"]


def test_padded_extents_run_from_start_to_next_start_and_to_the_guard():
    order, extents = _flat.extents(LAYOUT, padded=True)
    assert order == [2, 0, 1, 3, 4]
    assert extents == [(0, 128), (128, 192), (192, 256), (256, 320), (320, 384)]
    # equal keys merge across the padding (the empty tensor's granule included), another key breaks the run
    assert _flat.merge_spans(order, extents, ALL, KEYS) == [(0, 128, "b"), (128, 384, "a")]
    assert _flat.merge_spans(order, extents, WITHOUT_1, KEYS) == [(0, 128, "b"), (128, 192, "a"), (256, 384, "a")]
    assert _flat.merge_spans(order, extents, ALL, ["a", "c", "a", "c", "c"]) == [(0, 192, "a"), (192, 384, "c")]
    assert _flat.merge_spans(order, extents, [False] * 5, KEYS) == []


def test_exact_extents_skip_the_empty_tensor_and_merge_only_where_one_ends_where_the_next_begins():
    order, extents = _flat.extents(LAYOUT, padded=False)
    assert order == [2, 0, 1, 4]
    assert extents == [(0, 100), (128, 192), (192, 202), (320, 350)]
    assert _flat.merge_spans(order, extents, ALL) == [(0, 100, None), (128, 202, None), (320, 350, None)]
    assert _flat.merge_spans(order, extents, WITHOUT_1) == [(0, 100, None), (128, 192, None), (320, 350, None)]
    assert _flat.merge_spans(order, extents, ALL, ["a", "x", "a", "a", "a"]) == [(0, 100, "a"), (128, 192, "a"), (192, 202, "x"),
                                                                                 (320, 350, "a")]


def test_span_tables_cut_the_spans_into_launches():
    spans = [(0, 128, (3,)), (128, 192, (4,)), (256, 384, (5,))]
    tables = _flat.span_tables(spans, _lib.AdamSpan, 2, ("step",))
    assert [n for _, n in tables] == [2, 1]
    assert [(a.begin, a.end, a.step) for arr, n in tables for a in arr[:n]] == [(0, 128, 3), (128, 192, 4), (256, 384, 5)]


NAN_PAYLOAD = struct.unpack("<f", struct.pack("<I", 0x7FC12345))[0]      # a quiet fp32 NaN that carries a payload
INT32_MIN = -2 ** 31


def test_state_block_of_keep_best_round_trips_bit_patterns():
    """MfmKeepBestState: best_value (a float) in word 0, calls, best_call, taken, ticket"""
    layout = [(0, "float32"), (1, "int32"), (2, "int32"), (3, "int32")]
    for value, word0 in ((NAN_PAYLOAD, 0x7FC12345), (-0.0, INT32_MIN), (1.0, 0x3F800000)):
        values = [value, INT32_MIN + 1, -1, 1]
        host = _flat.pack_words(_lib.MFM_KEEP_STATE_WORDS, [(w, k, v) for (w, k), v in zip(layout, values)])
        assert host.dtype == torch.int32 and host.device.type == "cpu"
        assert host.tolist() == [word0, INT32_MIN + 1, -1, 1, 0, 0, 0, 0]
        back = _flat.unpack_words(host, layout)
        assert [type(v) for v in back] == [float, int, int, int] and back[1:] == values[1:]
        assert struct.pack("<f", back[0]) == struct.pack("<i", word0) == struct.pack("<f", value)


def test_state_block_of_the_plateau_scheduler_keeps_the_double():
    """MfmPlateauState: best (a double) in words 0-1, num_bad_epochs, cooldown_counter, last_epoch, reduced, reductions"""
    layout = [(0, "float64")] + [(w, "int32") for w in (2, 3, 4, 5, 6)]
    for value in (0.1, -0.0, float("inf"), 1.0 + 2.0 ** -40):          # (0.1 and the last one are no fp32 values)
        values = [value, INT32_MIN + 1, -1, 7, 1, 2 ** 31 - 1]
        host = _flat.pack_words(_lib.MFM_PLATEAU_STATE_WORDS, [(w, k, v) for (w, k), v in zip(layout, values)])
        low, high = struct.unpack("<ii", _double_bits(value))
        assert host.tolist() == [low, high, INT32_MIN + 1, -1, 7, 1, 2 ** 31 - 1, 0]
        back = _flat.unpack_words(host, layout)
        assert _double_bits(back[0]) == _double_bits(value) and back[1:] == values[1:]
    assert struct.unpack("<ii", _double_bits(0.1)) == (-1717986918, 1069128089)      # 0x3FB99999_9999999A, low word first


def test_capturing_is_false_outside_a_capture_and_does_not_need_a_gpu():
    assert _flat.capturing() is False
