"""The grouped GEMM's refusals without a GPU: every argument error of mfm_gemm_grouped_f32 / _bf16 is caught on the host
before anything is enqueued, with return code -1 and its own text.  The operand pointers are fake, aligned integers: no call
below gets as far as a launch, so none is ever dereferenced."""
import ctypes as C

import pytest

from factorized_amd import _lib

FAKE = 1 << 20                    # 16-byte aligned, never dereferenced


def desc(**over):
    """a plain 64 x 64 x 64 forward product (a, b k-contiguous) with the fields of `over` replaced"""
    d = _lib.GemmDesc()
    d.a, d.b, d.c = FAKE, FAKE, FAKE
    d.m, d.n, d.k, d.n_valid, d.batch = 64, 64, 64, 64, 1
    d.a_sm, d.a_sk, d.b_sk, d.b_sn, d.ldc = 64, 1, 1, 64, 64
    d.alpha = 1.0
    for name, v in over.items():
        if name == "reserved_":
            d.reserved_[0], d.reserved_[1] = v
        else:
            setattr(d, name, v)
    return d


def refused(entry, descs, msg):
    L = _lib.lib()
    arr = (_lib.GemmDesc * len(descs))(*descs)
    rc = getattr(L, entry)(arr, len(descs), None)
    err = L.mfm_last_error()
    assert rc == -1, (entry, msg, rc)
    assert msg in err, (entry, msg, err)


ENTRIES = ("mfm_gemm_grouped_f32", "mfm_gemm_grouped_bf16")


@pytest.mark.parametrize("entry", ENTRIES)
def test_entry_refuses_an_empty_call_and_reserved_fields_under_its_own_name(entry):
    L = _lib.lib()
    one = (_lib.GemmDesc * 1)(desc())
    for descs, count in ((None, 1), (one, 0), (one, -3)):
        assert getattr(L, entry)(descs, count, None) == -1
        assert L.mfm_last_error() == entry.encode() + b": no problems"
    refused(entry, [desc(reserved_=(1, 0))], entry.encode() + b": problem 0 has non-zero reserved_ fields (zero the struct before filling it)")
    refused(entry, [desc(), desc(reserved_=(0, 7))], entry.encode() + b": problem 1 has non-zero reserved_ fields")


# (fields replaced, fragment of the error text) -- refused alike by both entries
COMMON = [
    (dict(m=0), b"gemm[0]: bad dims m=0 n=64 k=64 batch=1"),
    (dict(n=-1, n_valid=0), b"gemm[0]: bad dims m=64 n=-1 k=64 batch=1"),
    (dict(k=-1), b"gemm[0]: bad dims m=64 n=64 k=-1 batch=1"),
    (dict(batch=0), b"gemm[0]: bad dims m=64 n=64 k=64 batch=0"),
    (dict(a=None), b"gemm[0]: null operand"),
    (dict(b=None), b"gemm[0]: null operand"),
    (dict(c=None), b"gemm[0]: null operand"),          # (a null c belongs to a squared-error epilogue, which no C entry carries)
    (dict(n_valid=65), b"gemm[0]: n_valid 65 > n 64"),
    (dict(n_valid=-1), b"gemm[0]: n_valid -1 > n 64"),
    (dict(split_k=2), b"gemm[0]: split_k needs accumulate"),
    (dict(a_sk=-1), b"gemm[0]: operand strides must lie in [0, 2^31) (a_sm=64 a_sk=-1 b_sk=1 b_sn=64)"),
    (dict(b_sn=-64), b"gemm[0]: operand strides must lie in [0, 2^31) (a_sm=64 a_sk=1 b_sk=1 b_sn=-64)"),
    (dict(a_sm=1 << 31), b"gemm[0]: operand strides must lie in [0, 2^31) (a_sm=2147483648 a_sk=1 b_sk=1 b_sn=64)"),
    (dict(b_sk=1 << 31), b"gemm[0]: operand strides must lie in [0, 2^31) (a_sm=64 a_sk=1 b_sk=2147483648 b_sn=64)"),
    # the span of one batch member, first to last element: 2^29 fp32 elements are one byte too many
    (dict(m=2, k=1, a_sm=(1 << 29) - 1), b"gemm[0]: operand a spans 536870912 elements (2147483648 bytes); the 32-bit byte offsets"),
    (dict(m=2, a_sm=1 << 29), b"gemm[0]: operand a spans 536870976 elements (2147483904 bytes)"),
    (dict(m=3, k=5, a_sm=1 << 28, a_sk=1 << 20), b"gemm[0]: operand a spans 541065217 elements (2164260868 bytes)"),
    (dict(n=2, n_valid=2, k=1, b_sn=(1 << 29) - 1), b"gemm[0]: operand b spans 536870912 elements (2147483648 bytes); the 32-bit byte offsets"),
    (dict(b_sk=1 << 24, b_sn=1), b"gemm[0]: operand b spans 1056964672 elements (4227858688 bytes)"),
    # only the valid columns of b count
    (dict(n=4, n_valid=2, k=1, b_sn=(1 << 29) - 1), b"gemm[0]: operand b spans 536870912 elements"),
    # the order of the checks: dims, null operand, n_valid, split_k, strides, span of a, span of b
    (dict(m=0, a=None), b"bad dims"),
    (dict(a=None, n_valid=65), b"null operand"),
    (dict(n_valid=65, split_k=2), b"n_valid 65 > n 64"),
    (dict(split_k=2, a_sk=-1), b"split_k needs accumulate"),
    (dict(a_sk=-1, m=2, a_sm=1 << 29), b"operand strides must lie"),
    (dict(m=2, a_sm=1 << 29, b_sk=1 << 24, b_sn=1), b"operand a spans"),
]


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("over,msg", COMMON, ids=["%02d-%s" % (i, "-".join(sorted(o))) for i, (o, _) in enumerate(COMMON)])
def test_per_problem_refusals(entry, over, msg):
    refused(entry, [desc(**over)], msg)
    # the same problem behind a sound one is named by its own index
    if msg.startswith(b"gemm[0]"):
        refused(entry, [desc(), desc(**over)], msg.replace(b"gemm[0]", b"gemm[1]"))


def test_bf16_resident_operands_are_refused_by_the_f32_entry():
    text = b"gemm[0]: bf16-resident operands (a_bf16 / c_bf16) are taken by the bf16 entry point only"
    refused("mfm_gemm_grouped_f32", [desc(a_bf16=1)], text)
    refused("mfm_gemm_grouped_f32", [desc(c_bf16=1)], text)
    # ... ahead of what the bf16 entry would say about them, behind dims and null operands
    refused("mfm_gemm_grouped_f32", [desc(c_bf16=1, accumulate=1)], text)
    refused("mfm_gemm_grouped_f32", [desc(a_bf16=1, a=FAKE + 8)], text)
    refused("mfm_gemm_grouped_f32", [desc(a_bf16=1, b=None)], b"null operand")
    refused("mfm_gemm_grouped_f32", [desc(a_bf16=1, n_valid=65)], text)


def test_bf16_entry_refuses_ill_shaped_bf16_resident_operands():
    entry = "mfm_gemm_grouped_bf16"
    plain = b"gemm[0]: c_bf16 needs a plain (non-accumulating, unsplit) product"
    refused(entry, [desc(c_bf16=1, accumulate=1)], plain)
    refused(entry, [desc(c_bf16=1, accumulate=1, split_k=2)], plain)
    refused(entry, [desc(c_bf16=1, split_k=2)], plain)          # (ahead of "split_k needs accumulate")
    axis = b"gemm[0]: a_bf16 needs a unit-stride axis on 16-byte boundaries "
    refused(entry, [desc(a_bf16=1, a=FAKE + 8)], axis + b"(a_sm=64 a_sk=1 a_sz=0)")
    refused(entry, [desc(a_bf16=1, a=FAKE + 2)], axis + b"(a_sm=64 a_sk=1 a_sz=0)")
    refused(entry, [desc(a_bf16=1, a_sm=60)], axis + b"(a_sm=60 a_sk=1 a_sz=0)")
    refused(entry, [desc(a_bf16=1, a_sz=4, batch=2)], axis + b"(a_sm=64 a_sk=1 a_sz=4)")
    refused(entry, [desc(a_bf16=1, a_sm=1, a_sk=68)], axis + b"(a_sm=1 a_sk=68 a_sz=0)")
    refused(entry, [desc(a_bf16=1, a_sm=2, a_sk=8)], axis + b"(a_sm=2 a_sk=8 a_sz=0)")
    refused(entry, [desc(a_bf16=1, a_sm=1, a_sk=1)], axis + b"(a_sm=1 a_sk=1 a_sz=0)")
    refused(entry, [desc(a_bf16=1, a=FAKE + 8, n_valid=65)], axis)          # (ahead of n_valid)


def test_bf16_resident_span_counts_two_byte_elements_in_whole_dwords():
    entry = "mfm_gemm_grouped_bf16"
    # 2^30 bf16 elements are one byte too many ...
    refused(entry, [desc(a_bf16=1, m=2, k=8, a_sm=(1 << 30) - 8)], b"gemm[0]: operand a spans 1073741824 elements (2147483648 bytes)")
    # ... and so are 2^30 - 1: the extent is rounded up to whole dwords
    refused(entry, [desc(a_bf16=1, m=2, k=7, a_sm=(1 << 30) - 8)], b"gemm[0]: operand a spans 1073741823 elements (2147483648 bytes)")
    refused(entry, [desc(a_bf16=1, m=2, k=1, a_sm=1 << 30)], b"gemm[0]: operand a spans 1073741825 elements (2147483652 bytes)")
    # b stays fp32 beside a bf16-resident a
    refused(entry, [desc(a_bf16=1, n=2, n_valid=2, k=1, b_sn=(1 << 29) - 1)], b"gemm[0]: operand b spans 536870912 elements (2147483648 bytes)")


def test_bf16_resident_operands_need_a_group_without_oddly_strided_members():
    entry = "mfm_gemm_grouped_bf16"
    whole = b": bf16-resident operands need unit-stride operands in the whole group"
    odd_a, odd_b = desc(a_sm=2, a_sk=3), desc(b_sk=2, b_sn=128)
    refused(entry, [desc(a_bf16=1), odd_a], b"gemm[0]" + whole)
    refused(entry, [odd_a, desc(c_bf16=1)], b"gemm[1]" + whole)
    refused(entry, [desc(), odd_b, desc(a_bf16=1, a_sm=1, a_sk=64)], b"gemm[2]" + whole)
    # a per-problem refusal of a later member comes first: the group rule is checked behind every problem's own
    refused(entry, [desc(a_bf16=1), desc(a_sm=2, a_sk=3, n_valid=65)], b"gemm[1]: n_valid 65 > n 64")
