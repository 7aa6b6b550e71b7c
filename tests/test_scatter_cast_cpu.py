"""ops.slice_scatter_cast without a GPU: the bit-arithmetic model (cast_model.py) against torch's and
NumPy's own converts on the value sets, then the ops host path (host addresses) and the table
validation against the model, every buffer compared whole, canaries included."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import cast_model as C
import shard_model as M
from zest_amd import ops

DEV = "cpu"
TORCH = {"F32": torch.float32, "F16": torch.float16, "BF16": torch.bfloat16}
NUMPY = {"F32": np.float32, "F16": np.float16}
INT = {2: torch.int16, 4: torch.int32}
PAIR_IDS = [f"{s}-{d}" for s, d in C.PAIRS]


def test_value_sets_are_the_ones_the_cases_need():
    assert all(len(C.values(s, d)) == 1 << 16 for s, d in C.PAIRS if s != "F32")
    assert len(C.values("F32", "BF16")) == 6 << 16
    f = C.values("F32", "F16")
    assert len(f) == 4 * 2 * 0x7BFF + 10 + (6 << 16)
    for bits in (0x477FEFFF, 0x477FF000, 0x33000000, 0x33000001, 0x33800000):
        assert bits in f[4 * 2 * 0x7BFF:4 * 2 * 0x7BFF + 5]
    assert C.convert(np.array([0x477FEFFF, 0x477FF000, 0x33000000, 0x33000001, 0x33800000], dtype="<u4"), "F32",
                     "F16").tolist() == [0x7BFF, 0x7C00, 0, 1, 1]


@pytest.mark.parametrize("pair", C.PAIRS, ids=PAIR_IDS)
def test_model_classifies_nans_as_numpy_does(pair):
    bits = C.values(*pair)
    if pair[0] == "BF16":  # NumPy has no bf16: a bf16 is the upper half of an f32
        ref = np.isnan((bits.astype(np.uint32) << np.uint32(16)).view(np.float32))
    else:
        ref = np.isnan(bits.view(NUMPY[pair[0]]))
    assert np.array_equal(C.is_nan(bits, pair[0]), ref)
    assert ref.any() and not ref.all()
    assert C.is_nan(C.convert(bits, *pair), pair[1])[ref].all()  # the model keeps a NaN a NaN


@pytest.mark.parametrize("pair", C.PAIRS, ids=PAIR_IDS)
def test_model_equals_torch_and_numpy_off_nan(pair):
    bits = C.values(*pair)
    got = C.convert(bits, *pair)
    keep = ~C.is_nan(bits, pair[0])
    signed = torch.from_numpy(bits.view(f"<i{bits.itemsize}").copy())
    t = signed.view(TORCH[pair[0]]).to(TORCH[pair[1]]).view(INT[C.ITEM[pair[1]]]).numpy().view(got.dtype)
    assert np.array_equal(got[keep], t[keep])
    if "BF16" not in pair:
        with np.errstate(over="ignore"):  # overflow to infinity is one of the cases
            n = bits.view(NUMPY[pair[0]]).astype(NUMPY[pair[1]]).view(got.dtype)
        assert np.array_equal(got[keep], n[keep])


@pytest.mark.parametrize("src_align", [0, 1, 2, 3])
def test_values(src_align):
    C.case_values(ops, DEV, src_align)


@pytest.mark.parametrize("pair", C.PAIRS, ids=PAIR_IDS)
def test_alignment_grid(pair):
    C.case_alignment_grid(ops, DEV, pair)


@pytest.mark.parametrize("stride", list(M.STRIDES))
@pytest.mark.parametrize("pair", C.PAIRS, ids=PAIR_IDS)
def test_run_grid(pair, stride):
    C.case_run_grid(ops, DEV, pair, stride)


@pytest.mark.parametrize("gap", [0, 2])
def test_mixed_kinds_share_blocks(gap):
    C.case_mixed_small(ops, DEV, gap)


def test_tiles_and_many_small_entries():
    C.case_tiles(ops, DEV)
    C.case_many_small(ops, DEV)


def test_three_allocations_descending_table():
    C.case_three_allocations(ops, DEV)


def test_empty_and_all_zero_tables_do_nothing(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("a table without output reached the conversion")

    monkeypatch.setattr(ops, "_slice_scatter_cast_cpu", boom)
    C.case_nothing_to_do(ops, DEV)


def test_refusals_leave_the_buffers_untouched():
    C.case_refusals(ops, DEV, pytest)


def test_kinds_are_the_six_float_pairs():
    assert set(ops.CAST_KINDS) == set(C.PAIRS) and sorted(ops.CAST_KINDS.values()) == list(range(6))
    assert ops.CAST_DTYPE.names == ops.SCATTER_DTYPE.names + ("kind",)
