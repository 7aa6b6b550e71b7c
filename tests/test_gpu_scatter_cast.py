"""GPU: the converting slice-scatter kernel (csrc/gpu/scatter_cast.hip, ops.slice_scatter_cast) against
the bit-arithmetic model (cast_model.py).  Destinations are carved out of canary-filled allocations at
every alignment, and every byte of every allocation is compared after the launch: outputs equal the
model bit for bit (a NaN where the source element is one), all other bytes still hold their
position-dependent canary."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import cast_model as C
import shard_model as M
from zest_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAIR_IDS = [f"{s}-{d}" for s, d in C.PAIRS]


@pytest.mark.parametrize("src_align", [0, 1, 2, 3])
def test_values(src_align):
    """Every kind over its whole value set (all 16-bit patterns; the F32 tie, carry, overflow and
    subnormal sets), six entries in one launch."""
    C.case_values(ops, DEV, src_align)


@pytest.mark.parametrize("pair", C.PAIRS, ids=PAIR_IDS)
def test_alignment_grid(pair):
    """dst & 15 x src & 15 x element count in one launch of 512 or 1024 entries: the 256-ary search and
    the overflow of the LDS cache both run."""
    C.case_alignment_grid(ops, DEV, pair)


@pytest.mark.parametrize("stride", list(M.STRIDES))
@pytest.mark.parametrize("pair", C.PAIRS, ids=PAIR_IDS)
def test_run_grid_equals_the_model_and_the_host_path(pair, stride):
    """The run grid at every destination alignment against the model, and the kernel's buffers
    against the ops host path's on the same inputs: bit for bit off NaN."""
    gpu = C.case_run_grid(ops, DEV, pair, stride)
    cpu = C.case_run_grid(ops, "cpu", pair, stride)
    assert len(gpu) == len(cpu) == 16 // C.ITEM[pair[1]]
    for (g, nan_g), (c, nan_c) in zip(gpu, cpu):
        assert np.array_equal(nan_g, nan_c) and np.array_equal(g[~nan_g], c[~nan_c])


@pytest.mark.parametrize("gap", [0, 2])
def test_mixed_kinds_share_blocks(gap):
    C.case_mixed_small(ops, DEV, gap)


def test_tiles_and_many_small_entries():
    C.case_tiles(ops, DEV)
    C.case_many_small(ops, DEV)


def test_three_allocations_descending_table():
    C.case_three_allocations(ops, DEV)


def test_empty_and_all_zero_tables_launch_nothing(monkeypatch):
    def boom():
        raise AssertionError("a table without output reached the launch")

    monkeypatch.setattr(ops, "hip", boom)
    C.case_nothing_to_do(ops, DEV)


def test_refusals_come_before_the_launch():
    C.case_refusals(ops, DEV, pytest)


def test_explicit_stream():
    src = torch.full((100,), 0x40, dtype=torch.uint8, device=DEV)  # f32 0x40404040 = 3.00392...: bf16 0x4040 = 3.0
    dst = torch.zeros(40, dtype=torch.int16, device=DEV)
    s = torch.cuda.Stream(DEV)
    s.wait_stream(torch.cuda.current_stream(DEV))
    tab = np.array([(3, 8, 9, 4, dst.data_ptr() + 2 * 17, ops.CAST_KINDS[("F32", "BF16")])], dtype=ops.CAST_DTYPE)
    ops.slice_scatter_cast(src, tab, [dst], stream=s)
    s.synchronize()
    assert dst.cpu().tolist() == [0] * 17 + [0x4040] * 8 + [0] * 15
