"""GPU: the slice-scatter kernel (csrc/gpu/scatter.hip, ops.slice_scatter) against the byte-by-byte
model (scatter_model.py).  Destinations are carved out of canary-filled allocations at every
alignment, and every byte of every allocation is compared after the launch: outputs equal the model,
all other bytes still hold their position-dependent canary."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import scatter_model as S
import shard_model as M
from zest_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def test_alignment_grid():
    """dst & 15 x src & 15 x size in one launch of 1536 entries: the 256-ary search and the overflow
    of the LDS cache both run."""
    S.case_alignment_grid(ops, DEV)


@pytest.mark.parametrize("gap", [0, 1])
def test_shared_blocks(gap):
    S.case_shared_blocks(ops, DEV, gap)


@pytest.mark.parametrize("start", S.GRID_STARTS)
@pytest.mark.parametrize("stride", list(M.STRIDES))
def test_run_grid(stride, start):
    S.case_run_grid(ops, DEV, stride, start)


def test_tiles_and_many_small_entries():
    S.case_tiles(ops, DEV)
    S.case_many_small(ops, DEV)


def test_three_allocations_descending_table():
    S.case_three_allocations(ops, DEV)


def test_empty_and_all_zero_tables_launch_nothing(monkeypatch):
    def boom():
        raise AssertionError("a table without output reached the launch")

    monkeypatch.setattr(ops, "hip", boom)
    S.case_nothing_to_do(ops, DEV)


def test_refusals_come_before_the_launch():
    S.case_refusals(ops, DEV, pytest)


def test_explicit_stream():
    src = torch.full((100,), 7, dtype=torch.uint8, device=DEV)
    dst = torch.zeros(80, dtype=torch.uint8, device=DEV)
    s = torch.cuda.Stream(DEV)
    s.wait_stream(torch.cuda.current_stream(DEV))
    ops.slice_scatter(src, np.array([(3, 5, 9, 4, dst.data_ptr() + 17)], dtype=ops.SCATTER_DTYPE), [dst], stream=s)
    s.synchronize()
    assert dst.cpu().tolist() == [0] * 17 + [7] * 20 + [0] * 43
