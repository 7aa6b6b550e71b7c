"""ops.slice_scatter without a GPU: the NumPy path (host addresses) and the table validation against
the byte-by-byte model (scatter_model.py), every buffer compared whole, canaries included."""
from __future__ import annotations

import pytest

import scatter_model as S
import shard_model as M
from zest_amd import ops

DEV = "cpu"


def test_alignment_grid():
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


def test_empty_and_all_zero_tables_do_nothing(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("a table without output reached the copy")

    monkeypatch.setattr(ops, "_slice_scatter_cpu", boom)
    S.case_nothing_to_do(ops, DEV)


def test_refusals_leave_the_buffers_untouched():
    S.case_refusals(ops, DEV, pytest)
