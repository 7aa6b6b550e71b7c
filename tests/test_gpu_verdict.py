"""GPU: the hash compare that ends every device pull (k_compare, zg_compare_hashes in
csrc/gpu/ingest.hip): engine.py runs merkle -> compare_hashes -> err, and whatever this kernel does
not report is accepted.  Two [n + 3, 32] tables and one error word; the rows past n always differ,
the word sits between canary bytes, and the verdict is read the way the engine reads it, through
ops.raise_on_error."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from scatter_model import canary, place_source
from zest_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ERR_AT = 24  # byte offset of the error word in its 64-byte canary buffer
SIZES = (1, 255, 256, 257, 1000)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    ops.hip()  # must load: no silent fallback


class Tables:
    """`want` and `got` hold the same n rows; the three rows behind them differ in every byte."""

    def __init__(self, n: int, seed: int = 1):
        self.n = n
        self.rows = np.random.default_rng(seed).integers(0, 256, (n + 3, 32), dtype=np.uint8)
        other = self.rows.copy()
        other[n:] ^= 0xFF
        self.other = other
        self.hold_w, self.want = place_source(self.rows.reshape(-1), DEV)
        self.hold_g, self.got = place_source(other.reshape(-1), DEV)
        self.err_buf = torch.from_numpy(canary(64)).to(DEV)
        self.err = self.err_buf[ERR_AT:ERR_AT + 8].view(torch.int64)
        assert self.got.data_ptr() % 16 == 0 and self.want.data_ptr() % 16 == 0 and self.err.data_ptr() % 8 == 0
        self.set_err(0)

    def set_err(self, v: int) -> None:
        self.err.fill_(v)

    def flip(self, row: int, bit: int) -> None:
        """Toggle one bit of `got` (twice: back to equal)."""
        self.got[32 * row + (bit >> 3)] ^= 1 << (bit & 7)
        self.other[row, bit >> 3] ^= 1 << (bit & 7)

    def compare(self, n=None) -> int:
        """Launch; check that nothing but the error word changed; return the word."""
        ops.hip().compare_hashes(self.got.data_ptr(), self.want.data_ptr(), self.n if n is None else n,
                                 self.err.data_ptr(), torch.cuda.current_stream().cuda_stream)
        word = int(self.err.item())
        around = self.err_buf.cpu().numpy()
        c = canary(64)
        assert np.array_equal(around[:ERR_AT], c[:ERR_AT]) and np.array_equal(around[ERR_AT + 8:], c[ERR_AT + 8:])
        assert np.array_equal(self.want.cpu().numpy(), self.rows.reshape(-1))  # the tables are only read
        assert np.array_equal(self.got.cpu().numpy(), self.other.reshape(-1))
        return word

    def verdict(self):
        """None, or (code, index) of the IngestError the engine would raise."""
        self.compare()
        try:
            ops.raise_on_error(self.err)
        except ops.IngestError as e:
            return e.code, e.index
        return None


@pytest.mark.parametrize("n", SIZES)
def test_equal_tables_pass_whatever_lies_behind_them(n):
    t = Tables(n, seed=n)
    assert t.compare() == 0
    ops.raise_on_error(t.err)


def test_one_flipped_bit_names_its_row():
    """n = 257 is two blocks, the second with one row.  One bit in rows 0 and 255, and each of the 256
    bits of row 256: every one of them is reported, with exactly that row."""
    t = Tables(257, seed=2)
    cases = [(0, 0), (0, 255), (255, 77), (255, 128)] + [(256, b) for b in range(256)]
    for row, bit in cases:
        t.flip(row, bit)
        t.set_err(0)
        assert t.compare() == (6 << 32) | row, (row, bit)
        assert t.verdict() == (6, row), (row, bit)
        t.flip(row, bit)
    t.set_err(0)
    assert t.verdict() is None  # all flips undone


def test_several_bad_rows_report_one_of_them():
    t = Tables(257, seed=3)
    for row, bit in ((3, 5), (200, 131), (256, 255)):
        t.flip(row, bit)
    code, index = t.verdict()
    assert code == 6 and index in (3, 200, 256)


def test_the_first_error_wins():
    t = Tables(257, seed=4)
    t.flip(100, 9)
    t.set_err((4 << 32) | 9)
    assert t.compare() == (4 << 32) | 9
    assert t.verdict() == (4, 9)


def test_no_rows_no_verdict():
    t = Tables(0, seed=5)  # three rows, all different
    assert t.compare() == 0
    t2 = Tables(5, seed=6)
    t2.flip(0, 0)
    assert t2.compare(n=0) == 0
