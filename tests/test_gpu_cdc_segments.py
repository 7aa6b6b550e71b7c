"""GPU: ops.cdc_candidates_segments (kernel K14, zg_cdc_candidates_segs in csrc/gpu/synth.hip) against
the CPU scalar scan of the concatenated bytes, with K5 on the packed buffer as a second witness.  A
dense mask (one candidate per about 256 bytes) puts candidates into every warm-up region; the Xet
mask runs over 1 MiB.  Segments are separate allocations of exactly their size unless a test says
otherwise, so a neighbour's bytes are never the file's next bytes by accident.  The tests compare
candidates; they do not prove the absence of an over-read (see the exact-storage test)."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from zest_amd import ops

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DENSE = 0xFF << 56


def _bytes(n: int, seed: int) -> np.ndarray:
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)


def _scalar(data: np.ndarray, mask: int) -> list:
    """The reference: the host's byte-by-byte scan."""
    return ops.cdc_candidates(torch.from_numpy(data), mask).tolist()


def _place(data: np.ndarray, mis: int) -> torch.Tensor:
    """`data` on the device in an allocation of its own that ends with its last byte, starting
    `mis` bytes after a 16-byte boundary."""
    if len(data) == 0:
        return torch.empty(0, dtype=torch.uint8, device=DEV)
    t = torch.empty(len(data) + mis, dtype=torch.uint8, device=DEV)[mis:]
    assert t.data_ptr() % 16 == mis % 16
    t.copy_(torch.from_numpy(data))
    return t


def _split(data: np.ndarray, lens, mis=None) -> list:
    assert sum(lens) == len(data)
    cuts = np.concatenate([[0], np.cumsum(lens)])
    return [_place(data[a:b], (5 * i + 3) % 16 if mis is None else mis[i])
            for i, (a, b) in enumerate(zip(cuts, cuts[1:]))]


def _k5(data: np.ndarray, mask: int) -> list:
    return ops.cdc_candidates(torch.from_numpy(data).to(DEV), mask).tolist()


def test_one_segment_equals_k5():
    data = _bytes(10_000, 1)
    want = _scalar(data, DENSE)
    assert len(want) > 20
    assert ops.cdc_candidates_segments([_place(data, 0)], DENSE).tolist() == want == _k5(data, DENSE)
    assert ops.cdc_candidates_segments([_place(data, 11)], DENSE).tolist() == want


@pytest.fixture(scope="module")
def eight_k():
    data = _bytes(8192, 2)
    want = _scalar(data, DENSE)
    assert len(want) > 20 and _k5(data, DENSE) == want
    return data, want


def test_two_segments_split_at_every_edge(eight_k):
    """8 KiB in two segments, split at every offset around the 64-byte warm-up, the 128-byte step
    and the 2 KiB window; both segments at misalignments that change with the split."""
    data, want = eight_k
    for k in list(range(1, 131)) + [2047, 2048, 2049, 4095, 4096, 4097]:
        segs = _split(data, [k, 8192 - k], mis=[k % 16, (3 * k + 5) % 16])
        got = ops.cdc_candidates_segments(segs, DENSE).tolist()
        assert got == want, f"split at {k}"


TINY = [1, 2, 3, 15, 16, 17, 63, 64, 65]


@pytest.mark.parametrize("lens", [[3000] + TINY + [3000], TINY + [2500], [2500] + TINY, [3000] + [100] * 40 + [3000],
                                  [1] * 70 + [2100], [7, 0, 0, 50, 0, 9, 4000, 0]],
                         ids=["tiny-middle", "tiny-first", "tiny-last", "forty-of-100", "seventy-of-1", "empties"])
def test_runs_of_tiny_segments(lens):
    """A 64-byte gear window that spans three and more segments, at the start, in the middle and at
    the end of the file; zero-element tensors are skipped."""
    data = _bytes(sum(lens), 3 + len(lens))
    want = _scalar(data, DENSE)
    assert len(want) > 5
    assert ops.cdc_candidates_segments(_split(data, lens), DENSE).tolist() == want
    addrs_of = [t for t in _split(data, lens) if t.numel()]
    by_addr = ops.cdc_candidates_segments(([t.data_ptr() for t in addrs_of], [t.numel() for t in addrs_of]), DENSE,
                                          buffers=addrs_of)
    assert by_addr.tolist() == want


def test_every_base_misalignment_first_and_middle():
    """Segments that are views at byte offsets into a larger tensor: each misalignment 0..15 for the
    first segment and for a middle one, bytes of other content on both sides of every view."""
    lens = [2500, 4300, 2100]
    data = _bytes(sum(lens), 4)
    want = _scalar(data, DENSE)
    big = torch.from_numpy(_bytes(40_000, 5)).to(DEV)
    assert big.data_ptr() % 16 == 0
    for mis in range(16):
        for which in (0, 1):
            at, segs = [64, 10_000, 20_000], []
            at[which] += mis
            at[2] += (mis + 7) % 16
            cut = 0
            for a, n in zip(at, lens):
                big[a:a + n].copy_(torch.from_numpy(data[cut:cut + n]))
                segs.append(big[a:a + n])
                cut += n
            assert segs[which].data_ptr() % 16 == mis
            assert ops.cdc_candidates_segments(segs, DENSE).tolist() == want, f"misalignment {mis} of segment {which}"


@pytest.mark.parametrize("k", [1, 4095, 4096, 8193])
def test_a_segment_that_is_a_whole_exact_storage(k):
    """torch.empty(k, dtype=uint8): the segment is the whole storage, nothing of it behind.  This
    checks the candidates at such a segment's edges.  It cannot detect an over-read: torch's caching
    allocator rounds a storage up to 512 bytes inside a larger mapped block, and a byte loaded past
    the segment is masked out of the hash.  That no load leaves the aligned 16-byte blocks holding a
    byte of a segment rests on the kernel's guard (a block at 16 m is loaded only when 16 m lies
    before the segment's end), which is read, not tested."""
    data = _bytes(1000 + k + 1000, 6 + k)
    want = _scalar(data, DENSE)
    mid = torch.empty(k, dtype=torch.uint8, device=DEV)
    assert mid.untyped_storage().nbytes() == k
    mid.copy_(torch.from_numpy(data[1000:1000 + k]))
    segs = [_place(data[:1000], 9), mid, _place(data[1000 + k:], 2)]
    assert ops.cdc_candidates_segments(segs, DENSE).tolist() == want
    alone = _scalar(data[1000:1000 + k], DENSE)
    assert ops.cdc_candidates_segments([mid], DENSE).tolist() == alone


def test_the_first_64_bytes_have_no_phantom_history():
    """Before the file there is nothing, which is not 64 zero bytes (the gear entry of byte 0 is not
    zero).  With the top bit as mask every second position is a candidate, so a scan that started
    from any history but none would differ within the first bytes."""
    top = 1 << 63
    data = _bytes(64, 8)
    want = _scalar(data, top)
    assert 16 < len(want) < 48
    zeros = _scalar(np.concatenate([np.zeros(64, np.uint8), data]), top)
    assert [e - 64 for e in zeros if e > 64] != want  # the test can tell the difference
    assert ops.cdc_candidates_segments([_place(data, 0)], top).tolist() == want
    assert ops.cdc_candidates_segments(_split(data, [5, 20, 39]), top).tolist() == want
    more = _bytes(5000, 9)
    assert ops.cdc_candidates_segments(_split(more, [30, 70, 4900]), top).tolist() == _scalar(more, top)


def test_a_mask_with_low_bits_takes_the_full_compare():
    lens = [2100, 60, 4000]
    data = _bytes(sum(lens), 10)
    mask = (0x3F << 58) | 0x1
    want = _scalar(data, mask)
    assert len(want) > 20
    assert ops.cdc_candidates_segments(_split(data, lens), mask).tolist() == want == _k5(data, mask)


def test_a_capacity_too_small_is_retried(eight_k):
    data, want = eight_k
    assert ops.cdc_candidates_segments(_split(data, [100, 5000, 3092]), DENSE, capacity=4).tolist() == want


def test_the_xet_mask_over_a_mebibyte():
    """About 1 MiB in tensor-like segments (several blocks of windows, segments of many windows)."""
    lens = [136, 300_000, 100, 100, 100, 262_144, 1, 400_001, 86_017]
    data = _bytes(sum(lens), 11)
    data[500_000:500_500] = 0  # a run of equal bytes, as padded weights have
    want = _scalar(data, ops.XET_MASK)
    assert len(want) >= 8
    got = ops.cdc_candidates_segments(_split(data, lens))
    assert got.dtype == np.uint64 and got.tolist() == want == _k5(data, ops.XET_MASK)
    ends = ops.select_chunks(got, len(data))
    assert ends.tolist() == ops.select_chunks(np.asarray(want, dtype=np.uint64), len(data)).tolist()
