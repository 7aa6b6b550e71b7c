"""ops.reuse_chunks without a GPU: the NumPy path against the model (reuse_model.py), every refusal
of the host validation (each names the offending record), and ResidentSet.lookup / merge."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import reuse_model as M
from zest_amd import ops
from zest_amd.delta import ResidentSet

LENS = [0, 1, 15, 16, 17, 63, 64, 65, 1023, 1024, 1025, 2048, 8191, 65536, 131071, 131072]


def _tables(rows):
    hashes = torch.full((rows, 32), 0x3C, dtype=torch.uint8)
    sizes = torch.full((rows,), -7, dtype=torch.int64)
    return hashes, sizes


def test_cpu_path_matches_the_model():
    rng = np.random.default_rng(12)
    srcs = [torch.from_numpy(rng.integers(0, 256, n, dtype=np.uint8)) for n in (300_000, 140_000, 9_000)]
    lens = np.asarray(LENS)
    pick = rng.integers(0, 3, len(lens))
    pick[lens > 9000] = rng.integers(0, 2, int((lens > 9000).sum()))
    starts = [int(rng.integers(0, srcs[b].numel() - n + 1)) for b, n in zip(pick, lens)]
    starts[-1] = srcs[pick[-1]].numel() - int(lens[-1])  # ends at the last byte of its buffer
    addrs = [srcs[b].data_ptr() + s for b, s in zip(pick, starts)]
    offs, total = M.layout(lens, rng.integers(0, 16, len(lens)), rng)
    index = rng.permutation(40)[:len(lens)]
    dst = torch.full((total,), M.SENTINEL, dtype=torch.uint8)
    hashes, sizes = _tables(40)
    chunks = [srcs[b].numpy()[s:s + n].tobytes() for b, s, n in zip(pick, starts, lens)]
    want = M.expect(chunks, offs, index, dst.numpy(), hashes.numpy(), sizes.numpy())
    ops.reuse_chunks(addrs, lens, dst, offs, hashes, index, sizes, buffers=srcs)
    assert np.array_equal(dst.numpy(), want[0])
    assert np.array_equal(hashes.numpy(), want[1])
    assert np.array_equal(sizes.numpy(), want[2])
    untouched = np.setdiff1d(np.arange(40), index)
    assert (hashes.numpy()[untouched] == 0x3C).all() and (sizes.numpy()[untouched] == -7).all()
    # sizes is optional
    h2, _ = _tables(40)
    ops.reuse_chunks(addrs, lens, dst, offs, h2, index, buffers=srcs)
    assert np.array_equal(h2.numpy(), want[1])


def _call(addrs, lens, offs, index, bufs, dst_n=4096, rows=4, ok=False):
    """One call on fresh tables; a refused call (ok=False) must leave dst and the tables as they were."""
    dst = torch.zeros(dst_n, dtype=torch.uint8)
    hashes, sizes = _tables(rows)
    before = (dst.clone(), hashes.clone(), sizes.clone())
    try:
        ops.reuse_chunks(addrs, lens, dst, offs, hashes, index, sizes, buffers=bufs)
    finally:
        if not ok:
            assert torch.equal(dst, before[0]) and torch.equal(hashes, before[1]) and torch.equal(sizes, before[2])


def test_every_refusal_names_the_record():
    a = torch.zeros(1000, dtype=torch.uint8)
    # two buffers that are neighbours in memory: views of one allocation
    both = torch.zeros(2000, dtype=torch.uint8)
    b0, b1 = both[:1000], both[1000:]
    pa = a.data_ptr()
    good = ([pa, pa + 100], [50, 60], [0, 64], [0, 1])
    _call(*good, [a], ok=True)  # the baseline is accepted
    with pytest.raises(ValueError, match=r"record 1: chunk .* outside every buffer"):
        _call([pa, pa + 990], [50, 60], [0, 64], [0, 1], [a])  # past the end of its buffer
    with pytest.raises(ValueError, match=r"record 0: chunk .* outside every buffer"):
        _call([pa - 1, pa + 100], [50, 60], [0, 64], [0, 1], [a])
    with pytest.raises(ValueError, match=r"record 1: chunk .* outside every buffer"):
        _call([pa, both.data_ptr() + 990], [50, 20], [0, 64], [0, 1], [a, b0, b1])  # straddles b0 | b1
    with pytest.raises(ValueError, match=r"record 0: chunk .* outside every buffer"):
        _call(*good, [])  # nothing vouches for the memory
    with pytest.raises(ValueError, match=r"record 1: output \[40, 100\) overlaps record 0's"):
        _call([pa, pa + 100], [50, 60], [0, 40], [0, 1], [a])
    with pytest.raises(ValueError, match=r"record 0: output \[10, 60\) overlaps record 1's"):
        _call([pa, pa + 100], [50, 60], [10, 0], [0, 1], [a])
    with pytest.raises(ValueError, match=r"record 1: output \[4040, 4100\) reaches past dst"):
        _call([pa, pa + 100], [50, 60], [0, 4040], [0, 1], [a])
    with pytest.raises(ValueError, match=r"record 1: index 0 is also record 0's"):
        _call([pa, pa + 100], [50, 60], [0, 64], [0, 0], [a])
    with pytest.raises(ValueError, match=r"record 1: index 4 is past the table \(4 rows\)"):
        _call([pa, pa + 100], [50, 60], [0, 64], [0, 4], [a])
    big = torch.zeros(131073, dtype=torch.uint8)
    with pytest.raises(ValueError, match=r"record 1: len 131073 is over the chunk maximum"):
        _call([pa, big.data_ptr()], [50, 131073], [0, 64], [0, 1], [a, big], dst_n=140000)
    _call([pa, big.data_ptr()], [50, 131072], [0, 64], [0, 1], [a, big], dst_n=140000, ok=True)
    # a zero-length record may sit anywhere (nothing is read or written), but still needs its own row
    _call([0, pa], [0, 60], [5, 0], [0, 1], [a], ok=True)
    with pytest.raises(ValueError, match="equally long"):
        _call([pa], [50, 60], [0, 64], [0, 1], [a])


def test_device_mismatch_is_refused():
    a = torch.zeros(100, dtype=torch.uint8)
    dst = torch.zeros(100, dtype=torch.uint8)
    hashes, sizes = _tables(2)
    meta = torch.zeros(100, dtype=torch.uint8, device="meta")
    with pytest.raises(ValueError, match=r"buffer 1 is on meta, dst on cpu"):
        ops.reuse_chunks([a.data_ptr()], [10], dst, [0], hashes, [0], sizes, buffers=[a, meta])
    with pytest.raises(ValueError, match=r"hashes is on meta, dst on cpu"):
        ops.reuse_chunks([a.data_ptr()], [10], dst, [0], hashes.to("meta"), [0], buffers=[a])
    with pytest.raises(ValueError, match=r"sizes is on meta, dst on cpu"):
        ops.reuse_chunks([a.data_ptr()], [10], dst, [0], hashes, [0], sizes.to("meta"), buffers=[a])


# ------------------------------------------------------------------------------------------------
# ResidentSet
# ------------------------------------------------------------------------------------------------
def _run(first, n, base):
    """A run of n chunks from chunk `first`: chunk c is 10 + c bytes at address base + 1000 c."""
    c = np.arange(first, first + n)
    return (first, (base + 1000 * c).astype(np.uint64), (10 + c).astype(np.uint32))


def _want(c0, c1, base):
    c = np.arange(c0, c1)
    return (base + 1000 * c).tolist(), (10 + c).tolist()


def _got(hit):
    return hit[0].tolist(), hit[1].tolist()


def test_lookup_subrange_adjacent_runs_holes_and_unknown():
    rs = ResidentSet({"x": [_run(20, 5, 0), _run(4, 6, 0), _run(10, 3, 0)], "y": [_run(0, 2, 7)]}, [], "cpu")
    assert len(rs) == 16
    assert _got(rs.lookup("x", 5, 8)) == _want(5, 8, 0)        # inside one run
    assert _got(rs.lookup("x", 4, 10)) == _want(4, 10, 0)      # a whole run
    assert _got(rs.lookup("x", 8, 12)) == _want(8, 12, 0)      # spans runs [4, 10) and [10, 13)
    assert _got(rs.lookup("x", 4, 13)) == _want(4, 13, 0)
    assert rs.lookup("x", 12, 21) is None                      # chunks 13..19 are not resident
    assert rs.lookup("x", 3, 6) is None and rs.lookup("x", 24, 26) is None
    assert rs.lookup("x", 13, 14) is None
    assert rs.lookup("z", 0, 1) is None                        # unknown xorb
    assert rs.lookup("x", 5, 5) is None                        # an empty range is no term
    one_hole = ResidentSet({"x": [_run(0, 4, 0), _run(5, 4, 0)]}, [], "cpu")
    assert one_hole.lookup("x", 2, 7) is None                  # chunk 4 is missing
    assert _got(one_hole.lookup("x", 5, 9)) == _want(5, 9, 0)


def test_merged_sets_resolve_from_both():
    ba, bb = torch.zeros(4, dtype=torch.uint8), torch.zeros(4, dtype=torch.uint8)
    a = ResidentSet({"x": [_run(0, 4, 0)], "y": [_run(0, 2, 0)]}, [ba], "cpu")
    b = ResidentSet({"x": [_run(3, 5, 50_000)], "z": [_run(7, 1, 50_000)]}, [bb, ba], "cpu")
    m = a | b
    assert a.lookup("x", 2, 6) is None and b.lookup("x", 2, 6) is None
    addrs, lens = _got(m.lookup("x", 2, 6))
    assert lens == _want(2, 6, 0)[1]
    assert addrs == _want(2, 4, 0)[0] + _want(4, 6, 50_000)[0]  # chunk 3 is in both: the left set's copy
    assert _got(m.lookup("y", 0, 2)) == _want(0, 2, 0) and _got(m.lookup("z", 7, 8)) == _want(7, 8, 50_000)
    assert len(m.plan["x"]) == 1 and m.plan["x"][0][0] == 0 and len(m.plan["x"][0][1]) == 8  # one maximal run
    assert len(m.buffers) == 2 and m.buffers[0] is ba and m.buffers[1] is bb
    assert len(a.plan["x"][0][1]) == 4  # the operands are unchanged
    with pytest.raises(ValueError, match="different devices"):
        a | ResidentSet({}, [], "meta")
