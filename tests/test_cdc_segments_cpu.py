"""Publishing loose tensors, the parts that need no GPU: the chunk classifier of a segmented file
(pure NumPy) on hand-made segment lists with the seam bound, the CPU paths of
ops.cdc_candidates_segments and ops.hash_chunks_at, TensorFile against pack_safetensors and the
plain-Python publish model, every refusal, and pack_safetensors' bytes against a literal header."""
from __future__ import annotations

import struct

import numpy as np
import pytest
import torch

import publish_model as M
import zest_amd
from zest_amd import _core, ops
from zest_amd.publish import TensorFile, classify_chunks, pack_safetensors, publish

MAX_CHUNK = 131072
DENSE = 0xFF << 56


def _rand(n: int, seed: int) -> torch.Tensor:
    return torch.from_numpy(np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8))


def _model(seg_lens, ends):
    """The classifier's rule byte by byte: per chunk, the segments that hold its bytes."""
    seg_of = np.repeat(np.arange(len(seg_lens)), seg_lens)
    first = np.concatenate([[0], np.cumsum(seg_lens)[:-1]])
    out, prev = [], 0
    for e in ends:
        segs = np.unique(seg_of[prev:e]).tolist()
        out.append((segs, prev - int(first[segs[0]])))
        prev = e
    return out


def _check(seg_lens, ends):
    """classify_chunks against the byte model; the arena holds every seam chunk's bytes once, in order;
    the seam bound holds."""
    cl = classify_chunks(seg_lens, ends)
    want = _model(seg_lens, ends)
    assert cl["seam"].tolist() == [len(s) > 1 for s, _ in want]
    assert cl["seg"].tolist() == [s[0] for s, _ in want]
    assert cl["off"].tolist() == [o for _, o in want]
    # copy the pieces as publish does and compare with the file's bytes
    segs = [np.random.default_rng(i).integers(0, 256, n, dtype=np.uint8) for i, n in enumerate(seg_lens)]
    data = np.concatenate(segs)
    arena = np.full(cl["seam_bytes"], 0xEE, dtype=np.uint8)
    written = np.zeros(cl["seam_bytes"], dtype=np.int64)
    for s, o, n, d in zip(cl["piece_seg"], cl["piece_off"], cl["piece_len"], cl["piece_dst"]):
        s, o, n, d = int(s), int(o), int(n), int(d)
        assert n > 0 and o + n <= seg_lens[s]
        arena[d:d + n] = segs[s][o:o + n]
        written[d:d + n] += 1
    assert (written == 1).all()
    starts = [0] + list(ends[:-1])
    for c, (a, b) in enumerate(zip(starts, ends)):
        if cl["seam"][c]:
            o = int(cl["arena_off"][c])
            assert arena[o:o + b - a].tobytes() == data[a:b].tobytes()
            assert sorted(set(cl["piece_seg"][cl["piece_chunk"] == c].tolist())) == want[c][0]
        else:
            s, o = int(cl["seg"][c]), int(cl["off"][c])
            assert segs[s][o:o + b - a].tobytes() == data[a:b].tobytes()
    live = sum(1 for n in seg_lens if n)
    assert cl["seam_chunks"] == int(cl["seam"].sum()) <= max(live - 1, 0)
    assert cl["seam_bytes"] == sum(b - a for c, (a, b) in enumerate(zip(starts, ends)) if cl["seam"][c])
    assert cl["seam_bytes"] <= MAX_CHUNK * max(live - 1, 0)
    return cl


def test_a_chunk_that_ends_on_a_boundary_is_no_seam():
    cl = _check([100, 50, 70], [100, 150, 220])
    assert not cl["seam"].any() and cl["seam_bytes"] == 0 and len(cl["piece_seg"]) == 0
    assert cl["seg"].tolist() == [0, 1, 2] and cl["off"].tolist() == [0, 0, 0]


def test_chunks_that_cross_one_two_and_forty_boundaries():
    cl = _check([100, 50, 70], [99, 101, 220])  # the second crosses one, the third one more
    assert cl["seam"].tolist() == [False, True, True]
    cl = _check([100, 50, 70], [90, 160, 220])  # crosses two: pieces of 10, 50, 10
    assert cl["seam"].tolist() == [False, True, False] and cl["piece_len"].tolist() == [10, 50, 10]
    assert cl["piece_dst"].tolist() == [0, 10, 60] and cl["seam_bytes"] == 70
    lens = [5000] + [100] * 40 + [5000]
    cl = _check(lens, [4990, 9010, 14000])  # 10 + forty whole segments + 10: forty-one boundaries
    assert cl["seam"].tolist() == [False, True, False] and len(cl["piece_seg"]) == 42
    cl = _check(lens, [4990, 8910, 14000])  # ends ten bytes into the fortieth small one: forty boundaries
    assert cl["seam"].tolist() == [False, True, True] and int((cl["piece_chunk"] == 1).sum()) == 41
    assert cl["piece_len"].tolist() == [10] + [100] * 39 + [10] + [90, 5000] and cl["seam_bytes"] == 3920 + 5090
    cl = _check(lens, [5000, 9000, 14000])  # exactly the forty segments: thirty-nine inner boundaries
    assert cl["seam"].tolist() == [False, True, False] and len(cl["piece_seg"]) == 40


def test_empty_segments_hold_nothing():
    cl = _check([0, 100, 0, 0, 50, 0], [60, 100, 150])
    assert cl["seam"].tolist() == [False, False, False] and cl["seg"].tolist() == [1, 1, 4]
    cl = _check([0, 100, 0, 0, 50, 0], [60, 120, 150])
    assert cl["seam"].tolist() == [False, True, False] and cl["piece_seg"].tolist() == [1, 4]
    assert cl["piece_len"].tolist() == [40, 20]


def test_a_single_segment_has_no_seams():
    cl = _check([300_000], [100_000, 231_072, 300_000])
    assert not cl["seam"].any() and cl["off"].tolist() == [0, 100_000, 231_072]
    with pytest.raises(ValueError, match="file size 300000"):
        classify_chunks([300_000], [100_000, 200_000])


def test_real_boundaries_over_many_small_segments():
    rng = np.random.default_rng(5)
    seg_lens = [int(v) for v in rng.integers(0, 40_000, 60)]
    data = rng.integers(0, 256, sum(seg_lens), dtype=np.uint8).tobytes()
    _check(seg_lens, [int(e) for e in _core.chunk_ends(data)])


def test_cpu_candidates_of_segments_equal_those_of_the_concatenation():
    parts = [_rand(n, 10 + i) for i, n in enumerate((5000, 1, 0, 63, 64, 65, 3000))]
    want = ops.cdc_candidates(torch.cat(parts), DENSE)
    assert len(want) > 20
    got = ops.cdc_candidates_segments(parts, DENSE)
    assert got.dtype == np.uint64 and got.tolist() == want.tolist()
    typed = [parts[0], torch.arange(500, dtype=torch.float32).reshape(20, 25), torch.zeros(0, 3, dtype=torch.int64),
             torch.arange(77, dtype=torch.int16)]
    assert ops.cdc_candidates_segments(typed, DENSE).tolist() == \
        ops.cdc_candidates(torch.cat([ops._flat_u8(t) for t in typed]), DENSE).tolist()
    live = [p for p in parts if p.numel()]
    by_addr = ops.cdc_candidates_segments(([p.data_ptr() for p in live], [p.numel() for p in live]), DENSE,
                                          buffers=live)
    assert by_addr.tolist() == want.tolist()
    assert ops.cdc_candidates_segments([]).tolist() == []
    with pytest.raises(ValueError, match="segment 0.*outside every buffer"):
        ops.cdc_candidates_segments(([live[0].data_ptr()], [live[0].numel() + 1]), buffers=live[:1])
    with pytest.raises(ValueError, match="segment 1 is empty"):
        ops.cdc_candidates_segments(([live[0].data_ptr()] * 2, [4, 0]), buffers=live[:1])
    with pytest.raises(ValueError, match="segment 0 must be a contiguous tensor"):
        ops.cdc_candidates_segments([torch.zeros(4, 4).t()])


def test_cpu_hash_chunks_at():
    buf = _rand(300_000, 3)
    offs, lens = [0, 7, 100_000, 299_999], [0, 131072, 65, 1]
    hashes = torch.full((6, 32), 0xAB, dtype=torch.uint8)
    sizes = torch.full((6,), -1, dtype=torch.int64)
    ops.hash_chunks_at([buf.data_ptr() + o for o in offs], lens, hashes, [4, 0, 5, 2], sizes=sizes, buffers=[buf])
    data = buf.numpy().tobytes()
    for o, n, r in zip(offs, lens, [4, 0, 5, 2]):
        assert bytes(hashes[r].numpy()) == _core.chunk_hash(data[o:o + n]) and int(sizes[r]) == n
    assert (hashes[[1, 3]] == 0xAB).all() and sizes[[1, 3]].tolist() == [-1, -1]
    a, b = buf[:1000], buf[1000:2000]  # two buffers that touch do not add up
    with pytest.raises(ValueError, match="record 0.*outside every buffer"):
        ops.hash_chunks_at([buf.data_ptr() + 990], [20], hashes, [0], buffers=[a, b])
    ops.hash_chunks_at([buf.data_ptr() + 990], [20], hashes, [0], buffers=[a, b, buf[500:1500]])  # nested: inside one
    with pytest.raises(ValueError, match="record 0.*outside every buffer"):
        ops.hash_chunks_at([buf.data_ptr() + 299_990], [20], hashes, [0], buffers=[buf])
    with pytest.raises(ValueError, match="record 1: index 3 is also record 0's"):
        ops.hash_chunks_at([buf.data_ptr()] * 2, [4, 4], hashes, [3, 3], buffers=[buf])
    with pytest.raises(ValueError, match=r"record 0: index 6 is past the table \(6 rows\)"):
        ops.hash_chunks_at([buf.data_ptr()], [4], hashes, [6], buffers=[buf])
    with pytest.raises(ValueError, match="record 0: len 131073 is over the chunk maximum"):
        ops.hash_chunks_at([buf.data_ptr()], [131073], hashes, [0], buffers=[buf])
    with pytest.raises(ValueError, match="^hash_chunks_at: lens must not be negative"):
        ops.hash_chunks_at([buf.data_ptr()], [-4], hashes, [0], buffers=[buf])
    with pytest.raises(ValueError, match="^cdc_candidates_segments: addrs must be integers"):
        ops.cdc_candidates_segments(([1.5], [4]), buffers=[buf])


def _tensors(seed: int = 1) -> dict:
    g = torch.Generator().manual_seed(seed)
    big = torch.randn(700_000, generator=g)
    return {"w.bf16": torch.randn(300, 500, generator=g).to(torch.bfloat16),
            "empty": torch.zeros(0, 4),
            "view": big[3:400_003],  # a contiguous view into a larger storage
            "b0": torch.randint(0, 256, (1,), generator=g, dtype=torch.uint8),
            "b1": torch.randint(0, 256, (33,), generator=g, dtype=torch.uint8),
            "b2": torch.randint(0, 256, (66,), generator=g, dtype=torch.uint8),
            "tied": big[3:400_003],
            "tail.f16": torch.randn(1234, generator=g).to(torch.float16)}


def test_tensor_file_on_the_cpu_publishes_the_packed_file():
    ts, md = _tensors(), {"step": 7}
    tf = TensorFile(ts, md)
    packed = pack_safetensors(ts, md)
    assert tf.nbytes == tf.numel() == packed.numel() and torch.equal(tf.pack(), packed)
    segs = tf.segments()
    assert len(segs) == 1 + sum(1 for t in ts.values() if t.numel()) and torch.equal(torch.cat(segs), packed)
    assert segs[1].data_ptr() == ts["w.bf16"].data_ptr() and segs[2].data_ptr() == ts["view"].data_ptr()
    assert zest_amd.TensorFile is TensorFile
    other = _rand(200_000, 9)
    stats = {}
    pub = publish({"m/a.safetensors": tf, "b.bin": other}, stats=stats, max_xorb_bytes=1 << 20)
    ref = publish({"m/a.safetensors": packed, "b.bin": other}, max_xorb_bytes=1 << 20)
    assert pub.manifest == ref.manifest
    assert pub.manifest == M.expected({"m/a.safetensors": packed.numpy().tobytes(), "b.bin": other.numpy().tobytes()},
                                      (), 1 << 20)[1]
    assert pub.manifest["files"][1]["size"] == packed.numel() > 2_000_000
    assert stats.keys() == ref.stats.keys() and stats["seconds"].keys() == ref.stats["seconds"].keys()
    with pytest.raises(ValueError, match="seed= serves from GPU memory"):
        publish({"a": tf}, seed=True)


def test_refusals():
    ok = torch.zeros(4, 4)
    with pytest.raises(ValueError, match=r"TensorFile: t is not contiguous.*\.contiguous\(\)"):
        TensorFile({"t": ok.t()})
    with pytest.raises(ValueError, match=r"TensorFile: tensors on more than one device \(cpu, meta\).*move the tensors"):
        TensorFile({"a": ok, "b": torch.zeros(4, device="meta")})
    with pytest.raises(ValueError, match=r"TensorFile: c: dtype torch.complex64 has no safetensors name"):
        TensorFile({"c": torch.zeros(2, dtype=torch.complex64)})
    with pytest.raises(ValueError, match=r"TensorFile: no tensors.*non-empty"):
        TensorFile({})
    with pytest.raises(ValueError, match=r"publish: files on more than one device \(cpu, meta\).*move the files"):
        publish({"a": TensorFile({"t": torch.zeros(4, device="meta")}), "b": _rand(100, 1)})
    with pytest.raises(ValueError, match=r"a must be a contiguous 1-D uint8 tensor.*TensorFile"):
        publish({"a": ok})


def test_pack_safetensors_bytes_are_what_they_were():
    ts = {"a": torch.arange(6, dtype=torch.int32).reshape(2, 3), "z": torch.zeros(0, dtype=torch.float16),
          "b": torch.tensor([1.5, -2.0], dtype=torch.bfloat16)}
    header = (b'{"__metadata__":{"step":"3"},"a":{"dtype":"I32","shape":[2,3],"data_offsets":[0,24]},'
              b'"z":{"dtype":"F16","shape":[0],"data_offsets":[24,24]},'
              b'"b":{"dtype":"BF16","shape":[2],"data_offsets":[24,28]}}')
    header += b" " * (-len(header) % 8)
    want = struct.pack("<Q", len(header)) + header + struct.pack("<6i", *range(6)) + bytes.fromhex("c03f00c0")
    assert pack_safetensors(ts, {"step": 3}).numpy().tobytes() == want
    assert TensorFile(ts, {"step": 3}).header == want[:8 + len(header)]
    assert torch.cat(TensorFile(ts, {"step": 3}).segments()).numpy().tobytes() == want
