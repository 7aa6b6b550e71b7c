"""Synthesised LZ4 frames (tests/lz4_synth.py) against the host decoder and the CPU model of the
batched GPU decoder.  The expected bytes are the synthesiser's own byte-at-a-time copy; nothing is
skipped or filtered.  The path counters at the end keep each case family on the decoder path it is
named for: the GPU tests (tests/test_gpu_lz4_synth.py) decode the same families.
"""
from __future__ import annotations

import numpy as np
import pytest

import lz4_synth as S
from test_lz4_batched_model import model_decode
from zest_amd import _core as C

FAMILY_NAMES = sorted(S.FAMILIES)
MODEL_MAX = 24 * 1024  # the pure-Python model takes about a second per 3 x 24 KiB


def test_bg4_join_np_matches_host_join():
    rng = np.random.default_rng(5)
    for n in (1, 2, 3, 4, 5, 6, 7, 8, 1023, 20001, 20002, 20003, 131071, 131072):
        g = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        assert S.bg4_join_np(g) == C.bg4_join(g), n


def test_build_block_reference_is_byte_sequential():
    # worked by hand: "abc", then 7 bytes from 3 back (overlapping), then "Z" and 4 bytes from 1 back
    blk, dec = S.build_block([(b"abc", 3, 7), (b"Z", 1, 4), (b"!", 0, 0)])
    assert dec == b"abcabcabcaZZZZZ!"
    assert blk == bytes([0x33]) + b"abc" + bytes([3, 0, 0x10]) + b"Z" + bytes([1, 0, 0x10]) + b"!"
    # lengths >= 15 take the 255-chain: 15 -> one 0 byte, 270 -> 255, 0; match 274 -> 255, 0; 275 -> 255, 1
    assert S.encode_seq(bytes(15), 1, 4)[:2] == bytes([0xF0, 0])
    assert S.encode_seq(bytes(270), 1, 4)[:3] == bytes([0xF0, 255, 0])
    assert S.encode_seq(b"", 1, 274) == bytes([0x0F, 1, 0, 255, 0])
    assert S.encode_seq(b"", 1, 275) == bytes([0x0F, 1, 0, 255, 1])
    assert S.seq_size(270, 275) == len(S.encode_seq(bytes(270), 9, 275))
    # a dependent block reaches into the history it is given
    blk, dec = S.build_block([(b"", 4, 6), (b"", 0, 0)], hist=b"wxyz")
    assert dec == b"wxyzwx"


@pytest.mark.parametrize("fam", FAMILY_NAMES)
def test_host_decoder_matches_reference(fam):
    for c in S.family(fam):
        assert C.decompress_chunk(1, c.frame, len(c.data)) == c.data, c.name
        assert C.decompress_chunk(2, c.frame, len(c.data)) == S.bg4_join_np(c.data), c.name


@pytest.mark.parametrize("scheme", [1, 2])
@pytest.mark.parametrize("fam", FAMILY_NAMES)
def test_host_xorb_walk_of_synthesised_run(fam, scheme):
    cases = S.family(fam)
    body = S.xorb_body([(scheme, c.frame, len(c.data)) for c in cases])
    idx = C.index_chunks(body)
    assert len(idx) == len(cases)
    pos = upos = 0
    for e, c in zip(idx, cases):
        assert tuple(e) == (pos, len(c.frame), scheme, len(c.data), upos), c.name
        pos += 8 + len(c.frame)
        upos += len(c.data)
    want = b"".join(c.data if scheme == 1 else S.bg4_join_np(c.data) for c in cases)
    assert C.extract_chunk_range(body, 0, len(cases)) == want


def _modelled(fam):
    """The cases the model runs: the small ones, and the small twins the families add for their big ones."""
    return [c for c in S.family(fam) if len(c.data) <= MODEL_MAX or "twin" in c.name]


@pytest.mark.parametrize("fam", FAMILY_NAMES)
def test_model_matches_reference(fam):
    cases = _modelled(fam)
    assert cases, "every family has cases small enough for the model"
    for c in cases:
        for batch in (64, 59, 37):
            assert model_decode(c.frame, len(c.data), batch) == c.data, (c.name, batch)


def _stats(fam, pick=lambda c: True, batch=64):
    st = {}
    n = 0
    for c in _modelled(fam):
        if pick(c):
            assert model_decode(c.frame, len(c.data), batch, st) == c.data, c.name
            n += 1
    assert n
    return st


def test_families_reach_their_paths():
    """The model's counters per family (batches of 64 records, as the records decoder forms them; the
    one-wave parse flushes at 57 to 64)."""
    st = _stats("offsets", lambda c: c.name in ("off_small_twin", "off_255_257", "off_4031_4033"))
    assert st["chase"] >= 50 and st["near"] > 0, st
    st = _stats("length_codes")
    assert st["chase"] > 0 and st["near"] > 0 and st.get("long_batches", 0) > 0, st
    st = _stats("modulo")
    assert st["split_records"] >= 2 and st["long_batches"] >= 2, st
    st = _stats("ring")
    assert st["far"] > 0 and st["near"] > 0 and st["long_batches"] > 0 and st["ring_rebuilds"] > 0, st
    # a single match with bytes on both sides of the ring edge
    st = _stats("ring", lambda c: c.name == "ring_off3839_m300_t7")
    assert st["far"] > 0 and st["near"] > 0, st
    # the long-batch switch: span 3839 stays short, 3840 and 3841 are long
    assert "long_batches" not in _stats("ring", lambda c: c.name == "ring_span3839")
    for span in (3840, 3841):
        st = _stats("ring", lambda c: c.name == f"ring_span{span}")
        assert st["long_batches"] == 1 and st["ring_rebuilds"] == 1 and st["wide_runs"] == 1, st
    st = _stats("wide")
    assert st["long_batches"] >= 10 and st["wide_runs"] >= 10, st
    assert _stats("wide", lambda c: c.name == "wide_511")["wide_runs"] == 2  # its 3601- and 600-byte runs only
    assert _stats("wide", lambda c: c.name == "wide_512")["wide_runs"] == 3
    st = _stats("block_tail")
    assert st["near"] > 0 and "long_batches" not in st, st
    st = _stats("batch_fill")
    assert st["near"] > 0 and st["chase"] > 0, st
    st = _stats("frame_shapes")
    assert st["near"] > 0, st
    for seed in (1, 2, 3, 4):
        st = _stats(f"random{seed}", lambda c: int(c.name.split("_")[1]) < 12)
        assert st["chase"] > 0 and st["near"] > 0 and st["far"] > 0 and st["long_batches"] > 0, (seed, st)


def test_big_cases_split_records():
    """The cases too big for the model still state what they are for: their record splits, counted by
    the model's parser alone (no decode)."""
    from test_lz4_batched_model import parse_frame

    for c in S.family("batch_fill"):
        if c.name.startswith("fill_big_at"):
            st = {}
            recs = parse_frame(c.frame, st)
            idx = int(c.name[len("fill_big_at"):])
            assert st["split_records"] == 2 and len(recs) == idx + 3 + 5 + 1, (c.name, st, len(recs))
            assert recs[idx][1] == 0xFFFF and recs[idx + 1][2] == 0x7FFF
        if c.name == "fill_big_first":
            st = {}
            assert len(parse_frame(c.frame, st)) == 5 and st["split_records"] == 3
    n = 0
    for c in S.family("modulo"):
        st = {}
        parse_frame(c.frame, st)
        n += st["split_records"]
    assert n >= len(S.MOD_OFFSETS) // 2  # three of every five matches are longer than 0x7FFF
    offs = set()
    for c in S.family("modulo"):
        offs |= {r[3] for r in parse_frame(c.frame) if r[2]}
    assert offs >= set(S.MOD_OFFSETS)


def test_family_contents_are_what_the_names_say():
    lits = {0, 14, 15, 16, 269, 270, 271, 525}
    mls = {4, 18, 19, 20, 273, 274, 275, 529}
    from test_lz4_batched_model import parse_frame

    for name in ("len_near", "len_far"):
        c = next(c for c in S.family("length_codes") if c.name == name)
        seen = {(r[1], r[2]) for r in parse_frame(c.frame)}
        assert seen >= {(a, b) for a in lits for b in mls}
    offs = set()
    for c in S.family("offsets"):
        offs |= {r[3] for r in parse_frame(c.frame) if r[2]}
    assert offs >= set(range(1, 131)) | {255, 256, 257, 4031, 4032, 4033, 65535}
    assert {c.name for c in S.family("block_tail")} == {f"tail_d{d}_t{t}" for d in range(3, 41) for t in (0, 5)}
    fills = {len(parse_frame(c.frame)) - 1 for c in S.family("batch_fill") if c.name.startswith("fill_n")}
    assert fills == set(range(55, 67)) | set(range(120, 131)) | {512}
    for c in S.family("ring") + S.family("wide") + S.family("random1"):
        assert len(c.data) <= S.MAX_CHUNK
    flags = {c.frame[4] for c in S.family("frame_shapes")}
    assert {0x68, 0x61, 0x70, 0x64, 0x7D, 0x40, 0x50} <= flags, [hex(f) for f in sorted(flags)]


def test_host_rejects_wrong_header_checksum():
    c = S.family("frame_shapes")[0]
    blk, dec = S.build_block([(b"header checksum", 5, 20), (b"", 0, 0)])
    for kw in ({}, {"content_size": len(dec)}, {"dict_id": 9, "content_size": len(dec)}):
        assert C.decompress_chunk(1, S.frame([(blk, False)], **kw), len(dec)) == dec
        for x in (1, 0x80, 0xFF):
            with pytest.raises(Exception, match="header checksum mismatch"):
                C.decompress_chunk(1, S.frame([(blk, False)], hc_xor=x, **kw), len(dec))
    assert C.decompress_chunk(1, c.frame, len(c.data)) == c.data


def test_host_accepts_wrong_content_checksum():
    """Present behaviour: the host stops at the end mark (as both GPU parsers do); integrity rests
    on the per-chunk BLAKE3."""
    blk, dec = S.build_block([(b"content checksum", 7, 33), (b"!", 0, 0)])
    good = S.frame([(blk, False)], content=dec)
    bad = S.frame([(blk, False)], content_checksum=(C.xxh32(dec, 0) ^ 0x5A5A5A5A))
    assert good != bad and len(good) == len(bad)
    assert C.decompress_chunk(1, good, len(dec)) == dec
    assert C.decompress_chunk(1, bad, len(dec)) == dec


@pytest.mark.parametrize("case", S.malformed(), ids=lambda m: m[0])
def test_host_rejects_malformed(case):
    name, frm, ulen, _ = case
    with pytest.raises(Exception, match="CorruptLz4"):
        C.decompress_chunk(1, frm, ulen)


# ------------------------------------------------------------------------------------------------
# the one-wave parse's own batching (kernel_batches: batches of 57 to 64 records, cut where the fast
# loop and the flush threshold cut them)
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam", FAMILY_NAMES)
def test_model_with_kernel_batching_matches_reference(fam):
    from test_lz4_batched_model import kernel_batches, parse_frame

    for c in S.family(fam):
        b = kernel_batches(c.frame)
        assert sum(b) == len(parse_frame(c.frame)) and max(b) <= 64 and all(x > 56 for x in b[:-1]), (c.name, b)
    cases = _modelled(fam)
    for c in cases:
        assert model_decode(c.frame, len(c.data), kernel_batches(c.frame)) == c.data, c.name


def test_families_sit_on_the_parse_thresholds():
    from test_lz4_batched_model import kernel_batches

    by = {c.name: c for f in ("batch_fill", "ring") for c in S.family(f)}
    # the sequence with the most records: appended to a batch of 55 or 56 records (the last that
    # still take it), or first of the next batch when 57, 58 or 63 records are already held
    want = {55: [58, 6], 56: [59, 6], 57: [57, 9], 58: [58, 9], 63: [63, 9]}
    for idx, b in want.items():
        assert kernel_batches(by[f"fill_big_at{idx}"].frame) == b, idx
        assert kernel_batches(by[f"fill_gen_at{idx}"].frame)[0] == {55: 61, 56: 57}.get(idx, idx), idx
    assert kernel_batches(by["fill_big_first"].frame) == [5]
    # every batch size the parse can cut, and every hand-over distance of the block tail sweep
    sizes, st = set(), {}
    for c in S.family("block_tail") + S.family("batch_fill"):
        sizes |= set(kernel_batches(c.frame, st)[:-1])
    assert sizes >= set(range(57, 65)), sorted(sizes)
    st = {}
    for c in S.family("block_tail"):
        kernel_batches(c.frame, st)
    assert st["handover"] >= set(range(4, 42)), sorted(st["handover"])
    # the long-batch switch under the parse's own batching: one batch is the whole chunk ...
    for span, long_ in ((3839, 0), (3840, 1), (3841, 1)):
        c = by[f"ring_span{span}"]
        b = kernel_batches(c.frame)
        assert len(b) == 1 and b[0] < 57
        st = {}
        assert model_decode(c.frame, len(c.data), b, st) == c.data
        assert st.get("long_batches", 0) == long_, (span, st)
        # ... or follows a full one (itself long: its 9000 literals), with far sources
        c = by[f"ring_hist_span{span}"]
        b = kernel_batches(c.frame)
        assert b[0] == 64 and len(b) == 2, b
        for batches in (b, 64):
            st = {}
            assert model_decode(c.frame, len(c.data), batches, st) == c.data
            assert st["long_batches"] == 1 + long_ and (st.get("far", 0) > 0 or long_), (span, st)
