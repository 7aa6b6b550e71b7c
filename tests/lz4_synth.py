"""LZ4 frame synthesiser for the decoder tests: frames are written sequence by sequence from a list
the test chooses, so the cases do not depend on what the project's own encoders happen to emit.

The expected bytes come from `build_block`'s own byte-at-a-time copy (out.append(out[-off])) --
independent of the host decoder (csrc/core/lz4.cpp) and of the HIP decoders (csrc/gpu/lz4seq.hip).
A case is (name, frame, decoded): the same frame serves scheme 1 (the chunk is `decoded`) and
scheme 2 (the chunk is bg4_join_np(decoded): the frame's output is the grouped stream).

Case families (each a function of fixed seeds, returning named chunks of <= 128 KiB) aim at one
decoder path each; tests/test_lz4_synth_cpu.py asserts, through the CPU model's counters, that they
reach it.  Numbers such as 56, 64, 3840 and 4096 are the kernel's kFlushAbove, wave size, long-batch
threshold (span + 256 >= kRing) and kRing.
"""
from __future__ import annotations

import functools
import struct
from typing import NamedTuple

import numpy as np

from zest_amd import _core as C

MAGIC = 0x184D2204
MAX_CHUNK = 128 * 1024


class Case(NamedTuple):
    name: str
    frame: bytes
    data: bytes  # what the LZ4 frame decodes to (scheme 2: the grouped stream)


# ------------------------------------------------------------------------------------------------
# blocks and frames
# ------------------------------------------------------------------------------------------------
def _len_bytes(extra: int) -> bytes:
    """The 255-chain of a length whose nibble is 15 (`extra` = length - 15)."""
    out = bytearray()
    while extra >= 255:
        out.append(255)
        extra -= 255
    out.append(extra)
    return bytes(out)


def encode_seq(lit: bytes, off: int, ml: int, last: bool = False) -> bytes:
    """One sequence's bytes, unchecked (malformed cases pass offsets / lengths no decoder accepts)."""
    n = len(lit)
    tok = (min(n, 15) << 4) | (0 if last else min(ml - 4, 15))
    out = bytearray([tok])
    if n >= 15:
        out += _len_bytes(n - 15)
    out += lit
    if not last:
        out += struct.pack("<H", off)
        if ml - 4 >= 15:
            out += _len_bytes(ml - 4 - 15)
    return bytes(out)


def seq_size(nlit: int, ml: int) -> int:
    """Encoded size of a match-bearing sequence."""
    return 1 + (1 + (nlit - 15) // 255 if nlit >= 15 else 0) + nlit + 2 + (1 + (ml - 19) // 255 if ml >= 19 else 0)


def build_block(seqs, hist: bytes = b""):
    """[(literal_bytes, offset, match_len), ...] (the last one literal-only: offset = match_len = 0)
    -> (block_bytes, decoded_bytes).  `hist`: output of the frame's earlier blocks that matches may
    reach into (dependent blocks)."""
    assert seqs and seqs[-1][1] == 0 and seqs[-1][2] == 0, "the last sequence carries literals only"
    out = bytearray(hist)
    blk = bytearray()
    for i, (lit, off, ml) in enumerate(seqs):
        last = i == len(seqs) - 1
        out += lit
        if not last:
            assert ml >= 4 and 1 <= off <= 65535 and off <= len(out), (i, off, ml, len(out))
        blk += encode_seq(lit, off, ml, last)
        if not last:
            for _ in range(ml):
                out.append(out[-off])
    return bytes(blk), bytes(out[len(hist):])


def frame(blocks, *, content_size: int | None = None, dict_id: int | None = None, block_checksum: bool = False,
          content: bytes | None = None, content_checksum: int | None = None, independent: bool = True,
          max_block: int = 0, version: int = 1, hc_xor: int = 0, end_mark: bool = True) -> bytes:
    """LZ4 frame around `blocks` = [(block_bytes, stored), ...].  content: the decoded bytes, given
    when a content checksum is wanted (content_checksum overrides its value); max_block: the largest
    decoded block (BD 64 KiB class, or 256 KiB above that); hc_xor: corrupts the header checksum."""
    want_cc = content is not None or content_checksum is not None
    flg = (version << 6) | (0x20 if independent else 0) | (0x10 if block_checksum else 0) | \
        (0x08 if content_size is not None else 0) | (0x04 if want_cc else 0) | (0x01 if dict_id is not None else 0)
    big = max([max_block] + [len(b) for b, _ in blocks]) > 65536
    desc = bytes([flg, 0x50 if big else 0x40])
    if content_size is not None:
        desc += struct.pack("<Q", content_size)
    if dict_id is not None:
        desc += struct.pack("<I", dict_id)
    out = bytearray(struct.pack("<I", MAGIC)) + desc
    out.append((((C.xxh32(desc, 0) >> 8) & 0xFF) ^ hc_xor) & 0xFF)
    for b, stored in blocks:
        out += struct.pack("<I", len(b) | (0x80000000 if stored else 0))
        out += b
        if block_checksum:
            out += struct.pack("<I", C.xxh32(b, 0))
    if end_mark:
        out += struct.pack("<I", 0)
    if want_cc:
        out += struct.pack("<I", C.xxh32(content, 0) if content_checksum is None else content_checksum)
    return bytes(out)


def one_block(name: str, seqs) -> Case:
    blk, dec = build_block(seqs)
    assert 0 < len(dec) <= MAX_CHUNK, (name, len(dec))
    return Case(name, frame([(blk, False)], max_block=len(dec)), dec)


def bg4_join_np(grouped: bytes) -> bytes:
    """Inverse of BG4: group k holds bytes k, k + 4, ... ((n + 3 - k) // 4 of them)."""
    g = np.frombuffer(grouped, dtype=np.uint8)
    n = g.size
    out = np.empty(n, dtype=np.uint8)
    pos = 0
    for k in range(4):
        m = (n + 3 - k) // 4
        out[k::4] = g[pos:pos + m]
        pos += m
    assert pos == n
    return out.tobytes()


def xorb_body(chunks) -> bytes:
    """[(scheme, payload, ulen), ...] -> a run of chunks, each behind its 8-byte header (version 0,
    clen le24, scheme, ulen le24)."""
    out = bytearray()
    for scheme, payload, ulen in chunks:
        assert len(payload) < 1 << 24 and ulen < 1 << 24
        out += bytes([0]) + len(payload).to_bytes(3, "little") + bytes([scheme]) + ulen.to_bytes(3, "little")
        out += payload
    return bytes(out)


# ------------------------------------------------------------------------------------------------
# case families
# ------------------------------------------------------------------------------------------------
def _rb(rng, n: int) -> bytes:
    return rng.integers(0, 256, int(n), dtype=np.uint8).tobytes()


def _shorts(rng, n: int, produced: int, max_off: int = 40, lit_hi: int = 14, ml_hi: int = 18):
    """n sequences the parse's fast loop takes (literals < 15, match < 19); `produced`: bytes before."""
    seqs = []
    for _ in range(n):
        nl = int(rng.integers(0, lit_hi + 1))
        if produced + nl == 0:
            nl = 4
        ml = int(rng.integers(4, ml_hi + 1))
        off = int(rng.integers(1, min(max_off, produced + nl) + 1))
        seqs.append((_rb(rng, nl), off, ml))
        produced += nl + ml
    return seqs, produced


def _full_batch(rng, lit0: int):
    """Exactly 64 records in every parser: one sequence with lit0 (15 .. 16383) literals, then 63
    fast-loop sequences.  Gives a chunk lit0 + ~1000 bytes of history and leaves the next batch to
    start empty."""
    assert 15 <= lit0 <= 0x3FFF
    head = [(_rb(rng, lit0), int(rng.integers(1, lit0)), 8)]
    rest, produced = _shorts(rng, 63, lit0 + 8)
    return head + rest, produced


def family_offsets():
    rng = np.random.default_rng(101)
    mls = (4, 63, 64, 65, 127, 129, 200)
    cases = []

    def chunk(name, lead, offs, mls_):
        """`lead` literals (>= every offset), then each offset with each match length, 0-3 literals
        apart: short matches share a 64-byte pass with their neighbours, long ones overlap their
        own source."""
        out = []
        for off in offs:
            for ml in mls_:
                out.append((_rb(rng, lead if not out else len(out) % 4), off, ml))
        out.append((_rb(rng, 5), 0, 0))
        return one_block(name, out)

    cases.append(chunk("off_1_130_a", 130, range(1, 131), mls[:4]))
    cases.append(chunk("off_1_130_b", 130, range(1, 131), mls[4:]))
    cases.append(chunk("off_small_twin", 40, range(1, 41), (4, 65, 129)))
    cases.append(chunk("off_255_257", 257, (255, 256, 257), mls))
    cases.append(chunk("off_4031_4033", 4033, (4031, 4032, 4033), mls))
    cases.append(chunk("off_65535", 65535, (65535,), mls))
    return cases


def family_length_codes():
    rng = np.random.default_rng(102)
    lits = (0, 14, 15, 16, 269, 270, 271, 525)
    mls = (4, 18, 19, 20, 273, 274, 275, 529)
    cases = []
    for name, near in (("len_near", True), ("len_far", False)):
        seqs = [(_rb(rng, 9), 3, 4)]
        produced = 13
        for nl in lits:
            for ml in mls:
                off = int(rng.integers(1, 9)) if near else int(rng.integers(max(1, (produced + nl) // 2), produced + nl + 1))
                off = min(off, produced + nl)
                seqs.append((_rb(rng, nl), off, ml))
                produced += nl + ml
        seqs.append((b"", 0, 0))
        cases.append(one_block(name, seqs))
    # each literal length with each match length as a chunk's only sequence pair (small twins)
    seqs = [(_rb(rng, 270), 270, 274), (_rb(rng, 15), 1, 275), (_rb(rng, 14), 2, 19), (_rb(rng, 16), 600, 18),
            (_rb(rng, 269), 5, 273), (b"", 7, 529), (_rb(rng, 525), 1000, 20), (_rb(rng, 3), 0, 0)]
    cases.append(one_block("len_twin", seqs))
    return cases


MOD_OFFSETS = sorted({2, 3, 5, 7, 11, 13, 31, 61, 127, 251, 509, 641, 1021, 4093, 8191, 16381, 21845, 32749, 32767,
                      32769, 65535} | {(1 << k) + d for k in range(2, 16) for d in (-1, 1)})


def family_modulo():
    rng = np.random.default_rng(103)
    mls = (32766, 32767, 32768, 32771, 40000)
    cases = []
    seqs, produced, k = [], 0, 0
    for i, off in enumerate(MOD_OFFSETS):
        ml = mls[i % len(mls)]
        need = max(off - produced, 1)
        if produced + need + ml + 1 > MAX_CHUNK:
            seqs.append((_rb(rng, 1), 0, 0))
            cases.append(one_block(f"mod_{k}", seqs))
            k += 1
            seqs, produced = [], 0
            need = off
        ml = min(ml, MAX_CHUNK - 1 - produced - need)
        assert ml >= 0x7FFE or off == 65535, (off, ml)  # k reaches 0x7FFE (the largest umod16 sees) or splits
        seqs.append((_rb(rng, need), off, ml))
        produced += need + ml
    seqs.append((_rb(rng, 1), 0, 0))
    cases.append(one_block(f"mod_{k}", seqs))
    # small twin: split matches at awkward offsets in one 33 KiB chunk
    cases.append(one_block("mod_twin", [(_rb(rng, 7), 7, 0x7FFF + 3), (b"", 0, 0)]))
    cases.append(one_block("mod_twin_641", [(_rb(rng, 641), 641, 0x8000), (_rb(rng, 2), 3, 100), (b"", 0, 0)]))
    return cases


def family_ring():
    rng = np.random.default_rng(104)
    cases = []
    # (a) short batch behind > 9000 bytes of history; one match whose source bytes lie on both
    #     sides of the ring edge: with T trailing literals, byte k of a match (length m, offset off)
    #     is m + T + off - k behind the batch end, so the match straddles 4096 when
    #     T + off < 4096 <= T + off + m
    for off in (3839, 3840, 3841, 4095, 4096, 4097, 8191, 8192):
        for m, tail in ((40, 0), (40, 4096 - off - 20 if off < 4090 else 3), (300, 7)):
            seqs, produced = _full_batch(rng, 9000)
            mid, produced = _shorts(rng, 20, produced)
            seqs += mid + [(_rb(rng, 2), off, m), (_rb(rng, max(tail, 0)), 0, 0)]
            cases.append(one_block(f"ring_off{off}_m{m}_t{max(tail, 0)}", seqs))
    # (b) one batch is the whole chunk: spans on both sides of the long-batch switch, sources inside
    for span in (3839, 3840, 3841):
        seqs, produced = _shorts(rng, 30, 0)
        rest = span - produced
        seqs += [(_rb(rng, rest - 700 - 5), 2, 700), (_rb(rng, 5), 0, 0)]
        c = one_block(f"ring_span{span}", seqs)
        assert len(c.data) == span
        cases.append(c)
    # (c) the same spans behind history, with far offsets (the batch after a full one)
    for span in (3839, 3840, 3841):
        seqs, produced = _full_batch(rng, 9000)
        b, p2 = _shorts(rng, 20, produced)
        used = p2 - produced
        seqs += b + [(_rb(rng, 100), 8192, 200), (_rb(rng, span - used - 300 - 400 - 3), 4096, 400), (_rb(rng, 3), 0, 0)]
        cases.append(one_block(f"ring_hist_span{span}", seqs))
    # (d) a long batch with sources inside itself, near and kRing apart
    seqs = [(_rb(rng, 3000), 2000, 100), (_rb(rng, 2000), 4500, 300), (_rb(rng, 10), 5409, 64), (_rb(rng, 1), 1, 70),
            (_rb(rng, 4), 0, 0)]
    cases.append(one_block("ring_long_self", seqs))
    # small twin of (a) for the CPU model
    seqs, produced = _full_batch(rng, 4200)
    seqs += [(_rb(rng, 2), 4090, 40), (_rb(rng, 1), 0, 0)]
    cases.append(one_block("ring_twin", seqs))
    return cases


def family_wide():
    rng = np.random.default_rng(105)
    cases = []
    for run in (511, 512, 1023, 1024, 1025, 16384):
        # the run sits in a long batch (a 3600-byte run before it), at an odd output position
        seqs = [(_rb(rng, 3601), 77, 9), (_rb(rng, run), 5, 11), (_rb(rng, 3), run + 20, 30), (_rb(rng, 600), 1, 5),
                (_rb(rng, 2), 0, 0)]
        cases.append(one_block(f"wide_{run}", seqs))
    # BG4 group boundaries inside a 1 KiB step of one literal run, at every ulen % 4; 20480: the
    # boundaries on step edges
    for ulen in (20000, 20001, 20002, 20003, 20480, 131072):
        run = ulen - 300 if ulen < MAX_CHUNK else 0xFFFF + 30000
        seqs = [(_rb(rng, run), 1234, ulen - run - 6), (_rb(rng, 6), 0, 0)]
        c = one_block(f"wide_bg4_{ulen}", seqs)
        assert len(c.data) == ulen
        cases.append(c)
    seqs = [(_rb(rng, 3700), 9, 20), (_rb(rng, 513), 3, 7), (b"", 0, 0)]
    cases.append(one_block("wide_twin", seqs))
    return cases


def _sized_seq(rng, d: int, produced: int):
    """A match-bearing sequence of encoded size d (>= 3)."""
    for nl, ml in ((d - 3, 6), (d - 4, 19), (d - 4 if d - 4 >= 15 else -1, 5), (d - 5, 30)):
        if nl >= 0 and seq_size(nl, ml) == d and produced + nl > 0:
            return (_rb(rng, nl), int(rng.integers(1, min(produced + nl, 50) + 1)), ml)
    raise AssertionError(d)


def family_block_tail():
    rng = np.random.default_rng(106)
    cases = []
    for d in range(3, 41):
        for tail in (0, 5):
            seqs, produced = _shorts(rng, 70 + d % 3, 0)
            s = _sized_seq(rng, d, produced)
            assert seq_size(len(s[0]), s[2]) == d
            seqs += [s, (_rb(rng, tail), 0, 0)]
            cases.append(one_block(f"tail_d{d}_t{tail}", seqs))
    return cases


def family_batch_fill():
    rng = np.random.default_rng(107)
    cases = []
    for n in list(range(55, 67)) + list(range(120, 131)) + [8 * 64]:
        seqs, _ = _shorts(rng, n, 0)
        cases.append(one_block(f"fill_n{n}", seqs + [(_rb(rng, 1), 0, 0)]))
    # the sequence that splits into the most records, at the batch's flush threshold
    for idx in (55, 56, 57, 58, 63):
        seqs, produced = _shorts(rng, idx, 0, lit_hi=1, ml_hi=5)
        tail, _ = _shorts(rng, 5, 1 << 17, lit_hi=1, ml_hi=5)
        tail_bytes = sum(len(s[0]) + s[2] for s in tail)
        nl = 0xFFFF + 7
        ml = MAX_CHUNK - produced - nl - tail_bytes - 2
        assert ml > 0x7FFF
        seqs += [(_rb(rng, nl), 40000, ml)] + tail + [(_rb(rng, 2), 0, 0)]
        c = one_block(f"fill_big_at{idx}", seqs)
        assert len(c.data) == MAX_CHUNK
        cases.append(c)
    cases.append(one_block("fill_big_first", [(_rb(rng, 65536), 65521, 65536), (b"", 0, 0)]))
    # small twin: a general (nibble 15) sequence at each of those indices
    for idx in (55, 56, 57, 58, 63):
        seqs, produced = _shorts(rng, idx, 0, lit_hi=2, ml_hi=6)
        tail, _ = _shorts(rng, 9, produced + 400)
        seqs += [(_rb(rng, 300), 17, 100)] + tail + [(_rb(rng, 2), 0, 0)]
        cases.append(one_block(f"fill_gen_at{idx}", seqs))
    return cases


def family_frame_shapes():
    rng = np.random.default_rng(108)
    cases = []

    def blocks(n, dependent=False, stored_at=()):
        out, dec = [], b""
        for i in range(n):
            if i in stored_at:
                raw = _rb(rng, int(rng.integers(1, 700)))
                out.append((raw, True))
                dec += raw
                continue
            hist = dec if dependent else b""
            seqs, produced = _shorts(rng, int(rng.integers(3, 90)), 0)
            if dependent and hist:  # matches that reach into the earlier blocks
                seqs = [(b"", len(hist), 30), (_rb(rng, 2), len(hist) // 2 + 1, 9)] + \
                    [(s[0], s[1] + (len(hist) if j % 2 else 0), s[2]) for j, s in enumerate(seqs)]
            seqs.append((_rb(rng, 300), 200 if not hist else len(hist) + 100, 500))
            blk, d = build_block(seqs + [(_rb(rng, int(rng.integers(0, 8))), 0, 0)], hist)
            out.append((blk, False))
            dec += d
        return out, dec

    def add(name, bl, dec, **kw):
        cases.append(Case(name, frame(bl, **kw), dec))

    bl, dec = blocks(1)
    add("shape_content_size", bl, dec, content_size=len(dec))
    add("shape_dict_id", bl, dec, dict_id=0xA1B2C3D4)
    add("shape_block_checksum", bl, dec, block_checksum=True)
    add("shape_content_checksum", bl, dec, content=dec)
    bl, dec = blocks(3, stored_at=(1,))
    add("shape_all_four", bl, dec, content_size=len(dec), dict_id=7, block_checksum=True, content=dec)
    for n in (2, 3, 4):
        bl, dec = blocks(n)
        add(f"shape_{n}_blocks", bl, dec, block_checksum=bool(n & 1))
    for name, at in (("first", (0,)), ("middle", (1,)), ("last", (2,)), ("all", (0, 1, 2))):
        bl, dec = blocks(3, stored_at=at)
        add(f"shape_stored_{name}", bl, dec)
    blk, dec = build_block([(_rb(rng, 20), 20, 44), (b"", 0, 0)])
    add("shape_empty_last_literals", [(blk, False)], dec)
    blk, dec = build_block([(_rb(rng, 1000), 0, 0)])
    add("shape_only_literals", [(blk, False)], dec)
    for n in (2, 3):
        bl, dec = blocks(n, dependent=True)
        add(f"shape_dependent_{n}", bl, dec, independent=False)
    bl, dec = blocks(3, dependent=True, stored_at=(0,))
    add("shape_dependent_after_stored", bl, dec, independent=False, block_checksum=True)
    for n in (1, 3):
        blk, dec = build_block([(_rb(rng, n), 0, 0)])
        add(f"shape_{n}_byte", [(blk, False)], dec)
        add(f"shape_{n}_byte_stored", [(dec, True)], dec, content_size=n)
    # a 128 KiB chunk in two stored blocks of the 64 KiB class and one of the 256 KiB class
    raw = _rb(rng, MAX_CHUNK)
    add("shape_stored_2x64k", [(raw[:65536], True), (raw[65536:], True)], raw)
    add("shape_stored_128k", [(raw, True)], raw)
    return cases


def family_random(seed: int):
    rng = np.random.default_rng(1000 + seed)
    edge_lit = (0, 0, 1, 2, 3, 14, 15, 16, 269, 270, 271, 511, 512, 525, 1024, 1025)
    edge_ml = (4, 4, 5, 18, 19, 20, 63, 64, 65, 127, 129, 200, 273, 274, 275, 529)
    edge_off = (1, 2, 3, 4, 7, 8, 15, 16, 63, 64, 65, 255, 256, 257, 641, 3839, 3840, 3841, 4095, 4096, 4097, 8191,
                8192)
    cases = []
    for c in range(48):
        target = int(rng.integers(1, 32 * 1024 + 1))
        style = int(rng.integers(0, 3))  # 0: mostly fast-loop sequences, 1: edge values, 2: mixed
        seqs, produced = [], 0
        while True:
            edge = style == 1 or (style == 2 and rng.random() < 0.3)
            nl = int(rng.choice(edge_lit)) if edge else int(rng.integers(0, 15))
            ml = int(rng.choice(edge_ml)) if edge else int(rng.integers(4, 19))
            if produced + nl == 0:
                nl = 1
            if produced + nl + ml + 1 > target:
                break
            r = rng.random()
            if r < 0.4:
                off = int(rng.choice(edge_off))
            elif r < 0.7:
                off = int(rng.integers(1, 65))
            else:
                off = int(rng.integers(1, produced + nl + 1))
            off = max(1, min(off, produced + nl, 65535))
            seqs.append((_rb(rng, nl), off, ml))
            produced += nl + ml
        seqs.append((_rb(rng, max(target - produced, 0 if produced else 1)), 0, 0))
        blk, dec = build_block(seqs)
        kw = {}
        if c % 6 == 5:
            kw = dict(content_size=len(dec), block_checksum=True, content=dec)
        cases.append(Case(f"rand{seed}_{c}", frame([(blk, False)], **kw), dec))
    return cases


FAMILIES = {
    "offsets": family_offsets,
    "length_codes": family_length_codes,
    "modulo": family_modulo,
    "ring": family_ring,
    "wide": family_wide,
    "block_tail": family_block_tail,
    "batch_fill": family_batch_fill,
    "frame_shapes": family_frame_shapes,
    "random1": functools.partial(family_random, 1),
    "random2": functools.partial(family_random, 2),
    "random3": functools.partial(family_random, 3),
    "random4": functools.partial(family_random, 4),
}


@functools.lru_cache(maxsize=None)
def family(name: str) -> tuple:
    """The family's cases, built once per process and never modified (bytes are immutable)."""
    cases = tuple(FAMILIES[name]())
    assert len({c.name for c in cases}) == len(cases)
    for c in cases:
        assert 0 < len(c.data) <= MAX_CHUNK, c.name
    return cases


# ------------------------------------------------------------------------------------------------
# malformed frames: (name, frame, ulen, expected ZG_ERR code).  Each is rejected by an explicit check
# of every GPU parser / of exec_batch before a byte of the bad record moves; the host rejects them too.
# ------------------------------------------------------------------------------------------------
ERR_LZ4, ERR_SIZE = 4, 5


def malformed():
    rng = np.random.default_rng(109)
    good, produced = _shorts(rng, 30, 0)
    gb = b"".join(encode_seq(*s) for s in good)
    fin = encode_seq(_rb(rng, 6), 0, 0, last=True)
    out = []

    def one(name, body, ulen, code, **kw):
        out.append((name, frame([(body, False)], **kw), ulen, code))

    # exec_batch: ml && (off == 0 || off > mstart)
    one("offset_zero", gb + encode_seq(b"ab", 0, 8) + fin, produced + 2 + 8 + 6, ERR_LZ4)
    one("offset_past_start", gb + encode_seq(b"ab", produced + 3, 8) + fin, produced + 2 + 8 + 6, ERR_LZ4)
    one("offset_first_sequence", encode_seq(b"abc", 4, 8) + fin, 3 + 8 + 6, ERR_LZ4)
    # exec_batch: mstart + ml > ulen (a literal-only record has ml = 0: its literals are checked too)
    one("match_past_ulen", gb + encode_seq(b"ab", 5, 400) + fin, produced + 2 + 100, ERR_LZ4)
    one("literals_past_ulen", gb + encode_seq(_rb(rng, 300), 0, 0, last=True), produced + 100, ERR_LZ4)
    # decode_chunk / exec_records / the pair consumer: obase != ulen after a clean parse
    one("short_of_ulen", gb + fin, produced + 6 + 9, ERR_SIZE)
    # both parsers: lit > bend - ip
    cut = gb + encode_seq(_rb(rng, 40), 0, 0, last=True)[:-10]
    one("literals_past_block_end", cut, produced + 30, ERR_LZ4)
    # both parsers: len > end - ip (the block length word runs past the payload)
    f = bytearray(frame([(gb + fin, False)]))
    struct.pack_into("<I", f, 7, len(gb + fin) + 50)
    out.append(("block_past_payload", bytes(f), produced + 6, ERR_LZ4))
    # both parsers: fewer than 4 bytes where a block length word / the end mark must stand
    one("no_end_mark", gb + fin, produced + 6, ERR_LZ4, end_mark=False)
    out.append(("end_mark_cut", frame([(gb + fin, False)])[:-2], produced + 6, ERR_LZ4))
    # both parsers: (flg >> 6) != 1
    one("version_0", gb + fin, produced + 6, ERR_LZ4, version=0)
    one("version_2", gb + fin, produced + 6, ERR_LZ4, version=2)
    return out
