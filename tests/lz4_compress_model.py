"""CPU side of the GPU LZ4 compressor tests (csrc/gpu/compress.hip, K7b): a strict validator of
the frames it writes, a scalar model of its parse, and the input families both are run on.

check_frame   every rule a conforming LZ4 frame decoder may enforce on a stored chunk, the
              end-of-block rules included (the host decoder, csrc/core/lz4.cpp, checks none of them);
              decodes with its own byte-at-a-time copy and its own xxh32.
compress_model  the parse the header comment of compress.hip documents, one lane at a time: the
              frame the kernels must write byte for byte, or None where they report the chunk raw.
              `stats` counts the paths a chunk reaches, `mutate` selects one deliberately wrong
              parse (tests/test_lz4_compress_cpu.py shows each is caught).
FAMILIES      seeded chunks aimed at one edge each: 27 is the shortest zero run that is stored, 32 the
              reach of the in-window compare, 64 the window, 65535 the largest offset, 255 the length
              chain's step, 1024 / 2048 / 4096 the default kernel's literal piece, flush and ring.
"""
from __future__ import annotations

import functools
import struct
from typing import NamedTuple

import numpy as np

MAGIC = b"\x04\x22\x4D\x18"
MAX_CHUNK = 128 * 1024
K = 2654435761
K_INV = pow(K, -1, 1 << 32)
TAB_LOG = 12
TAG_MASK = 0x3FFF
WAVE = 64
NEAR = 32
MAX_OFF = 65535

MUTANTS = ("dist65536", "mend4", "ok11", "noconfirm", "insert_all", "chain_drop0", "noback")


# ------------------------------------------------------------------------------------------------
# xxh32 (inputs shorter than 16 bytes: the frame descriptor is two)
# ------------------------------------------------------------------------------------------------
_P1, _P2, _P3, _P4, _P5 = 2654435761, 2246822519, 3266489917, 668265263, 374761393
_M = 0xFFFFFFFF


def _rotl(x: int, r: int) -> int:
    return ((x << r) | (x >> (32 - r))) & _M


def xxh32_short(data: bytes, seed: int = 0) -> int:
    assert len(data) < 16, "short path only"
    h = (seed + _P5 + len(data)) & _M
    i = 0
    while i + 4 <= len(data):
        h = (_rotl((h + struct.unpack_from("<I", data, i)[0] * _P3) & _M, 17) * _P4) & _M
        i += 4
    while i < len(data):
        h = (_rotl((h + data[i] * _P5) & _M, 11) * _P1) & _M
        i += 1
    h ^= h >> 15
    h = (h * _P2) & _M
    h ^= h >> 13
    h = (h * _P3) & _M
    h ^= h >> 16
    return h


def header_checksum(bd: int) -> int:
    """The HC byte of a frame descriptor FLG 0x60, BD `bd`."""
    return (xxh32_short(bytes([0x60, bd])) >> 8) & 0xFF


# ------------------------------------------------------------------------------------------------
# strict frame validator
# ------------------------------------------------------------------------------------------------
def parse_frame(frame: bytes, chunk_len: int):
    """-> (decoded bytes, [(literals, offset, match_len), ...]); AssertionError names the broken rule."""
    frame = bytes(frame)
    assert len(frame) >= 15, f"frame of {len(frame)} bytes: shorter than header + end mark"
    assert frame[:4] == MAGIC, f"magic {frame[:4].hex()}"
    assert frame[4] == 0x60, f"FLG {frame[4]:#x}: want 0x60 (version 1, independent blocks, no checksums, no sizes)"
    bd = 0x40 if chunk_len <= 65536 else 0x50
    assert frame[5] == bd, f"BD {frame[5]:#x}: want {bd:#x} for a chunk of {chunk_len}"
    assert frame[6] == header_checksum(bd), f"HC {frame[6]:#x}: want {header_checksum(bd):#x}"
    word = struct.unpack_from("<I", frame, 7)[0]
    assert not word & 0x80000000, "block size word has the high bit set: a stored block"
    bs = word
    assert bs > 0, "block size 0: the first block is the end mark"
    block_max = 65536 if bd == 0x40 else 262144
    assert bs <= block_max, f"block of {bs} bytes: above the BD class's {block_max}"
    assert 11 + bs + 4 <= len(frame), f"block of {bs} bytes runs past the frame ({len(frame)} bytes)"
    assert frame[11 + bs:11 + bs + 4] == b"\0\0\0\0", "the block is not followed by the end mark: more than one block"
    assert len(frame) == 11 + bs + 4, f"{len(frame) - 15 - bs} bytes after the end mark"
    blk = frame[11:11 + bs]
    out = bytearray()
    seqs = []
    ip = 0
    while True:
        assert ip < bs, "block ends where a token must stand (the last sequence carries a match)"
        tok = blk[ip]
        ip += 1
        nl = tok >> 4
        if nl == 15:
            while True:
                assert ip < bs, "literal length chain runs past the block"
                b = blk[ip]
                ip += 1
                nl += b
                if b != 255:
                    break
        assert ip + nl <= bs, "literals run past the block"
        out += blk[ip:ip + nl]
        ip += nl
        if ip == bs:
            assert tok & 15 == 0, "the last sequence is not literal-only (match nibble set)"
            assert nl >= 5, f"the last sequence has {nl} literals: the last 5 bytes must be literals"
            seqs.append((nl, 0, 0))
            break
        assert ip + 2 <= bs, "offset runs past the block"
        off = blk[ip] | (blk[ip + 1] << 8)
        ip += 2
        ml = (tok & 15) + 4
        if tok & 15 == 15:
            while True:
                assert ip < bs, "match length chain runs past the block"
                b = blk[ip]
                ip += 1
                ml += b
                if b != 255:
                    break
        assert 1 <= off <= len(out), f"offset {off} at output position {len(out)}"
        assert len(out) <= chunk_len - 12, f"match starts at {len(out)}: inside the last 12 bytes of {chunk_len}"
        assert len(out) + ml <= chunk_len - 5, f"match ends at {len(out) + ml}: inside the last 5 bytes of {chunk_len}"
        seqs.append((nl, off, ml))
        for _ in range(ml):
            out.append(out[-off])
    assert len(out) == chunk_len, f"decoded {len(out)} bytes, want {chunk_len}"
    assert len(frame) < chunk_len, f"frame of {len(frame)} bytes is no smaller than the chunk ({chunk_len})"
    return bytes(out), seqs


def check_frame(frame: bytes, chunk_len: int) -> bytes:
    return parse_frame(frame, chunk_len)[0]


# ------------------------------------------------------------------------------------------------
# scalar model of the parse
# ------------------------------------------------------------------------------------------------
def _hashes(data: bytes):
    """Per position p (p + 4 <= len): the 4-byte value, its bucket and its 14-bit tag."""
    n = len(data) - 3
    if n <= 0:
        return [], [], []
    a = np.frombuffer(data, dtype=np.uint8).astype(np.uint64)
    v = a[:n] | (a[1:n + 1] << 8) | (a[2:n + 2] << 16) | (a[3:n + 3] << 24)
    hv = (v * K) & _M
    return v.tolist(), (hv >> (32 - TAB_LOG)).tolist(), (hv & TAG_MASK).tolist()


def _put_len(out: bytearray, r: int, drop0: bool) -> None:
    out += b"\xFF" * (r // 255)
    if not (drop0 and r % 255 == 0):
        out.append(r % 255)


def _emit(out: bytearray, data: bytes, lit0: int, nl: int, off: int, ml: int, drop0: bool) -> None:
    m = ml - 4 if ml else 0
    out.append((min(nl, 15) << 4) | (min(m, 15) if ml else 0))
    if nl >= 15:
        _put_len(out, nl - 15, drop0)
    out += data[lit0:lit0 + nl]
    if ml:
        out += bytes([off & 0xFF, (off >> 8) & 0xFF])
        if m >= 15:
            _put_len(out, m - 15, drop0)


STAT_KEYS = ("far_hits", "near_hits", "max_off", "max_ml", "max_lit", "back_ext", "back_stop_anchor", "back_stop_mc0",
             "tag_reject", "too_far", "lane63_hits", "partial_windows", "windows", "sequences", "frame_len")


def compress_model(data: bytes, stats: dict | None = None, mutate: str | None = None):
    """The frame k_lz4_compress_v1 / k_lz4_compress write for `data` (after BG4 grouping, if any), or
    None where they report the chunk as raw (out_len 0)."""
    assert mutate is None or mutate in MUTANTS, mutate
    data = bytes(data)
    n = len(data)
    st = dict.fromkeys(STAT_KEYS, 0)
    vals, hs, tags = _hashes(data)
    tab = [0] * (1 << TAB_LOG)  # position + 1 of the highest inserted position of the bucket
    max_dist = MAX_OFF + 1 if mutate == "dist65536" else MAX_OFF
    ok_need = 11 if mutate == "ok11" else 12
    drop0 = mutate == "chain_drop0"
    mend = (n - 4 if mutate == "mend4" else n - 5) if n > 5 else 0
    out = bytearray()
    ip = anchor = 0
    while ip + 12 <= n:
        nok = min(WAVE, n - ok_need - ip + 1)  # lanes with p + 12 <= len
        st["windows"] += 1
        if nok < WAVE:
            st["partial_windows"] += 1
        seen = {}  # value -> last lane of this window that holds it
        j = cand = -1
        near_hit = False
        for lane in range(nok):
            p = ip + lane
            v = vals[p]
            prev = seen.get(v)
            seen[v] = lane
            if prev is not None and lane - prev <= NEAR:  # the nearest of the 32 preceding lanes
                j, cand, near_hit = lane, ip + prev, True
                break
            e = tab[hs[p]]
            if e:
                c = e - 1
                if vals[c] == v:
                    if c < p and p - c <= max_dist:
                        j, cand = lane, c
                        break
                    if c < p:
                        st["too_far"] += 1
                elif tags[c] == tags[p] and c < p and p - c <= max_dist:
                    if mutate == "noconfirm":
                        j, cand = lane, c
                        break
                    st["tag_reject"] += 1
        passed = nok if j < 0 else j + 1
        if mutate == "insert_all":
            passed = nok
        for lane in range(passed):
            tab[hs[ip + lane]] = max(tab[hs[ip + lane]], ip + lane + 1)
        if j < 0:
            ip += WAVE
            continue
        st["near_hits" if near_hit else "far_hits"] += 1
        if j == WAVE - 1:
            st["lane63_hits"] += 1
        mp, mc = ip + j, cand
        if mutate != "noback":
            while mp > anchor and mc > 0 and data[mp - 1] == data[mc - 1]:
                mp -= 1
                mc -= 1
            if mp < ip + j:
                st["back_ext"] += 1
                if mp == anchor:
                    st["back_stop_anchor"] += 1
                if mc == 0:
                    st["back_stop_mc0"] += 1
        maxlen = mend - mp
        ml = 4 + (ip + j - mp)
        while ml < maxlen and data[mc + ml] == data[mp + ml]:
            ml += 1
        ml = min(ml, maxlen)
        _emit(out, data, anchor, mp - anchor, mp - mc, ml, drop0)
        st["sequences"] += 1
        st["max_off"] = max(st["max_off"], mp - mc)
        st["max_ml"] = max(st["max_ml"], ml)
        st["max_lit"] = max(st["max_lit"], mp - anchor)
        ip = anchor = mp + ml
    _emit(out, data, anchor, n - anchor, 0, 0, drop0)
    st["sequences"] += 1
    st["max_lit"] = max(st["max_lit"], n - anchor)
    total = 11 + len(out) + 4
    st["frame_len"] = total
    if stats is not None:
        stats.update(st)
    if total >= n:
        return None
    bd = 0x40 if n <= 65536 else 0x50
    return MAGIC + bytes([0x60, bd, header_checksum(bd)]) + struct.pack("<I", len(out)) + bytes(out) + b"\0\0\0\0"


def bg4_split_np(data: bytes) -> bytes:
    """BG4 grouping: byte i goes to group i % 4, the groups are concatenated."""
    a = np.frombuffer(data, dtype=np.uint8)
    return b"".join(a[k::4].tobytes() for k in range(4))


# ------------------------------------------------------------------------------------------------
# input families
# ------------------------------------------------------------------------------------------------
class Chunk(NamedTuple):
    name: str
    data: bytes
    stored: bool  # ungrouped (scheme 1), the compressor must store a frame (True) / report raw (False)


def _nz(rng, n: int) -> bytes:
    """Random bytes without zeros: a zero run next to them starts and ends where the test puts it."""
    return rng.integers(1, 256, int(n), dtype=np.uint8).tobytes()


def _rb(rng, n: int) -> bytes:
    return rng.integers(0, 256, int(n), dtype=np.uint8).tobytes()


def _other(b: int) -> bytes:
    """A nonzero byte different from b."""
    return bytes([b % 255 + 1])


# Shortest stored length of a run of period d (d < 13): the parse emits d literals and one match of
# len - 5 - d (>= 19: one chain byte), then 5 literals: 11 + (1 + d + 2 + 1) + (1 + 5) + 4 = 25 + d
# bytes, stored iff that is < len.
def _period_min(d: int) -> int:
    return 26 + d


def family_lengths():
    cases = []
    for n in range(0, 81):
        cases.append(Chunk(f"zeros_{n}", bytes(n), n >= _period_min(1)))
        cases.append(Chunk(f"p3_{n}", (b"abc" * 27)[:n], n >= _period_min(3)))
        cases.append(Chunk(f"p7_{n}", (b"abcdefg" * 12)[:n], n >= _period_min(7)))
    for n in (65535, 65536, 65537):
        cases.append(Chunk(f"p7_{n}", (b"abcdefg" * (n // 7 + 1))[:n], True))
    cases.append(Chunk("zeros_131071", bytes(131071), True))
    cases.append(Chunk("p3_131072", (b"abc" * 43691)[:131072], True))
    return cases


DISTANCES = (65534, 65535, 65536, 65537)


def family_distance():
    rng = np.random.default_rng(201)
    cases = []
    for d in DISTANCES:
        r = _nz(rng, 64)
        # window 0 holds R and inserts it; the zero run is one match (inserts two zero positions)
        cases.append(Chunk(f"dist_{d}", r + bytes(d - 64) + r + _nz(rng, 256), True))
    return cases


def colliding_values(rng):
    """Two different 4-byte values of the same bucket and the same 14-bit tag, no zero byte in either."""
    while True:
        hv = int(rng.integers(0, 1 << 32))
        hv2 = hv ^ (int(rng.integers(1, 64)) << 14)
        v1, v2 = (hv * K_INV) & _M, (hv2 * K_INV) & _M
        b1, b2 = struct.pack("<I", v1), struct.pack("<I", v2)
        if 0 not in b1 and 0 not in b2:
            assert (v1 * K & _M) >> 20 == (v2 * K & _M) >> 20 and (v1 * K) & TAG_MASK == (v2 * K) & TAG_MASK and v1 != v2
            return b1, b2


# seeds whose random bytes leave the planted bucket alone between the two windows (the CPU test
# asserts tag_reject >= 1 for every one)
TAG_SEEDS = (301, 303, 304, 305)


def family_tag_collision():
    cases = []
    for i, seed in enumerate(TAG_SEEDS):
        rng = np.random.default_rng(seed)
        b1, b2 = colliding_values(rng)
        at = 16 + i  # the confirm load reads the candidate at every address & 3
        body = bytearray(_nz(rng, 192))
        body[at:at + 4] = b1
        body[128 + at + 3:128 + at + 7] = b2
        cases.append(Chunk(f"tag_{seed}", bytes(body) + bytes(200) + _nz(rng, 9), True))
    return cases


CHAIN_LITS = (14, 15, 16, 269, 270, 271, 524, 525)
CHAIN_MLS = (18, 19, 20, 273, 274, 275)


def family_chains():
    rng = np.random.default_rng(202)
    cases = []
    for nl in CHAIN_LITS:
        for ml in CHAIN_MLS:
            # the run's first zero is the last literal; the match is the rest of the run
            data = _nz(rng, nl - 1) + bytes(ml + 1) + _nz(rng, 13) + bytes(80) + _nz(rng, 3)
            cases.append(Chunk(f"chain_l{nl}_m{ml}", data, True))
    return cases


STAGING_LITS = (1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097, 40000)
STAGING_TOTALS = (2047, 2048, 2049, 2052, 4095, 4096, 4097, 4100)  # 2048 k + 4: the end mark starts a flush unit


def _sized_frame(rng, total: int) -> bytes:
    """A chunk whose frame is exactly `total` bytes: one long literal run, a zero run, a short tail."""
    body = _nz(rng, total + 40)
    for tail in range(6, 30):
        for nl in range(total - 60, total):
            data = body[:nl] + bytes(300) + body[nl:nl + tail]
            st = {}
            if compress_model(data, st) is not None and st["frame_len"] == total:
                return data
    raise AssertionError(total)


def family_staging():
    rng = np.random.default_rng(203)
    cases = []
    for nl in STAGING_LITS:
        data = _nz(rng, nl - 1) + bytes(100 + nl // 64) + _nz(rng, 7)
        cases.append(Chunk(f"stage_lit{nl}", data, True))
    for total in STAGING_TOTALS:
        cases.append(Chunk(f"stage_total{total}", _sized_frame(rng, total), True))
    cases.append(Chunk("stage_zeros_128k", bytes(MAX_CHUNK), True))
    w = (rng.standard_normal(8192).astype(np.float32) * 0.02)
    bf16 = (w.view(np.uint32) >> 16).astype(np.uint16).tobytes()
    cases.append(Chunk("stage_bf16_grouped_16k", bg4_split_np(bf16), True))
    return cases


WINDOW_MLS = (4, 5, 67, 68, 69, 131, 132, 133, 195, 196, 197)  # 4 + 64 k and its neighbours
REPEAT_DISTANCES = (32, 33, 64, 65)


def family_windows():
    rng = np.random.default_rng(204)
    zt = bytes(90)  # a compressible tail: the chunk is stored whatever the case costs
    cases = []
    # first hit in lane 63: W at 10 (window 0, inserted) and at 127; the byte before differs
    body = bytearray(_nz(rng, 160))
    w = bytes(body[10:18])
    body[126:127] = _other(body[9])
    body[127:135] = w
    cases.append(Chunk("win_lane63", bytes(body) + zt + _nz(rng, 5), True))
    # backward extension into anchor: a match of U ends before "0 G"; the run's last zero before G
    # was never inserted (it lies inside the run's match), so lane 0 misses, lane 1 hits G and takes
    # the zero back
    u, g = _nz(rng, 8), _nz(rng, 24)
    data = _nz(rng, 20) + u + _nz(rng, 36) + bytes(70) + g + _nz(rng, 70) + u + b"\0" + g + _nz(rng, 9) + zt + _nz(rng, 5)
    cases.append(Chunk("win_back_anchor", data, True))
    # the same over a whole 64-lane step: Z + S lies 65515 back, so after the match of Z + S ends at
    # the anchor every lane's candidate is 65555 away; the window misses and inserts S S, the next
    # window's lane 0 hits 40 back and extends 64 bytes backwards, onto the anchor
    z, s = _nz(rng, 8), _nz(rng, 40)
    head = z + s + _other(s[0]) + _nz(rng, 15)
    data = head + bytes(65515 - len(head)) + z + s + s + s + _nz(rng, 30)
    cases.append(Chunk("win_back_anchor_64", data, True))
    # backward extension into mc == 0: S S at the chunk's start, 40 apart (beyond the in-window
    # compare, inside the window): window 1's lane 0 hits position 24 and walks back to 0
    s = _nz(rng, 40)
    cases.append(Chunk("win_back_mc0", s + s + s + _nz(rng, 11) + zt + _nz(rng, 5), True))
    # forward matches of 4 + 64 k and +-1
    for ml in WINDOW_MLS:
        s = _nz(rng, 260)
        data = s + _nz(rng, 70) + _other(s[-1]) + s[:ml] + _other(s[ml]) + _nz(rng, 20) + zt + _nz(rng, 5)
        cases.append(Chunk(f"win_fwd{ml}", data, True))
    # repeats on either side of the in-window compare's reach and of the window
    for d in REPEAT_DISTANCES:
        a = _nz(rng, d)
        cases.append(Chunk(f"win_repeat{d}", a * 4 + _nz(rng, 10), True))
    # positions behind a window's first hit must not be inserted: B stands in window 0; later one
    # window holds "abcdabcd" (a hit in lane 4, a match of 4) and B again.  The next window finds B
    # in the table only because B's second copy did not replace it.
    b = _nz(rng, 40)
    q = _nz(rng, 4)
    data = _nz(rng, 10) + b + _nz(rng, 14 + 64) + q + q + _other(q[0]) + _nz(rng, 9) + b + _nz(rng, 12) + zt + _nz(rng, 5)
    cases.append(Chunk("win_insert_passed", data, True))
    return cases


TAIL_T = tuple(range(5, 21))


def family_tail():
    rng = np.random.default_rng(205)
    cases = []
    for t in TAIL_T:
        # W stands at 140 behind a zero run and again at len - t; the bytes before the two differ
        w = _nz(rng, 8)
        head = bytes(120) + _nz(rng, 20) + w + _nz(rng, 99 + t)
        rep = w[:t] if t < 8 else w + _nz(rng, t - 8)
        cases.append(Chunk(f"tail_t{t}", head + _other(head[139]) + rep, True))
    return cases


def family_random(seed: int):
    rng = np.random.default_rng(2000 + seed)
    cases = []
    for c in range(6):
        target = int(rng.integers(2000, 32 * 1024 + 1))
        out = bytearray(bytes(int(rng.integers(40, 300))))
        while len(out) < target:
            kind = int(rng.integers(0, 6))
            if kind == 0:
                out += _rb(rng, int(rng.choice((1, 3, 14, 15, 16, 63, 64, 65, 269, 270, 271, 1023, 1024, 1025, 2049))))
            elif kind == 1:
                out += bytes(int(rng.choice((4, 5, 13, 18, 19, 20, 64, 273, 274, 275, 529, 3000))))
            elif kind == 2 and len(out) > 100:  # an earlier slice again, near or far
                ln = int(rng.choice((4, 5, 8, 19, 63, 64, 65, 68, 132, 274, 600)))
                src = int(rng.integers(0, len(out) - 8))
                out += out[src:src + ln]
            elif kind == 3:
                per = _nz(rng, int(rng.choice((1, 2, 3, 7, 31, 32, 33, 40, 63, 64, 65))))
                out += per * int(rng.integers(2, 9))
            elif kind == 4:  # low entropy: many short sequences
                out += rng.integers(0, 4, int(rng.integers(50, 600)), dtype=np.uint8).tobytes()
            else:
                out += _rb(rng, int(rng.integers(1, 200)))
        n = min(len(out), 32 * 1024)
        cases.append(Chunk(f"rand{seed}_{c}", bytes(out[:n]), True))
    return cases


FAMILIES = {
    "lengths": family_lengths,
    "distance": family_distance,
    "tag_collision": family_tag_collision,
    "chains": family_chains,
    "staging": family_staging,
    "windows": family_windows,
    "tail": family_tail,
    "random1": functools.partial(family_random, 1),
    "random2": functools.partial(family_random, 2),
    "random3": functools.partial(family_random, 3),
    "random4": functools.partial(family_random, 4),
}


@functools.lru_cache(maxsize=None)
def family(name: str) -> tuple:
    """The family's chunks, built once per process and never modified (bytes are immutable)."""
    cases = tuple(FAMILIES[name]())
    assert len({c.name for c in cases}) == len(cases)
    for c in cases:
        assert len(c.data) <= MAX_CHUNK, c.name
    return cases


@functools.lru_cache(maxsize=None)
def modelled(name: str, bg4: bool) -> tuple:
    """Per chunk of the family: (the bytes the LZ4 stage sees, the model's frame or None, its stats);
    computed once and shared by every test that compares against it."""
    out = []
    for c in family(name):
        src = bg4_split_np(c.data) if bg4 else c.data
        st = {}
        out.append((src, compress_model(src, st), st))
    return tuple(out)
