"""Plain-Python model of the chunk-header index (csrc/gpu/ingest.hip, K4) and a synthesiser of the
runs that steer its two GPU walks (serial: k_index_terms; parallel: k_hdr_scan + k_hdr_link) onto
their edges.  No torch, no GPU.

walk        an integer transcription of walk_term: the records of one term and its error code.  The
            reference for BOTH GPU walks (the parallel walk promises walk_term's records and errors).
index       walk over every term of a launch: the record array (starting from the caller's sentinel)
            and the set of non-zero error words (code << 32 | term).  The device keeps the first
            word it sees, so with one failing term the word is exact, with several it is one of them.
candidates  the run offsets plausible_header accepts, as k_hdr_scan lists them.  For steering and
            counting candidates and for stating which path a term must take; never a reference for
            records.
dead_ends   True where every sound link rule keeps the fast path: see the function.
Run, Source the synthesiser: runs from (scheme, clen, ulen, payload) tuples, look-alike planting that
            refuses to touch a real header, and placement of a chosen header at a chosen absolute
            position of the source buffer.  Filler bytes are 1..255, so no header (version byte 0)
            starts in them and the synthesiser controls every candidate.
cases       the seeded launches of tests/test_gpu_index.py, by group (GROUPS).

A chunk header is 8 bytes: version 0, clen as LE u24, scheme (0 raw, 1 LZ4, 2 BG4+LZ4), ulen as LE
u24; the payload of a compressed chunk is an LZ4 frame and starts with its magic.
"""
from __future__ import annotations

import functools
from typing import NamedTuple

import numpy as np

MAGIC = b"\x04\x22\x4D\x18"
MAX_CHUNK = 128 * 1024
CAND_CAP = 8192       # kCandCap
SCAN_THREAD = 64      # kScanBytesPerThread
SCAN_BLOCK = 16384    # kScanThreads * kScanBytesPerThread
OK, ERR_HEADER, ERR_RANGE, ERR_COUNT, ERR_CAPACITY = 0, 1, 2, 3, 7

TERM_DTYPE = np.dtype([("src", "<u8"), ("src_len", "<u8"), ("dst", "<u8"), ("chunk_base", "<u4"),
                       ("n_chunks", "<u4"), ("ulen", "<u8")])
CHUNK_DTYPE = np.dtype([("src", "<u8"), ("dst", "<u8"), ("clen", "<u4"), ("ulen", "<u4"),
                        ("scheme", "<u4"), ("term", "<u4")])


class Term(NamedTuple):
    src: int
    src_len: int
    dst: int
    chunk_base: int
    n_chunks: int
    ulen: int  # 0: not checked


def as_term(tm) -> Term:
    return Term(*(int(x) for x in tm))


def header(scheme: int, clen: int, ulen: int, version: int = 0) -> bytes:
    return bytes([version]) + clen.to_bytes(3, "little") + bytes([scheme]) + ulen.to_bytes(3, "little")


def _fields(h) -> tuple:
    """(version, clen, scheme, ulen) of 8 header bytes."""
    return h[0], h[1] | h[2] << 8 | h[3] << 16, h[4], h[5] | h[6] << 8 | h[7] << 16


# ------------------------------------------------------------------------------------------------
# the model
# ------------------------------------------------------------------------------------------------
def walk(src, term, t: int = 0) -> tuple:
    """([n_chunks records (src, dst, clen, ulen, scheme, term)], error code) of term number t."""
    tm = as_term(term)
    zero = (0, 0, 0, 0, 0, t)
    recs = []
    off = uoff = 0

    def fail(code):
        return recs + [zero] * (tm.n_chunks - len(recs)), code

    for _ in range(tm.n_chunks):
        if off + 8 > tm.src_len:
            return fail(ERR_COUNT)
        version, clen, scheme, ulen = _fields(src[tm.src + off:tm.src + off + 8])
        if version != 0 or scheme > 2 or (scheme == 0 and clen != ulen):
            return fail(ERR_HEADER)
        if off + 8 + clen > tm.src_len or (tm.ulen != 0 and uoff + ulen > tm.ulen):
            return fail(ERR_RANGE)
        if ulen > MAX_CHUNK:
            return fail(ERR_CAPACITY)
        recs.append((tm.src + off + 8, tm.dst + uoff, clen, ulen, scheme, t))
        off += 8 + clen
        uoff += ulen
    if off != tm.src_len or (tm.ulen != 0 and uoff != tm.ulen):
        return recs, ERR_COUNT  # the records stay as written
    return recs, OK


def index(src, terms, records: np.ndarray) -> tuple:
    """(records after the launch, set of non-zero error words); `records` is the sentinel-filled
    CHUNK_DTYPE array the launch starts from and is not modified."""
    out = records.copy()
    words = set()
    for t, term in enumerate(terms):
        tm = as_term(term)
        recs, code = walk(src, tm, t)
        for c, r in enumerate(recs):
            out[tm.chunk_base + c] = r
        if code:
            words.add(code << 32 | t)
    return out, words


def candidates(src, term) -> list:
    """Run offsets at which k_hdr_scan's plausible_header holds, ascending.  The 4 bytes after the
    header are read from the buffer wherever they lie (bytes past its end read as zero)."""
    tm = as_term(term)
    if tm.src_len < 8:
        return []
    run = np.frombuffer(bytes(src[tm.src:tm.src + tm.src_len + 4]).ljust(tm.src_len + 4, b"\0"), dtype=np.uint8)
    out = []
    for p in np.flatnonzero(run[:tm.src_len - 7] == 0).tolist():
        _, clen, scheme, ulen = _fields(run[p:p + 8].tolist())
        if scheme > 2 or not 1 <= ulen <= MAX_CHUNK or clen < 1:
            continue
        if (clen != ulen) if scheme == 0 else (run[p + 8:p + 12].tobytes() != MAGIC):
            continue
        if p + 8 + clen <= tm.src_len:
            out.append(p)
    return out


def successor(src, term, p: int) -> int:
    tm = as_term(term)
    return p + 8 + _fields(src[tm.src + p:tm.src + p + 8])[1]


def chain_offsets(src, term) -> list:
    """Header offsets of the records walk() accepts, in order (the true chain, as far as it goes)."""
    tm = as_term(term)
    return [r[0] - 8 - tm.src for r in walk(src, tm)[0] if r[0]]


def dead_ends(src, term) -> bool:
    """True when the term must keep the fast path under any sound link rule: the walk succeeds, the
    candidates are within the cap and hold the whole chain, and every other candidate is a dead end
    (its successor is neither a candidate nor the run's end), so it can add nothing to a chain."""
    tm = as_term(term)
    recs, code = walk(src, tm)
    cand = candidates(src, tm)
    chain = [r[0] - 8 - tm.src for r in recs]
    if code or not tm.n_chunks or len(cand) > CAND_CAP or not set(chain) <= set(cand):
        return False
    ends = set(cand) | {tm.src_len}
    return all(successor(src, tm, p) not in ends for p in set(cand) - set(chain))


LINK_RULES = ("chain", "pointed")


def link_choice(src, term, rule: str = "chain") -> list | None:
    """The offsets k_hdr_link's fast path would turn into records, or None where it hands the term
    to the serial walk.  Not a reference: it is here so that the CPU tests can show which inputs
    tell a sound rule from an unsound one.  "chain": a member other than offset 0 must be the
    successor of a member.  "pointed": the successor of any candidate will do -- the rule that a
    short chain with a side branch defeats."""
    tm = as_term(term)
    cand = candidates(src, tm)
    if len(cand) < tm.n_chunks or not cand or len(cand) > CAND_CAP:
        return None
    have = set(cand)
    nxt = {p: successor(src, tm, p) for p in cand}
    linked = {p for p in cand if nxt[p] == tm.src_len or nxt[p] in have}
    pointed = set(nxt.values())
    good = {p for p in linked if p == 0 or p in pointed}
    if 0 not in good or any(nxt[p] != tm.src_len and nxt[p] not in good for p in good):
        return None
    if rule == "chain" and not good - {0} <= {nxt[q] for q in good}:
        return None
    ulen = sum(_fields(src[tm.src + p:tm.src + p + 8])[3] for p in good)
    if len(good) != tm.n_chunks or (tm.ulen and ulen != tm.ulen):
        return None
    return sorted(good)


# ------------------------------------------------------------------------------------------------
# the synthesiser
# ------------------------------------------------------------------------------------------------
def filler(rng, n: int) -> bytes:
    return rng.integers(1, 256, n, dtype=np.uint8).tobytes()


def raw(n: int, payload: bytes | None = None) -> tuple:
    return (0, n, n, payload)


def framed(scheme: int, clen: int, ulen: int) -> tuple:
    """A compressed chunk: the frame magic, then filler (the index does not decode it)."""
    assert scheme in (1, 2) and clen >= 4
    return (scheme, clen, ulen, None)


class Run:
    """One run: the chunks' headers and payloads back to back.  payload None: filler of clen bytes,
    after the frame magic for schemes 1 and 2.  A header may lie: the payload is what is stored."""

    def __init__(self, chunks, rng):
        self.buf = bytearray()
        self.hdrs = []   # offsets of the real headers
        self.ulens = []
        for scheme, clen, ulen, payload in chunks:
            if payload is None:
                payload = MAGIC + filler(rng, clen - 4) if scheme in (1, 2) else filler(rng, clen)
            self.hdrs.append(len(self.buf))
            self.ulens.append(ulen)
            self.buf += header(scheme, clen, ulen) + payload

    n = property(lambda self: len(self.hdrs))
    ulen = property(lambda self: sum(self.ulens))

    def __len__(self):
        return len(self.buf)

    def free(self, pos: int) -> bool:
        """8 bytes at pos lie inside the run and touch no real header."""
        return 0 <= pos and pos + 8 <= len(self.buf) and all(abs(pos - h) >= 8 for h in self.hdrs)

    def plant(self, pos: int, clen: int) -> int:
        """A raw-header look-alike for clen bytes at run offset pos; returns its successor offset."""
        if not self.free(pos) or not 1 <= clen <= MAX_CHUNK:
            raise ValueError(f"look-alike at {pos} for {clen} bytes would overwrite a real header or leave the run")
        self.buf[pos:pos + 8] = header(0, clen, clen)
        return pos + 8 + clen

    def plant_chain(self, pos: int, clens, to: int | None = None) -> list:
        """Look-alikes pointing at one another from pos on, one per entry of clens; with `to` (a real
        header's offset, or len(run) for the run's end) one more whose successor is exactly `to`.
        Returns their offsets."""
        at = []
        for clen in clens:
            at.append(pos)
            pos = self.plant(pos, clen)
        if to is not None:
            at.append(pos)
            assert to == len(self.buf) or to in self.hdrs
            if self.plant(pos, to - pos - 8) != to:
                raise ValueError("chain does not reach its target")
        return at


class Case(NamedTuple):
    name: str
    src: bytes
    terms: np.ndarray   # TERM_DTYPE
    n_records: int      # a few more than any term uses
    fast: tuple         # per term: True must keep the fast path, False must fall back, None not asserted
    kinds: tuple = ()   # per term, free text (the sweep's bookkeeping)


class Source:
    """A source buffer under construction: filler, gaps and runs, and the terms that describe them."""

    def __init__(self, rng, lead: int | bytes = 0, chunk_base: int = 0, dst: int = 0):
        self.rng = rng
        self.buf = bytearray(lead if isinstance(lead, bytes) else filler(rng, lead))
        self.terms = []
        self.base = chunk_base
        self.dst = dst

    def gap(self, n: int | bytes) -> None:
        self.buf += n if isinstance(n, bytes) else filler(self.rng, n)

    def pad_to(self, pos: int) -> None:
        assert pos >= len(self.buf), (pos, len(self.buf))
        self.gap(pos - len(self.buf))

    def add(self, run: Run, n_chunks: int | None = None, ulen: int | str = "sum", src_len: int | None = None,
            spare: int = 1) -> int:
        """Append the run and its term (n_chunks, ulen and src_len default to the truth; ulen 0 is
        "not checked"); `spare` records are left unused behind the term's.  Returns the term number."""
        n_chunks = run.n if n_chunks is None else n_chunks
        self.terms.append((len(self.buf), len(run) if src_len is None else src_len, self.dst, self.base, n_chunks,
                           run.ulen if ulen == "sum" else ulen))
        self.buf += run.buf
        self.base += n_chunks + spare
        self.dst += run.ulen + 3
        return len(self.terms) - 1

    def add_at(self, run: Run, i: int, pos: int, **kw) -> int:
        """Append the run so that its real header number i lies at absolute position pos."""
        self.pad_to(pos - run.hdrs[i])
        return self.add(run, **kw)

    def poke(self, pos: int, data: bytes) -> None:
        self.buf[pos:pos + len(data)] = data

    def case(self, name: str, fast=None, kinds=(), order=None) -> Case:
        terms = np.array(self.terms, dtype=TERM_DTYPE)
        if order is not None:
            terms = terms[list(order)]
        fast = tuple(fast) if fast is not None else (None,) * len(terms)
        assert len(fast) == len(terms)
        return Case(name, bytes(self.buf), terms, self.base + 2, fast, tuple(kinds))


# ------------------------------------------------------------------------------------------------
# the cases
# ------------------------------------------------------------------------------------------------
RAW_SIZES = (1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65, 4096)


def _mixed_chunks(rng) -> list:
    """Every RAW_SIZES chunk once, in a seeded order, with scheme 1 and 2 chunks in between."""
    out = []
    for i, n in enumerate(rng.permutation(RAW_SIZES).tolist()):
        out.append(raw(n))
        if i % 3 == 1:
            out.append(framed(1 + (i // 3) % 2, int(rng.integers(4, 300)), int(rng.integers(1, MAX_CHUNK + 1))))
    return out


def _small_run(rng, n: int = 5, lo: int = 30, hi: int = 400) -> Run:
    return Run([raw(int(rng.integers(lo, hi))) for _ in range(n)], rng)


def clean_cases() -> list:
    out = []
    for nt in (1, 2, 3, 7):  # mixed sizes and schemes; chunk_base not 0; ulen 0 and the true sum
        rng = np.random.default_rng(100 + nt)
        s = Source(rng, lead=int(rng.integers(0, 70)), chunk_base=5, dst=11)
        for t in range(nt):
            s.add(Run(_mixed_chunks(rng), rng), ulen="sum" if t % 2 else 0)
            s.gap(int(rng.integers(1, 71)))
        out.append(s.case(f"mixed_{nt}_terms", fast=[True] * nt))
    # a term starting at every residue mod 64 of the buffer
    rng = np.random.default_rng(164)
    s = Source(rng, chunk_base=1)
    for r in range(64):
        s.gap((r - len(s.buf) - 1) % 64 + 1)  # 1..64 bytes, up to the next position of residue r
        assert len(s.buf) % 64 == r
        s.add(Run([raw(int(n)) for n in rng.integers(1, 90, 3)], rng), ulen="sum" if r % 3 else 0)
    out.append(s.case("every_residue", fast=[True] * 64))
    # plausible raw headers in front of the first term and in the gaps (one pointing at the next
    # term's first header, one reaching into the next term, one alone in a gap of 8 bytes)
    rng = np.random.default_rng(165)
    s = Source(rng, lead=filler(rng, 9) + header(0, 20, 20) + filler(rng, 20), chunk_base=2)
    s.add(_small_run(rng, 4))
    s.gap(filler(rng, 5) + header(0, 30, 30) + filler(rng, 30))
    s.add(_small_run(rng, 4), ulen=0)
    s.gap(filler(rng, 3) + header(0, 100, 100) + filler(rng, 17))
    s.add(_small_run(rng, 4))
    s.gap(header(0, 1, 1))
    s.add(_small_run(rng, 3))
    s.gap(header(0, 2, 2) + filler(rng, 2))
    out.append(s.case("headers_in_gaps", fast=[True] * 4))
    # several whole terms inside one scan thread's 64 bytes: 1-byte chunks, one per term, back to
    # back from a position = 3 mod 64 (five terms in bytes [3, 48) of the slice, twelve in all)
    rng = np.random.default_rng(166)
    s = Source(rng, lead=64 * 3 + 3, chunk_base=3)
    for t in range(12):
        s.add(Run([raw(1)], rng), ulen=t % 2, spare=t % 2)
    out.append(s.case("terms_packed_in_a_slice", fast=[True] * 12))
    return out


def seam_cases() -> list:
    """A real header at 64*m - 8 + j (thread seam, m = 37) and at 16384*k - 8 + j (block seam,
    k = 1, 2), j = 0..8: one launch per j, one term per seam; each run ends in a raw chunk of 1..4
    bytes, so the last header lies 9..12 bytes before the run's end."""
    out = []
    for j in range(9):
        rng = np.random.default_rng(200 + j)
        s = Source(rng, chunk_base=j)
        for pos in (64 * 37, SCAN_BLOCK, 2 * SCAN_BLOCK):
            run = Run([raw(40), raw(23), raw(int(rng.integers(100, 300))), raw(j % 4 + 1)], rng)
            s.add_at(run, 1, pos - 8 + j, ulen="sum" if j % 2 else 0)
            assert s.terms[-1][0] + run.hdrs[1] == pos - 8 + j
        out.append(s.case(f"seam_j{j}", fast=[True] * 3))
    rng = np.random.default_rng(209)
    s = Source(rng, lead=5)
    for e in (1, 2, 3, 4):  # the last chunk: 1..4 raw bytes at the very end of the run
        s.add(Run([raw(77), raw(e)], rng))
        s.gap(e)
    out.append(s.case("last_chunk_1_to_4_bytes", fast=[True] * 4))
    return out


SORT_SIZES = (1023, 1024, 1025, 2049, 8191, 8192, 8193)


@functools.lru_cache(maxsize=None)
def sort_case(n: int) -> Case:
    """One term of n raw 1-byte chunks: n candidates.  P up to 8192 in the bitonic sort, 1..8
    candidates per thread in the prefix slices; 8193 is one over the candidate cap."""
    rng = np.random.default_rng(300)
    s = Source(rng, lead=16, chunk_base=1)
    s.add(Run([raw(1)] * n, rng), ulen=n if n % 2 else 0)
    return s.case(f"sort_{n}", fast=[n <= CAND_CAP])


def descending_case() -> Case:
    """Three healthy terms handed over in descending src order: the scan's binary search expects
    ascending terms, finds none of their candidates, and every term takes the serial walk."""
    rng = np.random.default_rng(310)
    s = Source(rng, lead=7)
    for _ in range(3):
        s.add(_small_run(rng, 6))
        s.gap(9)
    return s.case("descending_terms", fast=[False] * 3, order=(2, 1, 0))


def lookalike_cases() -> list:
    """Look-alikes planted in term 1 of three well-formed terms."""
    out = []

    def three(seed):
        rng = np.random.default_rng(seed)
        s = Source(rng, lead=21, chunk_base=4)
        runs = [Run([raw(300), raw(400), raw(90), raw(200)], rng) for _ in range(3)]
        return s, runs

    def finish(s, runs, name, fast=None):
        for i, r in enumerate(runs):
            s.add(r, ulen=0 if i == 2 else "sum")
            s.gap(13)
        return s.case(name, fast=fast)

    s, runs = three(400)   # lone ones, dead ends all: the fast path is kept
    runs[1].plant(20, 16)
    runs[1].plant(runs[1].hdrs[1] + 100, 33)
    runs[1].plant(runs[1].hdrs[3] + 9, 5)
    out.append(finish(s, runs, "lone", fast=[True] * 3))
    s, runs = three(401)   # a chain of two inside one payload
    runs[1].plant_chain(runs[1].hdrs[1] + 40, [16, 24])
    out.append(finish(s, runs, "chain_of_two"))
    s, runs = three(402)   # one that points at a real header
    runs[1].plant_chain(runs[1].hdrs[1] + 40, [], to=runs[1].hdrs[2])
    out.append(finish(s, runs, "points_at_real"))
    s, runs = three(403)   # two that point at the run's end, from two payloads
    runs[1].plant_chain(runs[1].hdrs[2] + 30, [], to=len(runs[1]))
    runs[1].plant_chain(runs[1].hdrs[3] + 50, [], to=len(runs[1]))
    out.append(finish(s, runs, "point_at_end"))
    # headers written over the run's last bytes: 8 bytes before the end (its one payload byte would
    # lie in the gap) and 4 bytes before the end (half of the header itself lies in the gap)
    for back in (8, 4):
        s, runs = three(404 + back)
        c = finish(s, runs, f"crosses_end_{back}")
        src = bytearray(c.src)
        end = int(c.terms[1]["src"] + c.terms[1]["src_len"])
        src[end - back:end - back + 8] = header(0, 1, 1)
        out.append(c._replace(src=bytes(src)))
    return out


MALFORMED = ("bad_version", "scheme_3", "raw_clen_ne_ulen", "clen_past_run", "past_term_ulen", "capacity",
             "one_too_few", "one_too_many", "trailing_bytes", "zero_length_raw", "no_magic", "zero_chunks")
# the error each reaches (zero_length_raw and no_magic are valid runs the scan cannot list)
MALFORMED_CODE = dict(bad_version=ERR_HEADER, scheme_3=ERR_HEADER, raw_clen_ne_ulen=ERR_HEADER,
                      clen_past_run=ERR_RANGE, past_term_ulen=ERR_RANGE, capacity=ERR_CAPACITY,
                      one_too_few=ERR_COUNT, one_too_many=ERR_COUNT, trailing_bytes=ERR_COUNT,
                      zero_length_raw=OK, no_magic=OK, zero_chunks=ERR_COUNT)


def malformed_term(kind: str, rng) -> tuple:
    """(run, add() keywords) of a five-chunk run steered to `kind`; the odd chunk is number 2."""
    sizes = [int(x) for x in rng.integers(30, 200, 5)]
    chunks = [raw(n) for n in sizes]
    kw = {}
    if kind == "scheme_3":
        chunks[2] = (3, sizes[2], sizes[2], None)
    elif kind == "raw_clen_ne_ulen":
        chunks[2] = (0, sizes[2], sizes[2] + 1, None)
    elif kind == "capacity":
        chunks[2] = framed(1, sizes[2], MAX_CHUNK + 1)
    elif kind == "zero_length_raw":
        chunks[2] = raw(0)
    elif kind == "no_magic":
        chunks[2] = (1, sizes[2], 1000, filler(rng, sizes[2]))
    run = Run(chunks, rng)
    if kind == "bad_version":
        run.buf[run.hdrs[2]] = 1
    elif kind == "clen_past_run":  # the header claims one byte more than the run holds behind it
        n = len(run) - run.hdrs[2] - 8 + 1
        run.buf[run.hdrs[2]:run.hdrs[2] + 8] = header(0, n, n)
    elif kind == "past_term_ulen":
        kw["ulen"] = run.ulen - 1
    elif kind == "one_too_few":
        kw["n_chunks"] = 6
    elif kind == "one_too_many":
        kw["n_chunks"] = 4
    elif kind == "trailing_bytes":
        run.buf += filler(rng, 3)
    elif kind == "zero_chunks":
        kw["n_chunks"] = 0
    return run, kw


@functools.lru_cache(maxsize=None)
def malformed_case(kind: str, where: int) -> Case:
    """Five terms, four healthy and the one at index `where` of `kind`."""
    rng = np.random.default_rng(500 + 7 * MALFORMED.index(kind) + where)
    s = Source(rng, lead=3, chunk_base=2)
    for t in range(5):
        if t == where:
            run, kw = malformed_term(kind, rng)
            s.add(run, **kw)
        else:
            s.add(_small_run(rng, 4), ulen="sum" if t % 2 else 0)
        s.gap(int(rng.integers(1, 40)))
    fast = [None] * 5
    if kind == "zero_length_raw":
        fast[where] = False
    return s.case(f"{kind}_at_{where}", fast=fast)


def the_construction(ulen: int) -> Case:
    """The short chain with a side branch, one run in one term: A (400 bytes, holding look-alike X
    for 16 bytes at payload byte 20 and, at X's successor, look-alike Y for 348 bytes whose successor
    is B), B (50 bytes), C (60 bytes), planned as 4 chunks."""
    rng = np.random.default_rng(600)
    run = Run([raw(400), raw(50, b"\x07" * 50), raw(60, b"\x09" * 60)], rng)
    assert run.plant_chain(8 + 20, [16], to=run.hdrs[1]) == [28, 52]
    s = Source(rng)
    s.add(run, n_chunks=4, ulen=ulen)
    return s.case(f"construction_ulen_{ulen}")


def branch_cases() -> list:
    """Short chains whose count a side branch makes up: the construction with and without the
    term's ulen; a branch of two (X -> Y -> Z -> real header, two chunks short); branches that end
    on the run's end; each among healthy terms."""
    out = [the_construction(0), the_construction(858)]
    for name, clens, to_end, with_ulen in (("branch_of_two", [16, 40], False, False),
                                           ("branch_of_two_ulen", [16, 40], False, True),
                                           ("branch_to_end", [16], True, False),
                                           ("branch_to_end_ulen", [24], True, True)):
        rng = np.random.default_rng(610 + len(out))
        s = Source(rng, lead=19, chunk_base=1)
        s.add(_small_run(rng, 3))
        s.gap(5)
        run = Run([raw(120), raw(500), raw(80), raw(300)], rng)
        # X in chunk 1's payload; the branch ends on chunk 2's header, or runs from the last payload
        # to the run's end
        at = run.plant_chain(run.hdrs[3] + 20 if to_end else run.hdrs[1] + 30, clens,
                             to=len(run) if to_end else run.hdrs[2])
        members = at[1:]  # every planted header but X is some candidate's successor
        extra = sum(_fields(run.buf[p:p + 8])[3] for p in members)
        s.add(run, n_chunks=run.n + len(members), ulen=run.ulen + extra if with_ulen else 0)
        s.gap(11)
        s.add(_small_run(rng, 3), ulen=0)
        out.append(s.case(name))
    return out


SWEEP_LAUNCHES, SWEEP_TERMS = 4, 50
# planted structure x how far n_chunks is from the true chain; cycled, so every launch holds each
SWEEP_PLANTS = ("none", "lone", "branch1", "none", "chain2", "lone", "branch2", "to_real", "none", "branch_end",
                "lone")


@functools.lru_cache(maxsize=None)
def sweep_case(launch: int) -> Case:
    """50 small steered terms.  kinds[t]: "fast" (dead_ends holds: the fast path must be kept),
    "branch" (short chain plus side branch: n_chunks = true chain + the branch's pointed members) or
    "other".  Most terms fail with COUNT, so the error word of a launch is one of the model's."""
    rng = np.random.default_rng(700 + launch)
    s = Source(rng, lead=int(rng.integers(0, 64)), chunk_base=launch)
    kinds = []
    for t in range(SWEEP_TERMS):
        plant = SWEEP_PLANTS[(t + launch) % len(SWEEP_PLANTS)]
        chunks = [raw(int(x)) for x in rng.integers(120, 420, int(rng.integers(3, 8)))]
        if t % 5 == 0:
            chunks[-1] = framed(1 + t % 2, int(rng.integers(8, 200)), int(rng.integers(1, 5000)))
        run = Run(chunks, rng)
        k = int(rng.integers(0, run.n - 1))   # the payload that takes the plant; never the last one
        p = run.hdrs[k] + 8 + int(rng.integers(4, 30))
        branch = []  # planted headers that are a look-alike's successor and lead on to the run's end
        if plant == "lone":
            run.plant(p, 7)
        elif plant == "chain2":
            run.plant_chain(p, [16, 9])
        elif plant == "to_real":
            run.plant_chain(p, [], to=run.hdrs[k + 1])
        elif plant == "branch1":
            branch = run.plant_chain(p, [16], to=run.hdrs[k + 1])[1:]
        elif plant == "branch2":
            branch = run.plant_chain(p, [16, 20], to=run.hdrs[k + 1])[1:]
        elif plant == "branch_end":  # from the payload in front of the last header to the run's end
            branch = run.plant_chain(run.hdrs[-1] - 60, [12], to=len(run))[1:]
        members = len(branch)
        if members:
            delta = members if t % 4 else members - 1
        else:
            delta = int(rng.choice((0, 0, 0, 0, 0, 1, -1, 2)))
        n_chunks = run.n + delta
        ulen = 0 if t % 2 else run.ulen + sum(_fields(run.buf[q:q + 8])[3] for q in branch[:delta])
        tn = s.add(run, n_chunks=n_chunks, ulen=ulen)
        s.gap(int(rng.integers(1, 71)))
        term = s.terms[tn]
        if members and delta == members:
            kinds.append("branch")
        else:
            kinds.append("fast" if dead_ends(s.buf, term) else "other")
    fast = [True if k == "fast" else None for k in kinds]
    return s.case(f"sweep_{launch}", fast=fast, kinds=kinds)


GROUPS = {
    "clean": clean_cases,
    "seams": seam_cases,
    "lookalikes": lookalike_cases,
    "branches": branch_cases,
}


@functools.lru_cache(maxsize=None)
def group(name: str) -> tuple:
    return tuple(GROUPS[name]())


def case_names(name: str) -> list:
    return [c.name for c in group(name)]


def by_name(grp: str, name: str) -> Case:
    return {c.name: c for c in group(grp)}[name]
