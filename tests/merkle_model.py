"""Plain-Python reference of the Xet Merkle aggregation and the seeded leaf families that steer the
GPU kernels of csrc/gpu/merkle.hip (K2) onto their edges.

merkle_model   the tree straight from the format rule: per level, groups are formed left to right;
               a group takes everything when 2 or fewer nodes remain, otherwise it closes after the
               first child at index >= 2 whose little-endian u64 of hash bytes 24..32 is 0 mod 4, and
               has at most 9 children.  A node hashes the lines "{xet_hex} : {size}\\n" of its children
               with the INTERNAL_NODE key and its size is the sum of theirs.  Only the keyed BLAKE3
               comes from the native core (C.internal_node_hash, C.blake3_keyed); grouping, hex and
               decimal printing are done here, independently of csrc/core/xet_hash.cpp and of the
               kernel.  `rule` selects one deliberately wrong rule (RULES) so that a CPU test can show
               which inputs tell a subtly wrong implementation from a right one.
stats          what a tree reached, per level: see level_stats().
FAMILIES       seeded cases (name, hashes uint8[n,32], sizes uint64[n]).  The cut flag of a leaf is
               steered through the low two bits of byte 24; every other byte is random.
"""
from __future__ import annotations

import functools
from collections import Counter
from typing import NamedTuple

import numpy as np

from zest_amd import _core as C

MAX_CHILDREN = 9
THREADS = 1024  # level_starts: thread t owns positions [t*B, (t+1)*B), B = ceil(n / 1024)
LDS_FLAG_NODES = 131072  # levels with more nodes keep their cut flags in global memory
U64 = 1 << 64

RULES = ("scan_from_1", "max8", "max10", "flag_byte31", "flag_byte0", "flag_be_word", "drop_digit17",
         "early_flush64")
# flag_be_word (u64 of bytes 24..32 read big-endian, % 4) is arithmetically the same as flag_byte31;
# both names are kept because they are two different mistakes in the source.


def xet_hex(h: bytes) -> str:
    """Four little-endian u64 words, each printed as 16 hex digits."""
    return b"".join(h[8 * w:8 * w + 8][::-1] for w in range(4)).hex()


def _hex_all(hashes) -> str:
    """xet_hex of every hash, concatenated (64 characters each)."""
    return np.frombuffer(b"".join(hashes), dtype=np.uint8).reshape(-1, 8)[:, ::-1].tobytes().hex()


def leaves_of(hashes: np.ndarray, sizes: np.ndarray) -> list:
    """[(hash bytes, size int)] as C.merkle_root and merkle_model take them."""
    hb = np.ascontiguousarray(hashes, dtype=np.uint8).tobytes()
    return [(hb[32 * i:32 * i + 32], s) for i, s in enumerate(np.asarray(sizes, dtype=np.uint64).tolist())]


def _flags(hashes, rule) -> bytes:
    if rule == "flag_byte31":
        return bytes([(h[31] & 3) == 0 for h in hashes])
    if rule == "flag_byte0":
        return bytes([(h[0] & 3) == 0 for h in hashes])
    if rule == "flag_be_word":
        return bytes([int.from_bytes(h[24:32], "big") % 4 == 0 for h in hashes])
    # int.from_bytes(h[24:32], "little") % 4 == 0 for every h, in one pass
    return ((np.frombuffer(b"".join(hashes), dtype=np.uint8)[24::32] & 3) == 0).astype(np.uint8).tobytes()


def group_starts(flags: bytes, rule=None) -> list:
    """Boundaries [0, ..., n] of the groups of one level."""
    n = len(flags)
    first = 1 if rule == "scan_from_1" else 2
    most = 8 if rule == "max8" else 10 if rule == "max10" else MAX_CHILDREN
    starts = [0]
    p = 0
    while p < n:
        rem = n - p
        if rem <= 2:
            cut = rem
        else:
            end = min(most, rem)
            k = flags.find(1, p + first, p + end)
            cut = end if k < 0 else k - p + 1
        p += cut
        starts.append(p)
    return starts


def chain_walk_starts(flags: bytes, entry_from: int = 0, threads: int = THREADS) -> list:
    """The boundaries as level_starts of merkle.hip finds them, step by step on the host: thread t
    owns [t*B, (t+1)*B), (A) maps each of the 9 entry offsets of its block to the offset at which
    that chain leaves it, (B) the maps are composed from the left, (C) thread t walks from
    composed[t-1][0].  entry_from = 1 is the wrong build that reads composed[t-1][1]; it is applied
    at B >= 2 only, because at B = 1 it splits a level of 2 nodes into 2 groups and the tree never
    shrinks to its root."""
    n = len(flags)
    B = max(1, -(-n // threads))

    def cut_at(p):
        rem = n - p
        if rem <= 2:
            return rem
        end = min(MAX_CHILDREN, rem)
        k = flags.find(1, p + 2, p + end)
        return end if k < 0 else k - p + 1

    composed = []
    for t in range(threads):
        lo, hi = t * B, min(t * B + B, n)
        if lo < hi:
            row = []
            for e in range(9):
                p = lo + e
                while p < hi:
                    p += cut_at(p)
                row.append(p - hi)
        else:
            row = list(range(9))  # past the end: identity
        assert all(0 <= x <= 8 for x in row)
        composed.append(row if t == 0 else [row[composed[t - 1][e]] for e in range(9)])
    starts = []
    for t in range(threads):
        lo, hi = t * B, min(t * B + B, n)
        p = lo + (0 if t == 0 else composed[t - 1][entry_from if B >= 2 else 0])
        while p < hi:
            starts.append(p)
            p += cut_at(p)
    return starts + [n]


def level_stats(n: int, starts: list, sizes: list, msg_lens: list, tail_straddles: int) -> dict:
    """What one level of n nodes reached.
      n, groups (Counter of group sizes), digits (set of digit counts printed),
      msg64 (set of (lines, total digits) of the messages whose length is a multiple of 64),
      mod64 (set of message length % 64), tail_straddles (lines whose " : size\\n" crosses a 64-byte
      boundary of the message),
      B = ceil(n/1024), active (threads that own a position), straddle (groups that cross a block
      edge), span3 (groups that touch three or more blocks), entries (set of offsets into a block of
      the first group start at or after the block's first position), max_entry,
      global_flags (the level keeps its flags in global memory)."""
    B = max(1, -(-n // THREADS))
    active = -(-n // B)
    groups = Counter()
    straddle = span3 = 0
    for a, b in zip(starts, starts[1:]):
        groups[b - a] += 1
        blocks = (b - 1) // B - a // B
        straddle += blocks >= 1
        span3 += blocks >= 2
    entries = set()
    g = 0
    for t in range(1, active):
        while starts[g] < t * B:
            g += 1
        entries.add(starts[g] - t * B)
    digits = {len(str(s)) for s in sizes}
    msg64 = set()
    for (a, b), m in zip(zip(starts, starts[1:]), msg_lens):
        if m % 64 == 0:
            msg64.add((b - a, m - 68 * (b - a)))
    return {"n": n, "groups": groups, "digits": digits, "msg64": msg64, "mod64": {m % 64 for m in msg_lens},
            "tail_straddles": tail_straddles, "B": B, "active": active, "straddle": straddle, "span3": span3,
            "entries": entries, "max_entry": max(entries, default=0), "global_flags": n > LDS_FLAG_NODES}


def merkle_model(leaves, file_hash: bool = False, stats: dict | None = None, rule: str | None = None) -> bytes:
    """Root (or file hash) of leaves [(hash bytes, size int)].  stats, when given, receives
    {"levels": [level_stats, ...]} with the leaf level first."""
    assert rule is None or rule in RULES, rule
    if stats is not None:
        stats["levels"] = []
    if not leaves:
        return bytes(32)
    hashes = [bytes(h) for h, _ in leaves]
    sizes = [int(s) for _, s in leaves]
    assert all(len(h) == 32 for h in hashes) and all(0 <= s < U64 for s in sizes)
    while len(hashes) > 1:
        n = len(hashes)
        starts = group_starts(_flags(hashes, rule), rule)
        hx = _hex_all(hashes)
        dec = [str(s) for s in sizes]
        if rule == "drop_digit17":
            dec = [d[1:] if len(d) > 16 else d for d in dec]
        lines = [hx[64 * j:64 * j + 64] + " : " + dec[j] + "\n" for j in range(n)]
        nh, ns, msg_lens = [], [], []
        for a, b in zip(starts, starts[1:]):
            msg = "".join(lines[a:b]).encode("ascii")
            total = sum(sizes[a:b])
            assert total < U64, "node size overflows 64 bits"
            if rule == "early_flush64" and len(msg) % 64 == 0:
                msg += b"\0"  # stands for a last block compressed without its end flags
            nh.append(C.internal_node_hash(msg))
            ns.append(total)
            msg_lens.append(len(msg))
        if stats is not None:
            # lines whose " : size\n" tail [t0, t1) crosses a 64-byte boundary of their message
            ll = np.fromiter(map(len, lines), dtype=np.int64, count=n)
            end = np.cumsum(ll)
            base = np.repeat((end - ll)[starts[:-1]], np.diff(starts))
            t0, t1 = end - ll - base + 64, end - base
            tail_straddles = int(((t0 // 64 != (t1 - 1) // 64) & (t0 % 64 != 0)).sum())
            stats["levels"].append(level_stats(n, starts, sizes, msg_lens, tail_straddles))
        hashes, sizes = nh, ns
    return C.blake3_keyed(bytes(32), hashes[0]) if file_hash else hashes[0]


def file_hash_of_root(root: bytes, n_leaves: int) -> bytes:
    return C.blake3_keyed(bytes(32), root) if n_leaves else bytes(32)


# ---- seeded families --------------------------------------------------------------------------------
class Case(NamedTuple):
    name: str
    hashes: np.ndarray  # uint8 [n, 32]
    sizes: np.ndarray  # uint64 [n]


def _rng(*key):
    return np.random.default_rng([0x4D4B, *key])


def steer(rng, flags, sizes=None) -> tuple:
    """Random leaves whose cut flags are exactly `flags` (a bool per leaf)."""
    flags = np.asarray(flags, dtype=bool)
    n = len(flags)
    hs = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    low = rng.integers(1, 4, size=n, dtype=np.uint8)  # a cleared flag is any of 1, 2, 3
    hs[:, 24] = (hs[:, 24] & 0xFC) | np.where(flags, 0, low).astype(np.uint8)
    if sizes is None:
        sizes = rng.integers(1, 131073, size=n).astype(np.uint64)
    sizes = np.asarray(sizes, dtype=np.uint64)
    assert sizes.shape == (n,)
    return hs, sizes


def _pattern(rng, n, kind, B=None):
    f = np.zeros(n, dtype=bool)
    if kind == "none":
        pass
    elif kind == "all":
        f[:] = True
    elif kind == "edges":  # only around the thread-block edges t*B - 2 .. t*B + 2
        B = B or max(1, -(-n // THREADS))
        for d in range(-2, 3):
            idx = np.arange(B, n + 3, B) + d
            f[idx[(idx >= 0) & (idx < n)]] = True
    elif kind == "idx01":  # indices 0 and 1 of every would-be group of 9: must be ignored
        f[0::9] = True
        f[1::9] = True
    elif kind.startswith("rand"):
        f = rng.random(n) < {"rand16": 1 / 16, "rand4": 1 / 4, "rand34": 3 / 4}[kind]
    else:
        raise KeyError(kind)
    return f


SHAPE_N = 2500  # B = 3: a group of 9 touches up to four blocks


def family_shape():
    cases = []
    for kind in ("none", "all", "idx01", "rand16", "rand4", "rand34"):
        rng = _rng(1, len(cases))
        cases.append(Case(f"shape_{kind}", *steer(rng, _pattern(rng, SHAPE_N, kind))))
    for period in range(1, 13):
        for phase in range(period):
            rng = _rng(1, 100, period, phase)
            f = np.zeros(SHAPE_N, dtype=bool)
            f[phase::period] = True
            cases.append(Case(f"shape_p{period}_{phase}", *steer(rng, f)))
    for n in (50, SHAPE_N):
        for k in list(range(11)) + [n - 3, n - 2, n - 1]:
            rng = _rng(1, 200, n, k)
            f = np.zeros(n, dtype=bool)
            f[k] = True
            cases.append(Case(f"shape_one_{n}_{k}", *steer(rng, f)))
    return cases


# 4096 is added to the sizes of the issue: it is the only one with B = 4 at the leaf level
BLOCKS_N = (1023, 1024, 1025, 2047, 2048, 2049, 3072, 4096, 4097, 8192, 8193, 9216, 9217, 20480)


def family_blocks():
    cases = []
    for n in BLOCKS_N:
        for kind in ("none", "all", "rand4", "edges"):
            rng = _rng(2, n, len(cases))
            cases.append(Case(f"blocks_{n}_{kind}", *steer(rng, _pattern(rng, n, kind))))
    return cases


def family_tails():
    cases = []
    for n in range(41):
        for kind in ("none", "all", "r1", "r2", "r3"):
            rng = _rng(3, n, len(cases))
            f = rng.random(n) < 0.25 if kind[0] == "r" else _pattern(rng, n, kind)
            cases.append(Case(f"tails_{n}_{kind}", *steer(rng, f)))
    return cases


FLAGWORDS_SMALL = (31, 32, 33, 63, 64, 65, 4095, 4096, 4097)
FLAGWORDS_LARGE = (131071, 131072, 131073, 131104, 131105, 140000)
FLAGWORDS_ALL_N = 393300  # level 1 has 131100 nodes: level 2 keeps its flags in global memory


def family_flagwords():
    """Small cases only; the large ones are built one at a time by flagwords_large()."""
    cases = []
    for n in FLAGWORDS_SMALL:
        rng = _rng(4, n)
        cases.append(Case(f"flagwords_{n}", *steer(rng, rng.random(n) < 0.25)))
    return cases


FLAGWORDS_LARGE_NAMES = tuple(f"flagwords_{n}" for n in FLAGWORDS_LARGE) + (f"flagwords_all_{FLAGWORDS_ALL_N}",)


def flagwords_large(name: str) -> Case:
    if name == f"flagwords_all_{FLAGWORDS_ALL_N}":
        rng = _rng(4, FLAGWORDS_ALL_N)
        return Case(name, *steer(rng, np.ones(FLAGWORDS_ALL_N, dtype=bool)))
    n = int(name.split("_")[1])
    assert n in FLAGWORDS_LARGE
    rng = _rng(4, n)
    return Case(name, *steer(rng, rng.random(n) < 0.25))


def _with_digits(rng, d: int, small_lead: bool = False) -> int:
    """A size with exactly d decimal digits (d = 1 includes 0)."""
    if d == 1:
        return int(rng.integers(0, 10))
    lo, hi = 10 ** (d - 1), 10 ** d
    if small_lead or d == 20:
        hi = min(hi, 2 * lo, U64)  # leading digit 1: several of them still sum below 2^64
    return lo + int(rng.integers(0, 1 << 62)) % (hi - lo)


DIGIT_EDGES = ([0] + [v for k in range(1, 20) for v in (10 ** k - 1, 10 ** k)] +
               [2 ** 32 - 1, 2 ** 32, 2 ** 63 - 1, 2 ** 63, 2 ** 64 - 1])


def family_digits():
    cases = []
    # every edge value up to 10^18 in one tree (sum ~2.2e18), in order and reversed
    small = [v for v in DIGIT_EDGES if v <= 10 ** 18]
    for tag, vals in (("up", small), ("down", small[::-1])):
        rng = _rng(5, len(cases))
        cases.append(Case(f"digits_ladder_{tag}", *steer(rng, rng.random(len(vals)) < 0.25, vals)))
    # one large value per tree, at the start, in the middle and at the end, the other leaves 0
    for v in [v for v in DIGIT_EDGES if v > 10 ** 18]:
        for where in (0, 13, 28):
            rng = _rng(5, len(cases))
            vals = [0] * 29
            vals[where] = v
            cases.append(Case(f"digits_{v}_at{where}", *steer(rng, rng.random(29) < 0.25, vals)))
    # node sums that cross a digit boundary from level to level: 1 -> 2 -> 3 digits, 16 -> 17 -> 18
    # (the packed digits move into their second word), 18 -> 19
    for tag, leaf, n in (("9", 9, 300), ("4e15", 4 * 10 ** 15, 300), ("4e17", 4 * 10 ** 17, 40)):
        for kind in ("none", "all", "rand4"):
            rng = _rng(5, len(cases))
            cases.append(Case(f"digits_cross_{tag}_{kind}", *steer(rng, _pattern(rng, n, kind), [leaf] * n)))
    # 19 -> 20 digits: three leaves of 4e18 close a group; its sum 1.2e19 is printed one level up
    rng = _rng(5, len(cases))
    f = np.zeros(9, dtype=bool)
    f[2::3] = True
    cases.append(Case("digits_cross_4e18", *steer(rng, f, [4 * 10 ** 18] * 3 + [0] * 6)))
    # every digit count 1..20 at random, leading digit 1 so that 29 of them cannot overflow
    for d in range(1, 21):
        rng = _rng(5, len(cases))
        vals = [0] * 29
        for i in (0, 7, 8, 28) if d < 20 else (11,):
            vals[i] = _with_digits(rng, d, small_lead=True)
        cases.append(Case(f"digits_d{d}", *steer(rng, rng.random(29) < 0.25, vals)))
    return cases


# (lines, total digits) with 68 * lines + digits == 64 * k
BLOCK64_SHAPES = ((3, 52), (4, 48), (5, 44), (6, 40), (7, 36), (8, 32), (9, 28))


def _split_digits(lines: int, digits: int) -> list:
    return [digits // lines + (i < digits % lines) for i in range(lines)]


def _tail_straddles(ds) -> bool:
    c = 0
    for d in ds:
        if c % 64 != 0 and c // 64 != (c + 3 + d) // 64:
            return True
        c += 4 + d
    return False


def family_block64():
    """Per shape one tree of five level-1 groups of `lines` children (the flag on the last child
    closes each): the exact multiple of 64, one byte short, one byte long, a message in which a
    " : size\\n" tail crosses a 64-byte boundary, and the exact multiple again as the last group."""
    cases = []
    for lines, digits in BLOCK64_SHAPES:
        assert (68 * lines + digits) % 64 == 0
        exact = _split_digits(lines, digits)
        short = _split_digits(lines, digits - 1)
        long_ = _split_digits(lines, digits + 1)
        cross = next(ds for ds in (_split_digits(lines, digits + lines * k) for k in (1, 2, 3)) if _tail_straddles(ds))
        rng = _rng(6, lines)
        vals, flags = [], []
        for ds in (exact, short, long_, cross, exact):
            vals += [_with_digits(rng, d, small_lead=True) for d in ds]
            flags += [False] * (lines - 1) + [True]
        cases.append(Case(f"block64_{lines}_{digits}", *steer(rng, flags, vals)))
        # the exact message alone: a tree of one node, whose only compression is the last one
        rng = _rng(6, lines, 1)
        vals = [_with_digits(rng, d, small_lead=True) for d in exact]
        cases.append(Case(f"block64_{lines}_{digits}_alone", *steer(rng, [False] * lines, vals)))
    return cases


def family_random():
    cases = []
    for seed in range(4):
        rng = _rng(7, seed)
        for hi in (100, 3000, 20000):
            n = int(rng.integers(hi // 2, hi + 1))
            hs = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
            kind = rng.integers(0, 4, size=n)
            sz = np.where(kind == 0, rng.integers(1, 131073, size=n),
                          np.where(kind == 1, rng.integers(1, 10, size=n) * 10 ** rng.integers(0, 14, size=n),
                                   np.where(kind == 2, 0, rng.integers(0, 1 << 40, size=n)))).astype(np.uint64)
            cases.append(Case(f"random{seed}_{n}", hs, sz))
    return cases


FAMILIES = {
    "shape": family_shape,
    "blocks": family_blocks,
    "tails": family_tails,
    "flagwords": family_flagwords,
    "digits": family_digits,
    "block64": family_block64,
    "random": family_random,
}


@functools.lru_cache(maxsize=None)
def family(name: str) -> tuple:
    """The family's cases, built once per process; the arrays are read-only."""
    cases = tuple(FAMILIES[name]())
    assert len({c.name for c in cases}) == len(cases)
    for c in cases:
        assert c.hashes.dtype == np.uint8 and c.hashes.shape == (len(c.sizes), 32) and c.sizes.dtype == np.uint64
        c.hashes.setflags(write=False)
        c.sizes.setflags(write=False)
    return cases


@functools.lru_cache(maxsize=None)
def modelled(name: str) -> tuple:
    """Per case of the family: (root, stats), computed once and shared by every test."""
    out = []
    for c in family(name):
        st = {}
        out.append((merkle_model(leaves_of(c.hashes, c.sizes), stats=st), st))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def modelled_large(name: str) -> tuple:
    """(case, root, stats) of one large flagwords case, once per process."""
    c = flagwords_large(name)
    c.hashes.setflags(write=False)
    c.sizes.setflags(write=False)
    st = {}
    return c, merkle_model(leaves_of(c.hashes, c.sizes), stats=st), st
