"""The plain-Python model of the chunk-header index (tests/index_model.py): its walk equals the host
oracle on real xorb bodies, every error code is reached by a steered run with the expected word and
zeroed tail, the synthesised cases are what they are named for (asserted from `candidates`), and the
sweep holds enough fast-path and short-chain-plus-branch terms -- so the GPU test that compares both
device walks with this model (tests/test_gpu_index.py) is sharp.
"""
from __future__ import annotations

import random

import numpy as np
import pytest

import index_model as M
from zest_amd import _core as C

SENTINEL = 0xEE


def _sentinel(n):
    return np.full(n * M.CHUNK_DTYPE.itemsize, SENTINEL, dtype=np.uint8).view(M.CHUNK_DTYPE)


def test_dtypes_match_the_package():
    from zest_amd import ops  # (imports torch; the model itself does not)

    assert M.TERM_DTYPE == ops.TERM_DTYPE and M.CHUNK_DTYPE == ops.CHUNK_DTYPE


@pytest.mark.parametrize("policy", ["none", "bg4", "auto"])
def test_walk_matches_host_oracle(policy):
    rng = random.Random(5)
    bf16 = (np.random.default_rng(5).standard_normal(100_000).astype(np.float32) * 0.02).view(np.uint32) >> 16
    data = rng.randbytes(250_000) + bf16.astype(np.uint16).tobytes() + b"zest index model line. " * 9000 + bytes(90_000)
    b = C.XorbBuilder(policy)
    prev = 0
    for e in C.chunk_ends(data):
        b.add_chunk(data[prev:e])
        prev = e
    body = b.serialize(False)
    want = C.index_chunks(body)
    assert len(want) == b.num_chunks() > 4
    for lead, ulen in ((0, 0), (13, len(data))):
        src = bytes(lead) + body
        recs, code = M.walk(src, M.Term(lead, len(body), 7, 0, len(want), ulen), t=3)
        assert code == M.OK
        assert recs == [(lead + ho + 8, 7 + uo, cl, ul, sc, 3) for ho, cl, sc, ul, uo in want]
    if policy != "none":
        assert {r[4] for r in recs} - {0}, "no compressed chunk in the body"
    # every chunk of a real body is a candidate: the fast path is the common case
    assert set(M.candidates(body, M.Term(0, len(body), 0, 0, len(want), 0))) >= {w[0] for w in want}


# chunk at which the term fails (None: the final check, the records stay), for malformed_term's runs
FAILS_AT = dict(bad_version=2, scheme_3=2, raw_clen_ne_ulen=2, clen_past_run=2, capacity=2, past_term_ulen=4,
                one_too_few=5, one_too_many=None, trailing_bytes=None, zero_chunks=None)


@pytest.mark.parametrize("kind", M.MALFORMED)
def test_error_codes_and_zeroed_tail(kind):
    rng = np.random.default_rng(17)
    run, kw = M.malformed_term(kind, rng)
    s = M.Source(rng, lead=9, chunk_base=3, dst=100)
    s.add(M.Run([M.raw(10)], rng))
    t = s.add(run, **kw)
    c = s.case(kind)
    tm = M.as_term(c.terms[t])
    recs, code = M.walk(c.src, tm, t)
    assert code == M.MALFORMED_CODE[kind]
    assert len(recs) == tm.n_chunks
    zero = (0, 0, 0, 0, 0, t)
    if code == M.OK:
        assert zero not in recs and [r[0] - 8 - tm.src for r in recs] == run.hdrs
    else:
        k = FAILS_AT[kind]
        written = recs if k is None else recs[:k]
        assert [r[0] - 8 - tm.src for r in written] == run.hdrs[:len(written)]
        assert k is None or (recs[k:] == [zero] * (tm.n_chunks - k) and tm.n_chunks > k)
    out, words = M.index(c.src, c.terms, _sentinel(c.n_records))
    assert words == ({code << 32 | t} if code else set())
    used = np.zeros(c.n_records, dtype=bool)
    for x in c.terms:
        used[int(x["chunk_base"]):int(x["chunk_base"] + x["n_chunks"])] = True
    assert (out[~used].view(np.uint8) == SENTINEL).all() and (~used).sum() >= 3
    assert out[used].tolist() == M.walk(c.src, c.terms[0], 0)[0] + recs
    # the valid runs the scan cannot list must not look listable
    if kind in ("zero_length_raw", "no_magic"):
        assert run.hdrs[2] not in M.candidates(c.src, tm) and M.link_choice(c.src, tm) is None


def test_the_construction():
    for ulen in (0, 858):
        c = M.the_construction(ulen)
        tm = M.as_term(c.terms[0])
        assert tm.n_chunks == 4 and tm.ulen == ulen and tm.src_len == 534
        assert M.candidates(c.src, tm) == [0, 28, 52, 408, 466]
        recs, code = M.walk(c.src, tm)
        assert code == M.ERR_COUNT
        assert recs == [(8, 0, 400, 400, 0, 0), (416, 400, 50, 50, 0, 0), (474, 450, 60, 60, 0, 0), (0, 0, 0, 0, 0, 0)]
        assert M.index(c.src, c.terms, _sentinel(c.n_records))[1] == {M.ERR_COUNT << 32}
        # what tells the link rules apart: any candidate's successor counts -> A, Y, B, C
        assert M.link_choice(c.src, tm, "pointed") == [0, 52, 408, 466]
        assert M.link_choice(c.src, tm, "chain") is None


def test_synthesiser_refuses_real_headers():
    rng = np.random.default_rng(1)
    run = M.Run([M.raw(100), M.raw(50)], rng)
    for pos in (0, 7, 101, 108, 115, len(run) - 7):
        with pytest.raises(ValueError):
            run.plant(pos, 3)
    with pytest.raises(ValueError):
        run.plant_chain(20, [75], to=len(run))  # the second look-alike would lie over the header at 108
    assert bytes(run.buf)[108:116] == M.header(0, 50, 50)
    run = M.Run([M.raw(100), M.raw(50)], rng)
    assert run.plant(8, 5) == 21 and run.plant_chain(40, [4, 6], to=108) == [40, 52, 66]
    assert M.candidates(bytes(run.buf), M.Term(0, len(run), 0, 0, 2, 0)) == [0, 8, 40, 52, 66, 108]
    # filler never holds a header
    assert 0 not in M.filler(rng, 50_000)
    s = M.Source(rng, lead=10)
    s.add_at(run, 1, 4096 - 3)
    assert s.terms[0][0] + run.hdrs[1] == 4093 and s.buf[4093:4101] == M.header(0, 50, 50)


ALL_CASES = ([(g, n) for g in M.GROUPS for n in M.case_names(g)]
             + [("sort", n) for n in M.SORT_SIZES] + [("sweep", i) for i in range(M.SWEEP_LAUNCHES)]
             + [("malformed", (k, w)) for k in M.MALFORMED for w in (0, 2, 4)] + [("descending", 0)])


def get_case(grp, key) -> M.Case:
    if grp == "sort":
        return M.sort_case(key)
    if grp == "sweep":
        return M.sweep_case(key)
    if grp == "malformed":
        return M.malformed_case(*key)
    if grp == "descending":
        return M.descending_case()
    return M.by_name(grp, key)


@pytest.mark.parametrize("grp,key", ALL_CASES, ids=lambda x: str(x).replace(" ", ""))
def test_cases_are_what_they_claim(grp, key):
    """Per term of every GPU case: the stated path follows from the candidates; a sound link rule
    never picks anything but the walk's own chain; records of different terms do not overlap; the
    launch is small."""
    c = get_case(grp, key)
    assert len(c.src) <= 160 << 10
    used = np.zeros(c.n_records, dtype=bool)
    failing = 0
    for t, term in enumerate(c.terms):
        tm = M.as_term(term)
        assert tm.src + tm.src_len <= len(c.src)
        assert not used[tm.chunk_base:tm.chunk_base + tm.n_chunks].any()
        used[tm.chunk_base:tm.chunk_base + tm.n_chunks] = True
        recs, code = M.walk(c.src, tm, t)
        failing += code != 0
        pick = M.link_choice(c.src, tm)
        if pick is not None:
            assert code == M.OK and pick == [r[0] - 8 - tm.src for r in recs], (c.name, t)
        if c.fast[t] is True:
            assert M.dead_ends(c.src, tm) and pick is not None, (c.name, t)
        elif c.fast[t] is False and grp != "descending":
            assert pick is None, (c.name, t)
    assert (~used).sum() >= 3
    if grp != "sweep":
        assert failing <= 1, "one failing term per launch: the device keeps the first word it sees"
    if grp == "malformed":
        assert failing == (M.MALFORMED_CODE[key[0]] != M.OK)


@pytest.mark.parametrize("n", M.SORT_SIZES)
def test_sort_cases_have_n_candidates(n):
    c = M.sort_case(n)
    assert len(M.candidates(c.src, c.terms[0])) == n == int(c.terms[0]["n_chunks"])
    assert c.fast == ((n <= M.CAND_CAP),)


def test_seams_are_hit():
    at = set()
    for c in M.group("seams"):
        for t, term in enumerate(c.terms):
            at |= {int(term["src"]) + p for p in M.chain_offsets(c.src, term)}
    for seam in (64 * 37, M.SCAN_BLOCK, 2 * M.SCAN_BLOCK):
        assert {seam - 8 + j for j in range(9)} <= at
    c = M.by_name("seams", "last_chunk_1_to_4_bytes")
    assert [int(x["src_len"]) - M.chain_offsets(c.src, x)[-1] for x in c.terms] == [9, 10, 11, 12]
    c = M.by_name("clean", "every_residue")
    assert sorted(int(x["src"]) % 64 for x in c.terms) == list(range(64))
    c = M.by_name("clean", "terms_packed_in_a_slice")
    assert [int(x["src"]) for x in c.terms[:5]] == [195 + 9 * i for i in range(5)] and 195 % 64 == 3


def test_lookalike_cases_hold_their_lookalikes():
    want_extra = {"lone": 3, "chain_of_two": 2, "points_at_real": 1, "point_at_end": 2, "crosses_end_8": 0,
                  "crosses_end_4": 0}
    for c in M.group("lookalikes"):
        tm = M.as_term(c.terms[1])
        extra = set(M.candidates(c.src, tm)) - set(M.chain_offsets(c.src, tm))
        assert len(extra) == want_extra[c.name], c.name
        assert M.walk(c.src, tm, 1)[1] == M.OK
    c = M.by_name("clean", "headers_in_gaps")
    for term in c.terms:  # the headers in the gaps are headers, and no term's
        assert M.candidates(c.src, term) == M.chain_offsets(c.src, term)
    assert c.src.count(M.header(0, 30, 30)) == 1 and c.src[9:17] == M.header(0, 20, 20)


def test_branch_cases_defeat_the_pointed_rule():
    for c in M.group("branches"):
        bad = [t for t, x in enumerate(c.terms) if M.walk(c.src, x, t)[1]]
        assert len(bad) == 1, c.name
        t = bad[0]
        assert M.walk(c.src, c.terms[t], t)[1] == M.ERR_COUNT
        assert M.link_choice(c.src, c.terms[t], "pointed") is not None, c.name
        assert M.link_choice(c.src, c.terms[t], "chain") is None, c.name


def test_sweep_conditions():
    """At least a quarter of the sweep's terms must keep the fast path and at least 20 are short
    chains whose count a side branch makes up (the walk says COUNT, the unsound rule accepts)."""
    kinds = []
    fooled = 0
    deltas = set()
    for i in range(M.SWEEP_LAUNCHES):
        c = M.sweep_case(i)
        assert len(c.terms) == M.SWEEP_TERMS
        kinds += c.kinds
        for t, (term, kind) in enumerate(zip(c.terms, c.kinds)):
            code = M.walk(c.src, term, t)[1]
            whole = M.as_term(term)._replace(n_chunks=100, ulen=0)  # walks the true chain to the run's end
            deltas.add(int(term["n_chunks"]) - len(M.chain_offsets(c.src, whole)))
            if kind == "branch":
                assert code == M.ERR_COUNT
                fooled += M.link_choice(c.src, term, "pointed") is not None
            assert M.link_choice(c.src, term, "chain") is None or code == M.OK
    assert len(kinds) == 200
    assert kinds.count("fast") * 4 >= len(kinds), kinds.count("fast")
    assert kinds.count("branch") >= 20 and fooled >= 20, (kinds.count("branch"), fooled)
    assert deltas >= {-1, 0, 1, 2}
