"""The three GPU LZ4/BG4 decoders (csrc/gpu/lz4seq.hip: one-kernel batched, two-kernel records,
producer/consumer pairs) and the ingest path on synthesised frames (tests/lz4_synth.py): frame
features and sequence shapes the project's own encoders never emit.  Expected bytes come from the
synthesiser's byte-at-a-time reference only; tests/test_lz4_synth_cpu.py checks the same cases
against the host decoder and the CPU model, and that each family reaches the path it is named for.

Marked `gpu`: runs on a real MI355X.
"""
import numpy as np
import pytest
import torch

import lz4_synth as S
from zest_amd import _core as C
from zest_amd import ops

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FILL = 0x5A
FAMILY_NAMES = sorted(S.FAMILIES)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    ops.hip()  # must load: no silent fallback


def _want(c, scheme):
    return c.data if scheme == 1 else S.bg4_join_np(c.data)


def _dev(buf) -> torch.Tensor:
    """Host bytes -> a device buffer of exactly that storage (the caller includes the pad)."""
    t = torch.empty(len(buf), dtype=torch.uint8, device=DEV)
    t.copy_(torch.frombuffer(bytearray(buf), dtype=torch.uint8))
    assert t.data_ptr() % 4 == 0
    return t


def _layout(chunks, rot=0):
    """[(scheme, payload, ulen, want or None)] -> (src bytes, chunk records, expected dst image, dst_n).
    Chunk i's payload starts at an address with (address & 3) == (i + rot) % 4, behind its 8-byte
    header and 0-3 bytes of filler; its output starts 3 + i % 5 fill bytes after chunk i - 1's, the
    first at offset 3.  The image is the whole dst storage (pad included): fill wherever no chunk
    lands.  want None: the chunk's own range is left out of the comparison (a malformed chunk)."""
    src = bytearray(b"\xEE" * 5)
    rec = np.zeros(len(chunks), dtype=ops.CHUNK_DTYPE)
    image = bytearray()
    free = []  # [lo, hi) ranges not compared
    for i, (scheme, payload, ulen, want) in enumerate(chunks):
        src += b"\xEE" * ((((i + rot) % 4) - (len(src) + 8)) % 4)
        src += S.xorb_body([(scheme, payload, ulen)])
        image += bytes([FILL]) * (3 + i % 5)
        rec[i] = (len(src) - len(payload), len(image), len(payload), ulen, scheme, 0)
        if want is None:
            free.append((len(image), len(image) + ulen))
            image += bytes([FILL]) * ulen
        else:
            assert len(want) == ulen
            image += want
    image += bytes([FILL]) * 11
    dst_n = len(image)
    image += bytes([FILL]) * ops.PAD
    src_n = len(src)
    src += b"\xEE" * ops.PAD
    assert len(chunks) < 4 or {int(r["src"]) & 3 for r in rec} == {0, 1, 2, 3}
    return bytes(src), src_n, rec, image, dst_n, free


def _first_diff(got, image, rec, names):
    g = np.frombuffer(got, dtype=np.uint8)
    w = np.frombuffer(bytes(image), dtype=np.uint8)
    bad = np.flatnonzero(g != w)
    if bad.size == 0:
        return None
    p = int(bad[0])
    for r, nm in zip(rec, names):
        if int(r["dst"]) <= p < int(r["dst"]) + int(r["ulen"]):
            return f"{bad.size} bytes differ, first at {p} = byte {p - int(r['dst'])} of {nm} (ulen {int(r['ulen'])})"
    return f"{bad.size} bytes differ, first at {p}: fill outside every chunk"


def _run_decoders(src_host, src_n, rec, dst_total, dst_n):
    """All three decoders over one launch each; returns [(name, dst storage bytes, error word)]."""
    H = ops.hip()
    n = len(rec)
    src = _dev(src_host)
    dst = torch.empty(dst_total, dtype=torch.uint8, device=DEV)
    chunks = torch.from_numpy(rec.view(np.uint8).copy()).to(DEV)
    err = torch.zeros(1, dtype=torch.int64, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    dec = ops.DecodeScratch(DEV)
    out = []
    for name in ("batched", "records", "pair"):
        dst.fill_(FILL)
        err.zero_()
        sp, sb = dec.get(n, src_n) if name == "records" else (0, 0)
        H.lz4_decode(src.data_ptr(), src_n, dst.data_ptr(), dst_n, chunks.data_ptr(), n, err.data_ptr(), st, 0, sp, sb,
                     name == "pair")
        torch.cuda.synchronize()
        out.append((name, dst.cpu().numpy().tobytes(), int(err.item())))
    counts = dec.buf[:4 * n].view(torch.int32).cpu().tolist()
    return out, counts


@pytest.mark.parametrize("scheme", [1, 2])
@pytest.mark.parametrize("fam", FAMILY_NAMES)
def test_three_decoders_match_reference(fam, scheme):
    """One launch per decoder over the whole family: error word 0, every chunk byte-exact, every fill
    byte before, between and after the chunks (and in the pad) untouched; payloads at every
    address & 3, outputs misaligned.  (The pair kernel runs its static schedule and decodes BG4 in
    place here; the ingest tests below run it with the dynamic schedule and the staging slice.)"""
    cases = S.family(fam)
    names = [c.name for c in cases]
    src, src_n, rec, image, dst_n, _ = _layout([(scheme, c.frame, len(c.data), _want(c, scheme)) for c in cases],
                                               rot=scheme)
    outs, counts = _run_decoders(src, src_n, rec, len(image), dst_n)
    for name, got, err in outs:
        assert err == 0, (name, hex(err), names[err & 0xFFFFFFFF])
        assert got == bytes(image), (name, _first_diff(got, image, rec, names))
    # the records path really ran: every chunk of >= 256 stored bytes parsed into records
    for c, cnt in zip(cases, counts):
        if len(c.frame) >= 256:
            assert cnt > 0, (c.name, cnt)


@pytest.mark.parametrize("scheme", [1, 2])
@pytest.mark.parametrize("fam", FAMILY_NAMES)
def test_ingest_of_synthesised_run(fam, scheme):
    """The pull engines' path: ops.ingest_terms (device header walk, pair decoder with fused hashing,
    dynamic chunk schedule over the family's unequal chunks, BG4 staging, place/hash pass) over the
    family as one xorb run: bytes, hashes and sizes."""
    cases = S.family(fam)
    n = len(cases)
    body = S.xorb_body([(scheme, c.frame, len(c.data)) for c in cases])
    want = [_want(c, scheme) for c in cases]
    data = b"".join(want)
    src_gap, dst_gap = 5, 7
    src = ops.padded_empty(len(body) + src_gap + 3, DEV)
    src.zero_()
    src[src_gap:src_gap + len(body)].copy_(torch.frombuffer(bytearray(body), dtype=torch.uint8))
    terms = np.zeros(1, dtype=ops.TERM_DTYPE)
    terms[0] = (src_gap, len(body), dst_gap, 0, n, len(data))
    dst = ops.padded_empty(len(data) + 2 * dst_gap, DEV)
    dst.fill_(FILL)
    hashes = torch.zeros((n, 32), dtype=torch.uint8, device=DEV)
    ws = ops.IngestWorkspace(DEV, 1, n)
    ops.ingest_terms(src, dst, terms, hashes, ws=ws)
    torch.cuda.synchronize()
    out = dst.cpu().numpy().tobytes()
    pos = dst_gap
    for c, w in zip(cases, want):
        assert out[pos:pos + len(w)] == w, c.name
        pos += len(w)
    assert out[:dst_gap] == bytes([FILL]) * dst_gap and out[pos:] == bytes([FILL]) * dst_gap
    got = hashes.cpu().numpy()
    for i, (c, w) in enumerate(zip(cases, want)):
        assert got[i].tobytes() == C.chunk_hash(w), c.name
    # the same records through the fused ingest with a sizes array
    H = ops.hip()
    hashes2 = torch.zeros((n, 32), dtype=torch.uint8, device=DEV)
    sizes = torch.full((n,), -1, dtype=torch.int64, device=DEV)
    dst.fill_(FILL)
    ws.err.zero_()
    sp, sb = ws.hash_scratch.get(n, len(data))
    H.ingest_chunks(src.data_ptr(), src.numel(), dst.data_ptr(), dst.numel(), ws.chunks.data_ptr(), n, True,
                    ws.err.data_ptr(), hashes2.data_ptr(), sizes.data_ptr(), 0,
                    torch.cuda.current_stream().cuda_stream, sp, sb)
    torch.cuda.synchronize()
    assert int(ws.err.item()) == 0
    assert dst.cpu().numpy().tobytes() == out
    assert torch.equal(hashes2, hashes)
    assert sizes.cpu().tolist() == [len(w) for w in want]


SWITCHES = (("1", "1", "1", "1"), ("1", "0", "1", "1"), ("0", "1", "1", "1"), ("1", "1", "0", "1"), ("1", "1", "1", "0"))


@pytest.mark.parametrize("scheme", [1, 2])
@pytest.mark.parametrize("fam", ["batch_fill", "wide", "frame_shapes"])
def test_ingest_switches_agree(fam, scheme, monkeypatch):
    """ZG_FUSED_HASH, ZG_BG4_STAGE, ZG_PAIR_DYNAMIC, ZG_PAIR_PREFETCH: each switched off in turn gives
    the bytes, hashes and sizes of the default, and those are the reference's."""
    cases = S.family(fam)
    n = len(cases)
    want = [_want(c, scheme) for c in cases]
    src_host, src_n, rec, image, dst_n, _ = _layout([(scheme, c.frame, len(c.data), w) for c, w in zip(cases, want)])
    H = ops.hip()
    src = _dev(src_host)
    chunks = torch.from_numpy(rec.view(np.uint8).copy()).to(DEV)
    base = 3
    st = torch.cuda.current_stream().cuda_stream
    got = {}
    for sw in SWITCHES:
        for k, v in zip(("ZG_FUSED_HASH", "ZG_BG4_STAGE", "ZG_PAIR_DYNAMIC", "ZG_PAIR_PREFETCH"), sw):
            monkeypatch.setenv(k, v)
        dst = torch.full((len(image),), FILL, dtype=torch.uint8, device=DEV)
        hashes = torch.full((n + base, 32), 0x77, dtype=torch.uint8, device=DEV)
        sizes = torch.full((n + base,), -1, dtype=torch.int64, device=DEV)
        err = torch.zeros(1, dtype=torch.int64, device=DEV)
        sp, sb = ops.HashScratch(DEV, ingest=True).get(n, dst_n)
        H.ingest_chunks(src.data_ptr(), src_n, dst.data_ptr(), dst_n, chunks.data_ptr(), n, True, err.data_ptr(),
                        hashes.data_ptr(), sizes.data_ptr(), base, st, sp, sb)
        torch.cuda.synchronize()
        assert int(err.item()) == 0, (sw, hex(int(err.item())))
        out = dst.cpu().numpy().tobytes()
        assert out == bytes(image), (sw, _first_diff(out, image, rec, [c.name for c in cases]))
        got[sw] = (hashes.cpu().numpy(), sizes.cpu().numpy())
    h1, s1 = got[SWITCHES[0]]
    for sw in SWITCHES[1:]:
        assert np.array_equal(got[sw][0], h1) and np.array_equal(got[sw][1], s1), sw
    assert (h1[:base] == 0x77).all() and (s1[:base] == -1).all()
    assert h1[base:].tobytes() == b"".join(C.chunk_hash(w) for w in want)
    assert s1[base:].tolist() == [len(w) for w in want]


@pytest.mark.parametrize("scheme", [1, 2])
@pytest.mark.parametrize("case", S.malformed(), ids=lambda m: m[0])
def test_malformed_frame_is_reported(case, scheme):
    """One malformed chunk among ten good ones: every decoder reports the same word -- the code the
    kernel prescribes and that chunk's index --, decodes every neighbour and writes nothing outside
    the bad chunk's own [dst, dst + ulen)."""
    name, frm, ulen, code = case
    good = S.family("block_tail")[:5] + S.family("frame_shapes")[:5]
    bad_at = 6
    chunks = [(scheme, c.frame, len(c.data), _want(c, scheme)) for c in good]
    chunks.insert(bad_at, (scheme, frm, ulen, None))
    names = [c[3] is None and name or "good" for c in chunks]
    src, src_n, rec, image, dst_n, free = _layout(chunks)
    outs, _ = _run_decoders(src, src_n, rec, len(image), dst_n)
    (lo, hi), = free
    for dec, got, err in outs:
        assert err == (code << 32) | bad_at, (dec, hex(err))
        masked = got[:lo] + bytes(image[lo:hi]) + got[hi:]
        assert masked == bytes(image), (dec, _first_diff(masked, image, rec, names))
    assert len({err for _, _, err in outs}) == 1


# ------------------------------------------------------------------------------------------------
# clipped launches (place_chunks with a window narrower than dst): the one-wave kernel's clipped
# instantiation -- a chunk the window cuts decodes into a slot of the clip scratch, and its part
# inside the window is copied out
# ------------------------------------------------------------------------------------------------
SENTINEL = 0xC3


def _place_clipped(src, src_n, rec, dst_total, dst_n, lo, hi):
    """One clipped place_chunks launch into FILL-ed storage; returns (dst storage bytes, error word)."""
    H = ops.hip()
    dst = torch.full((dst_total,), FILL, dtype=torch.uint8, device=DEV)
    chunks = torch.from_numpy(rec.view(np.uint8).copy()).to(DEV)
    err = torch.zeros(1, dtype=torch.int64, device=DEV)
    scratch = torch.full((H.CLIP_SCRATCH_BYTES,), SENTINEL, dtype=torch.uint8, device=DEV)
    H.place_chunks(src.data_ptr(), src_n, dst.data_ptr(), dst_n, chunks.data_ptr(), len(rec), lo, hi, err.data_ptr(),
                   torch.cuda.current_stream().cuda_stream, scratch.data_ptr())
    torch.cuda.synchronize()
    return dst.cpu().numpy().tobytes(), int(err.item())


def _clipped_image(image, lo, hi):
    return bytes([FILL]) * lo + bytes(image[lo:hi]) + bytes([FILL]) * (len(image) - hi)


def _windows(rec):
    """The clip windows of test_clipped_place_matches_reference, from the chunk records."""
    at = [int(r["dst"]) for r in rec]
    ul = [int(r["ulen"]) for r in rec]
    n = len(rec)
    inner = [i for i in range(1, n - 1) if ul[i] >= 3]  # chunks with a byte strictly inside
    a, b = inner[0], inner[-1]
    big = max(range(n), key=lambda i: ul[i])
    mid = inner[len(inner) // 2]
    assert a < b and ul[big] >= 16 and at[mid] - (at[mid - 1] + ul[mid - 1]) >= 3
    return {
        "two_cut": (at[a] + ul[a] // 2, at[b] + (ul[b] + 1) // 2),        # both slots in one launch
        "one_cut_twice": (at[big] + ul[big] // 3, at[big] + ul[big] - ul[big] // 5),
        "one_byte": (at[mid] + ul[mid] - 2, at[mid] + ul[mid] - 1),
        "on_chunk_edges": (at[a], at[b] + ul[b]),                        # a clipped launch, no chunk cut
        "in_gap": (at[mid] - 2, at[mid]),                                # nothing is written
    }


WINDOW_NAMES = ("two_cut", "one_cut_twice", "one_byte", "on_chunk_edges", "in_gap")
_clip_inputs = {}


def _clip_input(fam, scheme):
    """The family's layout and its device source, built once per (family, scheme) and not modified."""
    if (fam, scheme) not in _clip_inputs:
        cases = S.family(fam)
        src, src_n, rec, image, dst_n, _ = _layout([(scheme, c.frame, len(c.data), _want(c, scheme)) for c in cases],
                                                   rot=scheme)
        _clip_inputs[fam, scheme] = (_dev(src), src_n, rec, bytes(image), dst_n, [c.name for c in cases])
    return _clip_inputs[fam, scheme]


@pytest.mark.parametrize("window", WINDOW_NAMES)
@pytest.mark.parametrize("scheme", [1, 2])
@pytest.mark.parametrize("fam", ["frame_shapes", "wide", "ring"])
def test_clipped_place_matches_reference(fam, scheme, window):
    """A clipped launch over the whole family: error word 0, dst[lo:hi] byte-exact, every byte outside
    [lo, hi) (pad included) untouched.  frame_shapes: multi-block frames, stored blocks, checksums;
    wide: long batches and wide literal copies into a slot, BG4 group boundaries, the 131072-byte chunk
    that fills a slot; ring: far sources read back from a slot."""
    src, src_n, rec, image, dst_n, names = _clip_input(fam, scheme)
    lo, hi = _windows(rec)[window]
    assert 0 < lo < hi < dst_n
    if window == "one_cut_twice" and fam == "wide":
        assert hi - lo > 60000 and max(int(r["ulen"]) for r in rec) == 131072
    got, err = _place_clipped(src, src_n, rec, len(image), dst_n, lo, hi)
    assert err == 0, (hex(err), names[err & 0xFFFFFFFF])
    want = _clipped_image(image, lo, hi)
    assert got == want, _first_diff(got, want, rec, names)


@pytest.mark.parametrize("scheme", [1, 2])
@pytest.mark.parametrize("case", S.malformed(), ids=lambda m: m[0])
def test_clipped_malformed_is_reported(case, scheme):
    """The layout of test_malformed_frame_is_reported under a window that cuts the bad chunk at lo (and
    the last chunk at hi): the error word is the unclipped decoders', the good neighbours inside the
    window are exact, and nothing else is written -- a cut chunk that fails is not copied out of its
    slot, so not even the bad chunk's own range."""
    name, frm, ulen, code = case
    good = S.family("block_tail")[:5] + S.family("frame_shapes")[:5]
    bad_at = 6
    chunks = [(scheme, c.frame, len(c.data), _want(c, scheme)) for c in good]
    chunks.insert(bad_at, (scheme, frm, ulen, None))
    names = [c[3] is None and name or "good" for c in chunks]
    src, src_n, rec, image, dst_n, _ = _layout(chunks)
    lo = int(rec[bad_at]["dst"]) + ulen // 2
    hi = int(rec[-1]["dst"]) + max(1, int(rec[-1]["ulen"]) // 2)
    assert int(rec[bad_at]["dst"]) < lo < int(rec[bad_at]["dst"]) + ulen
    got, err = _place_clipped(_dev(src), src_n, rec, len(image), dst_n, lo, hi)
    assert err == (code << 32) | bad_at, hex(err)
    want = _clipped_image(image, lo, hi)  # (the image holds FILL over the bad chunk's range)
    assert got == want, _first_diff(got, want, rec, names)
