"""The GPU LZ4 compressor (csrc/gpu/compress.hip: k_bg4_split, k_lz4_compress_v1, k_lz4_compress,
k_pack_frames) against the scalar model of its parse and the strict frame validator
(tests/lz4_compress_model.py): every frame byte for byte, nothing written outside it, a chunk's
frame independent of its neighbours and its index, and the way back through pack_frames and the
ingest path.  tests/test_lz4_compress_cpu.py shows that the families reach the edges they are named
for and that a wrong parse is caught by them.

Marked `gpu`: runs on a real MI355X.
"""
import functools

import numpy as np
import pytest
import torch

import lz4_compress_model as M
import lz4_synth as S
from zest_amd import _core as C
from zest_amd import ops

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FILL = 0x5A
GAP = 0xEE
SPARE = 4  # out_len entries behind the launch's n
FAMILY_NAMES = sorted(M.FAMILIES)
# odd slots: with BG4 the LZ4 stage reads scratch slot i at every address & 3
SLOT_BIG = ops.LZ4_SLOT + 1
SLOT_SMALL = 20 * 1024 + 1
KERNELS = ("default", "v1")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    ops.hip()  # must load: no silent fallback


def _bound(n: int) -> int:
    """Bytes of its slot the compressor may touch for a chunk it reports raw."""
    return n + n // 255 + 32


def _slot_for(chunks) -> int:
    return SLOT_SMALL if max(len(d) for _, d in chunks) <= 16 * 1024 else SLOT_BIG


@functools.lru_cache(maxsize=None)
def _expect(data: bytes, bg4: bool):
    """(the bytes the LZ4 stage sees, the model's frame or None), once per distinct chunk."""
    src = M.bg4_split_np(data) if bg4 else data
    return src, M.compress_model(src)


def _family_chunks(fam):
    return [(c.name, c.data) for c in M.family(fam)]


def _select(monkeypatch, kernel):
    if kernel == "v1":
        monkeypatch.setenv("ZG_COMPRESS", "v1")
    else:
        monkeypatch.delenv("ZG_COMPRESS", raising=False)


def _dev(buf) -> torch.Tensor:
    t = torch.empty(len(buf), dtype=torch.uint8, device=DEV)
    t.copy_(torch.frombuffer(bytearray(buf), dtype=torch.uint8))
    assert t.data_ptr() % 4 == 0
    return t


class Launch:
    """One zg_compress_chunks call through the raw binding over buffers the test owns, every one
    pre-filled with a sentinel.  Chunk i starts at an address with (address & 3) == (i + rot) % 4."""

    def __init__(self, chunks, bg4, rot=0, slot=None, n=None):
        self.chunks = chunks
        self.bg4 = bg4
        self.n = len(chunks) if n is None else n
        self.slot = slot or _slot_for(chunks)
        assert all(_bound(len(d)) <= self.slot and len(d) <= M.MAX_CHUNK for _, d in chunks)
        src = bytearray()
        offs = []
        for i, (_, d) in enumerate(chunks):
            src += bytes([GAP]) * ((((i + rot) % 4) - len(src)) % 4)
            offs.append(len(src))
            src += d
        src += bytes([GAP]) * (3 + ops.PAD)
        self.src_host = bytes(src)
        self.offs = np.array(offs, dtype=np.uint64)
        self.lens = np.array([len(d) for _, d in chunks], dtype=np.uint32)
        self.src = _dev(src)
        if len(chunks) >= 4:
            assert {(self.src.data_ptr() + int(o)) & 3 for o in offs} == {0, 1, 2, 3}
        rows = max(1, len(chunks))
        self.frames = torch.full((rows * self.slot + ops.PAD,), FILL, dtype=torch.uint8, device=DEV)
        self.scratch = torch.full((rows * self.slot + ops.PAD if bg4 else 64,), FILL, dtype=torch.uint8, device=DEV)
        self.out_len = torch.full((4 * (len(chunks) + SPARE),), FILL, dtype=torch.uint8, device=DEV)
        self.offs_d = torch.from_numpy(self.offs.view(np.int64).copy()).to(DEV)
        self.lens_d = torch.from_numpy(self.lens.view(np.int32).copy()).to(DEV)

    def run(self):
        ops.hip().compress_chunks(self.src.data_ptr(), self.offs_d.data_ptr(), self.lens_d.data_ptr(), self.n,
                                  int(self.bg4), self.scratch.data_ptr(), self.slot, self.frames.data_ptr(), self.slot,
                                  self.out_len.data_ptr(), M.header_checksum(0x40), M.header_checksum(0x50),
                                  torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        self.h_frames = self.frames.cpu().numpy()
        self.h_scratch = self.scratch.cpu().numpy()
        self.h_len = self.out_len.cpu().numpy().view(np.uint32)
        self.h_src = self.src.cpu().numpy().tobytes()
        return self

    def frame(self, i) -> bytes:
        return self.h_frames[i * self.slot:i * self.slot + int(self.h_len[i])].tobytes()

    def check(self, tag=""):
        """Frames equal the model's and pass the validator; nothing else is written."""
        n, slot = self.n, self.slot
        assert self.h_src == self.src_host, (tag, "the source buffer changed")
        assert (self.h_len[n:] == 0x5A5A5A5A).all(), (tag, "out_len written past n", self.h_len[n:].tolist())
        for i, (name, d) in enumerate(self.chunks[:n]):
            src, want = _expect(d, self.bg4)
            flen = int(self.h_len[i])
            row = self.h_frames[i * slot:(i + 1) * slot]
            assert flen == (len(want) if want is not None else 0), (tag, name, flen, want and len(want))
            if want is not None:
                got = row[:flen].tobytes()
                if got != want:
                    diff = next(k for k in range(flen) if got[k] != want[k])
                    raise AssertionError((tag, name, f"frame differs from the model's at byte {diff} of {flen}"))
                assert M.check_frame(got, len(d)) == src, (tag, name)
                assert (row[flen:] == FILL).all(), (tag, name, "bytes written behind the frame")
            else:
                assert (row[_bound(len(d)):] == FILL).all(), (tag, name, "a raw report wrote past its bound")
            if self.bg4:
                srow = self.h_scratch[i * slot:(i + 1) * slot]
                assert srow[:len(d)].tobytes() == src, (tag, name, "BG4 scratch is not the grouped chunk")
                assert (srow[len(d):] == FILL).all(), (tag, name, "scratch written past the chunk")
        assert (self.h_frames[n * slot:] == FILL).all(), (tag, "frames written past slot n")
        if self.bg4:
            assert (self.h_scratch[n * slot:] == FILL).all(), (tag, "scratch written past slot n")
        else:
            assert (self.h_scratch == FILL).all(), (tag, "scratch written without bg4")
        return self


# ---- frames equal the model, nothing else is written --------------------------------------------
@pytest.mark.parametrize("bg4", [False, True], ids=["lz4", "bg4"])
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("fam", FAMILY_NAMES)
def test_frames_equal_model(fam, kernel, bg4, monkeypatch):
    """One launch over the whole family: every out_len and every frame byte is the model's, the GPU
    bytes pass the strict validator, and the slots, the BG4 scratch, out_len past n and the source
    keep their sentinel / their bytes everywhere else."""
    _select(monkeypatch, kernel)
    chunks = _family_chunks(fam)
    rot = (FAMILY_NAMES.index(fam) + (2 if kernel == "v1" else 0)) % 4
    Launch(chunks, bg4, rot=rot).run().check((fam, kernel, bg4))


# ---- a chunk's frame depends on its bytes only --------------------------------------------------
def _pool():
    out = []
    for fam in ("windows", "tail", "chains", "tag_collision"):
        out += [(c.name, c.data) for c in M.family(fam) if len(c.data) <= 16 * 1024]
    return out


# launch size -> where the two target chunks stand: every wave of a block (index % 4), full blocks
# and the partial last one (4 of 5, 69 of 70), the pool's chunks around them
PLACES = {1: (0,), 3: (1, 2), 5: (0, 2, 4), 70: (1, 3, 34, 35, 68, 69)}


@pytest.mark.parametrize("bg4", [False, True], ids=["lz4", "bg4"])
@pytest.mark.parametrize("kernel", KERNELS)
def test_frame_depends_on_chunk_bytes_only(kernel, bg4, monkeypatch):
    """The same chunk as each of a block's four waves, in a block's partial tail and next to
    different neighbours (launches of 1, 3, 5 and 70 chunks) gives the same frame -- the model's;
    a second launch over fresh buffers repeats the first byte for byte; n = 0 touches nothing."""
    _select(monkeypatch, kernel)
    by = {c.name: c.data for c in M.family("staging")}
    targets = [("T_bf16", by["stage_bf16_grouped_16k"]), ("T_lit4097", by["stage_lit4097"])]
    pool = _pool()
    seen = {}
    for k, n in enumerate((1, 3, 5, 70)):
        chunks = [pool[(7 * k + 3 * i) % len(pool)] for i in range(n)]
        for j, at in enumerate(PLACES[n]):
            chunks[at] = targets[(j + k) % 2]
        first = Launch(chunks, bg4, rot=k).run().check((kernel, bg4, n))
        for i, (name, _) in enumerate(chunks):
            if name.startswith("T_"):
                assert seen.setdefault(name, first.frame(i)) == first.frame(i), (name, n, i)
        again = Launch(chunks, bg4, rot=k).run()
        assert np.array_equal(again.h_len, first.h_len), n
        assert np.array_equal(again.h_frames, first.h_frames), n
        assert np.array_equal(again.h_scratch, first.h_scratch), n
    assert set(seen) == {"T_bf16", "T_lit4097"} and all(seen.values())
    Launch(pool[:3], bg4, n=0).run().check((kernel, bg4, "n=0"))
    empty = Launch(pool[:3], bg4, n=0).run()
    assert (empty.h_len == 0x5A5A5A5A).all() and (empty.h_frames == FILL).all() and (empty.h_scratch == FILL).all()


# ---- pack_frames and the way back ---------------------------------------------------------------
def _pack_chunks():
    pick = {"distance": ("dist_65535", "dist_65536"),
            "staging": ("stage_lit4097", "stage_total2048", "stage_zeros_128k", "stage_bf16_grouped_16k"),
            "lengths": ("zeros_1", "zeros_26", "zeros_27", "p3_28", "p7_33", "p7_65537")}
    out = []
    for fam, names in pick.items():
        by = {c.name: c.data for c in M.family(fam)}
        out += [(nm, by[nm]) for nm in names]
    rng = np.random.default_rng(31)
    out.insert(3, ("noise_3001", rng.integers(0, 256, 3001, dtype=np.uint8).tobytes()))
    out.append(("noise_70000", rng.integers(0, 256, 70000, dtype=np.uint8).tobytes()))
    return out


@pytest.mark.parametrize("bg4", [False, True], ids=["scheme1", "scheme2"])
def test_pack_frames_and_ingest_roundtrip(bg4):
    """GPU frames and raw chunks (out_len 0) serialized by ops.pack_frames at offsets 0-3 bytes
    apart are the xorb entries lz4_synth.xorb_body writes, the gaps untouched; ops.ingest_terms over
    them gives the chunks back, with their hashes."""
    chunks = _pack_chunks()
    n = len(chunks)
    la = Launch(chunks, bg4, rot=1).run().check(("pack", bg4))
    flen = la.h_len[:n].astype(np.int64)
    assert (flen == 0).sum() >= 3 and (flen > 0).sum() >= 6
    scheme = np.where(flen > 0, 2 if bg4 else 1, 0).astype(np.uint8)
    ulen = la.lens.copy()
    clen = np.where(flen > 0, flen, ulen).astype(np.uint32)
    addr = np.where(flen > 0, np.uint64(la.frames.data_ptr()) + np.arange(n, dtype=np.uint64) * np.uint64(la.slot),
                    np.uint64(la.src.data_ptr()) + la.offs).astype(np.uint64)
    image = bytearray()
    out_off = []
    for i, (name, d) in enumerate(chunks):
        image += bytes([FILL]) * ((i * 7 + 1) % 4)
        out_off.append(len(image))
        payload = la.frame(i) if flen[i] else d
        image += S.xorb_body([(int(scheme[i]), payload, len(d))])
    image += bytes([FILL]) * 3
    out = ops.padded_empty(len(image), DEV)
    out.fill_(FILL)
    ops.pack_frames(addr, clen, ulen, scheme, np.array(out_off, dtype=np.uint64), out)
    torch.cuda.synchronize()
    got = out.cpu().numpy().tobytes()
    for i, (name, d) in enumerate(chunks):
        a, b = out_off[i], out_off[i] + 8 + int(clen[i])
        assert got[a:a + 8] == bytes(image[a:a + 8]), (name, "header")
        assert got[a + 8:b] == bytes(image[a + 8:b]), (name, "payload")
    assert got == bytes(image), "bytes between the entries changed"
    assert {o & 3 for o in out_off} == {0, 1, 2, 3}
    # the way back: one term per entry (the entries are not adjacent)
    terms = np.zeros(n, dtype=ops.TERM_DTYPE)
    pos = 5
    for i, (name, d) in enumerate(chunks):
        terms[i] = (out_off[i], 8 + int(clen[i]), pos, i, 1, len(d))
        pos += len(d)
    dst = ops.padded_empty(pos + 5, DEV)
    dst.fill_(FILL)
    hashes = torch.zeros((n, 32), dtype=torch.uint8, device=DEV)
    ops.ingest_terms(out, dst, terms, hashes)
    torch.cuda.synchronize()
    back = dst.cpu().numpy().tobytes()
    assert back == bytes([FILL]) * 5 + b"".join(d for _, d in chunks) + bytes([FILL]) * 5
    hh = hashes.cpu().numpy()
    for i, (name, d) in enumerate(chunks):
        assert hh[i].tobytes() == C.chunk_hash(d), name


# ---- the wrapper --------------------------------------------------------------------------------
@pytest.mark.parametrize("bg4", [False, True], ids=["lz4", "bg4"])
def test_wrapper_matches_model_and_validates(bg4):
    chunks = [(c.name, c.data) for c in M.family("tail")] + [(c.name, c.data) for c in M.family("windows")]
    blob = b"".join(d for _, d in chunks)
    lens = [len(d) for _, d in chunks]
    offs = np.cumsum([0] + lens[:-1])
    buf = ops.padded_empty(len(blob), DEV)
    buf.copy_(torch.frombuffer(bytearray(blob), dtype=torch.uint8))
    frames, flen = ops.compress_chunks(buf, offs, lens, bg4=bg4)
    host = frames.cpu().numpy()
    for i, (name, d) in enumerate(chunks):
        src, want = _expect(d, bg4)
        assert int(flen[i]) == (len(want) if want is not None else 0), name
        if want is not None:
            assert host[i * ops.LZ4_SLOT:i * ops.LZ4_SLOT + len(want)].tobytes() == want, name
    with pytest.raises(ValueError):
        ops.compress_chunks(buf, [0], [131073], bg4=bg4)
    big = ops.padded_empty(131073, DEV)
    with pytest.raises(ValueError):
        ops.compress_chunks(big, [0], [131073], bg4=bg4)
    with pytest.raises(ValueError):
        ops.compress_chunks(buf, [len(blob) - 10], [11], bg4=bg4)
    with pytest.raises(ValueError):
        ops.compress_chunks(torch.zeros(4096, dtype=torch.uint8), [0], [100], bg4=bg4)
    f0, l0 = ops.compress_chunks(buf, [], [], bg4=bg4)
    assert len(l0) == 0
