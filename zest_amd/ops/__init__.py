"""Torch-facing wrappers of the HIP/CDNA4 kernels (zest_amd._hip) with CPU oracles.

Every op validates shapes, dtypes, devices and buffer padding on the host BEFORE launching, so a
bad descriptor can never become an out-of-bounds GPU access.  GPU tensors always take the HIP path
(there is no silent eager fallback: if the extension is missing on a GPU box the import raises);
CPU tensors take the C++ host oracle in zest_amd._core, which is what the gloo/CPU tests use.

Kernel map: K1 hash_ranges/hash_placed, K2 merkle_roots, K3+K4 ingest_terms,
K5 cdc_candidates, K7 pack_chunks, K9 serve_pack, K10 slice_gather, K11 slice_gather_peers,
K12 reuse_chunks, K13 dedup_chunks, K15 slice_scatter, K16 slice_scatter_cast.
"""
from __future__ import annotations

import functools
import os
from dataclasses import dataclass

import numpy as np
import torch

from .. import _core

PAD = 4096  # bytes every device buffer must have past its logical end (kernels read whole lines)

TERM_DTYPE = np.dtype([("src", "<u8"), ("src_len", "<u8"), ("dst", "<u8"), ("chunk_base", "<u4"),
                       ("n_chunks", "<u4"), ("ulen", "<u8")])
CHUNK_DTYPE = np.dtype([("src", "<u8"), ("dst", "<u8"), ("clen", "<u4"), ("ulen", "<u4"),
                        ("scheme", "<u4"), ("term", "<u4")])
MERKLE_JOB_DTYPE = np.dtype([("leaf_base", "<u8"), ("n_leaves", "<u8"), ("want_file_hash", "<u4"),
                             ("pad", "<u4")])

ERR_NAMES = {0: "ok", 1: "bad chunk header", 2: "chunk out of range", 3: "chunk count/size mismatch",
             4: "malformed LZ4", 5: "decoded size mismatch", 6: "hash mismatch", 7: "chunk exceeds capacity"}


class IngestError(RuntimeError):
    def __init__(self, code: int, index: int):
        super().__init__(f"{ERR_NAMES.get(code, code)} at index {index}")
        self.code = code
        self.index = index


@functools.lru_cache(maxsize=1)
def hip():
    """The compiled HIP extension.  Raises (loudly) when it is missing or built for no GPU."""
    from .. import _hip  # noqa: F401  (ImportError propagates: no silent fallback)

    assert _hip.TERM_BYTES == TERM_DTYPE.itemsize, "ZgTerm layout drift"
    assert _hip.CHUNK_BYTES == CHUNK_DTYPE.itemsize, "ZgChunk layout drift"
    assert _hip.MERKLE_JOB_BYTES == MERKLE_JOB_DTYPE.itemsize, "ZgMerkleJob layout drift"
    return _hip


def mem_origin_add(hexes, starts, ptrs, lens) -> int:
    """Serve fetch_info URLs mem://<name>/<xorb hex> from host memory (csrc/core/hub.h): run i is
    bytes [starts[i], starts[i] + lens[i]) of xorb hexes[i], at address ptrs[i] (kept alive by the
    caller).  Registered in both native modules (each links its own host core): _core's host fetches
    and _hip's DeviceXetPull read the same origin."""
    args = (list(hexes), [int(x) for x in starts], [int(x) for x in ptrs], [int(x) for x in lens])
    n = _core.mem_origin_add(*args)
    try:
        from .. import _hip
    except ImportError:
        return n
    _hip.mem_origin_add(*args)
    return n


def mem_origin_clear() -> None:
    _core.mem_origin_clear()
    try:
        from .. import _hip
    except ImportError:
        return
    _hip.mem_origin_clear()


def _stream(device: torch.device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


def padded_empty(nbytes: int, device, pad: int = PAD) -> torch.Tensor:
    """uint8 buffer of `nbytes` logical bytes backed by nbytes + pad of storage."""
    base = torch.empty(nbytes + pad, dtype=torch.uint8, device=device)
    return base[:nbytes]


def vmm_empty(nbytes: int, device, pad: int = PAD, chunk: int = 512 << 20) -> torch.Tensor:
    """Like :func:`padded_empty`, but the storage is a HIP virtual-memory arena built from
    ``chunk``-sized physical allocations that other processes can map (engine.map_peer_arenas
    passes the chunks as dmabuf fds).  Imports of torch allocations of >= 2 GiB through
    hipIpcOpenMemHandle hung on the MI355X box; this path mapped 16 GiB in tens of ms
    (csrc/bind/hip_vmm.cpp)."""
    from torch.utils.dlpack import from_dlpack
    device = torch.device(device)
    if device.type != "cuda":
        raise ValueError("vmm_empty is for GPU arenas")
    m = hip().vmm_alloc(nbytes + pad, device.index if device.index is not None else torch.cuda.current_device(),
                        chunk)
    t = from_dlpack(m.dlpack(nbytes + pad))[:nbytes]
    t._zest_vmm = m  # the DLPack deleter keeps the mapping alive for every view; this finds it
    return t


def vmm_mapping(t: torch.Tensor):
    """The VmmMapping behind a tensor returned by :func:`vmm_empty` (None otherwise)."""
    return getattr(t, "_zest_vmm", None)


def _has_pad(t: torch.Tensor, pad: int = PAD) -> bool:
    st = t.untyped_storage().nbytes()
    end = (t.storage_offset() + t.numel()) * t.element_size()
    return st - end >= pad


def _as_padded_u8(t: torch.Tensor) -> torch.Tensor:
    if t.dtype != torch.uint8:
        t = t.view(torch.uint8) if t.is_contiguous() else t.contiguous().view(torch.uint8)
    t = t.reshape(-1)
    if not t.is_contiguous() or not _has_pad(t):
        p = padded_empty(t.numel(), t.device)
        p.copy_(t)
        t = p
    return t


def _dev_array(a: np.ndarray, device) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).to(device, non_blocking=False)


# ----------------------------------------------------------------------------------------------
# K1: keyed BLAKE3 over (offset, len) ranges
# ----------------------------------------------------------------------------------------------
KEY_DATA, KEY_NODE, KEY_PLAIN, KEY_ZERO = 0, 1, 2, 3


def hash_ranges(buf: torch.Tensor, offsets, lens, key_mode: int = KEY_DATA) -> torch.Tensor:
    """Hash buf[off:off+len] for each range; returns uint8 [n, 32] on buf's device.

    key_mode: 0 Xet chunk (DATA_KEY), 1 Merkle node key, 2 plain BLAKE3, 3 all-zero key."""
    offsets = np.asarray(offsets, dtype=np.uint64)
    lens = np.asarray(lens, dtype=np.uint32)
    n = len(offsets)
    if n == 0:
        return torch.empty((0, 32), dtype=torch.uint8, device=buf.device)
    if np.any(offsets + lens > buf.numel() * buf.element_size()):
        raise ValueError("hash range past end of buffer")
    if buf.device.type != "cuda":
        data = buf.reshape(-1).view(torch.uint8).numpy()
        keys = {KEY_DATA: _core.DATA_KEY, KEY_NODE: _core.INTERNAL_NODE_KEY, KEY_ZERO: bytes(32)}
        out = np.empty((n, 32), dtype=np.uint8)
        for i, (o, l) in enumerate(zip(offsets.tolist(), lens.tolist())):
            mv = data[o:o + l]
            h = _core.blake3(mv) if key_mode == KEY_PLAIN else _core.blake3_keyed(keys[key_mode], mv)
            out[i] = np.frombuffer(h, dtype=np.uint8)
        return torch.from_numpy(out)
    if np.any(lens > 128 * 1024):
        raise ValueError("device hash_ranges supports messages up to 128 KiB")
    H = hip()
    buf = _as_padded_u8(buf)
    offs_d = torch.from_numpy(offsets.view(np.int64).copy()).to(buf.device)
    lens_d = torch.from_numpy(lens.view(np.int32).copy()).to(buf.device)
    out = torch.empty((n, 32), dtype=torch.uint8, device=buf.device)
    sb = H.hash_scratch_bytes(n, int(lens.sum(dtype=np.uint64)))
    scratch = torch.empty(sb, dtype=torch.uint8, device=buf.device)
    H.hash_ranges(buf.data_ptr(), offs_d.data_ptr(), lens_d.data_ptr(), n, out.data_ptr(), key_mode,
                  _stream(buf.device), scratch.data_ptr(), sb)
    return out


class HashScratch:
    """Device scratch of the leaf-flat K1 pipeline (blake3_flat.hip), grown on demand.  Use one per
    stream, and call get() with that stream current: launches on one stream are ordered, so they
    can share the buffer, and when it grows the caching allocator hands the old block only to later
    allocations on that same stream, i.e. after the launches already queued on it."""

    def __init__(self, device, ingest: bool = False):
        self.device = torch.device(device)
        self.buf = None
        self.ingest = ingest  # an ingest launch's scratch (also the decoder's BG4 staging)

    def get(self, n: int, total_bytes: int) -> tuple[int, int]:
        H = hip()
        need = (H.ingest_scratch_bytes if self.ingest else H.hash_scratch_bytes)(int(n), int(total_bytes))
        if self.buf is None or self.buf.numel() < need:
            self.buf = torch.empty(need + (need >> 3), dtype=torch.uint8, device=self.device)
        return self.buf.data_ptr(), self.buf.numel()


class DecodeScratch:
    """Device scratch of the experimental two-kernel LZ4/BG4 decoder (lz4seq.hip k_lz4_parse +
    k_lz4_exec: per-chunk sequence records, 3 bytes per compressed byte), grown on demand; one per
    stream.  Only `hip().lz4_decode(..., rec_scratch=...)` uses it (kbench, tests): the ingest path
    runs the one-kernel batched decoder, which is faster end to end (profiles/lz4_records_r3.md)."""

    def __init__(self, device):
        self.device = torch.device(device)
        self.buf = None

    def get(self, n: int, src_bytes: int) -> tuple[int, int]:
        need = hip().lz4_rec_scratch_bytes(int(n), int(src_bytes))
        if self.buf is None or self.buf.numel() < need:
            self.buf = torch.empty(need + (need >> 3), dtype=torch.uint8, device=self.device)
        return self.buf.data_ptr(), self.buf.numel()


# ----------------------------------------------------------------------------------------------
# K3 + K4: ingest fetched xorb runs into a destination arena, then K1 chunk hashes
# ----------------------------------------------------------------------------------------------
@dataclass
class IngestPlan:
    """Host-side description of a batch of fetched runs, pre-validated against the buffers."""
    terms: np.ndarray  # TERM_DTYPE
    n_chunks: int

    @staticmethod
    def make(terms: np.ndarray) -> "IngestPlan":
        terms = np.ascontiguousarray(terms, dtype=TERM_DTYPE)
        n = int(terms["n_chunks"].sum()) if len(terms) else 0
        if len(terms) and np.any(terms["chunk_base"][1:] < terms["chunk_base"][:-1] + terms["n_chunks"][:-1]):
            raise ValueError("term chunk ranges overlap")
        return IngestPlan(terms, n)


class IngestWorkspace:
    """Reusable device descriptors/error word for repeated ingests on one device (no per-call
    allocation inside the timed loop)."""

    def __init__(self, device, max_terms: int, max_chunks: int):
        self.device = torch.device(device)
        self.max_terms = max_terms
        self.max_chunks = max_chunks
        self.terms = torch.empty(max_terms * TERM_DTYPE.itemsize, dtype=torch.uint8, device=self.device)
        self.chunks = torch.empty(max_chunks * CHUNK_DTYPE.itemsize, dtype=torch.uint8, device=self.device)
        self.err = torch.zeros(1, dtype=torch.int64, device=self.device)
        self.terms_host = torch.empty(max_terms * TERM_DTYPE.itemsize, dtype=torch.uint8).pin_memory() \
            if self.device.type == "cuda" else None
        self._clip_scratch = None
        self.hash_scratch = HashScratch(self.device, ingest=True) if self.device.type == "cuda" else None

    def index_scratch(self, H, n_terms: int) -> tuple[int, int]:
        """(ptr, bytes) of this workspace's parallel header-walk scratch, grown to n_terms."""
        need = H.index_scratch_bytes(max(1, n_terms))
        if getattr(self, "_index_scratch", None) is None or self._index_scratch.numel() < need:
            self._index_scratch = torch.empty(need, dtype=torch.uint8, device=self.device)
        return self._index_scratch.data_ptr(), self._index_scratch.numel()

    def clip_scratch(self) -> int:
        """Device scratch for clipped decodes, private to this workspace (so to its stream)."""
        if self._clip_scratch is None:
            self._clip_scratch = torch.empty(hip().CLIP_SCRATCH_BYTES, dtype=torch.uint8, device=self.device)
        return self._clip_scratch.data_ptr()


FUSED_INGEST = os.environ.get("ZEST_FUSED_INGEST", "1") != "0"


# The parallel header walk is the default (ZEST_INDEX_SCAN=0: the serial walk).  History: it was
# opt-in after it measured slower than the serial walk (gpubench 256 MiB lz4_decode_gpu 3.96 -> 9.69
# ms, profiles/r5/gpubench256_scan_r5c.json): LZ4 streams of BG4 bf16 weights are full of header-like
# byte patterns.  Compressed candidates now need the LZ4 frame magic (millions of candidates -> a
# few), and the link picks the chain from offset 0 out of the candidates (a chain member is offset 0
# or a member's successor) instead of handing any term with a look-alike to the serial walk (which
# every term of a 256 MiB batch had; it still decides whatever is not exactly that chain with the
# planned count): scan 112 us + link 32 us
# against the serial walk's 761 us; lz4_decode_gpu 69.0 -> 85.4 GB/s, xorb_verify_gpu 267 -> 575
# GiB/s; the 70B engine bench is unchanged (64.34 / 64.30 GB/s serial / parallel: the walk is hidden
# under each round's H2D copy either way) (profiles/r5/index_scan_r5ab/).
INDEX_SCAN = os.environ.get("ZEST_INDEX_SCAN", "1") == "1"


def index_terms(H, src_ptr: int, src_n: int, terms_ptr: int, n_terms: int, chunks_ptr: int, err_ptr: int, stream: int,
                ws: "IngestWorkspace | None" = None) -> None:
    """Device header walk of n_terms runs in src[0, src_n) into chunk records (K4).  With a workspace
    for its scratch (and ZEST_INDEX_SCAN not 0): the parallel walk -- candidate-header scan of the
    span, per-term LDS sort/link + prefix sums (csrc/gpu/ingest.hip k_hdr_scan / k_hdr_link), serial
    fallback per term; identical records.  Otherwise one thread per term chases its headers (~0.5 ms
    per 64 MiB run whatever the GPU's width)."""
    if ws is not None and INDEX_SCAN and ws.device.type == "cuda":
        sp, sb = ws.index_scratch(H, n_terms)
        H.index_terms_scan(src_ptr, src_n, terms_ptr, n_terms, chunks_ptr, err_ptr, sp, sb, stream)
        return
    H.index_terms(src_ptr, terms_ptr, n_terms, chunks_ptr, err_ptr, stream)


def ingest_terms(src: torch.Tensor, dst: torch.Tensor, terms: np.ndarray, hashes: torch.Tensor,
                 hash_base: int = 0, clip=None, ws: IngestWorkspace | None = None,
                 check: bool = True, fused: bool | None = None, has_compressed: bool = True) -> None:
    """Decode + place + hash a batch of fetched runs.

    src: uint8 staging buffer holding the runs (padded); dst: uint8 arena (padded).
    terms: TERM_DTYPE records; chunk_base indexes `hashes` (uint8 [N, 32]) relative to hash_base.
    clip: optional (lo, hi) arena byte window this rank owns: bytes outside are not written, and
    the hashes of chunks not entirely inside the window are unspecified.
    LZ4 chunks take the batched decoder (lz4seq.hip); a clipped batch its one-wave clipped kernel.
    fused (default: ZEST_FUSED_INGEST != 0): unclipped batches run decode + one fused place/hash
    pass (zg_ingest_chunks) instead of place then hash; `has_compressed=False` skips the decoder.
    """
    terms = np.ascontiguousarray(terms, dtype=TERM_DTYPE)
    nt = len(terms)
    if nt == 0:
        return
    n_chunks = int((terms["chunk_base"] + terms["n_chunks"]).max())
    src_n = src.numel() * src.element_size()
    dst_n = dst.numel() * dst.element_size()
    if np.any(terms["src"] + terms["src_len"] > src_n):
        raise ValueError("term run past end of src buffer")
    if np.any((terms["ulen"] > 0) & (terms["dst"] + terms["ulen"] > dst_n)):
        raise ValueError("term output past end of dst buffer")
    if np.any(terms["ulen"] == 0):
        raise ValueError("terms must carry their expected uncompressed length")
    if hashes.shape[0] < hash_base + n_chunks or hashes.shape[1] != 32 or hashes.dtype != torch.uint8:
        raise ValueError("hashes buffer too small")
    lo, hi = (0, dst_n) if clip is None else (int(clip[0]), int(clip[1]))
    if src.device.type != "cuda":
        return _ingest_cpu(src, dst, terms, hashes, hash_base, lo, hi)
    H = hip()
    dev = src.device
    if dst.device != dev or hashes.device != dev:
        raise ValueError("src/dst/hashes must share a device")
    src = _as_padded_u8(src)
    if not _has_pad(dst.view(torch.uint8).reshape(-1)):
        raise ValueError("dst arena must be allocated with ops.padded_empty (needs PAD slack)")
    dst8 = dst.view(torch.uint8).reshape(-1)
    if ws is None or ws.max_terms < nt or ws.max_chunks < n_chunks:
        ws = IngestWorkspace(dev, nt, n_chunks)
    st = _stream(dev)
    tbytes = torch.from_numpy(terms.view(np.uint8).copy())
    if ws.terms_host is not None:
        ws.terms_host[: tbytes.numel()].copy_(tbytes)
        ws.terms[: tbytes.numel()].copy_(ws.terms_host[: tbytes.numel()], non_blocking=True)
    else:
        ws.terms[: tbytes.numel()].copy_(tbytes)
    ws.err.zero_()
    ws.chunks[: n_chunks * CHUNK_DTYPE.itemsize].zero_()  # gaps between terms become no-op descriptors
    index_terms(H, src.data_ptr(), src_n, ws.terms.data_ptr(), nt, ws.chunks.data_ptr(), ws.err.data_ptr(), st, ws)
    clipped = lo > 0 or hi < dst_n
    hptr = hashes.data_ptr() + 32 * hash_base
    sp, sb = ws.hash_scratch.get(n_chunks, int(terms["ulen"].sum()))
    if (FUSED_INGEST if fused is None else fused) and not clipped:
        H.ingest_chunks(src.data_ptr(), src_n, dst8.data_ptr(), dst_n, ws.chunks.data_ptr(), n_chunks,
                        has_compressed, ws.err.data_ptr(), hptr, 0, 0, st, sp, sb)
    else:
        H.place_chunks(src.data_ptr(), src_n, dst8.data_ptr(), dst_n, ws.chunks.data_ptr(), n_chunks, lo, hi,
                       ws.err.data_ptr(), st, ws.clip_scratch() if clipped else 0)
        H.hash_chunks(dst8.data_ptr(), dst_n, ws.chunks.data_ptr(), n_chunks, hptr, 0, 0, st, sp, sb)
    if check:
        raise_on_error(ws.err)


def raise_on_error(err: torch.Tensor) -> None:
    v = int(err.item())
    if v:
        raise IngestError(v >> 32, v & 0xFFFFFFFF)


def _ingest_cpu(src, dst, terms, hashes, hash_base, lo, hi):
    s = src.reshape(-1).view(torch.uint8).numpy()
    d = dst.reshape(-1).view(torch.uint8).numpy()
    for t in terms:
        run = s[int(t["src"]): int(t["src"] + t["src_len"])]
        idx = _core.index_chunks(run)
        if len(idx) != int(t["n_chunks"]):
            raise IngestError(3, 0)
        data, hs = _core.extract_chunk_range(run, 0, len(idx), True)
        if len(data) != int(t["ulen"]):
            raise IngestError(3, 0)
        a = int(t["dst"])
        b = a + len(data)
        wa, wb = max(a, lo), min(b, hi)
        if wa < wb:
            d[wa:wb] = np.frombuffer(data, dtype=np.uint8)[wa - a: wb - a]
        base = hash_base + int(t["chunk_base"])
        for i, (h, _) in enumerate(hs):
            hashes[base + i] = torch.from_numpy(np.frombuffer(h, dtype=np.uint8).copy())


def hash_placed(dst: torch.Tensor, chunk_offsets, chunk_lens) -> torch.Tensor:
    """Re-hash chunks already resident in an arena (verify-on-receive)."""
    return hash_ranges(dst, chunk_offsets, chunk_lens, KEY_DATA)


# ----------------------------------------------------------------------------------------------
# K2: Merkle roots / file hashes
# ----------------------------------------------------------------------------------------------
def merkle_roots(hashes: torch.Tensor, sizes: torch.Tensor, jobs, file_hash: bool = True) -> torch.Tensor:
    """jobs: list of (leaf_base, n_leaves). Returns uint8 [n_jobs, 32] roots (file hashes if
    `file_hash`).  hashes: uint8 [N, 32]; sizes: int64 [N]."""
    jobs = list(jobs)
    nj = len(jobs)
    if nj == 0:
        return torch.empty((0, 32), dtype=torch.uint8, device=hashes.device)
    N = hashes.shape[0]
    for b, n in jobs:
        if b < 0 or n < 0 or b + n > N:
            raise ValueError("merkle job out of range")
    if hashes.device.type != "cuda":
        hs = hashes.numpy()
        sz = sizes.to(torch.int64).contiguous().numpy().view(np.uint64)  # the same 64 bits the kernel reads
        out = np.empty((nj, 32), dtype=np.uint8)
        for j, (b, n) in enumerate(jobs):
            leaves = [(hs[i].tobytes(), int(sz[i])) for i in range(b, b + n)]
            r = _core.file_hash(leaves) if file_hash else _core.merkle_root(leaves)
            out[j] = np.frombuffer(r, dtype=np.uint8)
        return torch.from_numpy(out)
    H = hip()
    dev = hashes.device
    rec = np.zeros(nj, dtype=MERKLE_JOB_DTYPE)
    rec["leaf_base"] = [b for b, _ in jobs]
    rec["n_leaves"] = [n for _, n in jobs]
    rec["want_file_hash"] = 1 if file_hash else 0
    jobs_d = _dev_array(rec, dev)
    maxn = max(n for _, n in jobs)
    sb = H.merkle_scratch_bytes(maxn, nj)
    scratch = torch.empty(sb, dtype=torch.uint8, device=dev)
    roots = torch.empty((nj, 32), dtype=torch.uint8, device=dev)
    hashes = hashes.contiguous()
    sizes = sizes.to(torch.int64).contiguous()
    H.merkle(hashes.data_ptr(), sizes.data_ptr(), jobs_d.data_ptr(), nj, roots.data_ptr(), scratch.data_ptr(), sb,
             _stream(dev))
    return roots


# ----------------------------------------------------------------------------------------------
# K5 CDC, K7 pack, synthetic content
# ----------------------------------------------------------------------------------------------
XET_MASK = 0xFFFF << 48


def cdc_candidates(data: torch.Tensor, mask: int = XET_MASK, capacity: int | None = None) -> np.ndarray:
    """Sorted END offsets (i+1) whose 64-byte-window gear hash has (h & mask) == 0."""
    n = data.numel() * data.element_size()
    if data.device.type != "cuda":
        d = data.reshape(-1).view(torch.uint8).numpy().tobytes()
        out = []
        h = 0
        table = _gear_table()
        for i, b in enumerate(d):
            h = ((h << 1) + table[b]) & 0xFFFFFFFFFFFFFFFF
            if h & mask == 0:
                out.append(i + 1)
        return np.asarray(out, dtype=np.uint64)
    H = hip()
    data = _as_padded_u8(data)
    cap = capacity or max(1024, n // 4096)
    out = torch.empty(cap, dtype=torch.int64, device=data.device)
    count = torch.zeros(1, dtype=torch.int64, device=data.device)
    H.cdc_candidates(data.data_ptr(), n, mask, out.data_ptr(), count.data_ptr(), cap, _stream(data.device))
    k = int(count.item())
    if k > cap:
        return cdc_candidates(data, mask, k + 1024)
    return np.sort(out[:k].cpu().numpy().astype(np.uint64))


@functools.lru_cache(maxsize=1)
def _gear_table():
    # Recover the table from the host core (one value per byte via gear_window_hash of 1 byte).
    return [_core.gear_window_hash(bytes([b]), 0) for b in range(256)]


def select_chunks(candidates: np.ndarray, n: int, min_size: int = 8192, max_size: int = 131072) -> np.ndarray:
    """Apply the Xet min/max rule to sorted candidate END offsets -> chunk END offsets."""
    return np.asarray(_core.select_boundaries(np.ascontiguousarray(candidates, dtype=np.uint64), n, min_size,
                                              max_size), dtype=np.uint64)


def fill_synthetic(t: torch.Tensor, seed: int, stream_offset: int = 0, mode: int = 0) -> None:
    """Deterministic synthetic bytes: mode 0 uniform random, mode 1 bf16 ~ N(0, 0.02)."""
    H = hip()
    u8 = t.view(torch.uint8).reshape(-1)
    H.fill_synthetic(u8.data_ptr(), u8.numel(), seed & 0xFFFFFFFFFFFFFFFF, stream_offset, mode, _stream(t.device))


def sha1_info_hash(xorb_hashes: torch.Tensor) -> torch.Tensor:
    """uint8 [n, 32] xorb hashes -> uint8 [n, 20] BitTorrent info-hashes (K6)."""
    n = xorb_hashes.shape[0]
    if xorb_hashes.device.type != "cuda":
        hs = xorb_hashes.numpy()
        return torch.from_numpy(np.stack([np.frombuffer(_core.info_hash(hs[i].tobytes()), dtype=np.uint8)
                                          for i in range(n)]) if n else np.zeros((0, 20), np.uint8))
    src = xorb_hashes.contiguous()
    out = torch.empty((n, 20), dtype=torch.uint8, device=src.device)
    hip().sha1_info_hash(src.data_ptr(), n, out.data_ptr(), _stream(src.device))
    return out


def pack_chunks(data: torch.Tensor, data_off: np.ndarray, lens: np.ndarray, out_off: np.ndarray,
                out: torch.Tensor) -> None:
    """Serialize uncompressed chunks (8-byte header + payload) into `out` at out_off."""
    n = len(lens)
    if n == 0:
        return
    data_n = data.numel()
    out_n = out.numel()
    data_off = np.asarray(data_off, dtype=np.uint64)
    lens = np.asarray(lens, dtype=np.uint32)
    out_off = np.asarray(out_off, dtype=np.uint64)
    if np.any(data_off + lens > data_n) or np.any(out_off + lens + 8 > out_n):
        raise ValueError("pack_chunks range out of bounds")
    if np.any(lens >= (1 << 24)):
        raise ValueError("chunk too large for a u24 header")
    H = hip()
    dev = data.device
    data = _as_padded_u8(data)
    d_off = torch.from_numpy(data_off.view(np.int64).copy()).to(dev)
    d_len = torch.from_numpy(lens.view(np.int32).copy()).to(dev)
    o_off = torch.from_numpy(out_off.view(np.int64).copy()).to(dev)
    H.pack_chunks(data.data_ptr(), d_off.data_ptr(), d_len.data_ptr(), o_off.data_ptr(), n, out.data_ptr(),
                  _stream(dev))


# ----------------------------------------------------------------------------------------------
# K9: serve a byte window of a resident run (decoded chunks at scattered device addresses)
# ----------------------------------------------------------------------------------------------
class ServeRun:
    """A validated resident run: chunk i's decoded bytes sit at address src_addrs[i] (lens[i] bytes)
    inside one of `buffers` (tensors that vouch for the memory; every chunk is checked against them
    before anything is launched).  On a GPU the two tables the kernel reads (addresses, serialized
    ends) are uploaded once and reused by every serve_pack call on the run."""

    def __init__(self, src_addrs, lens, device=None, buffers=()):
        self.src = np.ascontiguousarray(src_addrs, dtype=np.uint64)
        lens64 = np.ascontiguousarray(lens).astype(np.uint64)
        if self.src.ndim != 1 or lens64.shape != self.src.shape or len(self.src) == 0:
            raise ValueError("serve_pack: src_addrs and lens must be equally long, non-empty 1-D arrays")
        if np.any(lens64 >= (1 << 24)):
            raise ValueError("chunk too large for a u24 header")
        buffers = list(buffers)
        if device is None and not buffers:
            raise ValueError("serve_pack: give the device or the buffers the chunks live in")
        self.device = torch.device(device) if device is not None else buffers[0].device
        ok = lens64 == 0
        for t in buffers:
            if t.device != self.device:
                raise ValueError("serve_pack: buffer on another device")
            b0 = np.uint64(t.data_ptr())
            b1 = np.uint64(t.data_ptr() + t.numel() * t.element_size())
            ok |= (self.src >= b0) & (self.src <= b1) & (lens64 <= b1 - np.minimum(self.src, b1))
        if not ok.all():
            raise ValueError("serve_pack: chunk outside every buffer")
        self.lens = lens64
        self.n = len(self.src)
        self.ser_end = np.cumsum(lens64 + np.uint64(8), dtype=np.uint64)
        self.total = int(self.ser_end[-1])
        self.buffers = buffers  # keeps the chunk memory alive
        self.tab = None
        if self.device.type == "cuda":
            tab = np.concatenate([self.src, self.ser_end]).view(np.int64)
            self.tab = torch.from_numpy(tab.copy()).to(self.device)


def serve_pack(src_addrs, lens=None, lo: int = 0, hi: int | None = None, out=None, device=None, buffers=()):
    """Bytes [lo, hi) of the scheme-0 serialized stream (per chunk: 8-byte header + payload) of a
    resident run, written by the K9 kernel (csrc/gpu/serve.hip) from the chunks' decoded bytes.

    src_addrs: chunk addresses (or a ServeRun, which skips validation and the table upload); lens:
    chunk lengths; buffers: the tensors holding the chunks.  out: None (a new device tensor), a
    uint8 tensor on the run's device or in pinned host memory, or (address, nbytes) of
    device-visible memory (ops.hip().host_malloc); 16-byte aligned.  Returns out[:hi - lo] (None for
    a raw address); the launch is asynchronous on the current stream.  CPU runs (host addresses)
    take a NumPy path that produces the same bytes."""
    run = src_addrs if isinstance(src_addrs, ServeRun) else ServeRun(src_addrs, lens, device, buffers)
    lo = int(lo)
    hi = run.total if hi is None else int(hi)
    if not 0 <= lo <= hi <= run.total:
        raise ValueError("serve_pack: window outside the run's serialized stream")
    n = hi - lo
    if run.device.type != "cuda":
        got = torch.from_numpy(_serve_pack_cpu(run, lo, hi))
        if out is None:
            return got
        if not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or out.numel() < n:
            raise ValueError("serve_pack: out must be a uint8 tensor of at least hi - lo bytes")
        out.reshape(-1)[:n].copy_(got)
        return out.reshape(-1)[:n]
    res = None
    if out is None:
        res = torch.empty(max(n, 1), dtype=torch.uint8, device=run.device)[:n]
        ptr = res.data_ptr()
    elif isinstance(out, torch.Tensor):
        if out.dtype != torch.uint8 or not out.is_contiguous() or out.numel() < n:
            raise ValueError("serve_pack: out must be a contiguous uint8 tensor of at least hi - lo bytes")
        if out.device != run.device and not (out.device.type == "cpu" and out.is_pinned()):
            raise ValueError("serve_pack: out must be on the run's device or in pinned host memory")
        res = out.reshape(-1)[:n]
        ptr = out.data_ptr()
        host = out.device.type == "cpu"
    else:
        ptr, cap = int(out[0]), int(out[1])
        host = True  # a raw address is pinned host memory: ask HIP where the device sees it
        if cap < n:
            raise ValueError("serve_pack: out too small")
    if n == 0:
        return res
    if out is not None and host:
        ptr = hip().host_device_pointer(ptr)
    if ptr & 15:
        raise ValueError("serve_pack: out must be 16-byte aligned")
    hip().serve_pack(run.tab.data_ptr(), run.tab.data_ptr() + 8 * run.n, run.n, lo, hi, ptr, _stream(run.device))
    return res


def _serve_pack_cpu(run: ServeRun, lo: int, hi: int) -> np.ndarray:
    import ctypes

    out = np.empty(hi - lo, dtype=np.uint8)
    c = int(np.searchsorted(run.ser_end, lo, side="right"))  # first chunk ending after lo
    while c < run.n:
        e = int(run.ser_end[c])
        ln = int(run.lens[c])
        s = e - ln - 8
        if s >= hi:
            break
        ser = np.empty(ln + 8, dtype=np.uint8)
        ser[:8] = np.frombuffer(bytes([0]) + ln.to_bytes(3, "little") + bytes([0]) + ln.to_bytes(3, "little"), np.uint8)
        if ln:
            ser[8:] = np.frombuffer(ctypes.string_at(int(run.src[c]), ln), dtype=np.uint8)
        a, b = max(lo, s), min(hi, e)
        out[a - lo:b - lo] = ser[a - s:b - s]
        c += 1
    return out


# ----------------------------------------------------------------------------------------------
# K10: gather the kept slices of many tensors out of one file buffer into a compact arena
# ----------------------------------------------------------------------------------------------
SLICE_DTYPE = np.dtype([("src_off", "<u8"), ("run_bytes", "<u8"), ("src_stride", "<u8"), ("n_runs", "<u8"),
                        ("dst_off", "<u8")])
SLICE_ALIGN = 16  # what the kernel relies on for dst and every dst_off (zest_amd.shard hands out 256)


def _check_slice_table(table, src_n: int, dst_n: int, what: str = "slice_gather: ",
                       end: int = 0) -> tuple[np.ndarray, np.ndarray]:
    """Validate a slice table against its buffers; returns (table, output bytes per entry).  `what`
    opens every message; `end` is where the outputs before this table end (slice_gather_peers)."""
    table = np.ascontiguousarray(table, dtype=SLICE_DTYPE).reshape(-1)
    big = lambda f: [int(x) for x in table[f]]  # Python ints: no uint64 wrap-around in the checks
    so, rb, st, nr, do = (big(f) for f in SLICE_DTYPE.names)
    size = []
    for i in range(len(table)):
        n = rb[i] * nr[i]
        size.append(n)
        if n and st[i] < rb[i]:
            raise ValueError(f"{what}entry {i}: src_stride {st[i]} < run_bytes {rb[i]}")
        if n and so[i] + (nr[i] - 1) * st[i] + rb[i] > src_n:
            raise ValueError(f"{what}entry {i}: runs reach past the source ({src_n} bytes)")
        if do[i] % SLICE_ALIGN:
            raise ValueError(f"{what}entry {i}: dst_off {do[i]} is not {SLICE_ALIGN}-byte aligned")
        if do[i] + n > dst_n:
            raise ValueError(f"{what}entry {i}: output reaches past the arena ({dst_n} bytes)")
        if do[i] < end:
            raise ValueError(f"{what}entry {i}: dst_off {do[i]} overlaps or precedes the entry before it")
        end = do[i] + n
    return table, np.asarray(size, dtype=np.uint64)


def slice_gather(src: torch.Tensor, table, dst: torch.Tensor, stream=None) -> None:
    """Copy the kept slices of many tensors out of `src` (uint8, e.g. a verified safetensors file)
    into the compact arena `dst` (uint8): K10, csrc/gpu/shard.hip.

    table: SLICE_DTYPE records.  Entry i is n_runs runs of run_bytes bytes, run r read at
    src_off + r * src_stride, laid end to end at dst_off.  Nothing is checked on the device, so a table
    is refused here (ValueError naming the entry) unless every run lies inside src, every output
    lies inside dst, and the outputs are disjoint, ascending and 16-byte aligned.  Zero-size entries
    are legal.  Only the outputs are written: padding between them keeps its bytes.  GPU tensors: one
    asynchronous launch on `stream` (default: the current stream); CPU tensors: a NumPy path."""
    if src.dtype != torch.uint8 or dst.dtype != torch.uint8 or not src.is_contiguous() or not dst.is_contiguous():
        raise ValueError("slice_gather: src and dst must be contiguous uint8 tensors")
    if src.device != dst.device:
        raise ValueError("slice_gather: src and dst must share a device")
    table, size = _check_slice_table(table, src.numel(), dst.numel())
    n = len(table)
    if n == 0 or not size.any():
        return
    if src.device.type != "cuda":
        return _slice_gather_cpu(src.reshape(-1).numpy(), table, dst.reshape(-1).numpy())
    if dst.data_ptr() % SLICE_ALIGN:
        raise ValueError(f"slice_gather: dst must be {SLICE_ALIGN}-byte aligned")
    H = hip()
    soa = np.empty((H.SLICE_ROWS, n), dtype=np.uint64)
    for k, f in enumerate(SLICE_DTYPE.names):
        soa[k] = table[f]
    soa[5] = table["dst_off"] + size
    if stream is None:
        st = _stream(src.device)
        tab = _dev_array(soa, src.device)
    else:
        st = stream.cuda_stream
        with torch.cuda.stream(stream):  # the table's upload and its free are ordered on the launch's stream
            tab = _dev_array(soa, src.device)
    H.slice_gather(src.data_ptr(), tab.data_ptr(), n, int(soa[5, -1]), dst.data_ptr(), st)


MAX_SLICE_SRCS = 16  # kZgMaxPeerSegs: source bases travel by value in the kernel's arguments


def slice_gather_peers(srcs, tables, dst: torch.Tensor, stream=None, max_blocks: int = 0) -> None:
    """:func:`slice_gather` out of several source buffers in one launch: K11, csrc/gpu/shard_peers.hip
    (a round of the collective sharded pull reads the owners' scratches, its own and its peers').

    srcs: up to 16 contiguous uint8 tensors on dst's device.  tables: one SLICE_DTYPE table per
    source; src_off is relative to that source, dst_off is absolute in `dst` and ascends across the
    concatenation of the tables, so each source owns one range of the arena.  A table may be empty.
    Validation is slice_gather's, per source against that source's length and globally for order,
    disjointness and alignment: a ValueError names the source and the entry before anything is
    launched.  Only the outputs are written.  GPU: one asynchronous launch on `stream` whose blocks
    interleave the sources; `max_blocks` caps the grid (0: the kernel's default of 512, which leaves
    room for the kernels of the next round's pull).  CPU tensors: the NumPy path, source by source."""
    srcs, tables = list(srcs), list(tables)
    if len(srcs) != len(tables):
        raise ValueError(f"slice_gather_peers: {len(srcs)} sources but {len(tables)} tables")
    if len(srcs) > MAX_SLICE_SRCS:
        raise ValueError(f"slice_gather_peers: {len(srcs)} sources, at most {MAX_SLICE_SRCS}")
    if dst.dtype != torch.uint8 or not dst.is_contiguous():
        raise ValueError("slice_gather_peers: dst must be a contiguous uint8 tensor")
    for s, src in enumerate(srcs):
        if src.dtype != torch.uint8 or not src.is_contiguous():
            raise ValueError(f"slice_gather_peers: source {s} must be a contiguous uint8 tensor")
        if src.device != dst.device:
            raise ValueError(f"slice_gather_peers: source {s} is on {src.device}, dst on {dst.device}")
    if int(max_blocks) < 0:
        raise ValueError("slice_gather_peers: max_blocks must be >= 0")
    checked, end = [], 0
    for s, (src, table) in enumerate(zip(srcs, tables)):
        table, size = _check_slice_table(table, src.numel(), dst.numel(), f"slice_gather_peers: source {s} ", end)
        if len(table):
            end = int(table["dst_off"][-1]) + int(size[-1])
        checked.append((table, size))
    if not any(size.any() for _, size in checked):
        return
    if dst.device.type != "cuda":
        d = dst.reshape(-1).numpy()
        for src, (table, _) in zip(srcs, checked):
            _slice_gather_cpu(src.reshape(-1).numpy(), table, d)
        return
    if dst.data_ptr() % SLICE_ALIGN:
        raise ValueError(f"slice_gather_peers: dst must be {SLICE_ALIGN}-byte aligned")
    H = hip()
    n = sum(len(t) for t, _ in checked)
    soa = np.empty((H.SLICE_PEER_ROWS, n), dtype=np.uint64)
    lo, hi, pos = [], [], 0
    for s, (table, size) in enumerate(checked):
        k = len(table)
        for r, f in enumerate(SLICE_DTYPE.names):
            soa[r, pos:pos + k] = table[f]
        ends = table["dst_off"] + size
        soa[5, pos:pos + k] = ends
        soa[6, pos:pos + k] = s
        live = np.flatnonzero(size)  # the source's arena range: its entries with output
        lo.append(int(table["dst_off"][live[0]]) if live.size else 0)
        hi.append(int(ends[live[-1]]) if live.size else 0)
        pos += k
    if stream is None:
        st = _stream(dst.device)
        tab = _dev_array(soa, dst.device)
    else:
        st = stream.cuda_stream
        with torch.cuda.stream(stream):  # the table's upload and its free are ordered on the launch's stream
            tab = _dev_array(soa, dst.device)
    H.slice_gather_peers([src.data_ptr() for src in srcs], lo, hi, tab.data_ptr(), n, int(soa[5, -1]),
                         dst.data_ptr(), int(max_blocks), st)


def _slice_gather_cpu(src: np.ndarray, table: np.ndarray, dst: np.ndarray) -> None:
    for e in table:
        so, rb, st, nr, do = (int(e[f]) for f in SLICE_DTYPE.names)
        if rb == 0 or nr == 0:
            continue
        if nr == 1 or st == rb:
            dst[do:do + rb * nr] = src[so:so + rb * nr]
            continue
        runs = np.lib.stride_tricks.as_strided(src[so:], shape=(nr, rb), strides=(st, 1), writeable=False)
        dst[do:do + rb * nr].reshape(nr, rb)[...] = runs


# ----------------------------------------------------------------------------------------------
# K15: scatter the kept slices of many tensors out of one file buffer to addresses the caller owns
# ----------------------------------------------------------------------------------------------
SCATTER_DTYPE = np.dtype([("src_off", "<u8"), ("run_bytes", "<u8"), ("src_stride", "<u8"), ("n_runs", "<u8"),
                          ("dst_addr", "<u8")])
MAX_SCATTER_ENTRIES = (1 << 32) - 1


def _check_scatter_table(table, src: torch.Tensor, buffers, cast: bool = False) -> tuple[np.ndarray, np.ndarray]:
    """Validate a scatter table against its source and the buffers that vouch for the destinations;
    returns (table, output bytes per entry).  Every message names the entry by its index in `table`.
    cast: a CAST_DTYPE table (K16); its kinds and item multiples are checked first, and everything on
    the destination side is computed on the converted sizes."""
    what = "slice_scatter_cast: " if cast else "slice_scatter: "
    n = table.size if isinstance(table, np.ndarray) else len(table)
    if n > MAX_SCATTER_ENTRIES:  # before anything is copied: the kernel indexes entries with 32 bits
        raise ValueError(f"{what}{n} entries, at most {MAX_SCATTER_ENTRIES}")
    table = np.ascontiguousarray(table, dtype=CAST_DTYPE if cast else SCATTER_DTYPE).reshape(-1)
    so, rb, st, nr, da = ([int(x) for x in table[f]] for f in SCATTER_DTYPE.names)  # Python ints: no wrap-around
    src_n = src.numel()
    size = [rb[i] * nr[i] for i in range(len(table))]
    if cast:
        for i, kind in enumerate(int(x) for x in table["kind"]):
            if kind not in _CAST_ITEMS:
                raise ValueError(f"{what}entry {i}: unknown kind {kind} (ops.CAST_KINDS)")
            si, di = _CAST_ITEMS[kind]
            if rb[i] % si:
                raise ValueError(f"{what}entry {i}: run_bytes {rb[i]} is no multiple of the source item ({si} bytes)")
            size[i] = size[i] // si * di
            if size[i] and da[i] % di:
                raise ValueError(f"{what}entry {i}: dst_addr {da[i]:#x} is no multiple of the destination item "
                                 f"({di} bytes)")
    for i, n in enumerate(size):
        if n and st[i] < rb[i]:
            raise ValueError(f"{what}entry {i}: src_stride {st[i]} < run_bytes {rb[i]}")
        if n and so[i] + (nr[i] - 1) * st[i] + rb[i] > src_n:
            raise ValueError(f"{what}entry {i}: runs reach past the source ({src_n} bytes)")
        if n and da[i] + n > 1 << 64:
            raise ValueError(f"{what}entry {i}: output [{da[i]:#x}, {da[i] + n:#x}) wraps around the address space")
    sizes = np.asarray(size, dtype=np.uint64)
    out = _outside_buffers(table["dst_addr"], sizes, buffers)
    if out.any():
        i = int(np.flatnonzero(out)[0])
        raise ValueError(f"{what}entry {i}: output [{da[i]:#x}, {da[i] + size[i]:#x}) does not lie inside one buffer")
    live = np.flatnonzero(sizes)
    order = live[np.argsort(table["dst_addr"][live], kind="stable")]
    for j, i in zip(order[:-1].tolist(), order[1:].tolist()):
        if da[i] < da[j] + size[j]:
            raise ValueError(f"{what}entry {max(i, j)}: output [{da[max(i, j)]:#x}, "
                             f"{da[max(i, j)] + size[max(i, j)]:#x}) overlaps entry {min(i, j)}'s")
    s0 = src.data_ptr()
    for i in live.tolist():
        if da[i] < s0 + src_n and s0 < da[i] + size[i]:
            raise ValueError(f"{what}entry {i}: output [{da[i]:#x}, {da[i] + size[i]:#x}) overlaps the source")
    return table, sizes


def scatter_soa(table: np.ndarray, size: np.ndarray) -> np.ndarray:
    """The [6][n] block K15 reads: a validated SCATTER_DTYPE table sorted by dst_addr, its fields row
    by row, and the block-prefix row (ZG_SCATTER_BLK_END) that is the kernel's search key."""
    return _scatter_soa(table, size, SCATTER_DTYPE)


def _scatter_soa(table: np.ndarray, size: np.ndarray, dtype: np.dtype) -> np.ndarray:
    order = np.argsort(table["dst_addr"], kind="stable")
    table, size = table[order], size[order]
    soa = np.empty((len(dtype.names) + 1, len(table)), dtype=np.uint64)
    for k, f in enumerate(dtype.names):
        soa[k] = table[f]
    # aligned 16-byte destination blocks per entry: floor(dst / 16) .. ceil((dst + size) / 16); the
    # end is formed from the last byte so that an output ending at 2^64 - 1 does not wrap
    da = table["dst_addr"]
    last = da + np.maximum(size, np.uint64(1)) - np.uint64(1)
    blocks = np.where(size > 0, (last >> np.uint64(4)) - (da >> np.uint64(4)) + np.uint64(1), np.uint64(0))
    soa[-1] = np.cumsum(blocks, dtype=np.uint64)
    return soa


def slice_scatter(src: torch.Tensor, table, buffers, stream=None) -> None:
    """Copy the kept slices of many tensors out of `src` (uint8, e.g. a verified safetensors file) to
    absolute addresses in memory the caller owns: K15, csrc/gpu/scatter.hip.  :func:`slice_gather`
    with the destination anywhere instead of in one arena.

    table: SCATTER_DTYPE records, in any order.  Entry i is n_runs runs of run_bytes bytes, run r read
    at src_off + r * src_stride, laid end to end at the address dst_addr (any alignment).  buffers: the
    tensors that vouch for the destination memory, on src's device (the convention of
    :func:`hash_chunks_at`).  Nothing can be checked on the device against absolute addresses, so a table
    is refused here (ValueError naming the entry, before any launch) unless every run lies inside src,
    every output lies inside the logical range of one tensor of `buffers`, the outputs are pairwise
    disjoint and disjoint from src, and there are at most 2^32 - 1 entries.  Zero-size entries are
    legal; empty and all-zero tables launch nothing.  Only output bytes are written, and no
    destination byte is read: whatever surrounds an output keeps its value, down to the byte.  GPU
    tensors: the table is sorted by dst_addr and uploaded with its block-prefix row as one block, then
    one asynchronous launch on `stream` (default: the current stream); CPU tensors (host addresses): a
    NumPy path with the same contract."""
    if src.dtype != torch.uint8 or not src.is_contiguous():
        raise ValueError("slice_scatter: src must be a contiguous uint8 tensor")
    buffers = list(buffers)
    for k, t in enumerate(buffers):
        if t.device != src.device:
            raise ValueError(f"slice_scatter: buffer {k} is on {t.device}, src on {src.device}")
    table, size = _check_scatter_table(table, src, buffers)
    n = len(table)
    if n == 0 or not size.any():
        return
    if src.device.type != "cuda":
        return _slice_scatter_cpu(src.reshape(-1).numpy(), table)
    H = hip()
    soa = scatter_soa(table, size)
    if stream is None:
        st = _stream(src.device)
        tab = _dev_array(soa, src.device)
    else:
        st = stream.cuda_stream
        with torch.cuda.stream(stream):  # the table's upload and its free are ordered on the launch's stream
            tab = _dev_array(soa, src.device)
    assert soa.shape[0] == H.SCATTER_ROWS, "ZG_SCATTER_ROWS drift"
    H.slice_scatter(src.data_ptr(), tab.data_ptr(), n, int(soa[5, -1]), st)


def _slice_scatter_cpu(src: np.ndarray, table: np.ndarray) -> None:
    import ctypes

    for e in table:
        so, rb, st, nr, da = (int(e[f]) for f in SCATTER_DTYPE.names)
        if rb == 0 or nr == 0:
            continue
        out = np.frombuffer((ctypes.c_ubyte * (rb * nr)).from_address(da), dtype=np.uint8)  # the caller's memory
        if nr == 1 or st == rb:
            out[:] = src[so:so + rb * nr]
            continue
        runs = np.lib.stride_tricks.as_strided(src[so:], shape=(nr, rb), strides=(st, 1), writeable=False)
        out.reshape(nr, rb)[...] = runs


# ----------------------------------------------------------------------------------------------
# K16: K15 with a float conversion on the way (a checkpoint's dtype -> the destinations' dtype)
# ----------------------------------------------------------------------------------------------
CAST_DTYPE = np.dtype(SCATTER_DTYPE.descr + [("kind", "<u8")])
# (stored dtype, destination dtype) by safetensors name -> ZG_CAST_* code
CAST_KINDS = {("F32", "BF16"): 0, ("F32", "F16"): 1, ("BF16", "F32"): 2, ("F16", "F32"): 3, ("BF16", "F16"): 4,
              ("F16", "BF16"): 5}
_CAST_TORCH = {"F32": torch.float32, "F16": torch.float16, "BF16": torch.bfloat16}
_CAST_ITEMS = {code: (_CAST_TORCH[s].itemsize, _CAST_TORCH[d].itemsize) for (s, d), code in CAST_KINDS.items()}


def scatter_cast_soa(table: np.ndarray, size: np.ndarray) -> np.ndarray:
    """The [7][n] block K16 reads: a validated CAST_DTYPE table sorted by dst_addr, its fields row by
    row (kind last), and the block-prefix row (ZG_CAST_BLK_END) over the converted sizes `size`."""
    return _scatter_soa(table, size, CAST_DTYPE)


def check_scatter_cast(src: torch.Tensor, table, buffers) -> tuple[np.ndarray, np.ndarray]:
    """Every refusal of :func:`slice_scatter_cast` without the launch, for a caller that has other
    launches to make first (zest_amd.into): returns (the CAST_DTYPE table, output bytes per entry)."""
    if src.dtype != torch.uint8 or not src.is_contiguous():
        raise ValueError("slice_scatter_cast: src must be a contiguous uint8 tensor")
    buffers = list(buffers)
    for k, t in enumerate(buffers):
        if t.device != src.device:
            raise ValueError(f"slice_scatter_cast: buffer {k} is on {t.device}, src on {src.device}")
    return _check_scatter_table(table, src, buffers, cast=True)


def slice_scatter_cast(src: torch.Tensor, table, buffers, stream=None) -> None:
    """:func:`slice_scatter` with a float conversion on the way: K16, csrc/gpu/scatter_cast.hip.  The
    kept slices of tensors stored in one float dtype go out of `src` (uint8, a verified file in its
    stored dtype) to destinations of another.

    table: CAST_DTYPE records, in any order: slice_scatter's fields, counted in SOURCE bytes, and
    `kind`, a CAST_KINDS code (F32, F16, BF16 to each other).  Entry i writes n_runs * run_bytes /
    source item * destination item bytes at dst_addr.  Round to nearest even in one rounding, overflow
    to infinity, subnormals and signed zeros kept; a NaN stays a NaN with unspecified sign and payload.
    Refused (ValueError naming the entry, before any launch): everything slice_scatter refuses, with
    the destination side computed on the converted sizes; an unknown kind; a run_bytes that is no
    multiple of the source item; a dst_addr that is no multiple of the destination item.  src_off and
    src_stride are arbitrary, so source elements may sit at any byte address.  Only output elements are
    written and no destination byte is read.  Empty and all-zero tables launch nothing.  GPU tensors:
    one sorted upload and one asynchronous launch on `stream`, as slice_scatter; CPU tensors (host
    addresses): torch's own converts, entry by entry."""
    table, size = check_scatter_cast(src, table, buffers)
    n = len(table)
    if n == 0 or not size.any():
        return
    if src.device.type != "cuda":
        return _slice_scatter_cast_cpu(src.reshape(-1).numpy(), table)
    H = hip()
    soa = scatter_cast_soa(table, size)
    if stream is None:
        st = _stream(src.device)
        tab = _dev_array(soa, src.device)
    else:
        st = stream.cuda_stream
        with torch.cuda.stream(stream):  # the table's upload and its free are ordered on the launch's stream
            tab = _dev_array(soa, src.device)
    assert soa.shape[0] == H.CAST_ROWS and len(CAST_KINDS) == H.CAST_KINDS, "ZG_CAST_ROWS drift"
    H.slice_scatter_cast(src.data_ptr(), tab.data_ptr(), n, int(soa[-1, -1]), st)


def _slice_scatter_cast_cpu(src: np.ndarray, table: np.ndarray) -> None:
    import ctypes

    dtypes = {code: (_CAST_TORCH[s], _CAST_TORCH[d]) for (s, d), code in CAST_KINDS.items()}
    for e in table:
        so, rb, st, nr, da, kind = (int(e[f]) for f in CAST_DTYPE.names)
        if rb == 0 or nr == 0:
            continue
        sdt, ddt = dtypes[kind]
        runs = np.lib.stride_tricks.as_strided(src[so:], shape=(nr, rb), strides=(st, 1), writeable=False)
        stored = torch.from_numpy(runs.copy().reshape(-1)).view(sdt)  # an aligned copy of the runs
        conv = stored.to(ddt).view(torch.uint8).numpy()
        out = np.frombuffer((ctypes.c_ubyte * len(conv)).from_address(da), dtype=np.uint8)  # the caller's memory
        out[:] = conv


# ----------------------------------------------------------------------------------------------
# K12: copy + re-hash chunks that are resident on the device under another revision
# ----------------------------------------------------------------------------------------------
REUSE_DTYPE =np.dtype([("src", "<u8"), ("dst", "<u8"), ("len", "<u4"), ("index", "<u4")])
MAX_CHUNK = 128 * 1024


REUSE_LAUNCH_BYTES = 1 << 30  # chunk bytes per launch: bounds the hash scratch (32 B per KiB) of a whole-model table


def _check_reuse(src, lens, offs, index, dst_n: int, rows: int, buffers) -> None:
    """Refuse a reuse table (ValueError naming the record) unless every chunk lies inside one of
    `buffers`, every output inside dst, outputs are pairwise disjoint and indices unique rows.
    src / lens / offs / index: int64-safe uint64 arrays of one length."""
    what = "reuse_chunks: "

    def first(mask):
        return int(np.flatnonzero(mask)[0])

    if (lens > MAX_CHUNK).any():
        i = first(lens > MAX_CHUNK)
        raise ValueError(f"{what}record {i}: len {int(lens[i])} is over the chunk maximum of {MAX_CHUNK} bytes")
    ok = lens == 0
    for t in buffers:  # one buffer must hold all of a chunk: neighbouring buffers do not add up
        b0 = np.uint64(t.data_ptr())
        b1 = np.uint64(t.data_ptr() + t.numel() * t.element_size())
        ok |= (src >= b0) & (src <= b1) & (lens <= b1 - np.minimum(src, b1))
    if not ok.all():
        i = first(~ok)
        raise ValueError(f"{what}record {i}: chunk [{int(src[i]):#x}, {int(src[i] + lens[i]):#x}) lies outside "
                         "every buffer")
    past = (offs > np.uint64(dst_n)) | (lens > np.uint64(dst_n) - np.minimum(offs, np.uint64(dst_n)))
    if past.any():
        i = first(past)
        raise ValueError(f"{what}record {i}: output [{int(offs[i])}, {int(offs[i]) + int(lens[i])}) reaches past dst "
                         f"({dst_n} bytes)")
    live = np.flatnonzero(lens)
    order = live[np.argsort(offs[live], kind="stable")]
    clash = offs[order][1:] < (offs[order] + lens[order])[:-1]
    if clash.any():
        k = first(clash)
        i, j = int(order[k + 1]), int(order[k])
        raise ValueError(f"{what}record {i}: output [{int(offs[i])}, {int(offs[i] + lens[i])}) overlaps record {j}'s")
    if (index >= np.uint64(rows)).any():
        i = first(index >= np.uint64(rows))
        raise ValueError(f"{what}record {i}: index {int(index[i])} is past the table ({rows} rows)")
    order = np.argsort(index, kind="stable")
    dup = index[order][1:] == index[order][:-1]
    if dup.any():
        k = first(dup)
        i, j = int(order[k + 1]), int(order[k])
        raise ValueError(f"{what}record {i}: index {int(index[i])} is also record {j}'s")


def _u64(a, name: str, what: str = "reuse_chunks: ") -> np.ndarray:
    a = np.asarray(a).reshape(-1)
    if a.dtype.kind not in "ui" and len(a):
        raise ValueError(f"{what}{name} must be integers")
    if a.dtype.kind == "i" and (a < 0).any():
        raise ValueError(f"{what}{name} must not be negative")
    return a.astype(np.uint64)


def reuse_chunks(src_addrs, lens, dst: torch.Tensor, dst_offs, hashes: torch.Tensor, hash_index, sizes=None,
                 buffers=(), stream=None) -> None:
    """Copy chunks that already sit in this device's memory into `dst` and re-hash them on the way:
    K12, csrc/gpu/blake3_flat.hip (zg_reuse_chunks).

    Record i copies lens[i] bytes from the absolute address src_addrs[i] (any alignment) to
    dst[dst_offs[i]:], writes their Xet chunk hash to hashes[hash_index[i]] (uint8 [N, 32]) and
    lens[i] to sizes[hash_index[i]] (int64 [N], optional).  Rows no record names and bytes of dst
    outside the outputs keep their values; a zero-length record writes the empty hash.  Nothing can
    be checked on the device against absolute addresses, so a table is refused here (ValueError
    naming the record) unless every chunk lies inside one of `buffers` (the tensors that vouch for
    the memory, on dst's device), every output inside dst, outputs are pairwise disjoint, indices
    are unique rows of the tables and no chunk is over 128 KiB.  GPU tensors: asynchronous on
    `stream` (default: the current stream), one launch per REUSE_LAUNCH_BYTES of chunks, table
    upload and scratch ordered on that stream; CPU tensors (host addresses): a NumPy path with the
    same bytes and hashes."""
    src, lens, offs, index = (_u64(a, k) for a, k in ((src_addrs, "src_addrs"), (lens, "lens"),
                                                      (dst_offs, "dst_offs"), (hash_index, "hash_index")))
    n = len(src)
    if not (len(lens) == len(offs) == len(index) == n):
        raise ValueError("reuse_chunks: src_addrs, lens, dst_offs and hash_index must be equally long")
    if dst.dtype != torch.uint8 or not dst.is_contiguous():
        raise ValueError("reuse_chunks: dst must be a contiguous uint8 tensor")
    if hashes.dtype != torch.uint8 or hashes.dim() != 2 or hashes.shape[1] != 32 or not hashes.is_contiguous():
        raise ValueError("reuse_chunks: hashes must be a contiguous uint8 [N, 32] tensor")
    rows = hashes.shape[0]
    if sizes is not None and (sizes.dtype != torch.int64 or sizes.dim() != 1 or sizes.shape[0] != rows
                              or not sizes.is_contiguous()):
        raise ValueError("reuse_chunks: sizes must be a contiguous int64 [N] tensor as long as hashes")
    dev = dst.device
    for name, t in (("hashes", hashes), ("sizes", sizes)):
        if t is not None and t.device != dev:
            raise ValueError(f"reuse_chunks: {name} is on {t.device}, dst on {dev}")
    buffers = list(buffers)
    for k, t in enumerate(buffers):
        if t.device != dev:
            raise ValueError(f"reuse_chunks: buffer {k} is on {t.device}, dst on {dev}")
    _check_reuse(src, lens, offs, index, dst.numel(), rows, buffers)
    if n == 0:
        return
    if dev.type != "cuda":
        import ctypes

        d = dst.reshape(-1).numpy()
        for a, ln, o, r in zip(src.tolist(), lens.tolist(), offs.tolist(), index.tolist()):
            data = ctypes.string_at(a, ln) if ln else b""
            d[o:o + ln] = np.frombuffer(data, dtype=np.uint8)
            hashes[r] = torch.from_numpy(np.frombuffer(_core.chunk_hash(data), dtype=np.uint8).copy())
            if sizes is not None:
                sizes[r] = ln
        return
    H = hip()
    assert H.REUSE_BYTES == REUSE_DTYPE.itemsize, "ZgReuse layout drift"
    if hashes.data_ptr() % 16:
        raise ValueError("reuse_chunks: hashes must be 16-byte aligned")
    rec = np.empty(n, dtype=REUSE_DTYPE)
    rec["src"], rec["dst"], rec["len"], rec["index"] = src, offs, lens, index
    # launches of at most REUSE_LAUNCH_BYTES: cut where the running byte count passes a multiple of it
    cum = np.cumsum(lens, dtype=np.uint64)
    cuts = [0] + (np.flatnonzero(np.diff(cum // np.uint64(REUSE_LAUNCH_BYTES))) + 1).tolist() + [n]
    parts = [(a, b, int(lens[a:b].sum(dtype=np.uint64))) for a, b in zip(cuts, cuts[1:]) if b > a]
    sb = max(H.hash_scratch_bytes(b - a, tot) for a, b, tot in parts)

    def alloc():
        return _dev_array(rec, dev), torch.empty(sb, dtype=torch.uint8, device=dev)

    if stream is None:
        st = _stream(dev)
        tab, scratch = alloc()
    else:
        st = stream.cuda_stream
        with torch.cuda.stream(stream):  # the uploads and frees are ordered on the launch's stream
            tab, scratch = alloc()
    sz = sizes.data_ptr() if sizes is not None else 0
    for a, b, _ in parts:  # one stream: the launches run in order and share the scratch
        H.reuse_chunks(tab.data_ptr() + a * REUSE_DTYPE.itemsize, b - a, dst.data_ptr(), hashes.data_ptr(), sz,
                       scratch.data_ptr(), sb, st)


# ----------------------------------------------------------------------------------------------
# Chunk hashes at absolute addresses (K12 without the copy) and K14, CDC over a segment list
# ----------------------------------------------------------------------------------------------
HASH_AT_DTYPE = np.dtype([("src", "<u8"), ("len", "<u4"), ("index", "<u4")])
SEG_DTYPE = np.dtype([("addr", "<u8"), ("len", "<u8"), ("vstart", "<u8")])
CDC_WINDOW = 2048  # kSeg in csrc/gpu/synth.hip: bytes of aligned address space per lane


def _outside_buffers(src: np.ndarray, lens: np.ndarray, buffers) -> np.ndarray:
    """Mask of the ranges [src, src + lens) with lens > 0 that lie inside none of `buffers`, in
    O((ranges + buffers) log buffers): with the buffers sorted by start and e[k] the largest end among
    the first k + 1 of them, a range lies inside some buffer exactly when the largest end among the
    buffers that start at or before src reaches src + lens.  Buffers may overlap or alias; two that
    merely touch do not add up."""
    if not len(buffers):
        return lens > 0
    b0 = np.asarray([t.data_ptr() for t in buffers], dtype=np.uint64)
    b1 = b0 + np.asarray([t.numel() * t.element_size() for t in buffers], dtype=np.uint64)
    order = np.argsort(b0, kind="stable")
    b0, b1 = b0[order], np.maximum.accumulate(b1[order])
    k = np.searchsorted(b0, src, side="right")  # buffers that start at or before src
    end = b1[np.maximum(k, 1) - 1]
    inside = (k > 0) & (src <= end) & (lens <= end - np.minimum(src, end))
    return (lens > 0) & ~inside


def hash_chunks_at(src_addrs, lens, hashes: torch.Tensor, hash_index, sizes=None, buffers=(), stream=None) -> None:
    """Hash chunks where they lie: `reuse_chunks` without the copy (zg_hash_chunks_at,
    csrc/gpu/blake3_flat.hip).

    Record i hashes lens[i] bytes at the absolute address src_addrs[i] (any alignment), writes their
    Xet chunk hash to hashes[hash_index[i]] (uint8 [N, 32]) and lens[i] to sizes[hash_index[i]]
    (int64 [N], optional).  Rows no record names keep their values; the source bytes are only read,
    and never past the aligned dwords that hold a byte of the chunk, so a chunk may end on the last
    byte of its allocation.  A table is refused here (ValueError naming the record) unless every chunk
    lies inside one of `buffers` (the tensors that vouch for the memory, on the device of `hashes`),
    indices are unique rows of the tables and no chunk is over 128 KiB.  GPU tensors: asynchronous on
    `stream` (default: the current stream), one launch per REUSE_LAUNCH_BYTES of chunks; CPU tensors
    (host addresses): a NumPy path with the same hashes."""
    what = "hash_chunks_at: "
    src, lens, index = (_u64(a, k, what) for a, k in ((src_addrs, "src_addrs"), (lens, "lens"),
                                                      (hash_index, "hash_index")))
    n = len(src)
    if not (len(lens) == len(index) == n):
        raise ValueError(f"{what}src_addrs, lens and hash_index must be equally long")
    if hashes.dtype != torch.uint8 or hashes.dim() != 2 or hashes.shape[1] != 32 or not hashes.is_contiguous():
        raise ValueError(f"{what}hashes must be a contiguous uint8 [N, 32] tensor")
    rows = hashes.shape[0]
    if sizes is not None and (sizes.dtype != torch.int64 or sizes.dim() != 1 or sizes.shape[0] != rows
                              or not sizes.is_contiguous()):
        raise ValueError(f"{what}sizes must be a contiguous int64 [N] tensor as long as hashes")
    dev = hashes.device
    if sizes is not None and sizes.device != dev:
        raise ValueError(f"{what}sizes is on {sizes.device}, hashes on {dev}")
    buffers = list(buffers)
    for k, t in enumerate(buffers):
        if t.device != dev:
            raise ValueError(f"{what}buffer {k} is on {t.device}, hashes on {dev}")

    def first(mask):
        return int(np.flatnonzero(mask)[0])

    if (lens > MAX_CHUNK).any():
        i = first(lens > MAX_CHUNK)
        raise ValueError(f"{what}record {i}: len {int(lens[i])} is over the chunk maximum of {MAX_CHUNK} bytes")
    out = _outside_buffers(src, lens, buffers)
    if out.any():
        i = first(out)
        raise ValueError(f"{what}record {i}: chunk [{int(src[i]):#x}, {int(src[i] + lens[i]):#x}) lies outside "
                         "every buffer")
    if (index >= np.uint64(rows)).any():
        i = first(index >= np.uint64(rows))
        raise ValueError(f"{what}record {i}: index {int(index[i])} is past the table ({rows} rows)")
    order = np.argsort(index, kind="stable")
    dup = index[order][1:] == index[order][:-1]
    if dup.any():
        k = first(dup)
        i, j = int(order[k + 1]), int(order[k])
        raise ValueError(f"{what}record {i}: index {int(index[i])} is also record {j}'s")
    if n == 0:
        return
    if dev.type != "cuda":
        import ctypes

        for a, ln, r in zip(src.tolist(), lens.tolist(), index.tolist()):
            data = ctypes.string_at(a, ln) if ln else b""
            hashes[r] = torch.from_numpy(np.frombuffer(_core.chunk_hash(data), dtype=np.uint8).copy())
            if sizes is not None:
                sizes[r] = ln
        return
    H = hip()
    assert H.HASH_AT_BYTES == HASH_AT_DTYPE.itemsize, "ZgHashAt layout drift"
    if hashes.data_ptr() % 16:
        raise ValueError(f"{what}hashes must be 16-byte aligned")
    rec = np.empty(n, dtype=HASH_AT_DTYPE)
    rec["src"], rec["len"], rec["index"] = src, lens, index
    cum = np.cumsum(lens, dtype=np.uint64)
    cuts = [0] + (np.flatnonzero(np.diff(cum // np.uint64(REUSE_LAUNCH_BYTES))) + 1).tolist() + [n]
    parts = [(a, b, int(lens[a:b].sum(dtype=np.uint64))) for a, b in zip(cuts, cuts[1:]) if b > a]
    sb = max(H.hash_scratch_bytes(b - a, tot) for a, b, tot in parts)

    def alloc():
        return _dev_array(rec, dev), torch.empty(sb, dtype=torch.uint8, device=dev)

    if stream is None:
        st = _stream(dev)
        tab, scratch = alloc()
    else:
        st = stream.cuda_stream
        with torch.cuda.stream(stream):  # the uploads and frees are ordered on the launch's stream
            tab, scratch = alloc()
    sz = sizes.data_ptr() if sizes is not None else 0
    for a, b, _ in parts:  # one stream: the launches run in order and share the scratch
        H.hash_chunks_at(tab.data_ptr() + a * HASH_AT_DTYPE.itemsize, b - a, hashes.data_ptr(), sz,
                         scratch.data_ptr(), sb, st)


def _flat_u8(t: torch.Tensor) -> torch.Tensor:
    """The bytes of a contiguous tensor as a 1-D uint8 view of the same memory."""
    return t.reshape(-1).view(torch.uint8)


def segment_table(addrs, lens) -> tuple[np.ndarray, np.ndarray]:
    """K14's host tables for segments at `addrs` of `lens` > 0 bytes, in file order: the SEG_DTYPE
    records (vstart = running sum of the lengths) and the prefix count of 2 KiB windows of each
    segment's 16-byte-aligned address space (len + 1 entries, the last is the launch's lane count)."""
    addrs, lens = np.asarray(addrs, dtype=np.uint64), np.asarray(lens, dtype=np.uint64)
    seg = np.empty(len(addrs), dtype=SEG_DTYPE)
    seg["addr"], seg["len"] = addrs, lens
    seg["vstart"] = np.cumsum(lens, dtype=np.uint64) - lens
    wins = ((addrs & np.uint64(15)) + lens + np.uint64(CDC_WINDOW - 1)) // np.uint64(CDC_WINDOW)
    return seg, np.concatenate([np.zeros(1, np.uint64), np.cumsum(wins, dtype=np.uint64)])


def cdc_candidates_segments(segments, mask: int = XET_MASK, capacity: int | None = None, buffers=()) -> np.ndarray:
    """`cdc_candidates` of a file that exists only as a list of segments: K14 (zg_cdc_candidates_segs,
    csrc/gpu/synth.hip).  Sorted END offsets (i + 1), in the coordinates of the concatenation, whose
    gear hash over the concatenated bytes has (h & mask) == 0: the same set `cdc_candidates` gives for
    the packed bytes, for any mask.

    segments: a list of contiguous tensors on one device, each read where it lies (any alignment, no
    pad behind it: loads touch only aligned 16-byte blocks that hold a byte of a segment; zero-element
    tensors are skipped), or `(addrs, lens)` arrays of absolute addresses and lengths > 0 with
    `buffers`, the tensors that vouch for the memory: every segment must lie inside one of them.  One
    table upload, two launches and one count read-back whatever the number of segments; a capacity
    that turns out too small is retried with the count the kernel reported.  CPU tensors are
    concatenated and scanned by `cdc_candidates`' host path."""
    what = "cdc_candidates_segments: "
    if isinstance(segments, tuple) and len(segments) == 2 and not isinstance(segments[0], torch.Tensor):
        addrs, lens = _u64(segments[0], "addrs", what), _u64(segments[1], "lens", what)
        buffers = list(buffers)
        if len(addrs) != len(lens):
            raise ValueError(f"{what}addrs and lens must be equally long")
        if (lens == 0).any():
            raise ValueError(f"{what}segment {int(np.flatnonzero(lens == 0)[0])} is empty: leave empty segments out")
        if not buffers and len(addrs):
            raise ValueError(f"{what}address segments need buffers= that vouch for the memory")
        out = _outside_buffers(addrs, lens, buffers)
        if out.any():
            i = int(np.flatnonzero(out)[0])
            raise ValueError(f"{what}segment {i}: [{int(addrs[i]):#x}, {int(addrs[i] + lens[i]):#x}) lies outside "
                             "every buffer")
        devs = {t.device for t in buffers}
        keep, by_addr = buffers, True
    else:
        segs = list(segments)
        for i, t in enumerate(segs):
            if not isinstance(t, torch.Tensor) or not t.is_contiguous():
                raise ValueError(f"{what}segment {i} must be a contiguous tensor (or pass (addrs, lens) and buffers=)")
        devs = {t.device for t in segs}
        keep, by_addr = [_flat_u8(t) for t in segs if t.numel()], False
        addrs = np.asarray([t.data_ptr() for t in keep], dtype=np.uint64)
        lens = np.asarray([t.numel() for t in keep], dtype=np.uint64)
    if len(devs) > 1:
        raise ValueError(f"{what}segments on more than one device ({', '.join(sorted(map(str, devs)))})")
    if len(addrs) == 0:
        return np.zeros(0, dtype=np.uint64)
    dev = devs.pop()
    if dev.type != "cuda":
        if by_addr:
            import ctypes

            data = b"".join(ctypes.string_at(a, ln) for a, ln in zip(addrs.tolist(), lens.tolist()))
            return cdc_candidates(torch.frombuffer(bytearray(data), dtype=torch.uint8), mask)
        return cdc_candidates(torch.cat(keep), mask)
    H = hip()
    assert H.SEG_BYTES == SEG_DTYPE.itemsize, "ZgSeg layout drift"
    seg, wpre = segment_table(addrs, lens)
    s, n = len(seg), int(lens.sum(dtype=np.uint64))
    # one upload: [segments | window prefix | room for the 64-byte lead-in rows the pre-pass fills]
    host = np.zeros(SEG_DTYPE.itemsize * s + 8 * (s + 1) + 64 * s, dtype=np.uint8)
    host[:SEG_DTYPE.itemsize * s] = seg.view(np.uint8)
    host[SEG_DTYPE.itemsize * s:SEG_DTYPE.itemsize * s + 8 * (s + 1)] = wpre.view(np.uint8)
    with torch.cuda.device(dev):
        tab = torch.from_numpy(host).to(dev)
        p_seg = tab.data_ptr()
        p_pre = p_seg + SEG_DTYPE.itemsize * s
        p_lead = p_pre + 8 * (s + 1)
        cap = capacity or max(1024, n // 4096)
        while True:
            out = torch.empty(cap, dtype=torch.int64, device=dev)
            count = torch.zeros(1, dtype=torch.int64, device=dev)
            H.cdc_candidates_segs(p_seg, p_pre, s, int(wpre[-1]), p_lead, mask, out.data_ptr(), count.data_ptr(), cap,
                                  _stream(dev))
            k = int(count.item())
            if k <= cap:
                break
            cap = k + 1024  # overflow: the kernel counted every candidate, so the retry fits
        del keep  # the segments were alive until the read-back above
        return np.sort(out[:k].cpu().numpy().astype(np.uint64))


# ----------------------------------------------------------------------------------------------
# K13: chunk dedup, a hash join of fresh chunk hashes against an index of known ones
# ----------------------------------------------------------------------------------------------
MAX_DEDUP_ROWS = 1 << 31


def dedup_slots(rows: int) -> int:
    """Slots of K13's table for `rows` rows (index + fresh): the next power of two >= 2 * rows, at
    least 64.  A row's home slot is (little-endian u64 of its hash bytes 0..8) & (slots - 1).  Part
    of the kernel's contract (csrc/gpu/zgpu.h, zg_dedup_slots computes the same number)."""
    rows = int(rows)
    if rows < 0:
        raise ValueError("dedup_slots: rows must not be negative")
    return max(64, 1 << (2 * rows - 1).bit_length()) if rows else 64


def _check_hashes(t, name: str) -> None:
    if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8:
        raise ValueError(f"dedup_chunks: {name} must be a uint8 tensor, got "
                         f"{t.dtype if isinstance(t, torch.Tensor) else type(t).__name__}")
    if t.dim() != 2 or t.shape[1] != 32:
        raise ValueError(f"dedup_chunks: {name} must have shape [k, 32] (one 32-byte hash per row), got "
                         f"{list(t.shape)}")
    if not t.is_contiguous():
        raise ValueError(f"dedup_chunks: {name} must be contiguous (rows of 32 bytes end to end); call .contiguous()")


def dedup_chunks(index_hashes: torch.Tensor, new_hashes: torch.Tensor, stream=None) -> torch.Tensor:
    """For every fresh chunk hash, the first row that holds the same 32 bytes: K13, csrc/gpu/dedup.hip.

    index_hashes: uint8 [m, 32], what is already known (m may be 0); new_hashes: uint8 [n, 32].  Rows
    are numbered index first, then fresh.  Returns int64 [n] on the inputs' device: a value < m is an
    index row; the value m + j is fresh row j with j <= i, and j == i means row i is the first of its
    kind.  Among equal rows the smallest wins, so an index row beats a fresh one and the first index
    row beats a later duplicate; the result is a pure function of the hashes.  Refused on the host
    (ValueError naming what is wrong): inputs that are not contiguous uint8 [k, 32], inputs on different
    devices, m + n >= 2**31.  n == 0 returns an empty tensor without a launch.  GPU tensors: three
    asynchronous launches on `stream` (default: the current stream), the table allocated and freed in
    that stream's order; CPU tensors: a dict over the rows' bytes with the same rule."""
    _check_hashes(index_hashes, "index_hashes")
    _check_hashes(new_hashes, "new_hashes")
    if index_hashes.device != new_hashes.device:
        raise ValueError(f"dedup_chunks: index_hashes is on {index_hashes.device}, new_hashes on {new_hashes.device}: "
                         "move the index to the device of the hashes it is joined with")
    m, n = index_hashes.shape[0], new_hashes.shape[0]
    if m + n >= MAX_DEDUP_ROWS:
        raise ValueError(f"dedup_chunks: {m} + {n} rows, the table's row ids hold fewer than 2**31")
    dev = new_hashes.device
    if n == 0:
        return torch.empty(0, dtype=torch.int64, device=dev)
    if dev.type != "cuda":
        seen: dict[bytes, int] = {}
        for r, row in enumerate(index_hashes.numpy()):
            seen.setdefault(row.tobytes(), r)
        out = np.empty(n, dtype=np.int64)
        for j, row in enumerate(new_hashes.numpy()):
            out[j] = seen.setdefault(row.tobytes(), m + j)
        return torch.from_numpy(out)
    H = hip()
    tb = H.dedup_table_bytes(m + n)
    assert tb == 4 * dedup_slots(m + n), "K13 table size drift"

    def alloc():
        # rows are 32 bytes, so only a view that starts off a 16-byte boundary needs a copy
        keys = [t.clone() if t.shape[0] and t.data_ptr() % 16 else t for t in (index_hashes, new_hashes)]
        return keys, torch.empty(tb, dtype=torch.uint8, device=dev), torch.empty(n, dtype=torch.int64, device=dev)

    if stream is None:
        st = _stream(dev)
        (ix, fr), table, first = alloc()
    else:
        st = stream.cuda_stream
        with torch.cuda.stream(stream):  # allocations, copies and frees are ordered on the launch's stream
            (ix, fr), table, first = alloc()
    H.dedup_chunks(ix.data_ptr() if m else 0, m, fr.data_ptr(), n, table.data_ptr(), tb, first.data_ptr(), st)
    return first


# ----------------------------------------------------------------------------------------------
# K7b: chunk compression (BG4 grouping + LZ4 frame) and serialization of compressed chunks
# ----------------------------------------------------------------------------------------------
LZ4_SLOT = 132 << 10  # device bytes per chunk for one frame (>= LZ4 bound of 128 KiB + frame overhead)


@functools.lru_cache(maxsize=1)
def _lz4_header_checksums() -> tuple[int, int]:
    """Frame-descriptor checksum bytes the host encoder writes for 64 KiB / 256 KiB blocks."""
    return _core.lz4_compress_frame(b"\0" * 16)[6], _core.lz4_compress_frame(b"\0" * 65537)[6]


def compress_chunks(buf: torch.Tensor, offsets, lens, bg4: bool = True):
    """Compress each chunk buf[off:off+len] on the GPU into an LZ4 frame (BG4-grouped first when
    `bg4`), the layout the host encoder and hf_xet use.  Returns (frames, frame_len): frames is a
    device buffer holding chunk i's frame at i * LZ4_SLOT; frame_len[i] == 0 means the chunk does
    not compress and is stored raw (scheme 0), as Xet does."""
    offsets = np.asarray(offsets, dtype=np.uint64)
    lens = np.asarray(lens, dtype=np.uint32)
    n = len(offsets)
    if buf.device.type != "cuda":
        raise ValueError("compress_chunks runs on the GPU")
    if n and (np.any(lens > 128 * 1024) or np.any(offsets + lens > buf.numel() * buf.element_size())):
        raise ValueError("compress_chunks: chunk larger than 128 KiB or past the buffer")
    dev = buf.device
    frames = padded_empty(max(1, n) * LZ4_SLOT, dev)
    flen = torch.zeros(max(1, n), dtype=torch.int32, device=dev)
    if n:
        H = hip()
        buf = _as_padded_u8(buf)
        scratch = padded_empty(n * LZ4_SLOT if bg4 else 1, dev)
        offs_d = torch.from_numpy(offsets.view(np.int64).copy()).to(dev)
        lens_d = torch.from_numpy(lens.view(np.int32).copy()).to(dev)
        hc64, hc256 = _lz4_header_checksums()
        H.compress_chunks(buf.data_ptr(), offs_d.data_ptr(), lens_d.data_ptr(), n, int(bg4), scratch.data_ptr(),
                          LZ4_SLOT, frames.data_ptr(), LZ4_SLOT, flen.data_ptr(), hc64, hc256,
                          torch.cuda.current_stream(dev).cuda_stream)
    return frames, flen[:n].cpu().numpy().astype(np.int64)


def pack_frames(src_addr: np.ndarray, clen: np.ndarray, ulen: np.ndarray, scheme: np.ndarray, out_off: np.ndarray,
                out: torch.Tensor) -> None:
    """Serialize chunks whose payload (compressed frame or raw bytes) sits at device address
    src_addr[i]: 8-byte header [0][clen u24][scheme][ulen u24] + payload, into `out` at out_off[i]."""
    n = len(clen)
    if n == 0:
        return
    clen = np.asarray(clen, dtype=np.uint32)
    out_off = np.asarray(out_off, dtype=np.uint64)
    if np.any(out_off + clen + 8 > out.numel()):
        raise ValueError("pack_frames range out of bounds")
    dev = out.device
    H = hip()
    t = [torch.from_numpy(np.ascontiguousarray(a).copy()).to(dev) for a in
         (np.asarray(src_addr, dtype=np.uint64).view(np.int64), clen.view(np.int32),
          np.asarray(ulen, dtype=np.uint32).view(np.int32), np.asarray(scheme, dtype=np.uint8),
          out_off.view(np.int64))]
    H.pack_frames(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(), t[4].data_ptr(), n,
                  out.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
