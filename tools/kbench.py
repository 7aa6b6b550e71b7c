#!/usr/bin/env python3
"""Kernel micro-benchmarks on one MI355X: throughput of every HIP kernel in zest_amd.ops.

Prints one JSON line per kernel: {"kernel", "gbps", "ms", "bytes", ...}.  Uses HIP events around
`--iters` back-to-back launches after a warm-up; data is random (not zero-filled).
"""
from __future__ import annotations

import argparse
import json
import os
import time

import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
if os.environ.get("ZEST_PKG_ROOT"):  # A/B of kernel builds: a package copy with another _hip .so
    sys.path.insert(0, os.environ["ZEST_PKG_ROOT"])

from zest_amd import _core as C
from zest_amd import ops


def timed(fn, iters):
    fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def emit(**kw):
    print(json.dumps(kw), flush=True)


def loose_layout(total: int, model: str = "llama-3.1-8b", max_tensor: int = 256 << 20) -> list:
    """[(name, bytes)] of `model`'s tensors in file order up to `total` bytes, the embeddings and
    other tensors over `max_tensor` left out and the last one cut to fit: the sizes a trainer holds as
    loose parameters (for 8B: 112 / 32 / 8 MiB projections and 8 KiB norms)."""
    from zest_amd import models

    out, left = [], total
    for t in models.get(model).tensors:
        if t.nbytes > max_tensor or not left:
            continue
        k = min(t.nbytes, left)
        out.append((t.name, k))
        left -= k
    return out


def loose_tensors(layout, dev, seed: int = 14) -> dict:
    """Each tensor of `layout` as its own allocation, a uint8 view starting at a staggered 0..15
    bytes after a 16-byte boundary and ending with the allocation's last byte (no pad), random bytes."""
    out = {}
    for i, (name, k) in enumerate(layout):
        t = torch.empty(k + i % 16, dtype=torch.uint8, device=dev)[i % 16:]
        ops.fill_synthetic(t, seed, sum(b for _, b in layout[:i]), 0)
        out[name] = t
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=4.0)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--only", default="")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    n = int(a.gib * (1 << 30))
    sel = set(a.only.split(",")) if a.only else None

    def want(k):
        return sel is None or k in sel

    H = ops.hip()
    st = torch.cuda.current_stream().cuda_stream
    arena = ops.padded_empty(n, dev)
    ops.fill_synthetic(arena, 1, 0, 0)
    torch.cuda.synchronize()

    if want("fill"):
        ms = timed(lambda: ops.fill_synthetic(arena, 1, 0, 0), a.iters)
        emit(kernel="fill_synthetic_random", bytes=n, ms=ms, gbps=n / ms / 1e6)

    if want("dedup_chunks"):
        # K13 at the scale of a 70B model: 2.2 M index rows, 2.2 M fresh rows of which half are index
        # rows and 1 % repeat an earlier fresh row.  Beside it, in the same run, the host alternative:
        # the fresh hashes copied to the host and joined there with NumPy on a 32-byte void view
        # (the index's host copy is taken as given).
        m_rows = n_rows = 2_200_000
        g = torch.Generator(device=dev).manual_seed(13)
        index_h = torch.randint(0, 256, (m_rows, 32), dtype=torch.uint8, device=dev, generator=g)
        fresh_h = torch.randint(0, 256, (n_rows, 32), dtype=torch.uint8, device=dev, generator=g)
        hit = torch.randperm(n_rows, device=dev, generator=g)[: n_rows // 2]
        fresh_h[hit] = index_h[torch.randint(0, m_rows, (len(hit),), device=dev, generator=g)]
        rep = torch.randint(n_rows // 100, n_rows, (n_rows // 100,), device=dev, generator=g)
        fresh_h[rep] = fresh_h[torch.randint(0, n_rows // 100, (len(rep),), device=dev, generator=g)]
        tb = H.dedup_table_bytes(m_rows + n_rows)
        table = torch.empty(tb, dtype=torch.uint8, device=dev)
        first = torch.empty(n_rows, dtype=torch.int64, device=dev)
        ms = timed(lambda: H.dedup_chunks(index_h.data_ptr(), m_rows, fresh_h.data_ptr(), n_rows, table.data_ptr(), tb,
                                          first.data_ptr(), st), a.iters)
        emit(kernel="dedup_chunks[3 launches]", index_rows=m_rows, fresh_rows=n_rows, table_bytes=tb, ms=ms,
             mrows_per_s=(m_rows + n_rows) / ms / 1e3, gbps=32 * (m_rows + n_rows) / ms / 1e6)

        def wall(fn, iters):
            fn()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(iters):
                r = fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / iters * 1e3, r

        ms_ops, got = wall(lambda: ops.dedup_chunks(index_h, fresh_h), a.iters)
        emit(kernel="ops.dedup_chunks[wall, with table allocation]", ms=ms_ops)
        assert torch.equal(got, first)
        index_host = np.ascontiguousarray(index_h.cpu().numpy()).view("V32").reshape(-1)
        ms_d2h, fresh_host = wall(lambda: fresh_h.cpu(), a.iters)

        def host_join():
            keys = np.concatenate([index_host, fresh_host.numpy().view("V32").reshape(-1)])
            _, where, inv = np.unique(keys, return_index=True, return_inverse=True)  # where: first row of each key
            return where[inv.reshape(-1)][m_rows:]

        t0 = time.perf_counter()
        host_first = host_join()
        ms_join = (time.perf_counter() - t0) * 1e3
        emit(kernel="host_join[d2h of fresh hashes + numpy unique on V32]", d2h_ms=ms_d2h, join_ms=ms_join,
             ms=ms_d2h + ms_join)
        assert np.array_equal(host_first, first.cpu().numpy()), "kernel and host join disagree"
        own = m_rows + np.arange(n_rows)
        emit(kernel="dedup_chunks[result]", matched=int((host_first < m_rows).sum()),
             duplicates=int(((host_first >= m_rows) & (host_first != own)).sum()), new=int((host_first == own).sum()))
        del index_h, fresh_h, table, first, got

    # fixed 64 KiB chunks over the arena
    csize = 65536
    nck = n // csize
    offs = np.arange(nck, dtype=np.uint64) * csize
    lens = np.full(nck, csize, dtype=np.uint32)
    offs_d = torch.from_numpy(offs.view(np.int64)).to(dev)
    lens_d = torch.from_numpy(lens.view(np.int32)).to(dev)
    out = torch.empty((nck, 32), dtype=torch.uint8, device=dev)
    hs = ops.HashScratch(dev)

    def hash_case(name, o, ln, check_n=4):
        """K1 over (offset, len) messages: wave-per-message kernel vs the leaf-flat pipeline."""
        o_d = torch.from_numpy(o.astype(np.int64)).to(dev)
        l_d = torch.from_numpy(ln.astype(np.uint32).view(np.int32)).to(dev)
        m = len(o)
        res = torch.empty((m, 32), dtype=torch.uint8, device=dev)
        nb = int(ln.sum())
        sp, sb = hs.get(m, nb)
        for path, scr in (("wave", (0, 0)), ("flat", (sp, sb))):
            ms = timed(lambda: H.hash_ranges(arena.data_ptr(), o_d.data_ptr(), l_d.data_ptr(), m, res.data_ptr(), 0,
                                             st, *scr), a.iters)
            emit(kernel=f"blake3_{name}[{path}]", bytes=nb, ms=ms, gbps=nb / ms / 1e6, chunks=m)
            h = res[:check_n].cpu().numpy()
            host = arena[: int(o[check_n - 1] + ln[check_n - 1])].cpu().numpy().tobytes()
            assert all(h[i].tobytes() == C.chunk_hash(host[int(o[i]):int(o[i]) + int(ln[i])]) for i in range(check_n))

    if want("hash"):
        hash_case("xet_chunks_64k", offs, lens)
        # CDC chunks land at arbitrary byte offsets in the arena: the misaligned load path
        hash_case("xet_chunks_64k_unaligned", offs + (np.arange(nck, dtype=np.uint64) * 13) % 61,
                  np.full(nck, csize - 64, dtype=np.uint32))
        # the real size mix: Xet CDC chunks (8-128 KiB) of the arena's own bytes
        ends = np.asarray(C.chunk_ends(arena[: min(n, 256 << 20)].cpu().numpy().tobytes()), dtype=np.uint64)
        starts = np.concatenate([[0], ends[:-1]]).astype(np.uint64)
        hash_case("xet_chunks_cdc", starts, (ends - starts).astype(np.uint32))

    if want("gather"):
        # K8 peer gather on local memory (copy engine vs kernel; on the 8-GPU node the same launch
        # reads the peers' arenas over xGMI): 7 segments, as for 8 ranks
        seg = n // 8
        dst_g = ops.padded_empty(n, dev)
        srcs = [arena.data_ptr() + i * seg + 3 for i in range(7)]
        dsts = [dst_g.data_ptr() + i * seg + 3 for i in range(7)]
        ms = timed(lambda: H.peer_gather(srcs, dsts, [seg - 64] * 7, st), a.iters)
        emit(kernel="peer_gather_k8_local(7 segs)", bytes=7 * seg, ms=ms, gbps=7 * seg / ms / 1e6)
        assert torch.equal(dst_g[3:seg - 61], arena[3:seg - 61])

        def dma():
            for i in range(7):
                H.memcpy_async(dsts[i], srcs[i], seg - 64, st)
        ms = timed(dma, a.iters)
        emit(kernel="hipMemcpyAsync_local(7 segs)", bytes=7 * seg, ms=ms, gbps=7 * seg / ms / 1e6)
        del dst_g

    if want("cdc"):
        cap = n // 4096
        cand = torch.empty(cap, dtype=torch.int64, device=dev)
        cnt = torch.zeros(1, dtype=torch.int64, device=dev)

        def run_cdc():
            cnt.zero_()
            H.cdc_candidates(arena.data_ptr(), n, ops.XET_MASK, cand.data_ptr(), cnt.data_ptr(), cap, st)
        ms = timed(run_cdc, a.iters)
        emit(kernel="cdc_candidates", bytes=n, ms=ms, gbps=n / ms / 1e6, candidates=int(cnt.item()))

    # serialized xorb body of uncompressed chunks for place/index
    if want("place") or want("ingest"):
        body_n = nck * (csize + 8)
        body = ops.padded_empty(body_n, dev)
        data_off = offs
        out_off = np.arange(nck, dtype=np.uint64) * (csize + 8)
        ops.pack_chunks(arena, data_off, lens, out_off, body)
        dst = ops.padded_empty(n, dev)
        per_term = 1024  # 64 MiB terms
        nterm = (nck + per_term - 1) // per_term
        terms = np.zeros(nterm, dtype=ops.TERM_DTYPE)
        for t in range(nterm):
            c0, c1 = t * per_term, min(nck, (t + 1) * per_term)
            terms[t] = (c0 * (csize + 8), (c1 - c0) * (csize + 8), c0 * csize, c0, c1 - c0, (c1 - c0) * csize)
        ws = ops.IngestWorkspace(dev, nterm, nck)
        hashes = torch.empty((nck, 32), dtype=torch.uint8, device=dev)
        ms = timed(lambda: ops.ingest_terms(body, dst, terms, hashes, ws=ws, check=False), a.iters)
        emit(kernel="ingest_none(index+place+hash)", bytes=n, ms=ms, gbps=n / ms / 1e6)
        ops.raise_on_error(ws.err)
        assert torch.equal(dst[:1 << 20], arena[:1 << 20])
        tdev = ws.terms
        ms = timed(lambda: H.index_terms(body.data_ptr(), tdev.data_ptr(), nterm, ws.chunks.data_ptr(),
                                         ws.err.data_ptr(), st), a.iters)
        emit(kernel="index_terms", bytes=body_n, ms=ms, gbps=body_n / ms / 1e6, terms=nterm)
        ms = timed(lambda: H.place_chunks(body.data_ptr(), body_n, dst.data_ptr(), n, ws.chunks.data_ptr(), nck, 0,
                                          n, ws.err.data_ptr(), st), a.iters)
        emit(kernel="place_raw(+lz4 scan)", bytes=n, ms=ms, gbps=n / ms / 1e6)
        ms = timed(lambda: H.hash_chunks(dst.data_ptr(), n, ws.chunks.data_ptr(), nck, hashes.data_ptr(), 0, 0, st),
                   a.iters)
        emit(kernel="hash_chunks[wave]", bytes=n, ms=ms, gbps=n / ms / 1e6)
        sp, sb = hs.get(nck, n)
        ms = timed(lambda: H.hash_chunks(dst.data_ptr(), n, ws.chunks.data_ptr(), nck, hashes.data_ptr(), 0, 0, st,
                                         sp, sb), a.iters)
        emit(kernel="hash_chunks[flat]", bytes=n, ms=ms, gbps=n / ms / 1e6)
        del body, dst

    def ingest_case(name, raw, policy, iters, fused=None, after=None):
        """Pack `raw` into xorb runs with `policy`, then time index+place/decode+hash on the GPU
        (fused: one place+hash pass; None = the ZEST_FUSED_INGEST default).  `after(src, dst, ws,
        n_chunks)` runs extra timings on the indexed batch."""
        m = len(raw)
        ends = C.chunk_ends(raw)
        b = C.XorbBuilder(policy)
        prev, terms_l, bodies, src_off, cbase, schemes = 0, [], [], 0, 0, {}

        def close():
            nonlocal src_off, cbase
            body_b = b.serialize(False)
            for e in C.index_chunks(body_b):
                schemes[e[2]] = schemes.get(e[2], 0) + 1
            bodies.append(body_b)
            terms_l.append((src_off, len(body_b), cbase, b.num_chunks(), b.unpacked_size()))
            src_off += len(body_b)
            cbase += b.num_chunks()
            b.clear()

        for e in ends:
            if not b.fits(e - prev):
                close()
            b.add_chunk(raw[prev:e])
            prev = e
        close()
        blob = b"".join(bodies)
        terms = np.zeros(len(terms_l), dtype=ops.TERM_DTYPE)
        uo = 0
        for i, t in enumerate(terms_l):
            terms[i] = (t[0], t[1], uo, t[2], t[3], t[4])
            uo += t[4]
        src = ops.padded_empty(len(blob), dev)
        src.copy_(torch.frombuffer(bytearray(blob), dtype=torch.uint8))
        dst = ops.padded_empty(m, dev)
        nck2 = int(terms["n_chunks"].sum())
        hashes = torch.empty((nck2, 32), dtype=torch.uint8, device=dev)
        ws = ops.IngestWorkspace(dev, len(terms), nck2)
        comp = policy != "none"
        ms = timed(lambda: ops.ingest_terms(src, dst, terms, hashes, ws=ws, check=False, fused=fused,
                                            has_compressed=comp), iters)
        ops.raise_on_error(ws.err)
        ok = dst[:m].cpu().numpy().tobytes() == raw
        tag = "" if fused is None else ("[fused]" if fused else "[place+hash]")
        emit(kernel=f"ingest_{policy}({name}){tag}", bytes=m, ms=ms, gbps=m / ms / 1e6, ratio=len(blob) / m,
             chunks=nck2, schemes={str(k): v for k, v in sorted(schemes.items())}, exact=ok)
        assert ok, name
        if after is not None:
            after(src, dst, ws, nck2)
        del src, dst, hashes, ws

    if want("lz4"):
        # bf16-like weights, compressed on the host (LZ4 / BG4 frames), decoded on the GPU
        m = min(n, 256 << 20)
        w = (np.random.default_rng(0).standard_normal(m // 2).astype(np.float32) * 0.02)
        raw = (w.view(np.uint32) >> 16).astype(np.uint16).tobytes()
        for policy in ("lz4", "bg4"):
            ingest_case("bf16", raw, policy, a.iters)

    if want("lz4big"):
        # a bench-sized round: 1 GiB of bf16 weights = ~16.7k chunks
        m = 1 << 30
        w = (np.random.default_rng(0).standard_normal(m // 2).astype(np.float32) * 0.02)
        raw = (w.view(np.uint32) >> 16).astype(np.uint16).tobytes()
        del w
        ingest_case("bf16_1g", raw, "bg4", max(3, a.iters // 4))
        del raw

    if want("lz4occ"):
        # K3 alone on a bench-sized BG4 round, persistent grid capped at 8 / 4 / 2 / 1 / 0.5 waves
        # per SIMD: latency-bound waves speed up with occupancy, an issue-bound decoder does not
        m = 1 << 30
        w = (np.random.default_rng(0).standard_normal(m // 2).astype(np.float32) * 0.02)
        raw = (w.view(np.uint32) >> 16).astype(np.uint16).tobytes()
        del w

        def occ(src, dst, ws, n):
            for g in (2048, 1024, 512, 256, 128):
                ms = timed(lambda: H.lz4_decode(src.data_ptr(), src.numel(), dst.data_ptr(), dst.numel(),
                                                ws.chunks.data_ptr(), n, ws.err.data_ptr(), st, g), 3)
                ops.raise_on_error(ws.err)
                emit(kernel=f"lz4_decode(bf16_1g,grid={g})", bytes=m, ms=ms, gbps=m / ms / 1e6,
                     waves_per_simd=g * 4 / 1024)
            assert dst[:m].cpu().numpy().tobytes() == raw
            # the two-kernel decoder: lane-per-chunk parse into records, then record-driven execute
            dec = ops.DecodeScratch(dev)
            sp, sb = dec.get(n, src.numel())
            dst.zero_()
            ms = timed(lambda: H.lz4_decode(src.data_ptr(), src.numel(), dst.data_ptr(), dst.numel(),
                                            ws.chunks.data_ptr(), n, ws.err.data_ptr(), st, 0, sp, sb), 3)
            ops.raise_on_error(ws.err)
            fb = int((dec.buf[:4 * n].view(torch.int32) == -1).sum())
            emit(kernel="lz4_decode(bf16_1g,records)", bytes=m, ms=ms, gbps=m / ms / 1e6, scratch_mb=sb >> 20,
                 fallback_chunks=fb)
            assert dst[:m].cpu().numpy().tobytes() == raw

        ingest_case("bf16_1g", raw, "bg4", 3, after=occ)
        del raw

    if want("k3pair") or want("index"):
        # round 4: producer/consumer wave pairs (k_lz4_pair) vs the one-wave decoder, and the serial
        # header walk k_index_terms, at a small launch (256 MiB, ~4 k chunks: fewer chunks than wave
        # slots) and a bench round (1 GiB).  (A scan-based header walk measured here at 5.4 / 12.3 ms
        # against 0.51 / 0.61 ms serial was removed: profiles/r4/kbench_k3pair_r4b.jsonl.)
        # `--only index`: just the header walks, serial and parallel (scan + link), at 256 MiB.
        sizes = ((128 << 20, "bf16_128m"), (256 << 20, "bf16_256m"), (512 << 20, "bf16_512m"),
                 (768 << 20, "bf16_768m"), (1 << 30, "bf16_1g"))
        for m, tag in sizes if want("k3pair") else sizes[1:2]:
            w = (np.random.default_rng(0).standard_normal(m // 2).astype(np.float32) * 0.02)
            raw = (w.view(np.uint32) >> 16).astype(np.uint16).tobytes()
            del w

            def pair(src, dst, ws, n, m=m, tag=tag, raw=raw):
                for label, kw in (("one-wave", {}), ("pair", {"pair": True})) if want("k3pair") else ():
                    dst.zero_()
                    ms = timed(lambda: H.lz4_decode(src.data_ptr(), src.numel(), dst.data_ptr(), dst.numel(),
                                                    ws.chunks.data_ptr(), n, ws.err.data_ptr(), st, 0, **kw), 5)
                    ops.raise_on_error(ws.err)
                    emit(kernel=f"lz4_decode({tag},{label})", bytes=m, ms=ms, gbps=m / ms / 1e6, chunks=n)
                    assert dst[:m].cpu().numpy().tobytes() == raw, label
                nt = ws.max_terms
                chunks0 = ws.chunks.clone()
                ws.err.zero_()
                ms = timed(lambda: H.index_terms(src.data_ptr(), ws.terms.data_ptr(), nt, ws.chunks.data_ptr(),
                                                 ws.err.data_ptr(), st), 5)
                ops.raise_on_error(ws.err)
                emit(kernel=f"index_terms({tag},serial)", bytes=src.numel(), ms=ms, gbps=src.numel() / ms / 1e6,
                     terms=nt, chunks=n, same_records=bool(torch.equal(ws.chunks, chunks0)))
                sp, sb = ws.index_scratch(H, nt)
                ws.chunks.zero_()
                ms = timed(lambda: H.index_terms_scan(src.data_ptr(), src.numel(), ws.terms.data_ptr(), nt,
                                                      ws.chunks.data_ptr(), ws.err.data_ptr(), sp, sb, st), 20)
                ops.raise_on_error(ws.err)
                fell_back = int((ws._index_scratch[:4 * nt].view(torch.int32) < 0).sum())
                emit(kernel=f"index_terms({tag},scan)", bytes=src.numel(), ms=ms, gbps=src.numel() / ms / 1e6,
                     terms=nt, chunks=n, fallback_terms=fell_back,
                     same_records=bool(torch.equal(ws.chunks, chunks0)))

            ingest_case(tag, raw, "bg4", 3, after=pair)
            del raw

    if want("fuse"):
        # a bench round of raw chunks (1 GiB random bytes): place then hash vs the fused one pass,
        # and the same for a BG4 bf16 round (decode + place/hash)
        m = 1 << 30
        raw = np.random.default_rng(2).integers(0, 256, m, dtype=np.uint8).tobytes()
        for fused in (False, True):
            ingest_case("random_1g", raw, "none", max(3, a.iters), fused=fused)
        w = (np.random.default_rng(0).standard_normal(m // 2).astype(np.float32) * 0.02)
        raw = (w.view(np.uint32) >> 16).astype(np.uint16).tobytes()
        del w
        for fused in (False, True):
            ingest_case("bf16_1g", raw, "bg4", max(3, a.iters // 4), fused=fused)
        del raw

    if want("lz4paths"):
        # one decoder path per data set: short matches, long literal runs, RLE, far matches
        m = 64 << 20
        rng = np.random.default_rng(1)
        sets = {
            "lowent": rng.integers(0, 8, m, dtype=np.uint8) * 31,
            "sparse": np.where(rng.random(m) < 0.02, rng.integers(0, 256, m), 0).astype(np.uint8),
            "mostly_random": np.where(rng.random(m) < 0.85, rng.integers(0, 256, m), 7).astype(np.uint8),
        }
        phrase = rng.integers(0, 256, 40_000, dtype=np.uint8)
        far = np.resize(phrase, m).copy()
        far[rng.integers(0, m, m // 64)] = rng.integers(0, 256, m // 64, dtype=np.uint8)
        sets["far_repeats"] = far
        for name, arr in sets.items():
            ingest_case(name, arr.tobytes(), "lz4", a.iters)

    if want("sha1"):
        # K6 parity row: sha1_info_hash over many xorb hashes at once (reference: 1 hash, 55 ns on a CPU core)
        nh = 1 << 22
        hs = torch.randint(0, 256, (nh, 32), dtype=torch.uint8, device=dev)
        ms = timed(lambda: ops.sha1_info_hash(hs), a.iters)
        emit(kernel="sha1_info_hash_gpu", hashes=nh, ms=ms, ns_per_hash=ms * 1e6 / nh,
             mbps=nh * 44 / (ms / 1e3) / 2**20)
        del hs

    if want("blake3_64kb"):
        # parity row blake3_64kb_gpu: plain BLAKE3 of many 64 KiB buffers
        nb = 1 << 15
        offs = np.arange(nb, dtype=np.uint64) * 65536
        lens = np.full(nb, 65536, dtype=np.uint32)
        ms = timed(lambda: ops.hash_ranges(arena, offs, lens, key_mode=2), a.iters)
        emit(kernel="blake3_64kb_gpu", bytes=nb * 65536, ms=ms, mbps=nb * 65536 / (ms / 1e3) / 2**20)

    if want("merkle"):
        nl = 80_000
        hs = torch.randint(0, 256, (nl * 8, 32), dtype=torch.uint8, device=dev)
        sz = torch.randint(8192, 131072, (nl * 8,), dtype=torch.int64, device=dev)
        jobs = [(i * nl, nl) for i in range(8)]
        ms = timed(lambda: ops.merkle_roots(hs, sz, jobs), a.iters)
        emit(kernel="merkle_8x80k_leaves", ms=ms, leaves=nl * 8)

    if want("serve"):
        # K9 serve_pack: a resident run of CDC-sized chunks (8-128 KiB at odd addresses) serialized in
        # the seeder's 8 MiB pieces, into HBM and into pinned host memory (what a resident seeder
        # does per response); next to it the serialized seeder's step, a D2H copy of the same pieces
        m = min(n, 1 << 30)
        rng = np.random.default_rng(5)
        ln = rng.integers(8192, 131073, m // 65536)
        gaps = rng.integers(0, 16, len(ln))
        so = np.cumsum(ln + gaps) - ln
        keep = so + ln <= m
        ln, so = ln[keep], so[keep]
        run = ops.ServeRun(np.uint64(arena.data_ptr()) + so.astype(np.uint64), ln, buffers=[arena])
        piece = 8 << 20
        wins = [(o, min(run.total, o + piece)) for o in range(0, run.total, piece)]
        d_out = ops.padded_empty(run.total, dev)
        host = H.host_malloc(run.total)

        def serve(base, cap):
            for lo, hi in wins:
                ops.serve_pack(run, lo=lo, hi=hi, out=(base + lo, cap - lo))

        try:
            for name, fn in (("serve_pack[hbm]", lambda: [ops.serve_pack(run, lo=lo, hi=hi, out=d_out[lo:hi])
                                                          for lo, hi in wins]),
                             ("serve_pack[pinned]", lambda: serve(host, run.total)),
                             ("d2h_memcpy_of_serialized[pinned]",
                              lambda: [H.memcpy_async(host + lo, d_out.data_ptr() + lo, hi - lo, st) for lo, hi in wins])):
                ms = timed(fn, a.iters)
                emit(kernel=name, bytes=run.total, ms=ms, gbps=run.total / ms / 1e6, chunks=run.n, pieces=len(wins),
                     piece_mib=piece >> 20)
            # the pinned copy now holds the D2H copy of serve_pack[hbm]'s output: check it on the host
            import ctypes

            got = np.ctypeslib.as_array((ctypes.c_uint8 * run.total).from_address(host))
            idx = C.index_chunks(got[:int(run.ser_end[7])])
            assert [e[1] for e in idx] == [int(x) for x in ln[:8]]
            assert got[8:8 + int(ln[0])].tobytes() == arena[int(so[0]):int(so[0] + ln[0])].cpu().numpy().tobytes()
        finally:
            torch.cuda.synchronize()
            H.host_free(host)
        del d_out

    if want("slice_gather") or want("slice_gather_peers"):
        # K10 slice_gather: one Llama-3.1-70B safetensors shard, rank 0 of 8 under the "llama-tp" plan,
        # next to its roof (a device-to-device copy of the kept bytes: read N + write N) and to what it
        # replaces (narrow(...).contiguous() per kept tensor); alternated, three rounds
        from zest_amd import device as zdev
        from zest_amd import models
        from zest_amd.shard import Shard, plan_file

        sf = models.get("llama-3.1-70b").shards()[1]
        start, meta = zdev.parse_safetensors_header(sf.header)
        plan = plan_file(start, meta, Shard(0, 8), sf.size)
        kept = sum(t.nbytes for t in plan.tensors)
        fbuf = arena if n >= sf.size else ops.padded_empty(sf.size, dev)
        if fbuf is not arena:
            ops.fill_synthetic(fbuf, 2, 0, 0)
        fbuf = fbuf[:sf.size]
        out = ops.padded_empty(plan.arena_bytes, dev)
        flat = ops.padded_empty(kept, dev)
        views = zdev.tensor_views(fbuf, start, meta)
        acts = {t.name: Shard(0, 8).resolve(t.name, meta[t.name]["shape"], t.dtype) for t in plan.tensors}
        tab = np.empty((H.SLICE_ROWS, len(plan.table)), dtype=np.uint64)
        for k, f in enumerate(ops.SLICE_DTYPE.names):
            tab[k] = plan.table[f]
        tab[5] = tab[4] + tab[1] * tab[3]
        tab_d = torch.from_numpy(tab.view(np.int64)).to(dev)

        def torch_loop(copy=lambda t: t.contiguous()):
            return [views[nm].clone() if act is None else copy(views[nm].narrow(act[0], act[1], act[2] - act[1]))
                    for nm, act in acts.items()]

        # contiguous() copies only the dim-1 slices: a dim-0 slice is contiguous already and stays a view
        # into the file buffer, which then cannot be freed.  The clone loop gives every kept tensor its
        # own memory, as the kernel does: that is the like-for-like row.
        k10 = ("slice_gather[kernel]", lambda: H.slice_gather(fbuf.data_ptr(), tab_d.data_ptr(), tab.shape[1],
                                                              int(tab[5, -1]), out.data_ptr(), st))
        rows = (("torch_narrow_clone_loop", lambda: torch_loop(lambda t: t.clone(memory_format=torch.contiguous_format))),("slice_gather[ops]", lambda: ops.slice_gather(fbuf, plan.table, out)),
                k10,
                ("d2d_copy_of_kept_bytes", lambda: flat.copy_(fbuf[:kept])),
                ("torch_narrow_contiguous_loop", torch_loop)) if want("slice_gather") else (k10,)
        if want("slice_gather_peers"):
            # K11 slice_gather_peers on the same table, in the same process as K10: one source, and the
            # file cut into 8 equal source buffers on this one GPU (entry i reads from the eighth that
            # holds its first byte); under the default grid cap (512 blocks) and with the cap lifted
            out11 = torch.zeros_like(out)
            live = np.flatnonzero(tab[1] * tab[3])
            span = (int(tab[4, live[0]]), int(tab[5, live[-1]]))

            def peers_row(nsrc, max_blocks):
                cut = -(-sf.size // nsrc)
                t = np.empty((H.SLICE_PEER_ROWS, tab.shape[1]), dtype=np.uint64)
                t[:6] = tab
                t[6] = tab[0] // cut
                t[0] = tab[0] - t[6] * cut
                assert (np.diff(t[6].astype(np.int64)) >= 0).all()  # each source's entries are contiguous
                lo, hi = [0] * nsrc, [0] * nsrc
                for s_ in range(nsrc):
                    mine = [i for i in live if t[6, i] == s_]
                    if mine:
                        lo[s_], hi[s_] = int(t[4, mine[0]]), int(t[5, mine[-1]])
                t_d = torch.from_numpy(t.view(np.int64)).to(dev)
                bases = [fbuf.data_ptr() + s_ * cut for s_ in range(nsrc)]
                return lambda: H.slice_gather_peers(bases, lo, hi, t_d.data_ptr(), t.shape[1], span[1],
                                                    out11.data_ptr(), max_blocks, st)

            rows += tuple((f"slice_gather_peers[{ns}src,{'cap512' if mb == 0 else 'lifted'}]", peers_row(ns, mb))
                          for ns in (1, 8) for mb in (0, 1 << 20))
        for rnd in range(3):
            for name, fn in rows:
                ms = timed(fn, a.iters)
                emit(kernel=name, round=rnd, bytes=kept, ms=ms, gbps=kept / ms / 1e6, file_bytes=sf.size,
                     tensors=len(plan.tensors), sliced=sum(a_ is not None for a_ in acts.values()))
        got = plan.views(out)
        for nm, t in zip(acts, torch_loop()):
            assert torch.equal(got[nm].view(torch.uint8), t.reshape(got[nm].shape).view(torch.uint8)), nm
        if want("slice_gather_peers"):
            for _, fn in rows[-4:]:  # every variant rewrites the whole arena
                out11.zero_()
                fn()
                got11 = plan.views(out11)
                assert all(torch.equal(got[nm].view(torch.uint8), got11[nm].view(torch.uint8)) for nm in acts)
            del out11, got11
        del out, flat, tab_d, views, got

    if want("slice_scatter"):
        # K15 slice_scatter on K10's table (the second Llama-3.1-70B shard, rank 0 of 8, then world 1:
        # every tensor whole), each destination a separately allocated tensor, next to K10 into its
        # arena in the same process and to the per-tensor dst.copy_(view) loop that into= replaces.
        # With 16-byte-aligned destinations K15 and K10 do the same work: the expectation to test is
        # parity.  Rows alternate, one timed launch per row and iteration; median and range per row.
        from zest_amd import device as zdev
        from zest_amd import models
        from zest_amd.shard import Shard, plan_file

        sf = models.get("llama-3.1-70b").shards()[1]
        start, meta = zdev.parse_safetensors_header(sf.header)
        fbuf = arena if n >= sf.size else ops.padded_empty(sf.size, dev)
        if fbuf is not arena:
            ops.fill_synthetic(fbuf, 2, 0, 0)
        fbuf = fbuf[:sf.size]
        views = zdev.tensor_views(fbuf, start, meta)
        for world in (8, 1):
            sh = Shard(0, world)
            plan = plan_file(start, meta, sh, sf.size)
            kept = sum(t.nbytes for t in plan.tensors)
            out = ops.padded_empty(plan.arena_bytes, dev)
            dests = [torch.empty(t.shape, dtype=zdev.ST_DTYPES[t.dtype], device=dev) for t in plan.tensors]
            tab10 = np.empty((H.SLICE_ROWS, len(plan.table)), dtype=np.uint64)
            for k, f in enumerate(ops.SLICE_DTYPE.names):
                tab10[k] = plan.table[f]
            tab10[5] = tab10[4] + tab10[1] * tab10[3]
            tab10_d = torch.from_numpy(tab10.view(np.int64)).to(dev)
            stab = np.empty(len(plan.table), dtype=ops.SCATTER_DTYPE)
            for f in ops.SCATTER_DTYPE.names[:4]:
                stab[f] = plan.table[f]
            stab["dst_addr"] = [d.data_ptr() for d in dests]
            tab15 = ops.scatter_soa(stab, stab["run_bytes"] * stab["n_runs"])
            tab15_d = torch.from_numpy(tab15.view(np.int64)).to(dev)
            srcs = []
            for t in plan.tensors:
                act = sh.resolve(t.name, meta[t.name]["shape"], t.dtype)
                srcs.append(views[t.name] if act is None else views[t.name].narrow(act[0], act[1], act[2] - act[1]))

            def copy_loop():
                for d, s_ in zip(dests, srcs):
                    d.copy_(s_)

            rows = (("slice_scatter[kernel]", lambda: H.slice_scatter(fbuf.data_ptr(), tab15_d.data_ptr(), tab15.shape[1],
                                                                      int(tab15[5, -1]), st)),
                    ("slice_scatter[ops]", lambda: ops.slice_scatter(fbuf, stab, dests)),
                    ("slice_gather[kernel]", lambda: H.slice_gather(fbuf.data_ptr(), tab10_d.data_ptr(), tab10.shape[1],
                                                                    int(tab10[5, -1]), out.data_ptr(), st)),
                    ("dst_copy_view_loop", copy_loop))
            ms = {name: [] for name, _ in rows}
            for _ in range(max(5, a.iters)):
                for name, fn in rows:
                    ms[name].append(timed(fn, 1))
            for name, v in ms.items():
                med = float(np.median(v))
                emit(kernel=name, world=world, bytes=kept, ms=med, ms_min=min(v), ms_max=max(v), iters=len(v),
                     gbps=kept / med / 1e6, file_bytes=sf.size, tensors=len(plan.tensors),
                     dst_misaligned=sum(d.data_ptr() % 16 != 0 for d in dests))
            for d in dests:
                d.zero_()
            rows[0][1]()  # the kernel row alone refills the destinations: compare with K10's arena
            got = plan.views(out)
            for t, d in zip(plan.tensors, dests):
                assert torch.equal(got[t.name].view(torch.uint8), d.view(torch.uint8)), t.name
            del out, dests, tab10_d, tab15_d, srcs, got
        del views

    if want("slice_scatter_cast"):
        # K16 slice_scatter_cast on K15's set-up (the second Llama-3.1-70B shard's table, rank 0 of 8, then
        # world 1; every destination a separately allocated tensor), the file's bytes read as F32 into
        # bf16 destinations and as BF16 into f32 ones, next to the per-tensor dst.copy_(file_view) loop
        # (torch's converting copy, what pull() + copy_ runs) and to K15 of as many source bytes, the
        # copy floor.  The expectation to test: K16 is no slower than the copy_ loop, which moves the same
        # bytes with one launch per tensor.  Rows alternate, one timed launch per row and iteration;
        # median and range per row.
        from zest_amd import device as zdev
        from zest_amd import models
        from zest_amd.shard import Shard, plan_file

        sf = models.get("llama-3.1-70b").shards()[1]
        start, meta = zdev.parse_safetensors_header(sf.header)
        fbuf = arena if n >= sf.size else ops.padded_empty(sf.size, dev)
        if fbuf is not arena:
            ops.fill_synthetic(fbuf, 2, 0, 0)
        fbuf = fbuf[:sf.size]
        for world in (8, 1):
            plan = plan_file(start, meta, Shard(0, world), sf.size)
            tb = {f: plan.table[f].astype(np.int64) for f in ops.SCATTER_DTYPE.names[:4]}
            live = np.flatnonzero(tb["run_bytes"] * tb["n_runs"])
            assert not ((tb["src_off"] | tb["run_bytes"] | tb["src_stride"])[live] % 4).any()  # whole F32 items
            flat = [ops.padded_empty(int(tb["run_bytes"][i] * tb["n_runs"][i]), dev) for i in live]  # K15's destinations
            t15 = np.empty(len(live), dtype=ops.SCATTER_DTYPE)
            for f in tb:
                t15[f] = tb[f][live]
            t15["dst_addr"] = [d.data_ptr() for d in flat]
            soa15 = ops.scatter_soa(t15, t15["run_bytes"] * t15["n_runs"])
            soa15_d = torch.from_numpy(soa15.view(np.int64)).to(dev)
            for s_name, d_name, sdt, ddt in (("F32", "BF16", torch.float32, torch.bfloat16),
                                             ("BF16", "F32", torch.bfloat16, torch.float32)):
                si = sdt.itemsize
                whole = fbuf[:sf.size // si * si].view(sdt)
                srcs = [torch.as_strided(whole, (int(tb["n_runs"][i]), int(tb["run_bytes"][i]) // si),
                                         (int(tb["src_stride"][i]) // si, 1), int(tb["src_off"][i]) // si) for i in live]
                dests = [torch.empty(s_.shape, dtype=ddt, device=dev) for s_ in srcs]
                t16 = np.empty(len(live), dtype=ops.CAST_DTYPE)
                for f in tb:
                    t16[f] = tb[f][live]
                t16["dst_addr"] = [d.data_ptr() for d in dests]
                t16["kind"] = ops.CAST_KINDS[(s_name, d_name)]
                src_bytes = int((t16["run_bytes"] * t16["n_runs"]).sum())
                out_bytes = src_bytes // si * ddt.itemsize
                soa16 = ops.scatter_cast_soa(t16, t16["run_bytes"] * t16["n_runs"] // np.uint64(si) * np.uint64(ddt.itemsize))
                soa16_d = torch.from_numpy(soa16.view(np.int64)).to(dev)

                def copy_loop():
                    for d, s_ in zip(dests, srcs):
                        d.copy_(s_)

                rows = (("slice_scatter_cast[kernel]", lambda: H.slice_scatter_cast(
                            fbuf.data_ptr(), soa16_d.data_ptr(), soa16.shape[1], int(soa16[-1, -1]), st)),
                        ("slice_scatter_cast[ops]", lambda: ops.slice_scatter_cast(fbuf, t16, dests)),
                        ("dst_copy_convert_loop", copy_loop),
                        ("slice_scatter[kernel, same source bytes]", lambda: H.slice_scatter(
                            fbuf.data_ptr(), soa15_d.data_ptr(), soa15.shape[1], int(soa15[-1, -1]), st)))
                ms = {name: [] for name, _ in rows}
                for _ in range(max(7, a.iters)):
                    for name, fn in rows:
                        ms[name].append(timed(fn, 1))
                med = {name: float(np.median(v)) for name, v in ms.items()}
                for name, v in ms.items():
                    moved = 2 * src_bytes if name.startswith("slice_scatter[") else src_bytes + out_bytes
                    emit(kernel=name, cast=f"{s_name}->{d_name}", world=world, src_bytes=src_bytes, out_bytes=out_bytes,
                         ms=med[name], ms_min=min(v), ms_max=max(v), iters=len(v), moved_gbps=moved / med[name] / 1e6,
                         tensors=len(live), k16_over_k15=med["slice_scatter_cast[kernel]"] / med[rows[3][0]],
                         k16_over_copy_loop=med["slice_scatter_cast[kernel]"] / med["dst_copy_convert_loop"])
                copy_loop()
                ref = [d.clone() for d in dests]
                for d in dests:
                    d.zero_()
                rows[0][1]()  # the kernel row alone refills the destinations: compare with torch's converts off NaN
                for d, r, s_ in zip(dests, ref, srcs):
                    ok = torch.isnan(s_) | (d.view(torch.int16 if ddt.itemsize == 2 else torch.int32)
                                            == r.view(torch.int16 if ddt.itemsize == 2 else torch.int32))
                    assert bool(ok.all()) and bool(torch.isnan(d)[torch.isnan(s_)].all())
                del dests, srcs, soa16_d, ref
            del flat, soa15_d

    if want("reuse_chunks"):
        # K12 reuse_chunks: 1 GiB of CDC-sized chunks (the size mix of 64 MiB of the arena's own bytes,
        # repeated) at random source and destination misalignments, next to the two passes it fuses, built
        # from what existed before it: K1 over the source (leaf-flat) plus a device copy of as many
        # bytes.  K12 moves 2 bytes per byte (one read, one write), the two passes 3.  Alternated, three
        # rounds; the spread between rounds is the noise to read the difference against.
        rng = np.random.default_rng(12)
        ends = np.asarray(C.chunk_ends(arena[: min(n, 64 << 20)].cpu().numpy().tobytes()), dtype=np.int64)
        mix = np.diff(np.concatenate([[0], ends]))
        ln = np.tile(mix, -(-(1 << 30) // int(mix.sum())))
        ln = ln[: int(np.searchsorted(np.cumsum(ln), 1 << 30)) + 1]
        m, nb = len(ln), int(ln.sum())
        gap_s, gap_d = rng.integers(0, 16, m), rng.integers(0, 16, m)
        s_off = np.cumsum(ln + gap_s) - ln
        d_off = np.cumsum(ln + gap_d) - ln
        src12 = ops.padded_empty(int(s_off[-1] + ln[-1]), dev)
        ops.fill_synthetic(src12, 3, 0, 0)
        dst12 = ops.padded_empty(int(d_off[-1] + ln[-1]), dev)
        flat12 = ops.padded_empty(nb, dev)
        h12 = torch.zeros((m, 32), dtype=torch.uint8, device=dev)
        h2p = torch.zeros((m, 32), dtype=torch.uint8, device=dev)
        sz12 = torch.zeros(m, dtype=torch.int64, device=dev)
        rec = np.empty(m, dtype=ops.REUSE_DTYPE)
        rec["src"], rec["dst"], rec["len"], rec["index"] = src12.data_ptr() + s_off, d_off, ln, rng.permutation(m)
        rec_d = torch.from_numpy(rec.view(np.uint8)).to(dev)
        o_d = torch.from_numpy(s_off.astype(np.int64)).to(dev)
        l_d = torch.from_numpy(ln.astype(np.uint32).view(np.int32)).to(dev)
        sp, sb = ops.HashScratch(dev).get(m, nb)  # (`hs` above is rebound by the sha1 / merkle rows)

        def two_pass():
            H.hash_ranges(src12.data_ptr(), o_d.data_ptr(), l_d.data_ptr(), m, h2p.data_ptr(), 0, st, sp, sb)
            flat12.copy_(src12[:nb])

        rows12 = (("reuse_chunks[kernel]", lambda: H.reuse_chunks(rec_d.data_ptr(), m, dst12.data_ptr(), h12.data_ptr(),
                                                                  sz12.data_ptr(), sp, sb, st)),
                  ("reuse_two_pass[hash_ranges+copy]", two_pass),
                  ("reuse_chunks[ops]", lambda: ops.reuse_chunks(rec["src"], ln, dst12, d_off, h12, rec["index"], sz12,
                                                                 buffers=[src12])))
        for rnd in range(3):
            for name, fn in rows12:
                ms = timed(fn, a.iters)
                emit(kernel=name, round=rnd, bytes=nb, ms=ms, gbps=nb / ms / 1e6, chunks=m)
        assert torch.equal(h12[torch.from_numpy(rec["index"].astype(np.int64)).to(dev)], h2p)  # same hashes, at their rows
        k = m // 2
        assert torch.equal(dst12[int(d_off[k]):int(d_off[k] + ln[k])], src12[int(s_off[k]):int(s_off[k] + ln[k])])
        del src12, dst12, flat12, rec_d

    if want("cdc_segments") or want("hash_chunks_at"):
        # K14 and the hash at absolute addresses over 1 GiB of loose tensors (Llama-3.1-8B sizes, each
        # its own allocation at a staggered 0..15 misalignment, no pad), next to K5 / K1 over the packed
        # copy of the same bytes in the same process.  Every iteration is timed on its own, alternating:
        # the spread of K5's (K1's) own iterations is the noise to read the difference against.
        from zest_amd.publish import classify_chunks

        lay = loose_layout(1 << 30)
        ts14 = list(loose_tensors(lay, dev).values())
        nb = sum(k for _, k in lay)
        packed = ops.padded_empty(nb, dev)
        at = 0
        for t in ts14:
            packed[at:at + t.numel()].copy_(t)
            at += t.numel()
        addrs = np.asarray([t.data_ptr() for t in ts14], dtype=np.uint64)
        seg_lens = np.asarray([t.numel() for t in ts14], dtype=np.uint64)
        cap = nb // 1024
        cand = torch.empty(cap, dtype=torch.int64, device=dev)
        cnt = torch.zeros(1, dtype=torch.int64, device=dev)

        def spread(rows, **kw):
            ms = {name: [] for name, _ in rows}
            for _ in range(a.iters):
                for name, fn in rows:
                    ms[name].append(timed(fn, 1))
            for name, v in ms.items():
                emit(kernel=name, bytes=nb, ms=[round(x, 4) for x in v], ms_min=min(v), ms_max=max(v),
                     ms_median=float(np.median(v)), gbps=nb / float(np.median(v)) / 1e6, **kw)
            (x, _), (y, _) = rows
            emit(ratio=f"{x} / {y}", median=float(np.median(ms[x]) / np.median(ms[y])),
                 best=min(ms[x]) / min(ms[y]))

        if want("cdc_segments"):
            seg, wpre = ops.segment_table(addrs, seg_lens)
            s = len(seg)
            tab = np.zeros(ops.SEG_DTYPE.itemsize * s + 8 * (s + 1) + 64 * s, dtype=np.uint8)
            tab[:ops.SEG_DTYPE.itemsize * s] = seg.view(np.uint8)
            tab[ops.SEG_DTYPE.itemsize * s:ops.SEG_DTYPE.itemsize * s + 8 * (s + 1)] = wpre.view(np.uint8)
            tab_d = torch.from_numpy(tab).to(dev)
            p_pre = tab_d.data_ptr() + ops.SEG_DTYPE.itemsize * s

            def run_k14():
                cnt.zero_()
                H.cdc_candidates_segs(tab_d.data_ptr(), p_pre, s, int(wpre[-1]), p_pre + 8 * (s + 1), ops.XET_MASK,
                                      cand.data_ptr(), cnt.data_ptr(), cap, st)

            def run_k5():
                cnt.zero_()
                H.cdc_candidates(packed.data_ptr(), nb, ops.XET_MASK, cand.data_ptr(), cnt.data_ptr(), cap, st)

            spread((("cdc_candidates_segs[K14, loose]", run_k14), ("cdc_candidates[K5, packed]", run_k5)),
                   segments=s, windows=int(wpre[-1]))
            assert np.array_equal(ops.cdc_candidates_segments(ts14), ops.cdc_candidates(packed))

        if want("hash_chunks_at"):
            ends = ops.select_chunks(ops.cdc_candidates(packed), nb)
            ln = np.diff(np.concatenate([[0], ends]).astype(np.uint64)).astype(np.uint32)
            m = len(ln)
            cl = classify_chunks(seg_lens, ends)
            arena = ops.padded_empty(max(cl["seam_bytes"], 1), dev)
            for sg, so, k, do in zip(cl["piece_seg"].tolist(), cl["piece_off"].tolist(), cl["piece_len"].tolist(),
                                     cl["piece_dst"].tolist()):
                arena[do:do + k].copy_(ts14[sg][so:so + k])
            src = addrs[cl["seg"]] + cl["off"]
            src[cl["seam"]] = np.uint64(arena.data_ptr()) + cl["arena_off"][cl["seam"]]
            rec = np.empty(m, dtype=ops.HASH_AT_DTYPE)
            rec["src"], rec["len"], rec["index"] = src, ln, np.arange(m)
            rec_d = torch.from_numpy(rec.view(np.uint8)).to(dev)
            o_d = torch.from_numpy((np.cumsum(ln, dtype=np.uint64) - ln).view(np.int64)).to(dev)
            l_d = torch.from_numpy(ln.view(np.int32)).to(dev)
            h_at = torch.zeros((m, 32), dtype=torch.uint8, device=dev)
            h_rg = torch.zeros((m, 32), dtype=torch.uint8, device=dev)
            sp, sb = ops.HashScratch(dev).get(m, nb)
            spread((("hash_chunks_at[loose]", lambda: H.hash_chunks_at(rec_d.data_ptr(), m, h_at.data_ptr(), 0, sp, sb, st)),
                    ("hash_ranges[packed]", lambda: H.hash_ranges(packed.data_ptr(), o_d.data_ptr(), l_d.data_ptr(), m,
                                                                  h_rg.data_ptr(), 0, st, sp, sb))),
                   chunks=m, seam_chunks=cl["seam_chunks"], seam_bytes=cl["seam_bytes"])
            assert torch.equal(h_at, h_rg)
        del ts14, packed

    if want("h2d"):
        pin = torch.empty(1 << 30, dtype=torch.uint8).pin_memory()
        d = torch.empty(1 << 30, dtype=torch.uint8, device=dev)
        ms = timed(lambda: d.copy_(pin, non_blocking=True), a.iters)
        emit(kernel="h2d_pinned_1GiB", bytes=1 << 30, ms=ms, gbps=(1 << 30) / ms / 1e6)


if __name__ == "__main__":
    t0 = time.time()
    main()
    print(json.dumps({"total_s": time.time() - t0}))
