"""The peer gather (K8, csrc/gpu/xgmi.hip) against a byte-by-byte model, for test_gpu_peer_gather.py.

  check_gather(H, device, segs, ...)   one launch on a random source and a canary-filled destination,
                                       every byte of both compared afterwards
  python peer_gather_child.py          the grid-stride loop under the ZG_PEER_GATHER_BLOCKS of the
                                       environment (read once per process, hence a process of its own);
                                       prints one JSON verdict

Both buffers are local: the kernel does not know whose memory a segment's source is."""
from __future__ import annotations

import json
import os
import sys
from pathlib import Path

import numpy as np

sys.path[:0] = [p for p in (str(Path(__file__).resolve().parent), str(Path(__file__).resolve().parents[1]))
                if p not in sys.path]

from scatter_model import canary, place_source  # noqa: E402

PASS = 256 * 8 * 16  # bytes one block moves per pass of its loop
CHILD_SIZES = (300 * 1024 + 9, 0, 37, PASS + 3 * 16 + 5, 7 * PASS + 1)


def gather_model(src: np.ndarray, dst: np.ndarray, segs) -> None:
    """segs: (source offset, destination offset, bytes).  Writes into `dst`."""
    for so, do, n in segs:
        for j in range(0, n, 1 << 16):  # slices of a copy, no arithmetic on the bytes
            k = min(n, j + (1 << 16))
            dst[do + j:do + k] = src[so + j:so + k]


def lay_out(sizes, align=(5,), gaps=(1, 2), shifts=(1, 4, 2, 7, 3)):
    """Destinations back to back, `gaps` canary bytes and then up to the next address with the wanted
    dst & 15 apart; each source the same number of bytes into its 16-byte block, at an offset that
    differs from the destination's by a multiple of 16 of its own.  -> (segs, src_len, dst_len)"""
    segs, dpos, spos = [], 3, 0
    for i, n in enumerate(sizes):
        dpos += gaps[i % len(gaps)]
        dpos += (align[i % len(align)] - dpos) & 15
        spos = max(spos, dpos) + 16 * shifts[i % len(shifts)]
        spos += (dpos - spos) & 15
        segs.append((spos, dpos, n))
        dpos += n
        spos += n
    return segs, spos + 5, dpos + 40


def check_gather(H, device, segs, src_len: int, dst_len: int, seed: int = 1, launches=None) -> dict:
    """Run the segments (all in one launch, or `launches` = lists of indices, one launch each) and
    compare the whole destination with the model after every launch, and the source at the end."""
    import torch

    src = np.random.default_rng(seed).integers(0, 256, src_len, dtype=np.uint8)
    hold, s = place_source(src, device)
    want = canary(dst_len, 77)
    d = torch.from_numpy(want.copy()).to(device)
    assert d.data_ptr() % 16 == 0
    for so, do, n in segs:
        assert so + n <= src_len and do + n <= dst_len and (so - do) % 16 == 0
    stream = torch.cuda.current_stream(device).cuda_stream
    for idx in launches or [range(len(segs))]:
        part = [segs[i] for i in idx]
        H.peer_gather([s.data_ptr() + so for so, _, _ in part], [d.data_ptr() + do for _, do, _ in part],
                      [n for _, _, n in part], stream)
        gather_model(src, want, part)
        bad = np.flatnonzero(d.cpu().numpy() != want)
        if bad.size:
            return {"ok": False, "differ": int(bad.size), "first": int(bad[0]), "launch": [list(p) for p in part]}
    return {"ok": bool(np.array_equal(s.cpu().numpy(), src)), "differ": 0, "bytes": int(sum(n for _, _, n in segs))}


def main() -> None:
    import torch

    from zest_amd import ops

    segs, src_len, dst_len = lay_out(CHILD_SIZES, align=(5, 0, 15, 9, 11))
    out = check_gather(ops.hip(), torch.device("cuda:0"), segs, src_len, dst_len, seed=8)
    out["blocks"] = os.environ.get("ZG_PEER_GATHER_BLOCKS")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
