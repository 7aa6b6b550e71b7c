#!/usr/bin/env python3
"""Delta pull against a plain pull of the same revision, end to end on one GPU.

A synthetic model (`--mb` of N(0, 0.02) bf16 weights in `--files` safetensors files) is published on
an in-process FakeHub (BG4/LZ4 xorbs, served over loopback HTTP) and pulled to the GPU.  For every
share in `--changed`, a second revision is published in which that share of each file's bytes is
replaced (eight regions per file) and a few KB are inserted near the front of the first file, so all
later chunks shift.  The plain pull and `pull(..., base=w0)` of it then alternate, `--rounds` times,
with the disk xorb cache off.  One JSON line per pull.

The origin here is the FakeHub's Python HTTP server, not an HBM seeder: its rate (not the GPU's)
bounds the plain pull, so read the ratio as "bytes not moved", not as a statement about HBM rates.

    python tools/delta_bench.py [--mb 256] [--files 4] [--changed 0.05,0.5] [--rounds 2]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import tempfile
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

import zest_amd  # noqa: E402
from zest_amd.testing import FakeHub  # noqa: E402


def safetensors(payload: bytes, name: str) -> bytes:
    head = json.dumps({name: {"dtype": "BF16", "shape": [len(payload) // 2], "data_offsets": [0, len(payload)]}}).encode()
    head += b" " * (-len(head) % 8)
    return len(head).to_bytes(8, "little") + head + payload


def bf16(rng, nbytes: int) -> bytes:
    return (rng.normal(0, 0.02, nbytes // 2).astype(np.float32).view(np.uint32) >> 16).astype(np.uint16).tobytes()


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", type=int, default=256)
    ap.add_argument("--files", type=int, default=4)
    ap.add_argument("--changed", default="0.05,0.5")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args()
    rng = np.random.default_rng(1)
    per = (a.mb << 20) // a.files // 2 * 2
    base = [bf16(rng, per) for _ in range(a.files)]
    hub = FakeHub(policy="auto")
    hub.start()
    os.environ.update(hub.env(tempfile.mkdtemp(prefix="zest-delta-")))
    os.environ["ZEST_CACHE_WRITES"] = "0"
    net = dict(p2p=False, dht=False, device=a.device)
    sync = torch.cuda.synchronize if a.device.startswith("cuda") else (lambda: None)
    try:
        t0 = time.time()
        hub.add_repo("bench/rev1", {f"m{i}.safetensors": safetensors(b, f"w{i}") for i, b in enumerate(base)},
                     xet_suffixes=(".safetensors",))
        print(json.dumps({"setup": "rev1 published", "bytes": per * a.files, "s": round(time.time() - t0, 2)}), flush=True)
        w0 = zest_amd.pull("bench/rev1", **net)  # also the warm-up of connections, allocator and kernels
        sync()
        for share in (float(x) for x in a.changed.split(",")):
            files = {}
            for i, b in enumerate(base):
                buf = bytearray(b)
                reg = int(per * share / 8) // 2 * 2
                for k in range(8):
                    at = (per // 8) * k + 4096
                    buf[at:at + reg] = bf16(rng, reg)
                if i == 0:
                    buf[10_000:10_000] = bf16(rng, 6_002)
                files[f"m{i}.safetensors"] = safetensors(bytes(buf), f"w{i}")
            repo = f"bench/rev2-{share}"
            hub.add_repo(repo, files, xet_suffixes=(".safetensors",))
            total = sum(len(v) for v in files.values())
            for rnd in range(a.rounds):
                for variant, kw in (("plain", {}), ("delta", {"base": w0})):
                    served, st = hub.xorb_bytes_served, {}
                    sync()
                    t0 = time.perf_counter()
                    w = zest_amd.pull(repo, stats=st, **kw, **net)
                    sync()
                    dt = time.perf_counter() - t0
                    row = {"changed": share, "round": rnd, "variant": variant, "s": round(dt, 4), "file_bytes": total,
                           "file_gbps": round(total / dt / 1e9, 3), "served_bytes": hub.xorb_bytes_served - served}
                    row.update({k: (round(v, 5) if isinstance(v, float) else v) for k, v in st.get("delta", {}).items()})
                    print(json.dumps(row), flush=True)
                    del w
        return 0
    finally:
        hub.stop()


if __name__ == "__main__":
    raise SystemExit(main())
