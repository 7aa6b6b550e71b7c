#!/usr/bin/env python3
"""Publish from HBM, then pull the published revision back, end to end on one GPU.

A synthetic model (`--mb` of N(0, 0.02) bf16 weights in `--files` safetensors files) is published on
an in-process FakeHub and pulled to the GPU (w0).  Its ChunkIndex is taken, `--changed` of every
file's bytes is then overwritten in place on the device (eight regions per file), and
`zest_amd.publish(w0, index=..., seed=True)` publishes the result: the phase times are printed.  The
manifest goes to the hub without payload, so every new byte has to come from the publisher's
resident seeder.  A second set of weights (a fresh pull of revision 1) then pulls the published
revision with `base=` from that seeder, alternating with a plain pull of the same revision from the
same seeder, `--rounds` times, disk xorb cache off.  One JSON line per step.

Publisher and puller share one GPU and one process here, and the plain pull's old bytes come from
the seeder over loopback: read the ratio as "bytes not moved", as for tools/delta_bench.py.

    python tools/publish_bench.py [--mb 1024] [--files 4] [--changed 0.05] [--rounds 2]

`--loose`: the write side for a producer that holds loose tensors.  `--mb` of random bytes laid out
as Llama-3.1-8B-shaped tensors (tools/kbench.py loose_layout: each its own allocation at a staggered
misalignment) are published as a `TensorFile`, and, in the same run, through the route this
replaces: `pack_safetensors` + `publish` of the packed buffer.  Alternated `--rounds` times after a
warm-up of each; one JSON line per publish with the phase times and the peak of
torch.cuda.max_memory_allocated above what was allocated before the call.

    python tools/publish_bench.py --loose [--mb 1024] [--rounds 3]
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
from zest_amd import seed as zseed  # noqa: E402
from zest_amd.publish import ChunkIndex, publish  # noqa: E402
from zest_amd.testing import FakeHub  # noqa: E402


def safetensors(payload: bytes, name: str) -> bytes:
    head = json.dumps({name: {"dtype": "BF16", "shape": [len(payload) // 2],
                              "data_offsets": [0, len(payload)]}}).encode()
    head += b" " * (-len(head) % 8)
    return len(head).to_bytes(8, "little") + head + payload


def bf16(rng, nbytes: int) -> np.ndarray:
    return (rng.normal(0, 0.02, nbytes // 2).astype(np.float32).view(np.uint32) >> 16).astype(np.uint16)


def rounded(d: dict) -> dict:
    return {k: (round(v, 5) if isinstance(v, float) else rounded(v) if isinstance(v, dict) else v)
            for k, v in d.items()}


def loose(a) -> int:
    from kbench import loose_layout, loose_tensors
    from zest_amd.publish import TensorFile, pack_safetensors

    dev = torch.device(a.device)
    tensors = loose_tensors(loose_layout(a.mb << 20), dev)
    sync = lambda: torch.cuda.synchronize(dev)

    def packed_route(st):
        return publish({"model.safetensors": pack_safetensors(tensors)}, stats=st)

    def loose_route(st):
        return publish({"model.safetensors": TensorFile(tensors)}, stats=st)

    routes = (("loose[TensorFile]", loose_route), ("packed[pack_safetensors+publish]", packed_route))
    manifests = {}
    for rnd in range(-1, a.rounds):  # round -1 warms allocator and kernels up
        for name, fn in routes:
            sync()
            torch.cuda.reset_peak_memory_stats(dev)
            before, st = torch.cuda.memory_allocated(dev), {}
            t0 = time.perf_counter()
            pub = fn(st)
            sync()
            dt = time.perf_counter() - t0
            peak = torch.cuda.max_memory_allocated(dev) - before
            manifests[name] = pub.manifest
            del pub
            if rnd >= 0:
                print(json.dumps(rounded({"step": "publish", "route": name, "round": rnd, "s": dt,
                                          "file_gbps": st["bytes"] / dt / 1e9, "peak_bytes_above_start": peak,
                                          "tensors": len(tensors), **st})), flush=True)
    (x, _), (y, _) = routes
    assert manifests[x] == manifests[y], "the two routes published different revisions"
    return 0


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", type=int, default=1024)
    ap.add_argument("--files", type=int, default=4)
    ap.add_argument("--changed", type=float, default=0.05)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--loose", action="store_true", help="loose tensors as a TensorFile against pack + publish")
    a = ap.parse_args()
    if a.loose:
        return loose(a)
    rng = np.random.default_rng(1)
    per = (a.mb << 20) // a.files // 2 * 2
    hub = FakeHub(policy="none")
    hub.start()
    os.environ.update(hub.env(tempfile.mkdtemp(prefix="zest-publish-")))
    os.environ["ZEST_CACHE_WRITES"] = "0"
    net = dict(p2p=False, dht=False, device=a.device)
    sync = lambda: torch.cuda.synchronize(a.device)
    try:
        t0 = time.time()
        hub.add_repo("bench/rev1", {f"m{i}.safetensors": safetensors(bf16(rng, per).tobytes(), f"w{i}")
                                    for i in range(a.files)}, xet_suffixes=(".safetensors",))
        print(json.dumps({"setup": "rev1 published by the hub", "bytes": per * a.files,
                          "s": round(time.time() - t0, 2)}), flush=True)
        w0 = zest_amd.pull("bench/rev1", **net)  # the publisher's weights
        w_peer = zest_amd.pull("bench/rev1", **net)  # a peer that holds the old revision
        sync()
        t0 = time.perf_counter()
        index = ChunkIndex.from_weights(w0)
        sync()
        print(json.dumps({"step": "index", "chunks": len(index), "s": round(time.perf_counter() - t0, 4)}), flush=True)
        reg = int(per * a.changed / 8) // 2 * 2
        for i in range(a.files):  # the training step: new values in place
            t = w0[f"w{i}"]
            for k in range(8):
                at = ((per // 8) * k + 4096) // 2
                t[at:at + reg // 2] = torch.from_numpy(bf16(rng, reg).view(np.int16)).view(torch.bfloat16).to(a.device)
        sync()
        publish(w0, index=index)  # warm-up of allocator and kernels
        st = {}
        sync()
        t0 = time.perf_counter()
        pub = publish(w0, index=index, seed=True, stats=st)
        sync()
        dt = time.perf_counter() - t0
        total = st["bytes"]
        print(json.dumps(rounded({"step": "publish", "s": dt, "file_gbps": total / dt / 1e9, **st})), flush=True)
        hub.add_manifest("bench/rev2", pub.manifest)
        peers = [f"127.0.0.1:{pub.port}"]
        for rnd in range(a.rounds):
            for variant, kw in (("plain", {}), ("delta", {"base": w_peer})):
                served, dst = hub.xorb_bytes_served, {}
                before = pub.server.stats()["bytes_served"]
                sync()
                t0 = time.perf_counter()
                w = zest_amd.pull("bench/rev2", device=a.device, peers=peers, dht=False, stats=dst, **kw)
                sync()
                dt = time.perf_counter() - t0
                row = {"changed": a.changed, "round": rnd, "variant": variant, "s": round(dt, 4), "file_bytes": total,
                       "file_gbps": round(total / dt / 1e9, 3), "hub_served_bytes": hub.xorb_bytes_served - served,
                       "seeder_served_bytes": pub.server.stats()["bytes_served"] - before}
                row.update(rounded(dst.get("delta", {})))
                print(json.dumps(row), flush=True)
                if rnd == 0 and variant == "delta":
                    assert all(torch.equal(w[k], w0[k]) for k in w0), "the pulled revision differs from the published"
                del w
        return 0
    finally:
        zseed.stop_all()
        hub.stop()


if __name__ == "__main__":
    raise SystemExit(main())
