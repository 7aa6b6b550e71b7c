#!/usr/bin/env python3
"""pull(..., into=params) against pull() followed by a copy_ loop, end to end on one GPU.

`--mb` of Llama-3.1-8B-shaped bf16 tensors (file order, the embeddings left out, N(0, 0.02) values)
in `--files` safetensors files with an index are published on an in-process FakeHub (BG4/LZ4 xorbs,
served over loopback HTTP).  The destinations, one separately allocated tensor per checkpoint tensor,
exist before either variant starts.  The two variants alternate, `--rounds` times, with the disk xorb
cache off; each prints its wall time and the peak of torch.cuda.max_memory_allocated above the level
at its start (the destinations are below that level).  `into` runs with a scratch of the largest file
(`--scratch-mb`, 0: the pull's default, which for a model this small is every file at once).

The origin is the FakeHub's Python HTTP server: its rate bounds both variants' wall time alike.  The
figure this tool exists for is the peak.

    python tools/into_bench.py [--mb 1024] [--files 4] [--rounds 3]

`--delta --changed FRACTION`: two revisions of the same tensors, of which about FRACTION of the bytes
(whole tensors, picked at random) are replaced in the second.  A plain `pull(into=)` of revision 2
alternates with `pull(into=, base=landed)` from destinations that hold revision 1 (that pull of
revision 1 is not timed).  Each row has the wall time, the bytes the hub served
(`hub.xorb_bytes_served`), the peak above the start and, for the delta pull, check_s / fetch_s /
apply_s and its counters.

    python tools/into_bench.py --delta --mb 1024 --changed 0.05
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
from zest_amd import models  # noqa: E402
from zest_amd.device import ST_DTYPES  # noqa: E402
from zest_amd.testing import FakeHub  # noqa: E402


def layout(total: int, max_tensor: int = 256 << 20) -> list:
    """TensorSpecs of Llama-3.1-8B in file order up to `total` bytes, tensors over `max_tensor` left out."""
    out, left = [], total
    for t in models.get("llama-3.1-8b").tensors:
        if t.nbytes <= max_tensor and t.nbytes <= left:
            out.append(t)
            left -= t.nbytes
    return out


def bf16(rng, nbytes: int) -> bytes:
    return (rng.normal(0, 0.02, nbytes // 2).astype(np.float32).view(np.uint32) >> 16).astype(np.uint16).tobytes()


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", type=int, default=1024)
    ap.add_argument("--files", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--scratch-mb", type=int, default=-1, help="-1: the largest file; 0: the pull's default")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--delta", action="store_true", help="plain pull(into=) against pull(into=, base=)")
    ap.add_argument("--changed", type=float, default=0.05, help="--delta: fraction of the bytes replaced")
    a = ap.parse_args()
    if a.delta:
        return delta_main(a)
    rng = np.random.default_rng(1)
    specs = layout(a.mb << 20)
    per = -(-sum(t.nbytes for t in specs) // a.files)
    groups, cur, cur_b = [], [], 0
    for t in specs:  # greedy, in order, about equal files
        if cur and cur_b + t.nbytes > per and len(groups) < a.files - 1:
            groups.append(cur)
            cur, cur_b = [], 0
        cur.append(t)
        cur_b += t.nbytes
    groups.append(cur)
    files, weight_map = {}, {}
    for i, g in enumerate(groups):
        head, _ = models.safetensors_header(g)
        path = f"model-{i + 1:05d}-of-{len(groups):05d}.safetensors"
        files[path] = head + b"".join(bf16(rng, t.nbytes) for t in g)
        weight_map.update({t.name: path for t in g})
    sizes = [len(v) for v in files.values()]
    files["model.safetensors.index.json"] = json.dumps({"metadata": {}, "weight_map": weight_map}).encode()
    hub = FakeHub(policy="auto")
    hub.start()
    os.environ.update(hub.env(tempfile.mkdtemp(prefix="zest-into-")))
    os.environ["ZEST_CACHE_WRITES"] = "0"
    net = dict(p2p=False, dht=False, device=a.device)
    cuda = a.device.startswith("cuda")
    sync = torch.cuda.synchronize if cuda else (lambda: None)
    try:
        t0 = time.time()
        hub.add_repo("bench/into", files, xet_suffixes=(".safetensors",))
        model_bytes = sum(t.nbytes for t in specs)
        print(json.dumps({"setup": "published", "tensors": len(specs), "model_bytes": model_bytes, "file_sizes": sizes,
                          "s": round(time.time() - t0, 2)}), flush=True)
        dests = {t.name: torch.empty(t.shape, dtype=ST_DTYPES[t.dtype], device=a.device) for t in specs}
        scratch = max(sizes) if a.scratch_mb < 0 else (a.scratch_mb << 20) or None
        w = zest_amd.pull("bench/into", **net)  # warm-up of connections, allocator and kernels; also the reference
        want = {k: v.clone() for k, v in w.items()} if not cuda else {k: v.cpu() for k, v in w.items()}
        del w
        for rnd in range(a.rounds):
            for variant in ("copy", "into"):
                for d in dests.values():
                    d.zero_()
                if cuda:
                    torch.cuda.empty_cache()
                    sync()
                    torch.cuda.reset_peak_memory_stats(a.device)
                    level = torch.cuda.memory_allocated(a.device)
                st = {}
                t0 = time.perf_counter()
                if variant == "copy":
                    w = zest_amd.pull("bench/into", **net)
                    for k, d in dests.items():
                        d.copy_(w[k])
                    sync()
                    del w
                else:
                    zest_amd.pull("bench/into", into=dests, scratch_bytes=scratch, stats=st, **net)
                dt = time.perf_counter() - t0
                row = {"round": rnd, "variant": variant, "s": round(dt, 4), "model_bytes": model_bytes,
                       "file_gbps": round(sum(sizes) / dt / 1e9, 3)}
                if cuda:
                    row["peak_above_start"] = torch.cuda.max_memory_allocated(a.device) - level
                    row["peak_over_model"] = round(row["peak_above_start"] / model_bytes, 3)
                row.update({k: (round(v, 5) if isinstance(v, float) else v) for k, v in st.get("into", {}).items()
                            if k not in ("skipped_files", "missing")})
                print(json.dumps(row), flush=True)
                assert all(torch.equal(d.cpu().view(torch.uint8), want[k].view(torch.uint8)) for k, d in dests.items())
        return 0
    finally:
        hub.stop()


def delta_main(a) -> int:
    rng = np.random.default_rng(1)
    specs = layout(a.mb << 20)
    model_bytes = sum(t.nbytes for t in specs)
    per = -(-model_bytes // a.files)
    groups, cur, cur_b = [], [], 0
    for t in specs:
        if cur and cur_b + t.nbytes > per and len(groups) < a.files - 1:
            groups.append(cur)
            cur, cur_b = [], 0
        cur.append(t)
        cur_b += t.nbytes
    groups.append(cur)
    changed, left = set(), a.changed * model_bytes
    for i in rng.permutation(len(specs)).tolist():  # whole tensors until the fraction is reached
        if left <= 0:
            break
        changed.add(specs[i].name)
        left -= specs[i].nbytes
    raw1 = {t.name: bf16(rng, t.nbytes) for t in specs}
    raw2 = {t.name: bf16(rng, t.nbytes) if t.name in changed else raw1[t.name] for t in specs}
    revs = []
    for raw in (raw1, raw2):
        files, weight_map = {}, {}
        for i, g in enumerate(groups):
            head, _ = models.safetensors_header(g)
            path = f"model-{i + 1:05d}-of-{len(groups):05d}.safetensors"
            files[path] = head + b"".join(raw[t.name] for t in g)
            weight_map.update({t.name: path for t in g})
        files["model.safetensors.index.json"] = json.dumps({"metadata": {}, "weight_map": weight_map}).encode()
        revs.append(files)
    hub = FakeHub(policy="auto")
    hub.start()
    os.environ.update(hub.env(tempfile.mkdtemp(prefix="zest-into-delta-")))
    os.environ["ZEST_CACHE_WRITES"] = "0"
    net = dict(p2p=False, dht=False, device=a.device)
    cuda = a.device.startswith("cuda")
    sync = torch.cuda.synchronize if cuda else (lambda: None)
    try:
        t0 = time.time()
        for repo, files in zip(("bench/into-1", "bench/into-2"), revs):
            hub.add_repo(repo, files, xet_suffixes=(".safetensors",))
        changed_bytes = sum(t.nbytes for t in specs if t.name in changed)
        print(json.dumps({"setup": "published", "tensors": len(specs), "model_bytes": model_bytes,
                          "changed_tensors": len(changed), "changed_bytes": changed_bytes,
                          "s": round(time.time() - t0, 2)}), flush=True)
        dests = {t.name: torch.empty(t.shape, dtype=ST_DTYPES[t.dtype], device=a.device) for t in specs}
        want = {k: torch.frombuffer(bytearray(v), dtype=torch.uint8) for k, v in raw2.items()}
        zest_amd.pull("bench/into-2", into=dests, **net)  # warm-up of connections, allocator and kernels
        for rnd in range(a.rounds):
            for variant in ("plain", "delta"):
                landed = zest_amd.pull("bench/into-1", into=dests, **net)  # not timed: the model holds revision 1
                if cuda:
                    torch.cuda.empty_cache()
                    sync()
                    torch.cuda.reset_peak_memory_stats(a.device)
                    level = torch.cuda.memory_allocated(a.device)
                st, served = {}, hub.xorb_bytes_served
                t0 = time.perf_counter()
                if variant == "plain":
                    zest_amd.pull("bench/into-2", into=dests, stats=st, **net)
                else:
                    zest_amd.pull("bench/into-2", into=dests, base=landed, stats=st, **net)
                dt = time.perf_counter() - t0
                row = {"round": rnd, "variant": variant, "s": round(dt, 4), "model_bytes": model_bytes,
                       "hub_bytes": hub.xorb_bytes_served - served}
                if cuda:
                    row["peak_above_start"] = torch.cuda.max_memory_allocated(a.device) - level
                    row["peak_over_model"] = round(row["peak_above_start"] / model_bytes, 4)
                d = st["into"].get("delta", {})
                row.update({k: (round(v, 5) if isinstance(v, float) else v) for k, v in d.items() if k != "files"})
                print(json.dumps(row), flush=True)
                del landed
                assert all(torch.equal(t.cpu().reshape(-1).view(torch.uint8), want[k]) for k, t in dests.items())
        return 0
    finally:
        hub.stop()


if __name__ == "__main__":
    raise SystemExit(main())
