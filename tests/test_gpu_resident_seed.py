"""GPU: seeding a device pull's weights straight from the HBM they live in
(`pull(..., device="cuda:0", seed=True)` -> seed.ResidentSeedServer -> _hip.HbmSeeder resident runs
-> csrc/gpu/serve.hip).  A `zest pull` leecher gets 100 % of the bytes from it with the CDN dead."""
from __future__ import annotations

import gc
import json
import struct

import numpy as np
import pytest
import torch

import serve_pack_model as M
from e2e_util import Node, assert_snapshot, free_port, p2p_ratio, sample_files
from zest_amd import _core, ops
from zest_amd import seed as zseed
from zest_amd.testing import FakeHub

pytestmark = pytest.mark.gpu

REPO = "org/resident"


def _safetensors(payload: bytes, name: str) -> bytes:
    head = json.dumps({name: {"dtype": "U8", "shape": [len(payload)], "data_offsets": [0, len(payload)]}}).encode()
    head += b" " * (-len(head) % 8)
    return struct.pack("<Q", len(head)) + head + payload


def _files() -> dict[str, bytes]:
    """sample_files with its weights wrapped as real safetensors, plus a second weights file that
    shares 1.5 MB with the first: its reconstruction points into the first file's xorbs (terms that
    start at a non-zero chunk), and its own chunks continue the xorb the first file left open."""
    files = sample_files(seed=7)
    big = files["model.safetensors"]
    rng = np.random.default_rng(8)
    other = rng.integers(0, 256, 700_000, dtype=np.uint8).tobytes()
    files["model.safetensors"] = _safetensors(big, "w")
    files["model-b.safetensors"] = _safetensors(other[:300_000] + big[500_000:2_000_000] + other[300_000:], "v")
    return files


@pytest.fixture(scope="module")
def seeded(tmp_path_factory):
    import zest_amd

    root = tmp_path_factory.mktemp("resident")
    hub = FakeHub(policy="auto", max_xorb_bytes=1 << 20)
    hub.start()
    mp = pytest.MonkeyPatch()
    state = {"hub": hub, "root": root, "files": _files()}
    try:
        state["commit"] = hub.add_repo(REPO, state["files"], xet_suffixes=(".safetensors",))
        for k, v in hub.env(str(root / "a")).items():
            mp.setenv(k, v)
        mp.setenv("ZEST_LISTEN_PORT", str(free_port()))
        state["tensors"] = zest_amd.pull(REPO, device="cuda:0", seed=True, p2p=False)
        state["gets"] = hub.counters.get("xorb_get", 0)
        hub.fail_xorbs = {x.hash_hex for x in hub.xorbs}  # from here on the CDN is dead
        (state["srv"],) = zseed.active()
        yield state
    finally:
        zseed.stop_all()
        mp.undo()
        hub.stop()


def _xorb_terms(hub):
    """{xorb index: sorted [(c0, c1), ...]} over every file's reconstruction."""
    out = {}
    for f in hub.file_index.values():
        for x, c0, c1 in f.terms:
            out.setdefault(x, set()).add((c0, c1))
    return {x: sorted(v) for x, v in out.items()}


def _fetch_and_check(hub, port, x, a, b):
    xorb = hub.xorbs[x]
    h = _core.from_xet_hex(xorb.hash_hex)
    conn = _core.PeerConnection(f"127.0.0.1:{port}", h)
    data, off = conn.fetch(h, a, b)
    assert off == a
    idx = _core.index_chunks(data)
    assert [(e[2], e[3]) for e in idx] == [(0, n) for n in xorb.ulens[a:b]]  # scheme 0, exactly chunks [a, b)
    want = _core.extract_chunk_range(xorb.data, a, b)
    assert _core.extract_chunk_range(data, 0, b - a) == want
    chunks = [want[xorb.cum[i] - xorb.cum[a]:xorb.cum[i + 1] - xorb.cum[a]] for i in range(a, b)]
    assert bytes(data) == M.serialize(chunks)


def test_leecher_pulls_everything_from_resident_hbm(seeded):
    hub, srv = seeded["hub"], seeded["srv"]
    assert srv.xorbs == sorted(x.hash_hex for x in hub.xorbs)
    assert any(len(t) > 1 for t in _xorb_terms(hub).values()), "the files must share / split xorbs"
    assert srv.stats()["resident_runs"] == len(srv.seeder) == len(hub.xorbs)  # every xorb merged into one run
    node = Node(hub, seeded["root"], "leecher")
    try:
        out = node.run("pull", REPO, "--peer", f"127.0.0.1:{srv.port}", "--no-dht").stdout
        assert p2p_ratio(out) == 100.0
        assert hub.counters.get("xorb_get", 0) == seeded["gets"]
        assert_snapshot(node, REPO, seeded["commit"], seeded["files"])
    finally:
        node.close()
    st = srv.stats()
    assert st["not_found"] == 0 and st["chunks_served"] > 0


def test_direct_fetch_across_a_term_boundary(seeded):
    hub, srv = seeded["hub"], seeded["srv"]
    for x, terms in _xorb_terms(hub).items():
        n = len(hub.xorbs[x].ulens)
        cuts = [c for c0, c1 in terms for c in (c0, c1) if 1 < c < n - 1]
        if cuts:
            e = cuts[0]
            _fetch_and_check(hub, srv.port, x, e - 2, e + 2)
            _fetch_and_check(hub, srv.port, x, e - 1, e + 1)
            break
    else:
        raise AssertionError("no xorb with a term boundary inside it")
    assert srv.stats()["not_found"] == 0


def test_unsupported_combinations_raise():
    import zest_amd

    with pytest.raises(ValueError, match="device='all'"):
        zest_amd.pull(REPO, device="all", seed=True)
    with pytest.raises(ValueError, match="direct=False"):
        zest_amd.pull(REPO, device="cuda:0", direct=False, seed=True)
    with pytest.raises(ValueError, match="cpu"):
        from zest_amd.direct import pull_to_device

        pull_to_device(REPO, device="cpu", seed=True)


def _one_chunk_seeder(length: int, from_end: int):
    """A seeder with one registered 4 KiB buffer and tables for one chunk of `length` bytes that
    starts `from_end` bytes before the buffer's end."""
    dev = torch.device("cuda:0")
    buf = ops.padded_empty(4096, dev)
    buf.copy_(torch.arange(4096, device=dev).to(torch.uint8))
    tab = torch.tensor([buf.data_ptr() + 4096 - from_end, length + 8], dtype=torch.int64).to(dev)
    torch.cuda.synchronize(dev)
    s = ops.hip().HbmSeeder(0, 0, 0, 0, False)
    s.add_resident_buffer(buf.data_ptr(), 4096)
    return s, buf, tab


def test_registration_rejects_a_chunk_past_its_buffer():
    h = bytes(range(32))
    s, buf, tab = _one_chunk_seeder(101, 100)  # one byte past the registered buffer
    with pytest.raises(_core.ZestError, match="outside every registered buffer"):
        s.add_resident_run(_core.xet_hex(h), 0, tab.data_ptr(), tab.data_ptr() + 8, [109])
    with pytest.raises(_core.ZestError, match="differs"):  # host ends must be what the kernel would read
        s.add_resident_run(_core.xet_hex(h), 0, tab.data_ptr(), tab.data_ptr() + 8, [108])
    with pytest.raises(_core.ZestError):  # unregistered memory is no buffer
        s.add_resident_buffer(0x1000, 4096)
    assert len(s) == 0 and s.stats()["resident_runs"] == 0
    s.start()
    try:
        with pytest.raises(Exception):
            _core.PeerConnection(f"127.0.0.1:{s.port}", h).fetch(h, 0, 1, 2000)
        assert s.stats()["chunks_served"] == 0 and s.stats()["bytes_served"] == 0
    finally:
        s.stop()


def test_registered_run_serves_exact_bytes():
    h = bytes(range(32))
    s, buf, tab = _one_chunk_seeder(100, 100)  # ends exactly at the buffer's last byte
    s.add_resident_run(_core.xet_hex(h), 0, tab.data_ptr(), tab.data_ptr() + 8, [108])
    assert len(s) == 1 and s.stats()["resident_runs"] == 1
    s.start()
    try:
        data, off = _core.PeerConnection(f"127.0.0.1:{s.port}", h).fetch(h, 0, 1)
        assert off == 0 and bytes(data) == M.header(100) + buf[-100:].cpu().numpy().tobytes()
    finally:
        s.stop()


def test_lifecycle_server_outlives_the_tensors(seeded):
    import zest_amd

    hub, srv = seeded["hub"], seeded["srv"]
    assert zseed.active() == [srv]
    seeded.pop("tensors").clear()
    gc.collect()
    torch.cuda.empty_cache()
    junk = torch.full((8 << 20,), 0x5A, dtype=torch.uint8, device="cuda:0")  # would reuse freed blocks
    torch.cuda.synchronize()
    x = max(range(len(hub.xorbs)), key=lambda i: len(hub.xorbs[i].ulens))
    _fetch_and_check(hub, srv.port, x, 0, len(hub.xorbs[x].ulens))
    del junk
    port = srv.port
    zest_amd.seed.stop_all()
    assert zseed.active() == [] and srv.stats()["chunks_served"] > 0
    with pytest.raises(Exception):
        h = _core.from_xet_hex(hub.xorbs[x].hash_hex)
        _core.PeerConnection(f"127.0.0.1:{port}", h, 1000).fetch(h, 0, 1, 1000)
