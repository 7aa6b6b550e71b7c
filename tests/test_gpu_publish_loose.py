"""GPU: zest_amd.publish of loose tensors (TensorFile: K14 over the segment list, chunk hashes at
absolute addresses, a seam arena for the chunks that cross a tensor boundary).  The manifest equals
the packed file's and the plain-Python model's, every resident address lies in a tensor, a header
tensor or the seam arena, publishing does not allocate a copy of the model, and a seeded revision is
pulled back, plain and as a delta after one tensor was edited in place, from the publisher's HBM."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import publish_model as M
import zest_amd
from e2e_util import free_port
from zest_amd import seed as zseed
from zest_amd.publish import TensorFile, pack_safetensors, publish
from zest_amd.testing import FakeHub

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
REPO = "org/published-loose"
XORB = 1 << 20
F1, F2, F3 = "model-1.safetensors", "model-2.safetensors", "model-3.safetensors"


def _u8(n: int, g) -> torch.Tensor:
    return torch.randint(0, 256, (n,), generator=g, dtype=torch.uint8).to(DEV)


def _sources():
    """Two files of loose tensors, 1 to 2 MiB each: bf16 / fp32 / uint8, a run of small tensors of 100
    bytes in all, views at odd byte and odd element offsets into larger storages, a tied pair; and one
    plain file buffer."""
    g = torch.Generator().manual_seed(31)
    store = _u8(700_001, g)
    wide = torch.randn(150_000, generator=g).to(DEV)
    t1 = {"embed": torch.randn(256, 700, generator=g).to(DEV).to(torch.bfloat16),
          "odd.u8": store[1:300_002],                     # starts one byte into its storage
          "s0": _u8(1, g), "s1": _u8(2, g), "s2": _u8(33, g), "s3": _u8(64, g),   # 100 bytes in four tensors
          "wide.f32": wide[3:100_003].reshape(400, 250),  # 12 bytes into its storage
          "tail.u8": store[300_005:700_001]}              # ends with its storage's last byte
    t2 = {"a.f32": torch.randn(120_000, generator=g).to(DEV),
          "none": torch.zeros((0, 8), dtype=torch.float16, device=DEV),
          "b.bf16": torch.randn(333, 777, generator=g).to(DEV).to(torch.bfloat16),
          "tied": wide[3:100_003].reshape(400, 250),      # the same memory as model-1's wide.f32
          "c.u8": _u8(99_999, g)}
    t3 = {"plain": _u8(1_200_000, g)}
    torch.cuda.synchronize()
    return t1, t2, t3


def _rows(index):
    """A ChunkIndex as publish_model's index rows."""
    hs = index.hashes.cpu().numpy()
    return [(bytes(hs[r]), index.xorbs[int(index.xorb_id[r])], int(index.chunk[r])) for r in range(len(index))]


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    hub = FakeHub(policy="none", max_xorb_bytes=XORB)
    hub.start()
    mp = pytest.MonkeyPatch()
    try:
        for k, v in hub.env(str(tmp_path_factory.mktemp("loosepublish"))).items():
            mp.setenv(k, v)
        mp.setenv("ZEST_CACHE_WRITES", "0")  # no disk xorb cache: what is not resident crosses the network
        mp.setenv("ZEST_LISTEN_PORT", str(free_port()))
        t1, t2, t3 = _sources()
        md = {"format": "pt", "step": 1}
        packed = {F1: pack_safetensors(t1, md), F2: pack_safetensors(t2), F3: pack_safetensors(t3)}
        assert all(1 << 20 <= b.numel() <= 2 << 20 for b in packed.values())
        yield {"hub": hub, "t": (t1, t2, t3), "md": md, "packed": packed,
               "bytes": {p: b.cpu().numpy().tobytes() for p, b in packed.items()}}
    finally:
        zseed.stop_all()
        mp.undo()
        hub.stop()


def _files(world):
    t1, t2, _ = world["t"]
    return {F1: TensorFile(t1, world["md"]), F2: TensorFile(t2), F3: world["packed"][F3]}


def _inside(a: int, n: int, t: torch.Tensor) -> bool:
    return t.data_ptr() <= a and a + n <= t.data_ptr() + t.numel() * t.element_size()


def test_manifest_equals_the_packed_files_and_the_model(world):
    stats = {}
    pub = publish(_files(world), max_xorb_bytes=XORB, stats=stats)
    ref = publish(world["packed"], max_xorb_bytes=XORB)
    assert pub.manifest == ref.manifest
    assert pub.manifest == M.expected(world["bytes"], (), XORB)[1]
    assert [bytes(h) for h in pub.index.hashes.cpu().numpy()] == [bytes(h) for h in ref.index.hashes.cpu().numpy()]
    t1, t2, _ = world["t"]
    segments = 2 + sum(1 for t in list(t1.values()) + list(t2.values()) if t.numel())
    assert stats["segments"] == segments
    assert 0 < stats["seam_chunks"] <= segments - 2
    assert 0 < stats["seam_bytes"] <= 131072 * (segments - 1)
    assert set(stats) - set(ref.stats) == {"segments", "seam_chunks", "seam_bytes"}
    assert set(stats["seconds"]) - set(ref.stats["seconds"]) == {"seam"}
    assert stats["chunks"] == ref.stats["chunks"] and stats["bytes"] == sum(len(d) for d in world["bytes"].values())
    print(f"publish loose stats {stats}")

    # every resident address lies in a source tensor, a header tensor or the seam arena, and the
    # buffers that are not views of the sources are no larger than headers + seams
    sources = [t for ts in world["t"][:2] for t in ts.values() if t.numel()] + [world["packed"][F3]]
    extra = [b for b in pub.resident.buffers if not any(_inside(b.data_ptr(), b.numel(), s) for s in sources)]
    heads = sorted(len(TensorFile(ts, m).header) for ts, m in ((t1, world["md"]), (t2, None)))
    assert sorted(b.numel() for b in extra) == sorted(heads + [stats["seam_bytes"]])
    n = 0
    for runs in pub.resident.plan.values():
        for _, addrs, lens in runs:
            for a, ln in zip(addrs.tolist(), lens.tolist()):
                assert any(_inside(a, ln, b) for b in pub.resident.buffers), hex(a)
                n += 1
    assert n == len(pub.resident) and pub.resident.nbytes == stats["new_bytes"] + stats["matched_bytes"]
    # and the bytes at those addresses are the chunks: re-hash them where the plan says they lie
    (hx, runs), = list(pub.resident.plan.items())[:1]
    first, addrs, lens = runs[0]
    again = torch.zeros((len(addrs), 32), dtype=torch.uint8, device=DEV)
    zest_amd.ops.hash_chunks_at(addrs, lens, again, np.arange(len(addrs)), buffers=pub.resident.buffers)
    want = pub.manifest["xorbs"][hx]["chunk_lens"][first:first + len(addrs)]
    assert lens.tolist() == want
    leaves = [(bytes(h), int(n)) for h, n in zip(again.cpu().numpy(), lens)]
    if first == 0 and len(addrs) == len(pub.manifest["xorbs"][hx]["chunk_lens"]):
        assert zest_amd._core.xet_hex(zest_amd._core.merkle_root(leaves)) == hx


def test_publishing_does_not_copy_the_model():
    """Four tensors of 8 MiB: tables, hash scratch (32 B per KiB), candidates and at most 3 x 128 KiB
    of seams are a few MiB; a packed copy would be 32 MiB."""
    g = torch.Generator().manual_seed(32)
    ts = {f"t{i}": _u8(8 << 20, g) for i in range(4)}
    total = 4 * (8 << 20)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    pub = publish({"big.safetensors": TensorFile(ts)}, max_xorb_bytes=8 << 20)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated()
    print(f"publish of {total} loose bytes: peak {peak - before} bytes above {before}; stats {pub.stats}")
    assert peak - before < total // 4
    assert pub.stats["bytes"] == total + len(TensorFile(ts).header) and pub.stats["seam_bytes"] <= 4 * 131072
    assert pub.resident.nbytes == pub.stats["bytes"]


def _assert_pulled(w, tensor_sets):
    want = {k: t for ts in tensor_sets for k, t in ts.items()}
    assert set(w.keys()) == set(want)
    for name, t in want.items():
        got = w[name]
        assert got.dtype == t.dtype and tuple(got.shape) == tuple(t.shape), name
        assert torch.equal(got.to(DEV), t), name


def test_seeded_loose_tensors_are_pulled_back_plain_and_as_a_delta(world):
    hub = world["hub"]
    t1, t2, t3 = world["t"]
    assert zseed.active() == []
    pub = publish(_files(world), max_xorb_bytes=XORB, seed=True)
    try:
        hub.add_manifest(REPO, pub.manifest, revision="step-1")  # no payload: the hub answers 404 for the xorbs
        served = hub.xorb_bytes_served
        w1 = zest_amd.pull(REPO, "step-1", device=DEV, peers=[f"127.0.0.1:{pub.port}"], dht=False)
        _assert_pulled(w1, (t1, t2, t3))
        assert hub.xorb_bytes_served == served and pub.server.stats()["not_found"] == 0
    finally:
        zseed.stop_all()  # the seeded tensors are about to change

    # one tensor edited in place, republished against the first call's index
    t1["odd.u8"][100_000:100_700] ^= 0x5A
    torch.cuda.synchronize()
    files2 = {F1: pack_safetensors(t1, world["md"]).cpu().numpy().tobytes(), F2: world["bytes"][F2],
              F3: world["bytes"][F3]}
    ref, want = M.expected(files2, _rows(pub.index), XORB)
    m = len(pub.index)
    new = int((ref == m + np.arange(len(ref))).sum())
    assert 0 < new < len(ref) // 4  # the chunks the 700 edited bytes touch, until the boundaries meet again
    pub2 = publish(_files(world), index=pub.index, max_xorb_bytes=XORB, seed=True)
    try:
        assert pub2.manifest == want
        assert pub2.stats["new_chunks"] == new and pub2.stats["matched_chunks"] == len(ref) - new
        hub.add_manifest(REPO, pub2.manifest, revision="step-2")
        new_terms = [t for f in pub2.manifest["files"] for t in f["terms"] if t[0] in pub2.manifest["xorbs"]]
        served, stats = hub.xorb_bytes_served, {}
        w2 = zest_amd.pull(REPO, "step-2", device=DEV, base=w1, peers=[f"127.0.0.1:{pub2.port}"], dht=False,
                           stats=stats)
        _assert_pulled(w2, (t1, t2, t3))
        d = stats["delta"]
        assert hub.xorb_bytes_served == served
        assert d["fetched_terms"] == len(new_terms) and d["refetched_terms"] == 0
        assert d["fetched_bytes"] == sum(t[3] for t in new_terms) == pub2.stats["new_bytes"]
        st = pub2.server.stats()
        assert st["not_found"] == 0 and st["chunks_served"] >= new
    finally:
        zseed.stop_all()
    assert zseed.active() == []


def test_refusals_on_the_device(world):
    t1, _, _ = world["t"]
    a = t1["embed"]
    with pytest.raises(ValueError, match=r"TensorFile: t is not contiguous"):
        TensorFile({"t": a.t()})
    with pytest.raises(ValueError, match=r"TensorFile: tensors on more than one device \(cpu, cuda:0\)"):
        TensorFile({"a": a, "b": a.cpu()})
    with pytest.raises(ValueError, match=r"publish: files on more than one device \(cpu, cuda:0\)"):
        publish({"a": TensorFile({"a": a}), "b": TensorFile({"b": a.cpu()})})
    with pytest.raises(ValueError, match=r"publish: files on more than one device \(cpu, cuda:0\)"):
        publish({"a": TensorFile({"a": a}), "b": world["packed"][F3].cpu()})
    with pytest.raises(ValueError, match=r"index is on cpu but the files are on cuda:0"):
        publish({"a": TensorFile({"a": a})}, index=zest_amd.ChunkIndex.empty("cpu"))
