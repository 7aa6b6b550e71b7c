"""zest_amd.publish without a GPU: revision 2 of the delta repo published from CPU tensors against the
index of a CPU pull of revision 1, compared with the plain-Python model (publish_model), with the hub's
own uploader (file hashes, xorb bodies) and pulled back through FakeHub.add_manifest."""
from __future__ import annotations

import json

import numpy as np
import pytest
import torch

import delta_repo as R
import publish_model as M
import zest_amd
from zest_amd.delta import ResidentSet, as_resident_set
from zest_amd.device import VerifyError, Weights
from zest_amd.publish import ChunkIndex, Published, pack_safetensors, publish
from zest_amd.testing import FakeHub

NET = dict(p2p=False, dht=False)
REPO = "org/published"
XORB = 1 << 20


def _u8(data: bytes) -> torch.Tensor:
    return torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy())


def _st(files: dict) -> dict:
    return {p: d for p, d in files.items() if p.endswith(".safetensors")}


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    hub = FakeHub(policy="none", max_xorb_bytes=XORB)
    hub.start()
    mp = pytest.MonkeyPatch()
    try:
        for k, v in hub.env(str(tmp_path_factory.mktemp("publish"))).items():
            mp.setenv(k, v)
        mp.setenv("ZEST_CACHE_WRITES", "0")
        rev1, rev2 = R.revisions()
        hub.add_repo(R.REPO1, rev1, xet_suffixes=(".safetensors",))
        w0 = zest_amd.pull(R.REPO1, device="cpu", **NET)
        index = ChunkIndex.from_weights(w0)
        rows = M.hub_index(hub, R.REPO1)
        stats = {}
        pub = publish({p: _u8(d) for p, d in _st(rev2).items()}, index=index, max_xorb_bytes=XORB, stats=stats)
        ref, manifest = M.expected(_st(rev2), rows, XORB)
        yield {"hub": hub, "rev1": rev1, "rev2": rev2, "w0": w0, "index": index, "rows": rows, "pub": pub,
               "stats": stats, "ref": ref, "manifest": manifest}
    finally:
        mp.undo()
        hub.stop()


def test_index_of_a_pull_lists_its_chunks(world):
    index, rows = world["index"], world["rows"]
    assert len(index) == len(rows) and index.device == torch.device("cpu")
    assert [bytes(h) for h in index.hashes.numpy()] == [h for h, _, _ in rows]
    assert [(index.xorbs[x], c) for x, c in zip(index.xorb_id.tolist(), index.chunk.tolist())] == \
        [(hx, c) for _, hx, c in rows]


def test_manifest_equals_the_model(world):
    pub, want = world["pub"], world["manifest"]
    assert isinstance(pub, Published)
    assert pub.manifest == want
    assert json.loads(json.dumps(pub.manifest)) == want  # plain JSON-able values
    assert [f["path"] for f in pub.manifest["files"]] == sorted(_st(world["rev2"]))
    m, ref = len(world["rows"]), world["ref"]
    own = m + np.arange(len(ref))
    st = world["stats"]
    assert st is not pub.stats and {k: v for k, v in st.items()} == pub.stats
    assert (st["chunks"], st["new_chunks"], st["matched_chunks"], st["duplicate_chunks"]) == \
        (len(ref), int((ref == own).sum()), int((ref < m).sum()), int(((ref >= m) & (ref != own)).sum()))
    assert st["new_chunks"] > 0 and st["matched_chunks"] > 0
    assert st["new_bytes"] + st["matched_bytes"] + st["duplicate_bytes"] == st["bytes"] == \
        sum(len(d) for d in _st(world["rev2"]).values())
    assert st["new_xorbs"] == len(want["xorbs"]) >= 1
    assert set(st["seconds"]) == {"cdc", "select", "hash", "dedup", "plan", "merkle"}
    assert all(v >= 0 for v in st["seconds"].values())


def test_file_hashes_equal_the_hubs_uploader(world):
    hub = world["hub"]
    other = FakeHub(policy="none", max_xorb_bytes=XORB)  # the host uploader, pinned against hf_xet elsewhere
    other.add_repo("org/oracle", world["rev2"], xet_suffixes=(".safetensors",))
    for f in world["pub"].manifest["files"]:
        assert f["xet_hash"] == other.xet_hash("org/oracle", f["path"])
    assert hub.xet_hash(R.REPO1, R.B) == {f["path"]: f["xet_hash"] for f in world["pub"].manifest["files"]}[R.B]


def test_hub_accepts_the_manifest_and_pulls_are_exact(world):
    hub, pub, rev2 = world["hub"], world["pub"], world["rev2"]
    n1 = len(hub.xorbs)
    hub.add_manifest(REPO, pub.manifest, revision="step-2", payload=_st(rev2),
                     extra_files={"config.json": rev2["config.json"]})  # the builders' hashes equal the manifest's
    new = hub.xorbs[n1:]
    assert [x.hash_hex for x in new] == list(pub.manifest["xorbs"])
    new_bytes = sum(len(x.data) for x in new)
    served, stats = hub.xorb_bytes_served, {}
    w1 = zest_amd.pull(REPO, "step-2", device="cpu", base=world["w0"], stats=stats, **NET)
    grew = hub.xorb_bytes_served - served
    R.assert_tensors(w1, rev2)
    assert stats["delta"]["reused_terms"] > 0 and stats["delta"]["refetched_terms"] == 0
    assert 0 < grew <= new_bytes  # the hub serves no more xorb bytes than the new xorbs hold
    w2 = zest_amd.pull(REPO, "step-2", device="cpu", **NET)  # without base=: old xorbs from the hub as well
    R.assert_tensors(w2, rev2)
    # the published resident set serves as a base like a pull's
    stats = {}
    w3 = zest_amd.pull(REPO, "step-2", device="cpu", base=pub, stats=stats, **NET)
    R.assert_tensors(w3, rev2)
    assert stats["delta"]["fetched_terms"] == 0
    assert as_resident_set(pub, "cpu") is pub.resident and isinstance(pub.resident, ResidentSet)
    assert pub.resident.nbytes == sum(len(d) for d in _st(rev2).values())


def test_add_manifest_refuses_what_it_cannot_resolve(world):
    hub, man = world["hub"], world["manifest"]
    hx = next(iter(man["xorbs"]))
    with pytest.raises(ValueError, match=r"does not know and the manifest does not describe"):
        FakeHub().add_manifest("org/x", dict(man, xorbs={}))
    bad = json.loads(json.dumps(man))
    t = next(t for f in bad["files"] for t in f["terms"] if t[0] == hx)
    t[3] += 1
    with pytest.raises(ValueError, match=r"does not match the xorb"):
        hub.add_manifest("org/x", bad)
    flipped = {p: d[:-1] + bytes([d[-1] ^ 1]) if p == R.C else d for p, d in _st(world["rev2"]).items()}
    fresh = FakeHub(policy="none", max_xorb_bytes=XORB)
    fresh.add_repo(R.REPO1, world["rev1"], xet_suffixes=(".safetensors",))
    with pytest.raises(ValueError, match=r"hash to"):
        fresh.add_manifest("org/x", man, payload=flipped)
    with pytest.raises(ValueError, match=r"version"):
        hub.add_manifest("org/x", dict(man, version=2))


def test_index_of_modified_weights_is_refused(world):
    w = zest_amd.pull(R.REPO1, device="cpu", **NET)
    w["a"][1234] ^= 0x10
    with pytest.raises(VerifyError, match=rf"{R.A}.*before modifying the tensors"):
        ChunkIndex.from_weights(w)
    with pytest.raises(ValueError, match=r"from_weights takes the Weights"):
        ChunkIndex.from_weights(dict(w))


def test_zero_filled_tensor_is_stored_once():
    files = {"z.safetensors": R.safetensors(bytes(1_000_000), "z")}
    pub = publish({p: _u8(d) for p, d in files.items()})
    ref, want = M.expected(files)
    assert pub.manifest == want
    st = pub.stats
    # A run of zeros never hits the CDC mask, so it is cut into maximum-size chunks.  Three chunks differ:
    # the first (it starts with the header), one full chunk of zeros, and the shorter tail; every other
    # chunk repeats the full one and is stored once.
    assert st["chunks"] == 8 and st["new_chunks"] == 3 and st["duplicate_chunks"] == 5 and st["matched_chunks"] == 0
    (xorb,) = pub.manifest["xorbs"].values()
    assert xorb["chunk_lens"][:2] == [131072, 131072] and xorb["chunk_lens"][2] < 131072
    assert st["new_bytes"] == sum(xorb["chunk_lens"]) < 3 * 131072
    assert st["new_bytes"] + st["duplicate_bytes"] == st["bytes"] == len(files["z.safetensors"])
    hub = FakeHub()
    hub.add_manifest("org/zero", pub.manifest, payload=files)
    assert sum(len(x.data) for x in hub.xorbs) < 3 * 131072 + 200


def test_unchanged_revision_adds_no_xorb(world):
    pub = publish(world["w0"], index=world["index"], max_xorb_bytes=XORB)
    assert pub.manifest["xorbs"] == {} and pub.stats["new_xorbs"] == 0 and pub.stats["new_chunks"] == 0
    hub = world["hub"]
    for f in pub.manifest["files"]:
        assert f["xet_hash"] == hub.xet_hash(R.REPO1, f["path"])
        want = [(hub.xorbs[x].hash_hex, c0, c1) for x, c0, c1 in hub.repos[("model", R.REPO1)].files[f["path"]].terms]
        assert [tuple(t[:3]) for t in f["terms"]] == want
    assert pub.manifest == M.expected(_st(world["rev1"]), world["rows"], XORB)[1]


def test_chain_of_publishes_after_in_place_edits(world):
    hub = world["hub"]
    w = zest_amd.pull(R.REPO1, device="cpu", **NET)
    index = ChunkIndex.from_weights(w)
    rows = list(world["rows"])
    state = {p: bytearray(d) for p, d in _st(world["rev1"]).items()}
    prev = None
    for step, (name, path, at) in enumerate((("a", R.A, 700_000), ("b", R.B, 123_456)), 1):
        w[name][at:at + 5000] = 7 * step  # in place: the file buffer behind the tensor changes
        off = len(state[path]) - w[name].numel()
        state[path][off + at:off + at + 5000] = bytes([7 * step]) * 5000
        files = {p: bytes(d) for p, d in state.items()}
        pub = publish(w, index=index, max_xorb_bytes=XORB)
        ref, want = M.expected(files, rows, XORB)
        assert pub.manifest == want
        assert 0 < pub.stats["new_chunks"] <= 3 and pub.stats["new_xorbs"] == 1
        if prev is not None:  # step 2 references step 1's new xorb through the chained index
            assert set(prev.manifest["xorbs"]) & {t[0] for f in pub.manifest["files"] for t in f["terms"]}
        hub.add_manifest("org/chain", pub.manifest, revision=f"step-{step}", payload=files)
        got = zest_amd.pull("org/chain", f"step-{step}", device="cpu", base=world["w0"], **NET)
        R.assert_tensors(got, files)
        # the next step's index is this call's: rows in this revision's order, located where the manifest says
        index = pub.index
        rows = [(h, hx, c) for h, (hx, c) in zip(
            [bytes(r) for r in index.hashes.numpy()],
            [(t[0], c) for f in want["files"] for t in f["terms"] for c in range(t[1], t[2])])]
        assert [(index.xorbs[x], c) for x, c in zip(index.xorb_id.tolist(), index.chunk.tolist())] == \
            [(hx, c) for _, hx, c in rows]
        prev = pub


def test_index_union_keeps_the_first_rows_first(world):
    index = world["index"]
    other = world["pub"].index
    both = index | other
    assert len(both) == len(index) + len(other) and both.xorbs[:len(index.xorbs)] == index.xorbs
    assert torch.equal(both.hashes[:len(index)], index.hashes) and torch.equal(both.hashes[len(index):], other.hashes)
    loc = lambda ix: [(ix.xorbs[x], c) for x, c in zip(ix.xorb_id.tolist(), ix.chunk.tolist())]
    assert loc(both) == loc(index) + loc(other)
    pub = publish({p: _u8(d) for p, d in _st(world["rev2"]).items()}, index=both, max_xorb_bytes=XORB)
    assert pub.manifest["xorbs"] == {}
    assert [f["terms"] for f in pub.manifest["files"]] == [f["terms"] for f in world["manifest"]["files"]]


def test_pack_safetensors_round_trips():
    from zest_amd.device import parse_safetensors_header, tensor_views

    ts = {"w": torch.arange(12, dtype=torch.float32).reshape(3, 4), "b": torch.tensor([1, 2, 3], dtype=torch.int16),
          "s": torch.tensor(2.5, dtype=torch.bfloat16), "e": torch.empty(0, dtype=torch.uint8)}
    buf = pack_safetensors(ts, metadata={"step": 3})
    assert buf.dtype == torch.uint8 and buf.dim() == 1 and buf.is_contiguous()
    start, meta = parse_safetensors_header(buf.numpy().tobytes())
    assert meta["__metadata__"] == {"step": "3"} and start % 8 == 0
    views = tensor_views(buf, start, meta)
    assert set(views) == set(ts) and all(torch.equal(views[k], ts[k]) and views[k].dtype == ts[k].dtype for k in ts)
    with pytest.raises(ValueError, match=r"no tensors"):
        pack_safetensors({})
    with pytest.raises(ValueError, match=r"complex64 has no safetensors name"):
        pack_safetensors({"c": torch.zeros(2, dtype=torch.complex64)})


def test_refusals_say_what_to_do(world):
    a = torch.zeros(10_000, dtype=torch.uint8)
    with pytest.raises(ValueError, match=r"file set is empty.*\{path: uint8 tensor"):
        publish({})
    with pytest.raises(ValueError, match=r"empty file set.*unsharded direct pull"):
        publish(Weights())
    with pytest.raises(ValueError, match=r"more than one device \(cpu, meta\).*one device"):
        publish({"a": a, "b": torch.zeros(10, dtype=torch.uint8, device="meta")})
    with pytest.raises(ValueError, match=r"seed= serves from GPU memory.*on cpu.*cuda:N"):
        publish({"a": a}, seed=True)
    with pytest.raises(ValueError, match=r"seed= serves from GPU memory"):
        publish({"a": a}, seed=6881)
    with pytest.raises(ValueError, match=r"index is on meta but the files are on cpu.*index\.to\(device\)"):
        publish({"a": a}, index=ChunkIndex.empty("meta"))
    with pytest.raises(ValueError, match=r"index= takes a ChunkIndex"):
        publish({"a": a}, index=world["w0"])
    with pytest.raises(ValueError, match=r"a must be a contiguous 1-D uint8 tensor.*pack_safetensors"):
        publish({"a": a.view(torch.int16)})
    with pytest.raises(ValueError, match=r"contiguous 1-D uint8"):
        publish({"a": torch.zeros(20_000, dtype=torch.uint8)[::2]})
    with pytest.raises(ValueError, match=r"a is empty"):
        publish({"a": a[:0]})
    with pytest.raises(ValueError, match=r"publish takes"):
        publish([a])


def test_public_names():
    assert zest_amd.ChunkIndex is ChunkIndex
    pub = zest_amd.publish({"x.safetensors": _u8(R.safetensors(bytes(range(256)) * 100, "x"))})
    assert isinstance(pub, Published) and pub.server is None and pub.port is None
    assert pub.manifest == M.expected({"x.safetensors": R.safetensors(bytes(range(256)) * 100, "x")})[1]


def test_weights_metadata_keeps_dict_behaviour(world):
    import pickle

    w0 = world["w0"]
    assert [p for p, _ in w0._meta] == sorted(_st(world["rev1"]))
    assert [h for _, h in w0._meta] == [world["hub"].xet_hash(R.REPO1, p) for p, _ in w0._meta]
    items = pickle.loads(pickle.dumps(dict(w0.items())))
    assert items.keys() == w0.keys() and all(torch.equal(items[k], w0[k]) for k in w0)
    assert w0 == dict(w0) and Weights()._meta == []
