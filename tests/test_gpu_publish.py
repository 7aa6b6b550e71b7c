"""GPU: zest_amd.publish from HBM.  The manifest of buffers on cuda:0 (K5 + K1 + K13 + K2) equals the
plain-Python model's, and a revision published with seed=True is pulled back, delta and plain, with
every new byte served from the publisher's HBM by the resident seeder."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import delta_repo as R
import publish_model as M
import zest_amd
from e2e_util import free_port
from zest_amd import _core
from zest_amd import seed as zseed
from zest_amd.publish import ChunkIndex, pack_safetensors, publish
from zest_amd.testing import FakeHub

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NET = dict(p2p=False, dht=False)
REPO = "org/published-gpu"
XORB = 1 << 20


def _st(files: dict) -> dict:
    return {p: d for p, d in files.items() if p.endswith(".safetensors")}


def _dev(data: bytes) -> torch.Tensor:
    return torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).to(DEV)


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    hub = FakeHub(policy="none", max_xorb_bytes=XORB)
    hub.start()
    mp = pytest.MonkeyPatch()
    try:
        for k, v in hub.env(str(tmp_path_factory.mktemp("gpupublish"))).items():
            mp.setenv(k, v)
        mp.setenv("ZEST_CACHE_WRITES", "0")  # no disk xorb cache: what is not resident crosses the network
        mp.setenv("ZEST_LISTEN_PORT", str(free_port()))
        rev1, rev2 = R.revisions()
        hub.add_repo(R.REPO1, rev1, xet_suffixes=(".safetensors",))
        w0 = zest_amd.pull(R.REPO1, device=DEV, **NET)
        index = ChunkIndex.from_weights(w0)
        # revision 2 on the device; file C goes through pack_safetensors, so its bytes are that buffer's
        bufs = {p: _dev(d) for p, d in _st(rev2).items() if p != R.C}
        c = rev2[R.C]
        bufs[R.C] = pack_safetensors({"c": _dev(c[len(c) - 600_000:])})
        files = {p: b.cpu().numpy().tobytes() for p, b in bufs.items()}
        assert files[R.A] == rev2[R.A] and len(files[R.C]) > 600_000
        yield {"hub": hub, "rev1": rev1, "files": files, "bufs": bufs, "w0": w0, "index": index,
               "rows": M.hub_index(hub, R.REPO1)}
    finally:
        zseed.stop_all()
        mp.undo()
        hub.stop()


def test_manifest_from_hbm_equals_the_model(world):
    index, rows = world["index"], world["rows"]
    assert index.device == torch.device(DEV) and len(index) == len(rows)
    assert [bytes(h) for h in index.hashes.cpu().numpy()] == [h for h, _, _ in rows]
    stats = {}
    pub = publish(world["bufs"], index=index, max_xorb_bytes=XORB, stats=stats)
    ref, want = M.expected(world["files"], rows, XORB)
    assert pub.manifest == want
    m = len(rows)
    own = m + np.arange(len(ref))
    assert (stats["new_chunks"], stats["matched_chunks"], stats["duplicate_chunks"]) == \
        (int((ref == own).sum()), int((ref < m).sum()), int(((ref >= m) & (ref != own)).sum()))
    assert stats["new_chunks"] > 0 and stats["matched_chunks"] > 0 and pub.server is None
    assert pub.index.device == torch.device(DEV) and pub.resident.device == torch.device(DEV)
    assert pub.resident.nbytes == sum(len(d) for d in world["files"].values())
    print(f"publish stats {stats}")


def test_weights_edited_in_place_publish_their_current_bytes(world):
    w = zest_amd.pull(R.REPO1, device=DEV, **NET)
    index = ChunkIndex.from_weights(w)
    w["a"][1_000_000:1_003_000] = 9  # in place: the file buffer behind the tensor changes
    torch.cuda.synchronize()
    state = dict(_st(world["rev1"]))
    a = bytearray(state[R.A])
    off = len(a) - w["a"].numel()
    a[off + 1_000_000:off + 1_003_000] = bytes([9]) * 3000
    state[R.A] = bytes(a)
    pub = publish(w, index=index, max_xorb_bytes=XORB)
    assert pub.manifest == M.expected(state, world["rows"], XORB)[1]
    assert 0 < pub.stats["new_chunks"] <= 3
    with pytest.raises(zest_amd.device.VerifyError, match=rf"{R.A}.*before modifying the tensors"):
        ChunkIndex.from_weights(w)


@pytest.fixture(scope="module")
def seeded(world):
    hub = world["hub"]
    assert zseed.active() == []
    pub = publish(world["bufs"], index=world["index"], max_xorb_bytes=XORB, seed=True)
    (srv,) = zseed.active()
    assert srv is pub.server and pub.port == srv.port
    n1 = len(hub.xorbs)
    hub.add_manifest(REPO, pub.manifest, revision="step-2")  # no payload: new xorbs answer 404 at the hub
    assert all(x.data is None for x in hub.xorbs[n1:]) and len(hub.xorbs) - n1 == len(pub.manifest["xorbs"])
    yield {"pub": pub, "srv": srv, "n1": n1}
    zseed.stop_all()
    assert zseed.active() == []


def test_delta_pull_takes_every_new_byte_from_the_publishers_hbm(world, seeded):
    hub, srv = world["hub"], seeded["srv"]
    served, missing, stats = hub.xorb_bytes_served, hub.counters.get("xorb_missing", 0), {}
    w1 = zest_amd.pull(REPO, "step-2", device=DEV, base=world["w0"], peers=[f"127.0.0.1:{srv.port}"], dht=False,
                       stats=stats)
    R.assert_tensors(w1, world["files"])
    assert hub.xorb_bytes_served == served  # the hub served no xorb payload byte
    assert hub.counters.get("xorb_missing", 0) == missing
    d = stats["delta"]
    assert d["reused_terms"] > 0 and d["fetched_terms"] > 0 and d["refetched_terms"] == 0
    new_bytes = seeded["pub"].stats["new_bytes"]
    assert d["fetched_bytes"] >= new_bytes
    st = srv.stats()
    assert st["not_found"] == 0 and st["chunks_served"] > 0
    assert all(t.device == torch.device(DEV) for t in w1.values())


def test_plain_pull_gets_old_xorb_chunks_from_their_new_addresses(world, seeded):
    hub, srv = world["hub"], seeded["srv"]
    served = hub.xorb_bytes_served
    w = zest_amd.pull(REPO, "step-2", device=DEV, peers=[f"127.0.0.1:{srv.port}"], dht=False)
    R.assert_tensors(w, world["files"])
    assert hub.xorb_bytes_served == served  # old xorbs too: the publisher serves the chunks the revision references
    assert srv.stats()["not_found"] == 0


def test_direct_fetches_of_a_new_and_a_referenced_old_xorb(world, seeded):
    hub, srv, pub = world["hub"], seeded["srv"], seeded["pub"]
    files = world["files"]

    def term_bytes(want_new: bool):
        """(xorb hex, c0, c1, the bytes of those chunks in the published files) of the first such term."""
        for f in pub.manifest["files"]:
            pos = 0
            for hx, c0, c1, ulen in f["terms"]:
                if (hx in pub.manifest["xorbs"]) == want_new and c1 - c0 >= 2:
                    return hx, c0, c1, files[f["path"]][pos:pos + ulen]
                pos += ulen
        raise AssertionError("no such term")

    for want_new in (True, False):
        hx, c0, c1, want = term_bytes(want_new)
        h = _core.from_xet_hex(hx)
        data, off = _core.PeerConnection(f"127.0.0.1:{srv.port}", h).fetch(h, c0, c1)
        assert off == c0
        assert [(e[2], e[3]) for e in _core.index_chunks(data)] == \
            [(0, n) for n in (pub.manifest["xorbs"][hx]["chunk_lens"] if want_new
                              else hub.xorbs[hub.xorb_index[hx]].ulens)[c0:c1]]
        assert bytes(_core.extract_chunk_range(data, 0, c1 - c0)) == want
        if not want_new:  # the same bytes the hub holds for the old xorb
            assert _core.extract_chunk_range(data, 0, c1 - c0) == \
                _core.extract_chunk_range(hub.xorbs[hub.xorb_index[hx]].data, c0, c1)
    assert srv.stats()["not_found"] == 0


def test_refusals_on_the_device(world):
    a = world["bufs"][R.B]
    with pytest.raises(ValueError, match=r"more than one device \(cpu, cuda:0\)"):
        publish({"a": a, "b": a.cpu()})
    with pytest.raises(ValueError, match=r"index is on cpu but the files are on cuda:0.*index\.to\(device\)"):
        publish({"a": a}, index=world["index"].to("cpu"))
    with pytest.raises(ValueError, match=r"index is on cuda:0 but the files are on cpu"):
        publish({"a": a.cpu()}, index=world["index"])
