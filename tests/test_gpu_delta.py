"""GPU: delta pull end to end, pull(device="cuda:0", base=w0) over a FakeHub whose new xorbs are
BG4/LZ4 compressed: fetched terms are decoded by the device pull's pipeline, reused terms are copied
out of the base's HBM by K12 (ops.reuse_chunks), every file is verified from the new buffers."""
from __future__ import annotations

import pytest
import torch

import delta_repo as R
import zest_amd
from e2e_util import free_port
from zest_amd import _core
from zest_amd import seed as zseed
from zest_amd.device import Weights
from zest_amd.testing import FakeHub

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NET = dict(p2p=False, dht=False)


@pytest.fixture(scope="module")
def two_revs(tmp_path_factory):
    hub = FakeHub(policy="auto", max_xorb_bytes=1 << 20)
    hub.start()
    mp = pytest.MonkeyPatch()
    try:
        for k, v in hub.env(str(tmp_path_factory.mktemp("gpudelta"))).items():
            mp.setenv(k, v)
        mp.setenv("ZEST_CACHE_WRITES", "0")  # no disk xorb cache: what is not reused crosses the network
        mp.setenv("ZEST_LISTEN_PORT", str(free_port()))
        rev1, rev2 = R.revisions()
        hub.add_repo(R.REPO1, rev1, xet_suffixes=(".safetensors",))
        w0 = zest_amd.pull(R.REPO1, device=DEV, **NET)
        n1 = len(hub.xorbs)
        hub.add_repo(R.REPO2, rev2, xet_suffixes=(".safetensors",))
        assert any(e[2] != 0 for x in hub.xorbs[n1:] for e in _core.index_chunks(x.data)), \
            "revision 2 must add compressed chunks"
        yield {"hub": hub, "rev1": rev1, "rev2": rev2, "w0": w0, "n1": n1}
    finally:
        zseed.stop_all()
        mp.undo()
        hub.stop()


def test_delta_pull_is_exact_and_bounded(two_revs):
    hub, w0 = two_revs["hub"], two_revs["w0"]
    assert isinstance(w0, Weights) and w0.resident.device == torch.device(DEV)
    R.assert_tensors(w0, two_revs["rev1"])
    served, stats = hub.xorb_bytes_served, {}
    w1 = zest_amd.pull(R.REPO2, device=DEV, base=w0, stats=stats, **NET)
    grew = hub.xorb_bytes_served - served
    R.assert_tensors(w1, two_revs["rev2"])
    R.assert_tensors(w0, two_revs["rev1"])
    d = stats["delta"]
    reused, fetched, files = R.model_counts(hub)
    assert reused > 0 and fetched > 0
    assert (d["reused_terms"], d["fetched_terms"], d["reused_files"], d["refetched_terms"]) == (reused, fetched, files, 0)
    new_xorbs = sum(len(x.data) for x in hub.xorbs[two_revs["n1"]:])
    print(f"served {grew} bytes, new xorbs {new_xorbs}; delta stats {d}")
    assert 0 < grew <= new_xorbs
    assert all(t.device == torch.device(DEV) for t in w1.values())
    assert w1.resident.nbytes == sum(len(v) for k, v in two_revs["rev2"].items() if k.endswith(".safetensors"))


def test_modified_base_on_the_device_is_repaired(two_revs):
    hub = two_revs["hub"]
    base = zest_amd.pull(R.REPO1, device=DEV, **NET)
    x, c0, c1, _ = R.reused_term_of(hub, R.A)
    addrs, lens = base.resident.lookup(hub.xorbs[x].hash_hex, c0, c1)
    at = int(addrs[-1]) - base["a"].data_ptr() + int(lens[-1]) - 1  # the last byte of the term
    assert 0 <= at < base["a"].numel()
    base["a"][at] ^= 0x01
    torch.cuda.synchronize()
    stats = {}
    w = zest_amd.pull(R.REPO2, device=DEV, base=base, stats=stats, **NET)
    R.assert_tensors(w, two_revs["rev2"])
    assert stats["delta"]["refetched_terms"] == R.model_counts(hub, new_paths={R.A})[0] > 0


def test_delta_pull_seeds_the_new_revision_from_hbm(two_revs):
    hub = two_revs["hub"]
    assert zseed.active() == []
    w = zest_amd.pull(R.REPO2, device=DEV, base=two_revs["w0"], seed=True, **NET)
    R.assert_tensors(w, two_revs["rev2"])
    (srv,) = zseed.active()
    try:
        assert srv.xorbs == sorted({hub.xorbs[x].hash_hex for f in R.xet_files(hub, R.REPO2) for x, _, _ in f.terms})
        x, c0, c1, _ = R.reused_term_of(hub, R.A)  # these bytes never crossed the network in this pull
        xorb = hub.xorbs[x]
        a, b = c0, min(c1, c0 + 3)
        h = _core.from_xet_hex(xorb.hash_hex)
        data, off = _core.PeerConnection(f"127.0.0.1:{srv.port}", h).fetch(h, a, b)
        assert off == a
        assert _core.extract_chunk_range(data, 0, b - a) == _core.extract_chunk_range(xorb.data, a, b)
        assert srv.stats()["not_found"] == 0 and srv.stats()["chunks_served"] == 1  # one CHUNK_RESPONSE
    finally:
        zseed.stop_all()


def test_base_on_another_device_is_refused(two_revs):
    cpu = zest_amd.pull(R.REPO1, device="cpu", include=[R.B], **NET)
    with pytest.raises(ValueError, match=r"resident on cpu but the pull targets cuda:0"):
        zest_amd.pull(R.REPO2, device=DEV, base=cpu, **NET)
    with pytest.raises(ValueError, match=r"resident on cuda:0 but the pull targets cpu"):
        zest_amd.pull(R.REPO2, device="cpu", base=two_revs["w0"], **NET)
