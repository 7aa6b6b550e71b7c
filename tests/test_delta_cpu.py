"""Delta pull without a GPU: pull(device="cpu", base=w0) end to end over a FakeHub (zest_amd.delta,
the NumPy path of ops.reuse_chunks, HostXetFetcher.fetch_terms)."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import delta_repo as R
import zest_amd
from zest_amd.delta import ResidentSet
from zest_amd.device import Weights
from zest_amd.testing import FakeHub

NET = dict(p2p=False, dht=False)


@pytest.fixture(scope="module")
def two_revs(tmp_path_factory):
    hub = FakeHub(policy="none", max_xorb_bytes=1 << 20)
    hub.start()
    mp = pytest.MonkeyPatch()
    try:
        for k, v in hub.env(str(tmp_path_factory.mktemp("delta"))).items():
            mp.setenv(k, v)
        mp.setenv("ZEST_CACHE_WRITES", "0")
        rev1, rev2 = R.revisions()
        hub.add_repo(R.REPO1, rev1, xet_suffixes=(".safetensors",))
        w0 = zest_amd.pull(R.REPO1, device="cpu", **NET)
        n1 = len(hub.xorbs)
        hub.add_repo(R.REPO2, rev2, xet_suffixes=(".safetensors",))  # published after the first pull
        assert n1 >= 4 and len(hub.xorbs) > n1
        yield {"hub": hub, "rev1": rev1, "rev2": rev2, "w0": w0, "n1": n1}
    finally:
        mp.undo()
        hub.stop()


def test_weights_is_a_dict_with_a_resident_set(two_revs):
    w0 = two_revs["w0"]
    assert isinstance(w0, Weights) and isinstance(w0, dict)
    plain = dict(w0.items())
    assert w0.keys() == plain.keys() and list(w0) == list(plain) and len(w0) == 2
    assert all(w0[k] is plain[k] for k in plain)
    assert {k: id(v) for k, v in w0.items()} == {k: id(v) for k, v in plain.items()}
    R.assert_tensors(w0, two_revs["rev1"])
    rs = w0.resident
    assert isinstance(rs, ResidentSet) and rs is w0.resident and rs.device == torch.device("cpu")
    hub = two_revs["hub"]
    assert set(rs.plan) == {hub.xorbs[x].hash_hex for f in R.xet_files(hub, R.REPO1) for x, _, _ in f.terms}
    assert rs.nbytes == sum(len(v) for k, v in two_revs["rev1"].items() if k.endswith(".safetensors"))
    assert Weights() == {} and Weights().resident is None
    assert Weights({"a": 1}) == {"a": 1} and Weights({"a": 1}) != {"a": 2}


def test_delta_pull_reuses_resident_terms(two_revs, monkeypatch):
    monkeypatch.setenv("ZEST_CACHE_WRITES", "0")  # no disk xorb cache: every byte not reused crosses the network
    hub, w0 = two_revs["hub"], two_revs["w0"]
    served, stats = hub.xorb_bytes_served, {}
    w1 = zest_amd.pull(R.REPO2, device="cpu", base=w0, stats=stats, **NET)
    assert 0 < hub.xorb_bytes_served - served
    R.assert_tensors(w1, two_revs["rev2"])
    R.assert_tensors(w0, two_revs["rev1"])  # the base is not touched
    d = stats["delta"]
    reused, fetched, files = R.model_counts(hub)
    assert reused > 0 and fetched > 0, "the revisions must share terms and differ in others"
    assert (d["reused_terms"], d["fetched_terms"], d["reused_files"]) == (reused, fetched, files)
    assert files == 1  # file B
    total = sum(len(v) for k, v in two_revs["rev2"].items() if k.endswith(".safetensors"))
    assert d["reused_bytes"] + d["fetched_bytes"] == total
    assert d["reused_bytes"] > 3_000_000  # A's unchanged chunks and all of B
    assert d["refetched_terms"] == 0
    assert all(d[k] >= 0 for k in ("reuse_s", "fetch_s", "verify_s"))
    # the new weights are a base themselves
    assert isinstance(w1, Weights) and w1.resident.nbytes == total


def test_delta_pull_network_bytes(two_revs, monkeypatch):
    """Bytes the CAS serves: a delta pull at most the xorbs revision 2 added, a plain pull of the same
    revision at least its file bytes.

    The first bound needs the fetched terms to share their CDN runs (RunMemo, csrc/core/bridge.h):
    file A's two changed regions are two terms whose new chunks are neighbours in one new xorb, the
    CAS covers both with ONE fetch entry, and a term fetch downloads its whole covering entry.  Without
    sharing, and with the xorb cache off as here, the entry was served once per term (1 934 442 bytes
    served for 1 268 221 bytes of new xorbs)."""
    monkeypatch.setenv("ZEST_CACHE_WRITES", "0")
    hub = two_revs["hub"]
    total = sum(len(v) for k, v in two_revs["rev2"].items() if k.endswith(".safetensors"))
    new_xorbs = sum(len(x.data) for x in hub.xorbs[two_revs["n1"]:])
    served = hub.xorb_bytes_served
    w1 = zest_amd.pull(R.REPO2, device="cpu", base=two_revs["w0"], **NET)
    delta = hub.xorb_bytes_served - served
    served = hub.xorb_bytes_served
    w2 = zest_amd.pull(R.REPO2, device="cpu", **NET)  # the same pull without base= fetches all of it
    plain = hub.xorb_bytes_served - served
    print(f"served: delta pull {delta}, plain pull {plain}; new xorbs {new_xorbs}, file bytes {total}")
    R.assert_tensors(w2, two_revs["rev2"])
    assert w1.keys() == w2.keys() and all(torch.equal(w1[k], w2[k]) for k in w1)
    assert plain >= total
    assert 0 < delta <= new_xorbs


def test_unchanged_file_costs_no_xorb_get(two_revs, monkeypatch):
    monkeypatch.setenv("ZEST_CACHE_WRITES", "0")
    hub = two_revs["hub"]
    gets, served, stats = hub.counters.get("xorb_get", 0), hub.xorb_bytes_served, {}
    w = zest_amd.pull(R.REPO2, device="cpu", base=two_revs["w0"].resident, include=[R.B], stats=stats, **NET)
    assert hub.counters.get("xorb_get", 0) == gets and hub.xorb_bytes_served == served
    assert list(w) == ["b"] and w["b"].numpy().tobytes() == two_revs["w0"]["b"].numpy().tobytes()
    assert w["b"].data_ptr() != two_revs["w0"]["b"].data_ptr()  # a copy, not a view of the base
    d = stats["delta"]
    assert d["fetched_terms"] == 0 and d["fetched_bytes"] == 0 and d["reused_files"] == 1 and d["reused_terms"] > 0


def test_modified_base_is_repaired_from_the_network(two_revs, monkeypatch):
    monkeypatch.setenv("ZEST_CACHE_WRITES", "0")
    hub = two_revs["hub"]
    base = zest_amd.pull(R.REPO1, device="cpu", **NET)
    x, c0, c1, off = R.reused_term_of(hub, R.A)
    # the term's bytes in the base: find them through the resident set, then flip one
    addrs, lens = base.resident.lookup(hub.xorbs[x].hash_hex, c0, c1)
    at = int(addrs[len(addrs) // 2]) - base["a"].data_ptr() + int(lens[len(addrs) // 2]) // 2
    assert 0 <= at < base["a"].numel()
    base["a"][at] ^= 0x40
    stats = {}
    w = zest_amd.pull(R.REPO2, device="cpu", base=base, stats=stats, **NET)
    R.assert_tensors(w, two_revs["rev2"])
    d = stats["delta"]
    reused, fetched, _ = R.model_counts(hub)
    a_reused = R.model_counts(hub, new_paths={R.A})[0]
    assert d["refetched_terms"] == a_reused > 0  # exactly file A's reused terms, not B's
    assert (d["reused_terms"], d["fetched_terms"]) == (reused, fetched)


def test_merged_bases_resolve_terms_from_both(two_revs, monkeypatch):
    monkeypatch.setenv("ZEST_CACHE_WRITES", "0")
    hub = two_revs["hub"]
    wa = zest_amd.pull(R.REPO1, device="cpu", include=[R.A], **NET)
    wb = zest_amd.pull(R.REPO1, device="cpu", include=[R.B], **NET)
    only_a, both = R.model_counts(hub, base_paths={R.A}), R.model_counts(hub)
    assert 0 < only_a[0] < both[0]
    for base, want in ((wa, only_a), ([wa, wb], both), (wa.resident | wb.resident, both),
                       ([wb.resident, wa], both)):
        stats = {}
        w = zest_amd.pull(R.REPO2, device="cpu", base=base, stats=stats, **NET)
        R.assert_tensors(w, two_revs["rev2"])
        d = stats["delta"]
        assert (d["reused_terms"], d["fetched_terms"], d["reused_files"]) == want


def test_refusals_say_what_to_do(two_revs):
    from zest_amd.direct import pull_to_device

    w0 = two_revs["w0"]
    with pytest.raises(ValueError, match=r"base=.*device='all'.*device='cuda:N'"):
        zest_amd.pull(R.REPO2, device="all", base=w0)
    with pytest.raises(ValueError, match=r"base=.*shard=.*unsharded"):
        zest_amd.pull(R.REPO2, device="cpu", base=w0, shard=(0, 2))
    with pytest.raises(ValueError, match=r"base=.*direct=False.*default"):
        zest_amd.pull(R.REPO2, device="cpu", base=w0, direct=False)
    with pytest.raises(ValueError, match=r"base= needs a device"):
        zest_amd.pull(R.REPO2, base=w0)
    with pytest.raises(ValueError, match=r"base= needs a device"):
        pull_to_device(R.REPO2, device=None, base=w0)
    with pytest.raises(ValueError, match=r"device='all'"):
        pull_to_device(R.REPO2, device="all", base=w0)
    with pytest.raises(ValueError, match=r"shard="):
        pull_to_device(R.REPO2, device="cpu", base=w0, shard=(0, 2))
    # a base on another device than the pull's
    elsewhere = ResidentSet({}, [], "meta")
    with pytest.raises(ValueError, match=r"resident on meta but the pull targets cpu"):
        zest_amd.pull(R.REPO2, device="cpu", base=elsewhere)
    with pytest.raises(ValueError, match=r"resident on meta but the pull targets cpu"):
        zest_amd.pull(R.REPO2, device="cpu", base=[w0, elsewhere])
    # a base that is no resident set
    for bad in (dict(w0), "step-100", [], Weights(), [w0, 3]):
        with pytest.raises(ValueError, match=r"base="):
            zest_amd.pull(R.REPO2, device="cpu", base=bad)
    with pytest.raises(ValueError, match=r"plain dict of tensors"):
        zest_amd.pull(R.REPO2, device="cpu", base=dict(w0))


def _entries(f):
    """{xorb index: [(c0, c1), ...]}: the fetch entries the CAS answers for a file, one per maximal
    union of its terms' chunk ranges in an xorb."""
    out = {}
    for x, c0, c1 in sorted(f.terms):
        runs = out.setdefault(x, [])
        if runs and c0 <= runs[-1][1]:
            runs[-1] = (runs[-1][0], max(runs[-1][1], c1))
        else:
            runs.append((c0, c1))
    return out


def test_two_files_whose_fetch_entries_share_a_start(tmp_path, monkeypatch):
    """Fetch entries are per file.  File Z puts a run of new chunks into the new xorb; P uses the
    first two and the next three of them in two terms, Q the first two and all the rest, so both
    have an entry that starts at the same chunk, P's ending before Q's, each wider than its terms.
    Terms that share downloads must tell the two apart: every byte exact, each entry served once."""
    from zest_amd import _core

    rng = np.random.default_rng(77)
    blob = rng.integers(0, 256, 3_000_000, dtype=np.uint8).tobytes()
    ends = [0] + list(_core.chunk_ends(blob))[:-1]  # whole chunks only: each re-chunks to itself
    c = [blob[a:b] for a, b in zip(ends, ends[1:])]
    assert len(c) >= 32
    cat = lambda *parts: b"".join(b"".join(c[i] for i in p) for p in parts)
    old = {"old.safetensors": R.safetensors(cat(range(0, 20)), "old")}
    new = {"a-z.safetensors": R.safetensors(cat(range(20, 32)), "z"),
           "p.safetensors": R.safetensors(cat((0, 1), (22, 23), range(2, 5), (24, 25, 26)), "p"),
           "q.safetensors": R.safetensors(cat((5, 6), (22, 23), range(7, 9), range(24, 32)), "q")}
    hub = FakeHub(policy="none", max_xorb_bytes=8 << 20)
    hub.start()
    try:
        for k, v in hub.env(str(tmp_path)).items():
            monkeypatch.setenv(k, v)
        monkeypatch.setenv("ZEST_CACHE_WRITES", "0")
        hub.add_repo("org/shared-old", old, xet_suffixes=(".safetensors",))
        n1 = len(hub.xorbs)
        hub.add_repo("org/shared-new", new, xet_suffixes=(".safetensors",))
        assert len(hub.xorbs) == n1 + 1
        fz, fp, fq = (hub.repos[("model", "org/shared-new")].files[k] for k in new)
        ez, ep, eq = (_entries(f)[n1] for f in (fz, fp, fq))
        (s0, pe), (q0, qe) = ep[0], eq[0]
        assert s0 == q0 and pe < qe, (ez, ep, eq)  # same start, different ends
        for f, (a, b) in ((fp, ep[0]), (fq, eq[0])):  # two terms in the entry: it is wider than either
            assert len([t for t in f.terms if t[0] == n1 and a <= t[1] and t[2] <= b]) == 2, f.terms
        xb = hub.xorbs[n1]
        entry_bytes = sum(xb.boundaries[b - 1] - (xb.boundaries[a - 1] if a else 0) for e in (ez, ep, eq) for a, b in e)
        w0 = zest_amd.pull("org/shared-old", device="cpu", **NET)
        served, stats = hub.xorb_bytes_served, {}
        w = zest_amd.pull("org/shared-new", device="cpu", base=w0, stats=stats, **NET)
        R.assert_tensors(w, new)
        d = stats["delta"]
        terms = [t for f in (fz, fp, fq) for t in f.terms]
        fetched = sum(t[0] == n1 for t in terms)
        assert (d["fetched_terms"], d["reused_terms"], d["refetched_terms"]) == (fetched, len(terms) - fetched, 0)
        assert d["reused_terms"] >= 4
        assert hub.xorb_bytes_served - served == entry_bytes  # every entry once, the shared-start ones for two terms each
    finally:
        hub.stop()
