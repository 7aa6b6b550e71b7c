"""pull(..., into=..., base=...) end to end over a FakeHub, shared by the CPU and the GPU tests.  The
revisions are into_delta_repo.py's, the expected counters into_delta_model.py's.  Destinations are
carved out of canary-filled allocations, some at odd byte offsets, and after every pull every byte
of every allocation is compared."""
from __future__ import annotations

import json

import numpy as np
import pytest
import torch

import into_delta_model as M
import into_delta_repo as R
import zest_amd
from scatter_model import canary
from zest_amd import delta as zdelta
from zest_amd import into as zinto
from zest_amd.device import ST_DTYPES

GUARD = 64
NET = dict(p2p=False, dht=False)
COUNTERS = ("kept_terms", "kept_bytes", "moved_chunks", "moved_bytes", "fetched_terms", "fetched_bytes",
            "applied_bytes")


class Dest:
    """A destination of `shape` / safetensors dtype `dt` inside its own canary-filled allocation,
    `shift` bytes past the guard (odd for one-byte items)."""

    def __init__(self, shape, dt: str, device, salt: int = 0):
        item = R.ITEMSIZE[dt]
        self.n = R.nbytes(dt, shape)
        self.at = GUARD + item * (1 + salt % 3)
        self.fill = canary(self.at + self.n + GUARD, salt)
        self.hold = torch.from_numpy(self.fill.copy()).to(device)
        self.t = self.hold[self.at:self.at + self.n].view(ST_DTYPES[dt]).view(list(shape))

    def check(self, raw: bytes | None, what: str = "") -> None:
        want = self.fill.copy()
        if raw is not None:
            assert len(raw) == self.n, what
            want[self.at:self.at + self.n] = np.frombuffer(raw, dtype=np.uint8)
        got = self.hold.cpu().numpy()
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, f"{what}: {bad.size} bytes differ, first at {int(bad[0]) - self.at} of {self.n}"

    def flip(self, k: int) -> None:
        self.hold[self.at + k] ^= 0x01


def make_dests(files: dict, device, names=None, salt: int = 0) -> dict:
    out = {}
    for i, (name, (dt, shape, _)) in enumerate(R.specs(files).items()):
        if names is None or name in names:
            out[name] = Dest(shape, dt, device, salt + i)
    return out


def tensors(dests: dict) -> dict:
    return {n: d.t for n, d in dests.items()}


def addrs(dests: dict) -> dict:
    return {n: d.t.data_ptr() for n, d in dests.items()}


def check_all(dests: dict, files: dict | None, what: str = "", only=None) -> None:
    """Every allocation: the tensors of `files` that `only` names (default: all) hold the revision's
    bytes, the others their canary."""
    raw = R.tensor_bytes(files) if files is not None else {}
    for name, d in dests.items():
        d.check(raw.get(name) if only is None or name in only else None, f"{what} {name}")


def pull(repo, device, **kw):
    return zest_amd.pull(repo, device=device, **NET, **kw)


def sync(device) -> None:
    if str(device).startswith("cuda"):
        torch.cuda.synchronize()


def assert_counters(d: dict, exp: dict) -> None:
    got = {k: d[k] for k in COUNTERS}
    assert got == {k: exp[k] for k in COUNTERS}, (got, {k: exp[k] for k in COUNTERS})
    for path, e in exp["files"].items():
        for k in ("kept_bytes", "moved_bytes", "fetched_bytes"):
            assert d["files"][path][k] == e[k], (path, k, d["files"][path], e[k])


def first_pull(ctx, device, names=None, salt: int = 0):
    """Revision 1 into fresh destinations (for every tensor of revisions 1 and 2): (landed, dests)."""
    rev1, rev2, _ = ctx["revs"]
    dests = make_dests({**rev1, **rev2}, device, names, salt)
    in1 = {n: d.t for n, d in dests.items() if n in R.specs(rev1)}
    landed = pull(R.REPO1, device, into=in1, strict=False)
    assert isinstance(landed, zinto.Landed) and set(landed) == set(in1) and all(landed[n] is in1[n] for n in in1)
    check_all(dests, rev1, "revision 1")
    return landed, dests


# ------------------------------------------------------------------------------------------------
def case_exact_and_bounded(ctx, device):
    hub, (rev1, rev2, _) = ctx["hub"], ctx["revs"]
    landed, dests = first_pull(ctx, device)
    resident, (seam_chunks, seam_bytes, boundaries) = M.bind(hub, R.REPO1, rev1, addrs({n: dests[n] for n in landed}))
    exp = M.expect(hub, R.REPO2, rev2, resident, addrs(dests))
    served, st = hub.xorb_bytes_served, {}
    got = pull(R.REPO2, device, into=tensors(dests), base=landed, stats=st)
    grew = hub.xorb_bytes_served - served
    check_all(dests, rev2, "revision 2")
    d = st["into"]["delta"]
    print(f"delta {({k: v for k, v in d.items() if k != 'files'})} served {grew}")
    assert_counters(d, exp)
    assert d["kept_bytes"] > 0 and d["fetched_bytes"] > 0 and d["fallback_files"] == 0
    assert (d["seam_chunks"], d["seam_bytes"]) == (seam_chunks, seam_bytes) and seam_bytes <= (128 << 10) * boundaries
    new_xorbs = sum(len(x.data) for x in hub.xorbs[ctx["n"][1]:ctx["n"][2]])
    assert 0 < grew <= new_xorbs, (grew, new_xorbs)
    # FILE2 kept its tensors behind a longer header: nothing but its first term or terms is fetched
    e2 = exp["files"][R.FILE2]
    k = len(e2["fetched_term_ids"])
    assert 1 <= k < len(e2["terms"]) and e2["fetched_term_ids"] == list(range(k)) and e2["kept_bytes"] > 0
    first_tensor = min(off for _, _, off, _ in R.header(rev2[R.FILE2])[1].values())
    assert e2["chunks"][e2["terms"][k - 1][1] - 1][2] < first_tensor + (128 << 10)  # they end by the first data chunk
    # FILE3's swapped tensors keep their destinations, so by the definition of "kept" their inner chunks are
    # verified where they lie; the chunks over the new tensor boundaries are new bytes and are fetched
    # (case_separate_base is where every resident chunk of these tensors is moved)
    e3 = exp["files"][R.FILE3]
    assert e3["kept_bytes"] > 0 and e3["fetched_bytes"] > 0
    for name in R.SWAPPED:
        _, _, off, n = R.header(rev2[R.FILE3])[1][name]
        inner = [i for i, (_, _, o, k) in enumerate(e3["chunks"]) if off <= o and o + k <= off + n]
        assert inner and sum(i in e3["kept_chunks"] for i in inner) >= len(inner) - 2, name
    assert isinstance(got, zinto.Landed) and set(got) == set(dests)
    assert sorted(f.path for f in got.record.files) == sorted(p for p in rev2 if p.endswith(".safetensors"))
    return got, dests, d, exp


def case_chained_and_back(ctx, device):
    rev1, rev2, rev3 = ctx["revs"]
    landed, dests = first_pull(ctx, device)
    st = {}
    landed = pull(R.REPO2, device, into=tensors(dests), base=landed, scratch_bytes=1, stats=st)  # several groups
    check_all(dests, rev2, "v1 -> v2")
    assert st["into"]["groups"] > 1 and st["into"]["delta"]["patch_bytes"] < (1 << 20)
    st = {}
    landed = pull(R.REPO3, device, into=tensors(dests), base=landed, stats=st)
    check_all(dests, rev3, "v2 -> v3")
    d = st["into"]["delta"]
    assert d["fallback_files"] == 0 and d["kept_bytes"] > 0
    assert 0 < d["fetched_bytes"] <= 3 * (128 << 10)  # the chunks around the 60 bytes that changed
    v1 = {n: t for n, t in tensors(dests).items() if n in R.specs(rev1)}
    st = {}
    landed = pull(R.REPO1, device, into=v1, base=landed, stats=st)
    raw3 = R.tensor_bytes(rev3)
    for name, dd in dests.items():
        dd.check(R.tensor_bytes(rev1).get(name, raw3.get(name)), f"v3 -> v1 {name}")
    assert st["into"]["delta"]["kept_bytes"] > 0 and set(landed) == set(v1)


def _dest_byte(files: dict, path: str, off: int):
    """(tensor name, byte in it) of file offset `off`."""
    for name, (_, _, t_off, n) in R.header(files[path])[1].items():
        if t_off <= off < t_off + n:
            return name, off - t_off
    raise AssertionError(f"offset {off} of {path} is in no tensor")


def case_modified_inside(ctx, device):
    """One bit flipped in the last byte of a kept term: the file misses its hash, falls back, ends exact."""
    hub, (rev1, rev2, _) = ctx["hub"], ctx["revs"]
    landed, dests = first_pull(ctx, device)
    resident, _ = M.bind(hub, R.REPO1, rev1, addrs({n: dests[n] for n in landed}))
    e = M.expect(hub, R.REPO2, rev2, resident, addrs(dests))["files"][R.FILE1]
    t = next(t for t, (a, b) in enumerate(e["terms"]) if all(i in e["kept_chunks"] for i in range(a, b)))
    _, _, off, n = e["chunks"][e["terms"][t][1] - 1]
    name, k = _dest_byte(rev2, R.FILE1, off + n - 1)
    dests[name].flip(k)
    sync(device)
    st = {}
    pull(R.REPO2, device, into=tensors(dests), base=landed, stats=st)
    check_all(dests, rev2, "after a modified destination")
    d = st["into"]["delta"]
    assert d["fallback_files"] == 1 and d["fallback_bytes"] == len(rev2[R.FILE1]) and d["files"][R.FILE1]["fallback"]


def seam_chunk(hub, files: dict, path: str, dests: dict, many: bool):
    """A seam chunk of the bound revision-1 file that revision 2 still references: (file offsets of a
    byte in each destination segment it touches).  many: one that touches at least three tensors."""
    segs = M.layout(files[path], addrs(dests))
    still = {(x, c) for x, c, _, _ in M.file_chunks(hub, R.REPO2, path)[0]}
    for x, c, off, n in M.file_chunks(hub, R.REPO1, path)[0]:
        touched = [s for s in segs if s[0] < off + n and off < s[1]]
        if M.place(segs, off, n) == M.ARENA and (x, c) in still and all(s[2] != M.HEADER for s in touched) \
                and (len(touched) >= 3 if many else len(touched) == 2):
            return [max(s[0], off) for s in touched]
    raise AssertionError(f"{path} has no such seam chunk")


def case_modified_seam(ctx, device, many: bool):
    """A byte under a seam chunk is modified after the record was taken: the arena is gathered at bind
    time, so the check sees it and the file falls back."""
    hub, (rev1, rev2, _) = ctx["hub"], ctx["revs"]
    landed, dests = first_pull(ctx, device)
    path = R.FILE2 if many else R.FILE1
    spots = seam_chunk(hub, rev1, path, {n: dests[n] for n in landed}, many)
    name, k = _dest_byte(rev1, path, spots[1])  # the second segment: a middle tiny tensor when there are many
    assert not many or name in R.TINY
    dests[name].flip(k)
    sync(device)
    st = {}
    pull(R.REPO2, device, into=tensors(dests), base=landed, stats=st)
    check_all(dests, rev2, "after a modified seam")
    d = st["into"]["delta"]
    assert d["fallback_files"] == 1 and d["files"][path]["fallback"]


def case_unscatterable_file(ctx, device):
    rev1, rev2, _ = ctx["revs"]
    landed, dests = first_pull(ctx, device)
    bad = Dest([2, 3], "I32", device, 99)
    into = dict(tensors(dests), **{"b.tail": bad.t})
    with pytest.raises(ValueError, match=r"b\.tail"):
        pull(R.REPO2, device, into=into, base=landed)
    sync(device)
    bad.check(None, "the wrong destination")
    s1, s2 = R.specs(rev1), R.specs(rev2)
    raw1, raw2 = R.tensor_bytes(rev1), R.tensor_bytes(rev2)
    for name, d in dests.items():
        if s2[name][2] == R.FILE3:  # scattered before the file that failed
            d.check(raw2[name], name)
        elif s2[name][2] == R.FILE1:
            d.check(raw1[name], name)  # to the byte
        else:
            d.check(raw1[name] if name in s1 else None, name)


HOLES = ["a.one", "b.wide", "c.tiny.03", "c.tiny.04", "c.tiny.09", "c.last"]


def case_holes(ctx, device):
    hub, (rev1, rev2, _) = ctx["hub"], ctx["revs"]
    names = [n for n in R.specs({**rev1, **rev2}) if n not in HOLES]
    landed, dests = first_pull(ctx, device, names)
    assert set(landed) == set(names) - {"d.new"}
    resident, _ = M.bind(hub, R.REPO1, rev1, addrs({n: dests[n] for n in landed}))
    exp = M.expect(hub, R.REPO2, rev2, resident, addrs(dests))
    st = {}
    pull(R.REPO2, device, into=tensors(dests), base=landed, stats=st, strict=False)
    check_all(dests, rev2, "holes")
    assert_counters(st["into"]["delta"], exp)
    fake = {n: (i + 1) << 40 for i, n in enumerate(R.specs({**rev1, **rev2}))}  # the same pull without holes
    whole = M.expect(hub, R.REPO2, rev2, M.bind(hub, R.REPO1, rev1, {n: fake[n] for n in R.specs(rev1)})[0], fake)
    assert exp["fetched_bytes"] > whole["fetched_bytes"]  # chunks that touch an unwanted tensor are fetched


def case_record_is_address_free(ctx, device):
    hub, (rev1, rev2, _) = ctx["hub"], ctx["revs"]
    landed, first = first_pull(ctx, device)
    rec = zinto.IntoRecord.from_state(json.loads(json.dumps(landed.record.state())))
    other = make_dests({**rev1, **rev2}, device, salt=1000)
    for n in landed:
        other[n].t.copy_(first[n].t)
    rs = rec.bind({n: other[n].t for n in landed}, device)
    assert isinstance(rs, zdelta.ResidentSet)
    exp = M.expect(hub, R.REPO2, rev2, M.bind(hub, R.REPO1, rev1, addrs({n: other[n] for n in landed}))[0], addrs(other))
    exp1 = M.expect(hub, R.REPO2, rev2, M.bind(hub, R.REPO1, rev1, addrs({n: first[n] for n in landed}))[0], addrs(first))
    assert {k: exp[k] for k in COUNTERS} == {k: exp1[k] for k in COUNTERS}
    st = {}
    pull(R.REPO2, device, into=tensors(other), base=rs, stats=st)
    check_all(other, rev2, "the other tensors")
    check_all(first, rev1, "the first tensors")
    assert_counters(st["into"]["delta"], exp)


def case_landed_as_plain_base(ctx, device):
    rev1, rev2, _ = ctx["revs"]
    landed, dests = first_pull(ctx, device)
    st = {}
    w = pull(R.REPO2, device, base=landed, stats=st)
    raw = R.tensor_bytes(rev2)
    assert set(w) == set(raw)
    for name, t in w.items():
        assert t.cpu().reshape(-1).view(torch.uint8).numpy().tobytes() == raw[name], name
    assert st["delta"]["reused_terms"] > 0
    check_all(dests, rev1, "the destinations")


def case_separate_base(ctx, device):
    hub, (rev1, rev2, _) = ctx["hub"], ctx["revs"]
    w0 = pull(R.REPO1, device)
    whole = {path: buf.data_ptr() for (path, _), (buf, _, _) in zip(w0._meta, w0._files)}
    dests = make_dests(rev2, device, salt=7)
    exp = M.expect(hub, R.REPO2, rev2, M.bind(hub, R.REPO1, rev1, {}, whole)[0], addrs(dests))
    st = {}
    pull(R.REPO2, device, into=tensors(dests), base=w0, stats=st)
    check_all(dests, rev2, "fresh destinations")
    d = st["into"]["delta"]
    assert_counters(d, exp)
    assert d["kept_bytes"] == 0 and d["kept_terms"] == 0 and d["moved_bytes"] == exp["moved_bytes"] > 0
    e3 = exp["files"][R.FILE3]  # the swapped tensors: what is not fetched is moved
    for name in R.SWAPPED:
        _, _, off, n = R.header(rev2[R.FILE3])[1][name]
        over = lambda ids: sum(max(0, min(o + k, off + n) - max(o, off)) for i, (_, _, o, k) in enumerate(e3["chunks"])
                               if i in ids)
        fetched = {i for t in e3["fetched_term_ids"] for i in range(*e3["terms"][t])}
        assert over(e3["moved_set"]) + over(fetched) == n and over(e3["moved_set"]) > 0, name
    raw = R.tensor_bytes(rev1)
    for name, t in w0.items():
        assert t.cpu().reshape(-1).view(torch.uint8).numpy().tobytes() == raw[name], name


def case_traded_destinations(ctx, device, split: bool):
    """The ordering invariant.  The record is bound so that a.end (FILE3) lies in c.first's destination
    and c.first (FILE2) in a.end's: each file's scatter overwrites the other file's moved source.  In
    one group every gather is queued before the first scatter, so nothing falls back; with a group per
    file FILE3 is scattered first, FILE2's check then hashes clobbered bytes, misses and falls back."""
    hub, (rev1, rev2, _) = ctx["hub"], ctx["revs"]
    ta, tc = R.TWINS
    rev12 = {**rev1, **rev2}
    dests = make_dests(rev12, device, [n for n in R.specs(rev12) if n != ta], salt=50)
    dests[ta] = Dest(R.specs(rev1)[tc][1], R.specs(rev1)[tc][0], device, 49)  # aligned for either dtype
    dests[ta].t = dests[ta].t.view(-1).view(torch.uint8)
    assert dests[ta].n == dests[tc].n == R.nbytes(*R.specs(rev1)[ta][:2])
    landed = pull(R.REPO1, device, into={n: d.t for n, d in dests.items() if n in R.specs(rev1)})
    check_all(dests, rev1, "revision 1")
    a, c = dests[ta].t, dests[tc].t
    keep = a.clone()
    a.copy_(c.view(-1).view(torch.uint8))  # the two tensors trade their bytes ...
    c.view(-1).view(torch.uint8).copy_(keep)
    traded = dict(landed)
    traded[ta], traded[tc] = c.view(-1).view(torch.uint8), a.view(torch.float32).view(c.shape)  # ... and the record its addresses
    rs = landed.record.bind(traded, device)
    addr = addrs({n: dests[n] for n in landed})
    addr[ta], addr[tc] = addr[tc], addr[ta]
    exp = M.expect(hub, R.REPO2, rev2, M.bind(hub, R.REPO1, rev1, addr)[0], addrs(dests))
    for path, name in ((R.FILE3, ta), (R.FILE2, tc)):  # each is a moved source that the other file's scatter writes
        e = exp["files"][path]
        _, _, off, n = R.header(rev2[path])[1][name]
        assert any(off <= o and o + k <= off + n for i, (_, _, o, k) in enumerate(e["chunks"]) if i in e["moved_set"]), name
    st = {}
    pull(R.REPO2, device, into=tensors(dests), base=rs, stats=st, **(dict(scratch_bytes=1) if split else {}))
    check_all(dests, rev2, "traded destinations")
    d = st["into"]["delta"]
    if split:
        assert st["into"]["groups"] > 1 and d["files"][R.FILE2]["fallback"] and not d["files"][R.FILE3]["fallback"]
    else:
        assert st["into"]["groups"] == 1 and d["fallback_files"] == 0
        assert_counters(d, exp)


def case_refusals(ctx, device):
    hub, (rev1, _, _) = ctx["hub"], ctx["revs"]
    dests = make_dests(rev1, device, ["b.bias"])
    into = tensors(dests)
    elsewhere = "cpu" if str(device).startswith("cuda") else "cuda:0"
    before = hub.counters.get("requests", 0)
    ok = zdelta.ResidentSet({}, [], device)
    for kw, word in ((dict(base=ok, shard=(0, 2)), "shard="), (dict(base=ok, cast=True), "cast=True"),
                     (dict(base=zdelta.ResidentSet({}, [], elsewhere)), "resident on"),
                     (dict(base=zinto.Landed({}, zinto.IntoRecord(), elsewhere)), "resident on"),
                     (dict(base={"b.bias": dests["b.bias"].t}), "base=")):
        with pytest.raises(ValueError, match=word):
            pull(R.REPO2, device, into=into, **kw)
    assert hub.counters.get("requests", 0) == before
    check_all(dests, None)
