"""pull(device="cpu", into=..., base=...) end to end over a FakeHub (cases: into_delta_cases.py), the
binding of a record against the oracle (into_delta_model.py) and the hole-aware chunk classifier
against a byte-by-byte model."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

import into_delta_cases as C
import into_delta_model as M
import into_delta_repo as R
from zest_amd import ops
from zest_amd.publish import classify_chunks_with_holes
from zest_amd.testing import FakeHub

DEV = "cpu"


def make_ctx(tmp_path_factory, name: str):
    """The hub with the three revisions (shared with the GPU tests)."""
    hub = FakeHub(policy="auto", max_xorb_bytes=1 << 20)
    hub.start()
    mp = pytest.MonkeyPatch()
    try:
        for k, v in hub.env(str(tmp_path_factory.mktemp(name))).items():
            mp.setenv(k, v)
        mp.setenv("ZEST_CACHE_WRITES", "0")  # no disk xorb cache: what is not resident crosses the network
        revs = R.revisions()
        n = [len(hub.xorbs)]
        for repo, files in zip((R.REPO1, R.REPO2, R.REPO3), revs):
            hub.add_repo(repo, files, xet_suffixes=(".safetensors",))
            n.append(len(hub.xorbs))
        yield {"hub": hub, "revs": revs, "n": n}
    finally:
        mp.undo()
        hub.stop()


@pytest.fixture(scope="module")
def ctx(tmp_path_factory):
    yield from make_ctx(tmp_path_factory, "intodelta")


def test_repository_is_what_the_cases_need(ctx):
    hub, (rev1, rev2, rev3) = ctx["hub"], ctx["revs"]
    sizes = [len(rev1[p]) for p in (R.FILE1, R.FILE2, R.FILE3)]
    assert all(1_000_000 <= s <= 8_000_000 for s in sizes)
    assert R.header(rev1[R.FILE1])[0] % 16 == 8 and R.header(rev2[R.FILE2])[0] == R.header(rev1[R.FILE2])[0] + 8
    assert {R.ITEMSIZE[dt] for dt, _, _ in R.specs(rev1).values()} == {1, 2, 4}
    assert R.specs(rev1)["c.empty"][1] == [0, 7] and len(R.TINY) >= 12
    order = lambda files: list(R.header(files[R.FILE3])[1])
    assert order(rev1) != order(rev2) and sorted(order(rev1)) == sorted(order(rev2))
    # one chunk of revision 1 spans many of the tiny tensors
    segs = M.layout(rev1[R.FILE2], {n: 1 << 40 for n in R.specs(rev1)})
    assert max(sum(1 for s in segs if s[0] < off + n and off < s[1])
               for _, _, off, n in M.file_chunks(hub, R.REPO1, R.FILE2)[0]) >= 8


def test_exact_and_bounded(ctx):
    C.case_exact_and_bounded(ctx, DEV)


def test_chained_and_back(ctx):
    C.case_chained_and_back(ctx, DEV)


def test_modified_destination_inside_one_tensor(ctx):
    C.case_modified_inside(ctx, DEV)


@pytest.mark.parametrize("many", [False, True], ids=["two-tensors", "tiny-run"])
def test_modified_destination_under_a_seam_chunk(ctx, many):
    C.case_modified_seam(ctx, DEV, many)


def test_a_file_that_cannot_be_scattered_writes_nothing(ctx):
    C.case_unscatterable_file(ctx, DEV)


def test_holes(ctx):
    C.case_holes(ctx, DEV)


def test_record_is_address_free(ctx):
    C.case_record_is_address_free(ctx, DEV)


def test_landed_as_a_plain_base(ctx):
    C.case_landed_as_plain_base(ctx, DEV)


def test_separate_base(ctx):
    C.case_separate_base(ctx, DEV)


@pytest.mark.parametrize("split", [False, True], ids=["one-group", "group-per-file"])
def test_gathers_come_before_the_scatters_that_overwrite_them(ctx, split):
    C.case_traded_destinations(ctx, DEV, split)


def test_refusals_come_before_any_request(ctx):
    C.case_refusals(ctx, DEV)


def test_peak_memory_bound_holds_on_the_counters(ctx):
    """The arithmetic of the GPU peak-memory test, on the CPU path's counters: the bound is below half
    the largest file."""
    _, _, d, exp = C.case_exact_and_bounded(ctx, DEV)
    bound = peak_bound(ctx, exp, d["seam_bytes"])
    assert d["patch_bytes"] <= sum(-(-e["fetched_bytes"] // ops.PAD) * ops.PAD + ops.PAD for e in exp["files"].values())
    assert bound < max(len(v) for v in ctx["revs"][1].values()) // 2, bound


def peak_bound(ctx, exp: dict, seam_bytes: int) -> int:
    """Upper bound of the device memory a delta pull holds above the model, from the oracle: the patch
    slots with their ops.PAD, the seam arena, the moved bytes (the bounce area), 64 bytes per chunk
    of tables and 32 bytes per KiB hashed in one launch (the resident chunks, which are hashed where
    they lie)."""
    slots = sum(-(-e["fetched_bytes"] // ops.PAD) * ops.PAD + ops.PAD for e in exp["files"].values())
    chunks = sum(len(e["chunks"]) for e in exp["files"].values())
    fetched = [{i for t in e["fetched_term_ids"] for i in range(*e["terms"][t])} for e in exp["files"].values()]
    hashed = sum(n for e, f in zip(exp["files"].values(), fetched) for i, (_, _, _, n) in enumerate(e["chunks"])
                 if i not in f)
    return slots + seam_bytes + exp["moved_bytes"] + 64 * chunks + 32 * (-(-hashed // 1024))


@pytest.mark.parametrize("holes", [[], C.HOLES], ids=["whole", "holes"])
def test_binding_places_every_chunk_like_the_oracle(ctx, holes):
    hub, (rev1, rev2, _) = ctx["hub"], ctx["revs"]
    names = [n for n in R.specs(rev1) if n not in holes]
    landed, dests = C.first_pull(ctx, DEV, names)
    assert "c.empty" in landed and dests["c.empty"].n == 0  # a zero-size tensor is written and binds to nothing
    rs = landed.record.bind(landed, DEV)
    resident, (seam_chunks, seam_bytes, boundaries) = M.bind(hub, R.REPO1, rev1, C.addrs({n: dests[n] for n in landed}))
    assert (rs.seam_chunks, rs.seam_bytes) == (seam_chunks, seam_bytes) and 0 < seam_bytes <= (128 << 10) * boundaries
    arena = rs.buffers[-1]
    assert arena.numel() == seam_bytes
    inside = lambda a, n, t: t.data_ptr() <= a and a + n <= t.data_ptr() + t.numel() * t.element_size()
    seen = {"arena": 0, "header": 0, "dest": 0, "hole": 0, "pieces": 0}
    for path in M.xet_paths(hub, R.REPO1):
        data = rev1[path]
        segs = M.layout(data, C.addrs({n: dests[n] for n in landed}))
        for x, c, off, n in M.file_chunks(hub, R.REPO1, path)[0]:
            hit = rs.lookup(hub.xorbs[x].hash_hex, c, c + 1)
            want = resident.get((x, c))
            if want is None:
                assert hit is None, (path, off)
                seen["hole"] += 1
                continue
            (addr,), (ln,) = (int(v[0]) for v in hit[0:1]), (int(v[0]) for v in hit[1:2])
            assert ln == n and ctypes.string_at(addr, n) == data[off:off + n], (path, off)
            if want == M.ARENA:
                assert inside(addr, n, arena)
                seen["arena"] += 1
                seen["pieces"] = max(seen["pieces"], sum(1 for s in segs if s[0] < off + n and off < s[1]))
            elif isinstance(want, tuple):
                assert any(inside(addr, n, b) for b in rs.buffers) and not inside(addr, n, arena)
                seen["header"] += 1
            else:
                assert addr == want, (path, off)
                seen["dest"] += 1
    assert seen["arena"] == seam_chunks and seen["dest"] > 0 and seen["pieces"] >= (3 if holes else 8)
    assert (seen["hole"] > 0) == bool(holes)
    if holes:  # holes at the start, in the middle and at the end of a file's data
        first = lambda p: min(R.header(rev1[p])[1].items(), key=lambda kv: kv[1][2])[0]
        last = lambda p: max(R.header(rev1[p])[1].items(), key=lambda kv: kv[1][2])[0]
        assert first(R.FILE3) in holes and last(R.FILE2) in holes and "b.wide" in holes


def test_classifier_with_holes_equals_a_byte_model():
    rng = np.random.default_rng(5)
    for _ in range(200):
        k = int(rng.integers(1, 9))
        seg = rng.integers(0, 12, k)
        if seg.sum() == 0:
            seg[0] = 3
        hole = rng.random(k) < 0.35
        n = int(seg.sum())
        cuts = np.sort(rng.choice(np.arange(1, n), size=min(int(rng.integers(0, 6)), n - 1), replace=False)) if n > 1 else []
        ends = np.concatenate([cuts, [n]]).astype(np.uint64)
        pl = classify_chunks_with_holes(seg, hole, ends)
        owner = np.repeat(np.arange(k), seg)  # the segment of every byte
        arena, at = {}, 0
        for c, (a, b) in enumerate(zip(np.concatenate([[0], ends[:-1]]).astype(int), ends.astype(int))):
            own = owner[a:b]
            res = not hole[own].any()
            assert bool(pl["resident"][c]) == res
            seam = res and len(set(own.tolist())) > 1
            assert bool(pl["seam"][c]) == seam
            if res and not seam:
                s = int(own[0])
                assert int(pl["seg"][c]) == s and int(pl["off"][c]) == a - int(seg[:s].sum())
            if seam:
                assert int(pl["arena_off"][c]) == at
                for p in range(a, b):
                    arena[at + p - a] = (int(owner[p]), p - int(seg[:owner[p]].sum()))
                at += b - a
        assert pl["seam_bytes"] == at
        got = {}
        for s, so, ln, do in zip(pl["piece_seg"].tolist(), pl["piece_off"].tolist(), pl["piece_len"].tolist(),
                                 pl["piece_dst"].tolist()):
            for j in range(ln):
                assert do + j not in got
                got[do + j] = (s, so + j)
        assert got == arena
