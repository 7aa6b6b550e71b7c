"""GPU: pull(device="cuda:0", into=..., base=...) end to end over a FakeHub (cases: into_delta_cases.py).
Resident chunks are hashed where they lie (ops.hash_chunks_at), moved chunks gathered and re-hashed by
K12 (ops.reuse_chunks), fetched terms decoded by the device pull's pipeline into the patch scratch,
and K15 (ops.slice_scatter) writes only the fetched and the moved pieces; the memory bound tells the
delta pull from a plain pull(into=)."""
from __future__ import annotations

import pytest
import torch

import into_delta_cases as C
import into_delta_model as M
import into_delta_repo as R
from e2e_util import free_port
from test_into_delta_cpu import make_ctx, peak_bound
from zest_amd import _core

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def ctx(tmp_path_factory):
    mp = pytest.MonkeyPatch()
    mp.setenv("ZEST_LISTEN_PORT", str(free_port()))
    try:
        for c in make_ctx(tmp_path_factory, "gpuintodelta"):
            hub, n = c["hub"], c["n"]
            assert any(e[2] != 0 for x in hub.xorbs[n[1]:n[2]] for e in _core.index_chunks(x.data)), \
                "revision 2 must add compressed chunks"
            yield c
    finally:
        mp.undo()


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


def test_peak_memory_is_the_changed_bytes(ctx):
    """Peak torch memory above the start: the delta pull stays within the oracle's bound (patch slots,
    seam arena, moved bytes, tables, hash scratch), which is below half the largest file; a plain
    pull(into=) of the same revision holds at least the largest file."""
    hub, (rev1, rev2, _) = ctx["hub"], ctx["revs"]
    largest = max(len(v) for v in rev2.values())
    landed, dests = C.first_pull(ctx, DEV)
    resident, (_, seam_bytes, _) = M.bind(hub, R.REPO1, rev1, C.addrs({n: dests[n] for n in landed}))
    exp = M.expect(hub, R.REPO2, rev2, resident, C.addrs(dests))
    bound = peak_bound(ctx, exp, seam_bytes)
    assert bound < largest // 2, (bound, largest)
    into = C.tensors(dests)

    def peak(**kw):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()  # a cached block that is handed out whole would count with its unused tail
        torch.cuda.reset_peak_memory_stats(DEV)
        start = torch.cuda.memory_allocated(DEV)
        out = C.pull(R.REPO2, DEV, into=into, **kw)
        return torch.cuda.max_memory_allocated(DEV) - start, out

    st = {}
    p_delta, _ = peak(base=landed, stats=st)
    C.check_all(dests, rev2, "delta")
    assert st["into"]["delta"]["fallback_files"] == 0
    p_plain, _ = peak()
    C.check_all(dests, rev2, "plain")
    print(f"peak: delta {p_delta}, bound {bound}, plain {p_plain}, largest file {largest}")
    assert p_delta <= bound, (p_delta, bound)
    assert p_plain >= largest, (p_plain, largest)
