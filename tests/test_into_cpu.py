"""pull(device="cpu", into=...) end to end over a FakeHub (cases: into_cases.py), and the planner that
zest_amd.into shares with zest_amd.shard."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import into_cases as C
import shard_model as M
from zest_amd import into as zinto
from zest_amd.shard import Shard, plan_file, tensor_runs
from zest_amd.testing import FakeHub

DEV = "cpu"


@pytest.fixture(scope="module")
def ctx(tmp_path_factory):
    files = M.build_repo()
    hub = FakeHub(policy="auto", max_xorb_bytes=1 << 20)
    hub.start()
    mp = pytest.MonkeyPatch()
    try:
        hub.add_repo(M.REPO, files, xet_suffixes=(".safetensors",))
        for k, v in hub.env(str(tmp_path_factory.mktemp("into"))).items():
            mp.setenv(k, v)
        yield {"hub": hub, "files": files}
    finally:
        mp.undo()
        hub.stop()


def test_planner_shares_the_run_arithmetic():
    """plan_file_into's rows are plan_file's with the destination's address for dst_off, for whole
    tensors and for every rank's slices."""
    data = M.build_repo()[M.ODD_START_FILE]
    start, meta = M.header(data)
    for sh in [None] + [Shard(r, M.WORLD) for r in range(M.WORLD)]:
        ref = plan_file(start, meta, sh or Shard(0, 1, {}), len(data))
        dests = {t.name: torch.empty(t.shape, dtype=zinto.zdev.ST_DTYPES[t.dtype]) for t in ref.tensors}
        target = zinto.Target(dests, torch.device("cpu"))
        table, names, total = zinto.plan_file_into(start, meta, target.shard(sh), target.dests, len(data))
        assert names == [t.name for t in ref.tensors] and total == sum(t.nbytes for t in ref.tensors)
        for f in ("src_off", "run_bytes", "src_stride", "n_runs"):
            assert np.array_equal(table[f], ref.table[f]), f
        assert [int(x) for x in table["dst_addr"]] == [dests[n].data_ptr() for n in names]
    ent = {"dtype": "F32", "shape": [6, 4], "data_offsets": [0, 96]}
    assert tensor_runs("w", ent, 8, Shard(1, 2, {"w": 1})) == ((6, 2), 8 + 8, 8, 16, 6, 48)
    assert tensor_runs("w", ent, 8, Shard(1, 2, {"w": "drop"})) is None


def test_whole_tensors_land_byte_for_byte(ctx):
    C.case_whole(ctx, DEV)


@pytest.mark.parametrize("rank", range(M.WORLD))
def test_sharded_into_equals_the_model(ctx, rank):
    C.case_sharded(ctx, DEV, rank)


def test_fused_destinations(ctx):
    C.case_fused(ctx, DEV)


def test_module_with_tied_weights(ctx):
    C.case_module_tied(ctx, DEV)


def test_subset_skips_the_other_files_and_ignores_extras(ctx):
    C.case_subset_of_last_file(ctx, DEV)


@pytest.mark.parametrize("strict", [True, False])
def test_strict_raises_after_the_pull(ctx, strict):
    C.case_strict(ctx, DEV, strict)


@pytest.mark.parametrize("kind", ["shape", "dtype"])
def test_mismatch_names_the_tensor_and_spares_the_file(ctx, kind):
    C.case_mismatch(ctx, DEV, kind)


def test_refusals_come_before_any_request(ctx):
    C.case_refusals(ctx, DEV)


def test_plain_safetensors_take_the_host_route(ctx):
    data = ctx["files"][M.ODD_START_FILE]
    ctx["hub"].add_repo("org/into-plain", {"model.safetensors": data}, xet_suffixes=(".none",))
    want = {n: v for n, v in M.expected_shard(ctx["files"], 3).items() if M.FILE_OF[n] == M.ODD_START_FILE}
    dests = {n: C.Dest(shape, C.spec(n)[0], DEV, i) for i, (n, (_, shape)) in enumerate(want.items())}
    import zest_amd

    got = zest_amd.pull("org/into-plain", device=DEV, p2p=False, dht=False, shard=(3, M.WORLD),
                        into={n: d.t for n, d in dests.items()})
    assert set(got) == set(want)
    for n, d in dests.items():
        d.check(want[n][0], n)
