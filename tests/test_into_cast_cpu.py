"""pull(device="cpu", into=..., cast=True) end to end over a FakeHub (cases: into_cast_cases.py), and the
cast=True plan of zest_amd.into.plan_file_into."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import into_cast_cases as C
import shard_model as M
import zest_amd
from into_cases import spec
from zest_amd import into as zinto
from zest_amd import ops
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
        for k, v in hub.env(str(tmp_path_factory.mktemp("intocast"))).items():
            mp.setenv(k, v)
        yield {"hub": hub, "files": files}
    finally:
        mp.undo()
        hub.stop()


def test_cast_plan_marks_what_is_converted():
    """The cast=True plan has the cast=False plan's runs (in stored bytes) for every tensor, the kind of
    each converted tensor and SAME for the rest; destination bytes are counted."""
    data = M.build_repo()[M.ODD_START_FILE]
    start, meta = M.header(data)
    names = [n for n in meta]
    same = {n: torch.empty(meta[n]["shape"], dtype=zinto.zdev.ST_DTYPES[meta[n]["dtype"]]) for n in names}
    plain = zinto.plan_file_into(start, meta, zinto.Target(same, torch.device("cpu")).shard(None), same, len(data))
    other = {"BF16": torch.float32, "F32": torch.float16}
    dests = {n: torch.empty(meta[n]["shape"], dtype=other.get(meta[n]["dtype"], same[n].dtype)) for n in names}
    target = zinto.Target(dests, torch.device("cpu"))
    table, got_names, total = zinto.plan_file_into(start, meta, target.shard(None), target.dests, len(data), cast=True)
    assert got_names == plain[1] and table.dtype == ops.CAST_DTYPE
    for f in ("src_off", "run_bytes", "src_stride", "n_runs"):
        assert np.array_equal(table[f], plain[0][f]), f
    want = {"BF16": ops.CAST_KINDS[("BF16", "F32")], "F32": ops.CAST_KINDS[("F32", "F16")]}
    assert [int(k) for k in table["kind"]] == [want.get(meta[n]["dtype"], zinto.SAME) for n in got_names]
    assert total == sum(t.numel() * t.element_size() for t in dests.values()) != plain[2]
    with pytest.raises(ValueError, match="converts nothing"):
        zinto.plan_file_into(start, meta, target.shard(None), target.dests, len(data))


def test_whole_tensors_are_converted_bit_for_bit(ctx):
    C.case_whole(ctx, DEV)


@pytest.mark.parametrize("rank", range(M.WORLD))
def test_sharded_into_equals_the_model(ctx, rank):
    C.case_sharded(ctx, DEV, rank)


def test_fused_destinations(ctx):
    C.case_fused(ctx, DEV)


def test_module_with_tied_weights(ctx):
    C.case_module_tied(ctx, DEV)


def test_without_cast_nothing_is_converted(ctx):
    C.case_plain_without_cast(ctx, DEV)


def test_unconvertible_pair_names_the_tensor_and_spares_the_file(ctx):
    C.case_unconvertible(ctx, DEV)


def test_cast_without_into_is_refused_before_any_request(ctx):
    C.case_cast_needs_into(ctx, DEV)


def test_plain_safetensors_take_the_host_route(ctx):
    """A non-Xet file, sharded, converted: the same plan and the same two scatters."""
    data = ctx["files"][M.ODD_START_FILE]
    ctx["hub"].add_repo("org/into-cast-plain", {"model.safetensors": data}, xet_suffixes=(".none",))
    want = {n: v for n, v in M.expected_shard(ctx["files"], 3).items() if M.FILE_OF[n] == M.ODD_START_FILE}
    dests = C.make_dests({n: shape for n, (_, shape) in want.items()}, DEV)
    st = {}
    got = zest_amd.pull("org/into-cast-plain", device=DEV, p2p=False, dht=False, shard=(3, M.WORLD), cast=True,
                        into={n: d.t for n, d in dests.items()}, stats=st)
    assert set(got) == set(want)
    for n, d in dests.items():
        C.check_dest(d, want[n][0], spec(n)[0], C.dest_dtype(n), n)
    assert st["into"]["cast_tensors"] == C.cast_counts({n: raw for n, (raw, _) in want.items()})[0] > 0
