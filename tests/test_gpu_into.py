"""GPU: pull(device="cuda:0", into=...) end to end over a FakeHub (cases: into_cases.py, at most one
device pull per test), its result against the CPU pull's, and the memory bound that tells it from
pull-then-copy."""
from __future__ import annotations

import pytest
import torch

import into_cases as C
import shard_model as M
import zest_amd
from e2e_util import free_port
from zest_amd import ops
from zest_amd.testing import FakeHub

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def ctx(tmp_path_factory):
    files = M.build_repo()
    hub = FakeHub(policy="auto", max_xorb_bytes=1 << 20)
    hub.start()
    mp = pytest.MonkeyPatch()
    try:
        hub.add_repo(M.REPO, files, xet_suffixes=(".safetensors",))
        mp.setenv("ZEST_LISTEN_PORT", str(free_port()))
        for k, v in hub.env(str(tmp_path_factory.mktemp("cpuinto"))).items():
            mp.setenv(k, v)
        cpu = zest_amd.pull(M.REPO, device="cpu", p2p=False, dht=False)
        for k, v in hub.env(str(tmp_path_factory.mktemp("gpuinto"))).items():  # empty caches for the device pulls
            mp.setenv(k, v)
        yield {"hub": hub, "files": files, "cpu": cpu}
    finally:
        mp.undo()
        hub.stop()


def test_whole_tensors_land_byte_for_byte_and_equal_the_cpu_pull(ctx):
    got = C.case_whole(ctx, DEV)
    cpu = ctx["cpu"]
    assert set(got) == set(cpu)
    for name, t in got.items():
        w = cpu[name]
        assert t.device.type == "cuda" and t.dtype == w.dtype and t.shape == w.shape, name
        assert torch.equal(t.cpu().reshape(-1).view(torch.uint8), w.reshape(-1).view(torch.uint8)), name


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


def test_peak_memory_is_one_scratch_above_the_destinations(ctx):
    """Destinations allocated beforehand, scratch_bytes = the largest file: every file is a group of
    its own.  Peak torch memory above the start stays within the scratch slot + the largest file +
    ops.PAD + 256 bytes per tensor (the allowance of the sharded bound test, without arenas), which is
    less than the files together: pull() followed by copy_ holds all of them and cannot meet it."""
    files = ctx["files"]
    sizes = [len(files[p]) for p in M.FILES]
    largest = max(sizes)
    dests = {name: C.Dest(C.spec(name)[1], C.spec(name)[0], DEV, i) for i, name in enumerate(M.SPLIT_DIM)}
    into = {n: d.t for n, d in dests.items()}
    scratch = -(-largest // ops.PAD) * ops.PAD + ops.PAD  # the slot of the largest file
    bound = scratch + largest + ops.PAD + 256 * len(dests)
    assert bound < sum(sizes), (bound, sum(sizes))  # else the bound could not tell this path from pull-then-copy
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(DEV)
    base = torch.cuda.memory_allocated(DEV)
    st = {}
    zest_amd.pull(M.REPO, device=DEV, p2p=False, dht=False, into=into, scratch_bytes=largest, stats=st)
    peak = torch.cuda.max_memory_allocated(DEV) - base
    print(f"peak {peak} bound {bound} files {sum(sizes)} scratch {st['into']['scratch_bytes']}")
    assert st["into"]["groups"] == len(M.FILES) and st["into"]["scratch_bytes"] == scratch
    for name, d in dests.items():
        d.check(C.whole(files, name), name)
    assert peak <= bound, (peak, bound)
