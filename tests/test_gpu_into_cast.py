"""GPU: pull(device="cuda:0", into=..., cast=True) end to end over a FakeHub (cases: into_cast_cases.py,
at most one device pull per test), its result against the CPU into= pull's, and the memory bound that
tells it from pull-then-copy_."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import into_cast_cases as C
import shard_model as M
import zest_amd
from e2e_util import free_port
from into_cases import GUARD, spec
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
        for k, v in hub.env(str(tmp_path_factory.mktemp("gpuintocast"))).items():
            mp.setenv(k, v)
        yield {"hub": hub, "files": files}
    finally:
        mp.undo()
        hub.stop()


def test_whole_tensors_are_converted_and_equal_the_cpu_pull(ctx):
    """Against the model on the device, then destination by destination against the CPU into= pull
    (torch's own converts): bit for bit off NaN."""
    gpu = C.case_whole(ctx, DEV)
    cpu = C.case_whole(ctx, "cpu")
    assert set(gpu) == set(cpu)
    for name, d in gpu.items():
        g, c = d.hold.cpu().numpy(), cpu[name].hold.numpy()
        stored = np.frombuffer(M.tensor_slice(ctx["files"][M.FILE_OF[name]], name)[0], dtype=np.uint8)
        _, loose = C.expected(stored.tobytes(), spec(name)[0], C.dest_dtype(name))
        keep = np.ones(len(g), dtype=bool)
        keep[GUARD:GUARD + d.n] = ~loose
        assert np.array_equal(g[keep], c[keep]), name


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


def test_peak_memory_is_one_scratch_above_the_destinations(ctx):
    """test_gpu_into's bound with every float destination in the other width (BF16 -> F32, F32 ->
    BF16): destinations allocated beforehand, scratch_bytes = the largest file, so every file is a
    group of its own.  Peak torch memory above the start stays within the scratch slot + the largest
    file + ops.PAD + 256 bytes per tensor, which is less than the files together: pull() followed by a
    converting copy_ holds all of them next to the destinations and cannot meet it."""
    files = ctx["files"]
    sizes = [len(files[p]) for p in M.FILES]
    largest = max(sizes)
    dests = C.make_dests({name: spec(name)[1] for name in M.SPLIT_DIM}, DEV, C.OTHER_WIDTH)
    into = {n: d.t for n, d in dests.items()}
    scratch = -(-largest // ops.PAD) * ops.PAD + ops.PAD  # the slot of the largest file
    bound = scratch + largest + ops.PAD + 256 * len(dests)
    assert bound < sum(sizes), (bound, sum(sizes))  # else the bound could not tell this path from pull-then-copy_
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(DEV)
    base = torch.cuda.memory_allocated(DEV)
    st = {}
    zest_amd.pull(M.REPO, device=DEV, p2p=False, dht=False, into=into, cast=True, scratch_bytes=largest, stats=st)
    peak = torch.cuda.max_memory_allocated(DEV) - base
    print(f"peak {peak} bound {bound} files {sum(sizes)} scratch {st['into']['scratch_bytes']}")
    assert st["into"]["groups"] == len(M.FILES) and st["into"]["scratch_bytes"] == scratch
    assert st["into"]["cast_tensors"] == sum(spec(n)[0] in C.OTHER_WIDTH and n != C.KEPT_F32 for n in dests)
    for name, d in dests.items():
        C.check_dest(d, M.tensor_slice(files[M.FILE_OF[name]], name)[0], spec(name)[0],
                     C.dest_dtype(name, C.OTHER_WIDTH), name)
    assert peak <= bound, (peak, bound)
