"""Sharded pull without a GPU: the planner (zest_amd.shard), the NumPy path of ops.slice_gather and
its table validation against the model (shard_model.py), and pull(device="cpu", shard=...) end to
end over a FakeHub."""
from __future__ import annotations

import json

import numpy as np
import pytest
import torch

import shard_model as M
import zest_amd
from zest_amd import ops
from zest_amd.shard import ARENA_ALIGN, Shard, files_to_skip, plan_file
from zest_amd.testing import FakeHub


def _rows(plan):
    return [tuple(int(x) for x in e) for e in plan.table]


# ------------------------------------------------------------------------------------------------
# planner
# ------------------------------------------------------------------------------------------------
META = {"__metadata__": {"format": "pt"},
        "a": {"dtype": "F32", "shape": [8], "data_offsets": [0, 32]},
        "b": {"dtype": "BF16", "shape": [4, 6], "data_offsets": [32, 80]},
        "c": {"dtype": "U8", "shape": [2, 3, 4], "data_offsets": [80, 104]},
        "d": {"dtype": "I64", "shape": [], "data_offsets": [104, 112]}}


def test_plan_tables_by_hand():
    """(src_off, run_bytes, src_stride, n_runs, dst_off) worked out on paper for data_start = 100."""
    sh = Shard(1, 2, {"a": 0, "b": 1, "c": (1, 1, 3)})
    p = plan_file(100, META, sh, 100 + 112)
    assert _rows(p) == [
        (100 + 16, 16, 16, 1, 0),             # a[4:8]: contiguous, one run
        (100 + 32 + 6, 6, 12, 4, 256),        # b[:, 3:6]: 4 rows, 3 items of 2 bytes out of 6
        (100 + 80 + 4, 8, 12, 2, 512),        # c[:, 1:3, :]: 2 runs of 2 * 4 bytes out of 3 * 4
        (100 + 104, 8, 8, 1, 768)]            # d: a scalar kept whole
    assert p.arena_bytes == 768 + 8
    assert [(t.name, t.dtype, t.shape, t.dst_off, t.nbytes) for t in p.tensors] == [
        ("a", "F32", (4,), 0, 16), ("b", "BF16", (4, 3), 256, 24), ("c", "U8", (2, 2, 4), 512, 16),
        ("d", "I64", (), 768, 8)]
    assert all(t.dst_off % ARENA_ALIGN == 0 for t in p.tensors)
    # rank 0 of the same plan; a dim-0 slice of a 2-D tensor is one run
    p0 = plan_file(100, META, Shard(0, 2, {"a": 0, "b": 0, "c": "drop", "d": "drop"}))
    assert _rows(p0) == [(100, 16, 16, 1, 0), (132, 24, 24, 1, 256)]
    assert p0.dropped == ["c", "d"] and p0.arena_bytes == 256 + 24
    # nothing kept
    pn = plan_file(100, META, Shard(0, 2, {"*": "drop"}))
    assert len(pn.table) == 0 and pn.arena_bytes == 0 and pn.tensors == []


@pytest.mark.parametrize("shape,dim,world", [((8, 6), 0, 4), ((8, 6), 1, 3), ((4, 6, 10), 1, 2), ((4, 6, 10), 2, 5),
                                             ((4, 6, 10), -1, 2), ((12,), 0, 12)])
def test_plan_matches_torch_chunk(shape, dim, world):
    t = torch.arange(int(np.prod(shape)), dtype=torch.int32).reshape(shape)
    raw = t.numpy().tobytes()
    meta = {"t": {"dtype": "I32", "shape": list(shape), "data_offsets": [0, len(raw)]}}
    src = torch.from_numpy(np.frombuffer(b"\x07" * 13 + raw, dtype=np.uint8).copy())
    for r in range(world):
        p = plan_file(13, meta, Shard(r, world, {"t": dim}), len(src))
        arena = torch.zeros(p.arena_bytes, dtype=torch.uint8)
        ops.slice_gather(src, p.table, arena)
        got = p.views(arena)["t"]
        want = torch.chunk(t, world, dim)[r]
        assert got.dtype == torch.int32 and got.is_contiguous() and torch.equal(got, want)


def test_plan_patterns_ranges_and_callables():
    names = {"x.q_proj.weight": [8, 4], "x.q_proj.bias": [8], "x.o_proj.weight": [4, 8], "x.o_proj.bias": [4],
             "x.norm.weight": [4], "model.embed_tokens.weight": [8, 4], "lm_head.weight": [8, 4],
             "x.mlp.down_proj.weight": [4, 8], "x.mlp.gate_proj.weight": [8, 4]}
    sh = Shard(1, 4)  # built in: llama-tp
    got = {n: sh.resolve(n, s, "BF16") for n, s in names.items()}
    assert got == {"x.q_proj.weight": (0, 2, 4), "x.q_proj.bias": (0, 2, 4), "x.o_proj.weight": (1, 2, 4),
                   "x.o_proj.bias": None, "x.norm.weight": None, "model.embed_tokens.weight": (0, 2, 4),
                   "lm_head.weight": (0, 2, 4), "x.mlp.down_proj.weight": (1, 2, 4),
                   "x.mlp.gate_proj.weight": (0, 2, 4)}
    # first match wins; no match keeps whole
    first = Shard(0, 2, {"*.weight": 1, "x.*": "drop", "*": 0})
    assert first.resolve("x.q_proj.weight", [8, 4], "F32") == (1, 0, 2)
    assert first.resolve("x.q_proj.bias", [8], "F32") == "drop"
    assert first.resolve("y", [8], "F32") == (0, 0, 4)
    assert Shard(0, 2, {"x.*": 0}).resolve("y", [3], "F32") is None
    # explicit ranges: uneven, empty, negative dim
    rng = Shard(3, 4, {"k": (0, 5, 8), "e": (1, 2, 2), "n": (-1, 0, 3)})
    assert rng.resolve("k", [8, 2], "F32") == (0, 5, 8)
    assert rng.resolve("e", [8, 2], "F32") == (1, 2, 2)
    assert rng.resolve("n", [8, 3], "F32") == (1, 0, 3)

    def stage(name, shape, dtype):  # a pipeline stage: the plan sees rank and world through its Shard
        s = stage.shard
        return None if name.startswith(f"layers.{s.rank}.") else "drop" if name.startswith("layers.") else 0

    for r in range(3):
        s = Shard(r, 3, stage)
        assert [s.resolve(f"layers.{i}.w", [3], "F32") for i in range(3)] == \
            [None if i == r else "drop" for i in range(3)]
        assert s.resolve("embed", [6, 2], "F32") == (0, 2 * r, 2 * r + 2)
    assert zest_amd.shard.as_shard((1, 2)).plan is zest_amd.shard.PLANS["llama-tp"]


def test_plan_errors():
    ent = {"dtype": "F32", "shape": [6, 4], "data_offsets": [0, 96]}
    with pytest.raises(ValueError, match="w.*not divisible"):
        plan_file(8, {"w": ent}, Shard(0, 4, {"w": 0}))
    with pytest.raises(ValueError, match="w.*out of range"):
        plan_file(8, {"w": ent}, Shard(0, 2, {"w": 2}))
    with pytest.raises(ValueError, match="w.*out of range"):
        plan_file(8, {"w": {"dtype": "F32", "shape": [], "data_offsets": [0, 4]}}, Shard(0, 2, {"w": 0}))
    for bad in ((0, 4, 7), (0, 3, 2), (0, -1, 2)):
        with pytest.raises(ValueError, match="w.*range"):
            plan_file(8, {"w": ent}, Shard(0, 2, {"w": bad}))
    with pytest.raises(ValueError, match="w.*not None"):
        plan_file(8, {"w": ent}, Shard(0, 2, {"w": "keep"}))
    for r, w in ((2, 2), (-1, 2), (0, 0)):
        with pytest.raises(ValueError, match="rank"):
            Shard(r, w)
    with pytest.raises(ValueError, match="unknown plan"):
        Shard(0, 2, "gpt-tp")
    with pytest.raises(ValueError, match="w: unsupported dtype C64"):
        plan_file(8, {"w": dict(ent, dtype="C64")}, Shard(0, 2))
    with pytest.raises(ValueError, match="w.*do not match"):
        plan_file(8, {"w": dict(ent, data_offsets=[0, 92])}, Shard(0, 2))
    with pytest.raises(ValueError, match="w.*past the file"):
        plan_file(8, {"w": ent}, Shard(0, 2), file_size=8 + 95)
    plan_file(8, {"w": ent}, Shard(0, 2), file_size=8 + 96)
    with pytest.raises(ValueError):
        zest_amd.shard.as_shard(3)


def test_files_to_skip():
    idx = {"weight_map": {"layers.0.a": "f0", "layers.0.b": "f0", "layers.1.a": "f1", "embed": "f1",
                          "layers.2.a": "f2"}}
    names = ["f0", "f1", "f2", "unlisted"]
    drop0 = Shard(0, 2, {"layers.0.*": "drop", "layers.2.*": "drop", "layers.1.*": "drop"})
    assert files_to_skip(json.dumps(idx), names, drop0) == {"f0", "f2"}  # f1 keeps `embed`
    assert files_to_skip(idx, names, Shard(0, 2)) == set()
    seen = []

    def by_shape(name, shape, dtype):  # decides with the shape: cannot drop without it
        seen.append(shape)
        return "drop" if shape is not None and len(shape) == 1 else None

    assert files_to_skip(idx, names, Shard(0, 2, by_shape)) == set() and set(seen) == {None}
    assert files_to_skip(idx, names, Shard(0, 2, lambda n, s, d: "drop" if len(s) == 1 else None)) == set()
    assert files_to_skip(idx, names, Shard(0, 2, lambda n, s, d: "drop")) == {"f0", "f1", "f2"}


# ------------------------------------------------------------------------------------------------
# ops.slice_gather, CPU path
# ------------------------------------------------------------------------------------------------
def _src(n, seed=3):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)


@pytest.mark.parametrize("stride", list(M.STRIDES))
def test_slice_gather_cpu_grid(stride):
    entries, src_len, arena = M.lay_out(M.grid_specs(stride))
    src = _src(src_len)
    for align in (0, 5, 15):
        M.check_gather(ops, "cpu", src, entries, arena, align)


def test_slice_gather_cpu_shapes():
    for specs, step in (([(50_001, 3, 50_008)], 256),                      # several output tiles
                        ([(24, 1, 24)] * 600, 32),                          # more tensors than the boundary cache
                        ([(0, 5, 0), (7, 0, 9), (33, 2, 40), (0, 0, 0), (5, 3, 5), (9, 0, 9), (0, 1, 4)], 16),
                        ([(17, 1, 17)], 256)):                              # a single entry
        entries, src_len, arena = M.lay_out(specs, dst_step=step)
        M.check_gather(ops, "cpu", _src(src_len), entries, arena, 7)
    M.check_gather(ops, "cpu", _src(10), [], 0)  # an empty table


def test_slice_gather_refuses_bad_tables():
    src = torch.zeros(100, dtype=torch.uint8)
    dst = torch.zeros(64, dtype=torch.uint8)

    def run(*entries):
        ops.slice_gather(src, np.array(list(entries), dtype=ops.SLICE_DTYPE), dst)

    run((90, 10, 10, 1, 0), (0, 4, 48, 3, 16), (100, 0, 0, 0, 32), (0, 1, 1, 16, 48))  # all legal, to the last byte
    with pytest.raises(ValueError, match="entry 1.*past the source"):
        run((0, 10, 10, 1, 0), (91, 10, 10, 1, 16))
    with pytest.raises(ValueError, match="entry 0.*past the source"):
        run((0, 4, 49, 3, 0))  # the last run ends at 102
    with pytest.raises(ValueError, match="entry 0.*past the source"):
        run((1 << 63, 2, 1 << 63, 3, 0))  # would wrap around 64 bits
    with pytest.raises(ValueError, match="entry 1.*past the arena"):
        run((0, 10, 10, 1, 0), (0, 17, 17, 1, 48))
    with pytest.raises(ValueError, match="entry 1.*overlaps"):
        run((0, 17, 17, 1, 0), (0, 4, 4, 1, 16))
    with pytest.raises(ValueError, match="entry 2.*overlaps"):
        run((0, 4, 4, 1, 0), (0, 4, 4, 1, 32), (0, 4, 4, 1, 16))  # descending
    with pytest.raises(ValueError, match="entry 0.*aligned"):
        run((0, 4, 4, 1, 8))
    with pytest.raises(ValueError, match="entry 0.*src_stride"):
        run((0, 4, 3, 2, 0))
    with pytest.raises(ValueError, match="uint8"):
        ops.slice_gather(src.view(torch.int16), np.zeros(0, dtype=ops.SLICE_DTYPE), dst)


# ------------------------------------------------------------------------------------------------
# end to end over a FakeHub
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def e2e(tmp_path_factory):
    files = M.build_repo()
    sizes = sorted(len(v) for k, v in files.items() if k.endswith(".safetensors"))
    assert 0.29e6 < sizes[0] and sizes[-1] < 2e6 and len(sizes) == 4
    assert len(files[next(iter(M.FILES))]) == sizes[-1]  # the largest file comes first in the listing
    assert M.header(files[M.ODD_START_FILE])[0] % 16 == 5
    hub = FakeHub(policy="auto", max_xorb_bytes=1 << 20)
    hub.start()
    asked = []
    recon = hub.reconstruction
    hub.reconstruction = lambda h, r=None: (asked.append(h), recon(h, r))[1]
    mp = pytest.MonkeyPatch()
    try:
        hub.add_repo(M.REPO, files, xet_suffixes=(".safetensors",))
        for k, v in hub.env(str(tmp_path_factory.mktemp("shard"))).items():
            mp.setenv(k, v)
        full = zest_amd.pull(M.REPO, device="cpu", p2p=False, dht=False)
        assert set(full) == set(M.SPLIT_DIM)
        yield {"hub": hub, "files": files, "full": full, "asked": asked, "mp": mp,
               "hash": {p: hub.xet_hash(M.REPO, p) for p in M.FILES}}
    finally:
        mp.undo()
        hub.stop()


def _raw(t: torch.Tensor) -> bytes:
    return t.contiguous().reshape(-1).view(torch.uint8).numpy().tobytes() if t.numel() else b""


def _pull(shard, **kw):
    return zest_amd.pull(M.REPO, device="cpu", p2p=False, dht=False, shard=shard, **kw)


def test_e2e_cpu_every_rank_is_exact(e2e):
    full, parts = e2e["full"], []
    for r in range(M.WORLD):
        st = {}
        got = _pull((r, M.WORLD), stats=st)
        want = M.expected_shard(e2e["files"], r)
        assert set(got) == set(full) == set(want)
        for name, t in got.items():
            dim = M.SPLIT_DIM[name]
            ref = full[name] if dim is None else torch.chunk(full[name], M.WORLD, dim)[r]
            assert t.dtype == ref.dtype and t.shape == ref.shape and t.is_contiguous(), name
            assert _raw(t) == _raw(ref) == want[name][0] and list(t.shape) == want[name][1], name
        s = st["shard"]
        assert s["file_bytes"] == sum(len(e2e["files"][p]) for p in M.FILES) and s["skipped_files"] == []
        assert s["kept_bytes"] == sum(t.numel() * t.element_size() for t in got.values()) < s["file_bytes"] // 3
        assert s["groups"] == 1 and s["gather_s"] >= 0
        parts.append(got)
    for name, dim in M.SPLIT_DIM.items():  # the four shards rebuild every tensor
        if dim is not None:
            whole = torch.cat([p[name].view(torch.uint8) if p[name].element_size() == 1 else p[name] for p in parts],
                              dim)
            assert _raw(whole) == _raw(full[name]), name


def test_e2e_cpu_dropped_file_is_never_requested(e2e):
    def stage(name, shape, dtype):  # pipeline stages by layer; the rest replicated
        if ".layers." not in name:
            return None
        return None if int(name.split(".layers.")[1].split(".")[0]) % M.WORLD == stage.shard.rank else "drop"

    del e2e["asked"][:]
    st = {}
    got = _pull(Shard(2, M.WORLD, stage), stats=st)
    layer2 = "model-00003-of-00004.safetensors"
    kept = {n for n in M.SPLIT_DIM if ".layers." not in n or ".layers.2." in n}
    assert set(got) == kept
    for n in kept:
        assert _raw(got[n]) == _raw(e2e["full"][n]) and got[n].shape == e2e["full"][n].shape
    # file 2 holds only other stages' layers; files 1 and 4 also hold replicated tensors
    assert st["shard"]["skipped_files"] == ["model-00002-of-00004.safetensors"]
    assert e2e["hash"]["model-00002-of-00004.safetensors"] not in e2e["asked"]
    assert {e2e["hash"][p] for p in M.FILES if p != "model-00002-of-00004.safetensors"} <= set(e2e["asked"])
    assert e2e["hash"][layer2] in e2e["asked"]


def test_e2e_cpu_small_scratch_reuses_the_slot(e2e):
    sizes = [len(e2e["files"][p]) for p in M.FILES]
    st = {}
    got = _pull((1, M.WORLD), scratch_bytes=sizes[0] + sizes[1] - 1, stats=st)  # smaller than two files
    assert st["shard"]["groups"] >= 2 and st["shard"]["scratch_bytes"] < sizes[0] + sizes[1] + 2 * ops.PAD
    want = M.expected_shard(e2e["files"], 1)
    assert set(got) == set(want)
    for name, (raw, shape) in want.items():  # the second file landed where the largest one was
        assert _raw(got[name]) == raw and list(got[name].shape) == shape, name
    st = {}
    got = _pull((1, M.WORLD), scratch_bytes=1, stats=st)  # a file larger than the scratch grows it
    assert st["shard"]["groups"] == 4 and st["shard"]["scratch_bytes"] >= sizes[0]
    assert all(_raw(got[n]) == raw for n, (raw, _) in want.items())


def test_e2e_cpu_plain_safetensors(e2e):
    """A safetensors file that is not Xet-backed takes the host route, then the same plan and gather."""
    data = e2e["files"][M.ODD_START_FILE]
    e2e["hub"].add_repo("org/shard-plain", {"model.safetensors": data}, xet_suffixes=(".none",))
    got = zest_amd.pull("org/shard-plain", device="cpu", p2p=False, dht=False, shard=(3, M.WORLD))
    want = {n: v for n, v in M.expected_shard(e2e["files"], 3).items() if M.FILE_OF[n] == M.ODD_START_FILE}
    assert set(got) == set(want)
    for name, (raw, shape) in want.items():
        assert _raw(got[name]) == raw and list(got[name].shape) == shape, name


def test_refused_combinations(e2e):
    for kw, word in ((dict(device="all"), "one process per GPU"), (dict(device="cuda:0", seed=True), "seed"),
                     (dict(device="cpu", save_snapshot=True), "save_snapshot"),
                     (dict(device="cpu", direct=False), "direct=False"), (dict(), "needs a device")):
        with pytest.raises(ValueError, match=word):
            zest_amd.pull(M.REPO, shard=(0, 2), p2p=False, dht=False, **kw)


def test_e2e_cpu_corrupt_xorb_fails_the_pull(e2e, tmp_path):
    hub = e2e["hub"]
    with pytest.MonkeyPatch.context() as mp:
        for k, v in hub.env(str(tmp_path)).items():  # empty caches: every byte comes from the hub
            mp.setenv(k, v)
        hub.corrupt_xorbs = {x.hash_hex for x in hub.xorbs}
        try:
            with pytest.raises(Exception) as ei:
                _pull((0, M.WORLD))
            assert not isinstance(ei.value, (AssertionError, ValueError, TypeError))
        finally:
            hub.corrupt_xorbs = set()
        got = _pull((0, M.WORLD))  # and with the corruption gone the same caches serve a clean pull
        assert all(_raw(got[n]) == raw for n, (raw, _) in M.expected_shard(e2e["files"], 0).items())
