"""Collective sharded pull without a GPU: the NumPy path of ops.slice_gather_peers and its table
validation against the model (shard_model.py), and pull(device="all", shard=...) over gloo ranks and
a FakeHub: every file crosses the network once per group, every rank ends with exactly its slices."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import shard_collective_util as U
import shard_model as M
import zest_amd
from zest_amd import ops
from zest_amd.device import ST_DTYPES
from zest_amd.testing import FakeHub


# ------------------------------------------------------------------------------------------------
# ops.slice_gather_peers, CPU path
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 2, 3, 16])
@pytest.mark.parametrize("stride", list(M.STRIDES))
def test_slice_gather_peers_cpu_grid(stride, k):
    parts, arena = U.deal(M.grid_specs(stride), k)
    assert len(parts) == k and all(e for _, e in parts)
    U.check_gather_peers(ops, "cpu", parts, arena)


@pytest.mark.parametrize("where", [0, 1, 2])
def test_slice_gather_peers_cpu_source_without_entries(where):
    parts, arena = U.deal([(33, 2, 40), (5, 3, 5), (0, 1, 4), (2048, 2, 2049)], 2, dst_step=16)
    parts.insert(where, (U.source_bytes(64, 9), []))
    U.check_gather_peers(ops, "cpu", parts, arena)
    U.check_gather_peers(ops, "cpu", [(U.source_bytes(0, 1), []), (U.source_bytes(8, 2), [])], 0)  # nothing at all


def test_slice_gather_peers_refuses_bad_tables():
    U.check_refusals(ops, "cpu")


# ------------------------------------------------------------------------------------------------
# end to end: gloo ranks over a FakeHub; each world is started once and runs its scenarios in sequence
# ------------------------------------------------------------------------------------------------
ST_FILES = list(M.FILES)


def _expected_stage(files, rank, world):
    return {n: M.tensor_slice(files[M.FILE_OF[n]], n) for n in M.SPLIT_DIM if U.stage_keeps(n, rank, world)}


def _expected_drop14(files, rank, world):
    return {n: v for n, v in M.expected_shard(files, rank, world).items()
            if ".layers.1." not in n and ".layers.4." not in n}


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """Every scenario's per-rank results, with the hub's counters around each."""
    files = M.build_repo()
    hub = FakeHub(policy="auto", max_xorb_bytes=1 << 20)
    hub.start()
    asked = []
    recon = hub.reconstruction
    hub.reconstruction = lambda h, r=None: (asked.append(h), recon(h, r))[1]
    root = tmp_path_factory.mktemp("collective")
    out = {"hub": hub, "files": files, "root": root, "hash": None}
    worlds = []

    def run(w, name, **sc):
        b0, a0 = hub.xorb_bytes_served, len(asked)
        res = w.run(**sc)
        out[name] = {"res": res, "served": hub.xorb_bytes_served - b0, "asked": asked[a0:]}

    try:
        hub.add_repo(M.REPO, files, xet_suffixes=(".safetensors",))
        out["hash"] = {p: hub.xet_hash(M.REPO, p) for p in M.FILES}
        sizes = [len(files[p]) for p in ST_FILES]
        w4 = U.World(4, hub, root)
        worlds.append(w4)
        w3 = U.World(3, hub, root)
        worlds.append(w3)
        w2 = U.World(2, hub, root)
        worlds.append(w2)
        run(w4, "w4")
        run(w3, "w3_stage", plan="stage", kw={"scratch_bytes": 1})
        run(w2, "w2")
        run(w2, "w2_rounds", kw={"scratch_bytes": max(sizes)})  # less than any two files in their slots
        run(w2, "w2_drop", plan="drop14")
        run(w2, "w2_send", kw={"exchange": "send"})
        run(w2, "refuse_rank", as_rank={1: 0})
        run(w2, "refuse_exchange", kw={"exchange": "bogus"})
        run(w2, "refuse_seed", kw={"seed": True})
        run(w2, "w2_after_refusals")  # the group is still usable: no rank was left in a collective
        hub.corrupt_xorbs = {x.hash_hex for x in hub.xorbs}
        try:
            run(w2, "corrupt", die=True)
            out["corrupt"]["codes"] = w2.stop(timeout=60)
        finally:
            hub.corrupt_xorbs = set()
        yield out
    finally:
        for w in worlds:
            w.stop()
        hub.stop()


def _check_dtypes(tensors):
    for specs in M.FILES.values():
        for name, dt, _, _ in specs:
            if name in tensors:
                assert tensors[name][2] == str(ST_DTYPES[dt]), name


@pytest.mark.parametrize("world,key", [(4, "w4"), (2, "w2"), (2, "w2_send"), (2, "w2_after_refusals")])
def test_every_rank_gets_exactly_its_slices(runs, world, key):
    res = runs[key]["res"]
    assert [r[0] for r in res] == ["ok"] * world, res
    for rank, (_, tensors, st) in enumerate(res):
        U.assert_exact(tensors, M.expected_shard(runs["files"], rank, world))
        _check_dtypes(tensors)
        assert st["exchange"] == "send" and st["skipped_files"] == []


def test_pipeline_stages_at_world_3(runs):
    """Four files over three ranks, one file per round: some rank owns no file in the last round, and
    under the stage plan some owner keeps nothing of a file it fetched."""
    res = runs["w3_stage"]["res"]
    assert [r[0] for r in res] == ["ok"] * 3, res
    fruitless = 0
    for rank, (_, tensors, st) in enumerate(res):
        U.assert_exact(tensors, _expected_stage(runs["files"], rank, 3))
        assert st["rounds"] == 2 and st["groups"] == len(st["owned_files"])
        fruitless += sum(1 for p in st["owned_files"] if not any(M.FILE_OF[n] == p for n in tensors))
    assert sorted(st["groups"] for _, _, st in res) == [1, 1, 2]
    assert sorted(p for _, _, st in res for p in st["owned_files"]) == ST_FILES
    assert fruitless >= 1


def test_each_file_crosses_the_network_once(runs, monkeypatch):
    """The world-4 collective serves no more xorb bytes than one unsharded pull; four independent
    sharded pulls, each from its own empty cache, serve four times that."""
    hub, root = runs["hub"], runs["root"]
    assert [r[0] for r in runs["w4"]["res"]] == ["ok"] * 4

    def served(name, **kw):
        for k, v in hub.env(str(root / name)).items():
            monkeypatch.setenv(k, v)
        b0 = hub.xorb_bytes_served
        zest_amd.pull(M.REPO, device="cpu", p2p=False, dht=False, **kw)
        return hub.xorb_bytes_served - b0

    one = served("unsharded")
    assert one > 0.99 * sum(len(runs["files"][p]) for p in ST_FILES)  # random tensor bytes: no dedup across files
    assert 0 < runs["w4"]["served"] <= one
    assert sum(served(f"alone{r}", shard=(r, 4)) for r in range(4)) == 4 * one


def test_file_no_rank_keeps_is_never_requested(runs):
    res = runs["w2_drop"]["res"]
    assert [r[0] for r in res] == ["ok"] * 2, res
    for rank, (_, tensors, st) in enumerate(res):
        U.assert_exact(tensors, _expected_drop14(runs["files"], rank, 2))
        assert st["skipped_files"] == [U.DROPPED_FILE]
    asked = runs["w2_drop"]["asked"]
    assert runs["hash"][U.DROPPED_FILE] not in asked
    assert {runs["hash"][p] for p in ST_FILES if p != U.DROPPED_FILE} <= set(asked)


def test_small_scratch_takes_several_rounds(runs):
    res = runs["w2_rounds"]["res"]
    assert [r[0] for r in res] == ["ok"] * 2, res
    sizes = [len(runs["files"][p]) for p in ST_FILES]
    for rank, (_, tensors, st) in enumerate(res):
        U.assert_exact(tensors, M.expected_shard(runs["files"], rank, 2))
        assert st["rounds"] >= 2 and st["groups"] >= 2 and st["rounds"] == max(s["groups"] for _, _, s in res)
        assert st["scratch_bytes"] <= max(sizes) + 2 * ops.PAD
        assert len(st["round_gather_s"]) == st["rounds"]


@pytest.mark.parametrize("world,key", [(4, "w4"), (3, "w3_stage"), (2, "w2"), (2, "w2_rounds")])
def test_stats_account_for_every_byte(runs, world, key):
    res = runs[key]["res"]
    total = sum(len(runs["files"][p]) for p in ST_FILES)
    assert sum(st["fetched_bytes"] for _, _, st in res) == total
    for _, tensors, st in res:
        kept = sum(len(t[0]) for t in tensors.values())
        own = sum(len(t[0]) for n, t in tensors.items() if M.FILE_OF[n] in st["owned_files"])
        assert st["kept_bytes"] == kept and st["received_bytes"] + own == kept
        assert st["file_bytes"] == total and st["fetched_bytes"] == sum(len(runs["files"][p]) for p in st["owned_files"])
        assert st["p2p_ratio"] == pytest.approx(st["received_bytes"] / kept) and st["gather_s"] >= 0


def test_corrupt_xorbs_end_every_rank(runs):
    got = runs["corrupt"]
    assert all(r[0] != "ok" and r[0] not in ("AssertionError", "ValueError", "TypeError") for r in got["res"]), got
    assert all(c is not None and c != 0 for c in got["codes"]), got["codes"]  # ended, none left alive


def test_refusals(runs):
    with pytest.raises(ValueError, match="one process per GPU.*init_from_env"):
        zest_amd.pull(M.REPO, device="all", shard=(0, 2), p2p=False, dht=False)
    res = runs["refuse_rank"]["res"]  # one rank's Shard names another rank: every rank raises
    assert all(r[0] == "ValueError" and "does not match the process group" in r[1] for r in res), res
    assert all(r[0] == "ValueError" and "bogus" in r[1] for r in runs["refuse_exchange"]["res"])
    assert all(r[0] == "ValueError" and "seed" in r[1] for r in runs["refuse_seed"]["res"])
