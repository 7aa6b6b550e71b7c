"""pull(..., into=...) end to end over a FakeHub, shared by the CPU and the GPU tests: destinations
are carved out of canary-filled allocations, and after each pull every byte of every allocation is
compared with the model (shard_model.py reads the safetensors bytes with frombuffer / reshape /
slice): written bytes equal the checkpoint's, everything around them still holds its canary."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import shard_model as M
import zest_amd
from scatter_model import canary
from zest_amd.device import ST_DTYPES

GUARD = 64  # canary bytes before and after every destination
LAST_FILE = "model-00004-of-00004.safetensors"


class Dest:
    """A destination tensor of `shape` / safetensors dtype `dt` inside its own canary-filled allocation."""

    def __init__(self, shape, dt: str, device, salt: int = 0):
        self.n = int(np.prod(shape, dtype=np.int64)) * M.ITEMSIZE[dt]
        self.fill = canary(self.n + 2 * GUARD, salt)
        self.hold = torch.from_numpy(self.fill.copy()).to(device)
        self.t = self.hold[GUARD:GUARD + self.n].view(ST_DTYPES[dt]).view(list(shape))

    def check(self, raw: bytes | None, what: str = "") -> None:
        """raw: the bytes the destination must hold (None: still canary).  The guards always are."""
        want = self.fill.copy()
        if raw is not None:
            assert len(raw) == self.n, what
            want[GUARD:GUARD + self.n] = np.frombuffer(raw, dtype=np.uint8)
        got = self.hold.cpu().numpy()
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, f"{what}: {bad.size} bytes differ, first at {int(bad[0]) - GUARD} of {self.n}"


def spec(name: str):
    """(dtype, shape) of a tensor of the test repository."""
    return next((dt, shape) for specs in M.FILES.values() for n, dt, shape, _ in specs if n == name)


def whole(files, name: str) -> bytes:
    return M.tensor_slice(files[M.FILE_OF[name]], name)[0]


def pull(device, **kw):
    return zest_amd.pull(M.REPO, device=device, p2p=False, dht=False, **kw)


def file_sizes(files) -> dict:
    return {p: len(files[p]) for p in M.FILES}


# ------------------------------------------------------------------------------------------------
def case_whole(ctx, device):
    files = ctx["files"]
    dests = {name: Dest(spec(name)[1], spec(name)[0], device, i) for i, name in enumerate(M.SPLIT_DIM)}
    st = {}
    got = pull(device, into={n: d.t for n, d in dests.items()}, stats=st)
    assert set(got) == set(dests) and all(got[n] is dests[n].t for n in dests)
    for name, d in dests.items():
        d.check(whole(files, name), name)
    s = st["into"]
    assert s["file_bytes"] == sum(file_sizes(files).values()) and s["skipped_files"] == [] and s["missing"] == []
    assert s["written_bytes"] == sum(d.n for d in dests.values()) and s["tensors"] == len(dests)
    assert s["groups"] == 1 and s["scatter_s"] >= 0 and s["scratch_bytes"] > max(file_sizes(files).values())
    return got


def case_sharded(ctx, device, rank: int):
    want = M.expected_shard(ctx["files"], rank)
    dests = {name: Dest(shape, spec(name)[0], device, i) for i, (name, (_, shape)) in enumerate(want.items())}
    assert dests["model.layers.1.scale"].n == 4 and dests["model.layers.1.mlp.up_proj.bias"].n == 0
    assert M.FILE_OF["model.layers.1.scale"] == M.ODD_START_FILE
    st = {}
    got = pull(device, into={n: d.t for n, d in dests.items()}, shard=(rank, M.WORLD), stats=st)
    assert set(got) == set(want)
    for name, d in dests.items():
        d.check(want[name][0], name)
    assert st["into"]["written_bytes"] == sum(len(raw) for raw, _ in want.values())
    return got


def case_fused(ctx, device):
    """q, k and v of layer 0 are row ranges of one [.., 256] tensor with two canary rows on each side."""
    p = "model.layers.0.self_attn."
    hold = Dest([2 + 512 + 128 + 128 + 2, 256], "BF16", device, 77)
    qkv = hold.t
    into = {p + "q_proj.weight": qkv[2:514], p + "k_proj.weight": qkv[514:642], p + "v_proj.weight": qkv[642:770]}
    st = {}
    got = pull(device, into=into, stats=st)
    assert set(got) == set(into)
    want = hold.fill.copy()
    a = GUARD + 2 * 512
    raw = b"".join(whole(ctx["files"], p + x + "_proj.weight") for x in "qkv")
    want[a:a + len(raw)] = np.frombuffer(raw, dtype=np.uint8)
    assert np.array_equal(hold.hold.cpu().numpy(), want)
    assert st["into"]["skipped_files"] == sorted(set(M.FILES) - {M.FILE_OF[p + "q_proj.weight"]})


class _Inner(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.embed_tokens = torch.nn.Embedding(512, 256)
        self.norm = torch.nn.LayerNorm(256, bias=False)


class Tied(torch.nn.Module):
    """state_dict: model.embed_tokens.weight, model.norm.weight, lm_head.weight (tied to the embedding)."""

    def __init__(self):
        super().__init__()
        self.model = _Inner()
        self.lm_head = torch.nn.Linear(256, 512, bias=False)
        self.lm_head.weight = self.model.embed_tokens.weight


def case_module_tied(ctx, device):
    with torch.no_grad():
        m = Tied().to(torch.bfloat16).to(device)
    assert m.lm_head.weight is m.model.embed_tokens.weight
    addr = m.lm_head.weight.data_ptr()
    st = {}
    got = pull(device, into=m, stats=st)
    assert set(got) == {"model.embed_tokens.weight", "model.norm.weight", "lm_head.weight"}
    assert m.lm_head.weight.data_ptr() == addr and got["lm_head.weight"].data_ptr() == addr
    raw = lambda t: t.detach().cpu().reshape(-1).view(torch.uint8).numpy().tobytes()
    files = ctx["files"]
    # the checkpoint's own lm_head.weight (other bytes) is not kept: the first name wins
    assert whole(files, "lm_head.weight") != whole(files, "model.embed_tokens.weight")
    assert raw(m.lm_head.weight) == whole(files, "model.embed_tokens.weight")
    assert raw(m.model.norm.weight) == whole(files, "model.norm.weight")
    assert st["into"]["tensors"] == 2 and st["into"]["missing"] == []
    assert st["into"]["skipped_files"] == ["model-00002-of-00004.safetensors", "model-00003-of-00004.safetensors"]


def case_subset_of_last_file(ctx, device):
    names = ["model.norm.weight", "lm_head.weight"]
    assert all(M.FILE_OF[n] == LAST_FILE for n in names)
    dests = {n: Dest(spec(n)[1], spec(n)[0], device, i) for i, n in enumerate(names)}
    st = {}
    got = pull(device, into={n: d.t for n, d in dests.items()}, stats=st)
    assert set(got) == set(names)  # the file's third tensor is an extra: not kept, no error
    for n, d in dests.items():
        d.check(whole(ctx["files"], n), n)
    s = st["into"]
    assert s["skipped_files"] == sorted(set(M.FILES) - {LAST_FILE}) and len(s["skipped_files"]) == 3
    assert s["file_bytes"] == len(ctx["files"][LAST_FILE]) and s["tensors"] == 2


def case_strict(ctx, device, strict: bool):
    ok = Dest([256], "BF16", device)
    lost = Dest([4], "F32", device, 5)
    into = {"model.norm.weight": ok.t, "model.nowhere.weight": lost.t}
    st = {}
    if strict:
        with pytest.raises(KeyError, match="model.nowhere.weight"):
            pull(device, into=into, stats=st)
    else:
        got = pull(device, into=into, stats=st, strict=False)
        assert set(got) == {"model.norm.weight"}
    ok.check(whole(ctx["files"], "model.norm.weight"))  # raised after the pull: what was found is written
    lost.check(None)
    assert st["into"]["missing"] == ["model.nowhere.weight"]


def case_mismatch(ctx, device, kind: str):
    """The second file holds a tensor that does not fit: ValueError naming it, none of that file's
    destinations written, the first file's written."""
    files = ctx["files"]
    first, ln, bad = "model.embed_tokens.weight", "model.layers.1.input_layernorm.weight", "model.layers.1.scale"
    order = list(M.FILES)
    assert order.index(M.FILE_OF[first]) < order.index(M.FILE_OF[ln]) and M.FILE_OF[bad] == M.FILE_OF[ln]
    d_first, d_ln = Dest(spec(first)[1], spec(first)[0], device), Dest(spec(ln)[1], spec(ln)[0], device, 1)
    d_bad = Dest([2], "F32", device, 2) if kind == "shape" else Dest([], "I32", device, 2)
    with pytest.raises(ValueError, match=r"model\.layers\.1\.scale"):
        pull(device, into={first: d_first.t, ln: d_ln.t, bad: d_bad.t})
    d_first.check(whole(files, first), first)
    d_ln.check(None, ln)
    d_bad.check(None, bad)


def case_refusals(ctx, device):
    """Every refusal comes before the hub sees a request."""
    hub = ctx["hub"]
    d = Dest([256], "BF16", device)
    into = {"model.norm.weight": d.t}
    before = hub.counters.get("requests", 0)
    for kw, word in ((dict(device="all"), "one process per GPU"), (dict(device=device, base=object()), "base="),
                     (dict(device=device, seed=True), "seed"),
                     (dict(device=device, save_snapshot=True), "save_snapshot"),
                     (dict(device=device, direct=False), "direct=False"), (dict(), "needs a device")):
        with pytest.raises(ValueError, match=word):
            zest_amd.pull(M.REPO, into=into, p2p=False, dht=False, **kw)
    elsewhere = torch.empty(256, dtype=torch.bfloat16, device="meta" if device == "cpu" else "cpu")
    rows = Dest([4, 64], "BF16", device, 3)
    for bad, word in (({"model.norm.weight": elsewhere}, "is on"),
                      ({"model.norm.weight": rows.t[:, :32]}, "not contiguous"),
                      ({"model.norm.weight": torch.empty(256, dtype=torch.complex64, device=device)}, "dtype"),
                      ({"model.norm.weight": rows.t[0], "lm_head.weight": rows.t[0, 32:]}, "overlap"),
                      ([d.t], "dict or a torch.nn.Module")):
        with pytest.raises(ValueError, match=word):
            pull(device, into=bad)
    assert hub.counters.get("requests", 0) == before
    d.check(None)
    rows.check(None)
