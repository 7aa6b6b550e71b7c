"""pull(..., into=..., cast=True) end to end over a FakeHub, shared by the CPU and the GPU tests.  The
repository is shard_model's: its tensor bytes are random bits, so subnormals, infinities and NaNs
occur, and its second file starts at an odd offset, so that file's F32 tensors sit at odd addresses.
Destinations are into_cases.Dest allocations in ANOTHER float dtype than the checkpoint's; after each
pull every byte of every allocation is compared: a destination equals the bit-arithmetic model
(cast_model.convert) applied to shard_model's bytes, bit for bit except where the stored element is a
NaN (there a NaN is required), and the guards still hold their canary."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import cast_model as K
import shard_model as M
import zest_amd
from into_cases import GUARD, Dest, pull, spec

KEPT_F32 = "model.layers.0.mlp.gate_proj.weight"  # F32 into F32: its file needs K15 and K16
NARROW = {"BF16": "F16", "F32": "BF16"}            # the dtype map of most cases
OTHER_WIDTH = {"BF16": "F32", "F32": "BF16"}       # the peak-memory case


def dest_dtype(name: str, dtype_map=NARROW) -> str:
    dt = spec(name)[0]
    return dt if name == KEPT_F32 else dtype_map.get(dt, dt)


def expected(raw: bytes, src: str, dst: str) -> tuple[bytes, np.ndarray]:
    """(the bytes a destination must hold, mask of the bytes where any NaN will do)."""
    if src == dst:
        return raw, np.zeros(len(raw), dtype=bool)
    bits = np.frombuffer(raw, dtype=K._utype(src))
    return K.convert(bits, src, dst).tobytes(), np.repeat(K.is_nan(bits, src), K.ITEM[dst])


def check_bytes(got: np.ndarray, raw: bytes, src: str, dst: str, what: str) -> None:
    want, loose = expected(raw, src, dst)
    assert len(got) == len(want), what
    bad = np.flatnonzero((got != np.frombuffer(want, dtype=np.uint8)) & ~loose)
    assert bad.size == 0, f"{what}: {bad.size} bytes differ, first at {int(bad[0])} of {len(want)}"
    if loose.any():
        elems = np.frombuffer(got.tobytes(), dtype=K._utype(dst))
        assert K.is_nan(elems, dst)[loose[::K.ITEM[dst]]].all(), f"{what}: a NaN came out as a number"


def check_dest(d: Dest, raw: bytes | None, src: str, dst: str, what: str) -> None:
    """raw: the stored bytes the destination was filled from (None: still canary).  The guards always
    hold theirs."""
    got = d.hold.cpu().numpy()
    assert np.array_equal(got[:GUARD], d.fill[:GUARD]) and np.array_equal(got[GUARD + d.n:], d.fill[GUARD + d.n:]), what
    if raw is None:
        assert np.array_equal(got, d.fill), what
    else:
        check_bytes(got[GUARD:GUARD + d.n], raw, src, dst, what)


def make_dests(shapes: dict, device, dtype_map=NARROW) -> dict:
    return {name: Dest(shape, dest_dtype(name, dtype_map), device, i) for i, (name, shape) in enumerate(shapes.items())}


def cast_counts(stored: dict, dtype_map=NARROW) -> tuple[int, int]:
    """(tensors converted, stored bytes converted) of {name: stored bytes}."""
    conv = [n for n in stored if dest_dtype(n, dtype_map) != spec(n)[0]]
    return len(conv), sum(len(stored[n]) for n in conv)


# ------------------------------------------------------------------------------------------------
def case_whole(ctx, device):
    """Every BF16 tensor into F16, every F32 one into BF16 but KEPT_F32, U8 and F8 as they are.
    Returns the destinations, for comparing two devices."""
    files = ctx["files"]
    stored = {name: M.tensor_slice(files[M.FILE_OF[name]], name)[0] for name in M.SPLIT_DIM}
    dests = make_dests({name: spec(name)[1] for name in M.SPLIT_DIM}, device)
    kinds = {(spec(n)[0], dest_dtype(n)) for n in dests}
    assert {("BF16", "F16"), ("F32", "BF16"), ("F32", "F32"), ("U8", "U8"), ("F8_E4M3", "F8_E4M3")} == kinds
    st = {}
    got = pull(device, into={n: d.t for n, d in dests.items()}, cast=True, stats=st)
    assert set(got) == set(dests) and all(got[n] is dests[n].t for n in dests)
    for name, d in dests.items():
        check_dest(d, stored[name], spec(name)[0], dest_dtype(name), name)
    s = st["into"]
    assert (s["cast_tensors"], s["cast_bytes_in"]) == cast_counts(stored)
    assert 0 < s["cast_bytes_in"] and s["written_bytes"] == sum(d.n for d in dests.values()) < sum(map(len, stored.values()))
    assert s["tensors"] == len(dests) and s["missing"] == [] and s["skipped_files"] == []
    return dests


def case_sharded(ctx, device, rank: int):
    want = M.expected_shard(ctx["files"], rank)
    dests = make_dests({name: shape for name, (_, shape) in want.items()}, device)
    assert dests["model.layers.1.scale"].n == 2 and dests["model.layers.1.mlp.up_proj.bias"].n == 0
    st = {}
    got = pull(device, into={n: d.t for n, d in dests.items()}, shard=(rank, M.WORLD), cast=True, stats=st)
    assert set(got) == set(want)
    for name, d in dests.items():
        check_dest(d, want[name][0], spec(name)[0], dest_dtype(name), name)
    s = st["into"]
    assert (s["cast_tensors"], s["cast_bytes_in"]) == cast_counts({n: raw for n, (raw, _) in want.items()})
    assert s["written_bytes"] == sum(d.n for d in dests.values())


def case_fused(ctx, device):
    """q, k and v of layer 0 (BF16) are row ranges of one F32 [.., 256] tensor with two canary rows on
    each side."""
    p = "model.layers.0.self_attn."
    hold = Dest([2 + 512 + 128 + 128 + 2, 256], "F32", device, 77)
    qkv = hold.t
    into = {p + "q_proj.weight": qkv[2:514], p + "k_proj.weight": qkv[514:642], p + "v_proj.weight": qkv[642:770]}
    st = {}
    got = pull(device, into=into, cast=True, stats=st)
    assert set(got) == set(into)
    files = ctx["files"]
    raw = b"".join(M.tensor_slice(files[M.FILE_OF[p + x + "_proj.weight"]], p + x + "_proj.weight")[0] for x in "qkv")
    a = GUARD + 2 * 256 * 4
    g = hold.hold.cpu().numpy()
    assert np.array_equal(g[:a], hold.fill[:a]) and np.array_equal(g[a + 2 * len(raw):], hold.fill[a + 2 * len(raw):])
    check_bytes(g[a:a + 2 * len(raw)], raw, "BF16", "F32", "qkv")
    assert st["into"]["cast_tensors"] == 3 and st["into"]["cast_bytes_in"] == len(raw)
    assert st["into"]["written_bytes"] == 2 * len(raw)


def case_module_tied(ctx, device):
    """An F32 module with tied weights from the BF16 checkpoint."""
    from into_cases import Tied

    with torch.no_grad():
        m = Tied().to(device)
    assert m.lm_head.weight is m.model.embed_tokens.weight and m.lm_head.weight.dtype == torch.float32
    addr = m.lm_head.weight.data_ptr()
    st = {}
    got = pull(device, into=m, cast=True, stats=st)
    assert set(got) == {"model.embed_tokens.weight", "model.norm.weight", "lm_head.weight"}
    assert m.lm_head.weight.data_ptr() == addr and got["lm_head.weight"].data_ptr() == addr
    raw = lambda t: t.detach().cpu().reshape(-1).view(torch.uint8).numpy()
    files = ctx["files"]
    for t, name in ((m.lm_head.weight, "model.embed_tokens.weight"), (m.model.norm.weight, "model.norm.weight")):
        check_bytes(raw(t), M.tensor_slice(files[M.FILE_OF[name]], name)[0], "BF16", "F32", name)
    assert st["into"]["tensors"] == st["into"]["cast_tensors"] == 2 and st["into"]["missing"] == []


def case_plain_without_cast(ctx, device):
    """cast=False keeps today's refusal, message included."""
    name = "model.norm.weight"
    d = Dest(spec(name)[1], "F32", device)
    with pytest.raises(ValueError, match=r"model\.norm\.weight: the checkpoint holds BF16, the destination is "
                                         r"torch\.float32 \(into= converts nothing\)"):
        pull(device, into={name: d.t})
    check_dest(d, None, "BF16", "F32", name)


def case_unconvertible(ctx, device):
    """An F8_E4M3 tensor of the second file into a BF16 destination: ValueError naming it, none of that
    file's destinations written, the first file's written (and converted)."""
    files = ctx["files"]
    first, ln = "model.embed_tokens.weight", "model.layers.1.input_layernorm.weight"
    bad = "model.layers.1.self_attn.k_proj.weight"
    order = list(M.FILES)
    assert order.index(M.FILE_OF[first]) < order.index(M.FILE_OF[ln]) and M.FILE_OF[bad] == M.FILE_OF[ln]
    assert spec(bad)[0] == "F8_E4M3"
    d_first, d_ln = Dest(spec(first)[1], "F16", device), Dest(spec(ln)[1], "BF16", device, 1)
    d_bad = Dest(spec(bad)[1], "BF16", device, 2)
    with pytest.raises(ValueError, match=r"model\.layers\.1\.self_attn\.k_proj\.weight.*F8_E4M3"):
        pull(device, into={first: d_first.t, ln: d_ln.t, bad: d_bad.t}, cast=True)
    check_dest(d_first, M.tensor_slice(files[M.FILE_OF[first]], first)[0], "BF16", "F16", first)
    check_dest(d_ln, None, "F32", "BF16", ln)
    check_dest(d_bad, None, "F8_E4M3", "BF16", bad)


def case_cast_needs_into(ctx, device):
    hub = ctx["hub"]
    before = hub.counters.get("requests", 0)
    with pytest.raises(ValueError, match="cast=True needs into="):
        zest_amd.pull(M.REPO, device=device, p2p=False, dht=False, cast=True)
    with pytest.raises(ValueError, match="cast=True needs into="):
        zest_amd.pull(M.REPO, p2p=False, dht=False, cast=True)
    assert hub.counters.get("requests", 0) == before
