"""The plain-Python model of the Xet Merkle aggregation (tests/merkle_model.py): it equals the host
core on every case of every family, each family reaches the path of csrc/gpu/merkle.hip it is named
for (asserted from the model's stats), and every deliberately wrong rule (`rule=`) is told from the
right one by a named case -- so the GPU test that compares the kernels with this model
(tests/test_gpu_merkle.py) is sharp.
"""
from __future__ import annotations

import numpy as np
import pytest
import torch

import merkle_model as M
from zest_amd import _core as C
from zest_amd import ops

FAMILY_NAMES = sorted(M.FAMILIES)


def _by_name(fam):
    return {c.name: (c, root, st) for c, (root, st) in zip(M.family(fam), M.modelled(fam))}


def _rule_root(fam, name, rule):
    c = _by_name(fam)[name][0]
    return M.merkle_model(M.leaves_of(c.hashes, c.sizes), rule=rule)


def test_xet_hex_matches_core():
    rng = np.random.default_rng(1)
    for _ in range(8):
        h = rng.integers(0, 256, 32, dtype=np.uint8).tobytes()
        assert M.xet_hex(h) == C.xet_hex(h)
        assert M._hex_all([h, h[::-1]]) == C.xet_hex(h) + C.xet_hex(h[::-1])


# ---- a. the model equals the host core --------------------------------------------------------------
@pytest.mark.parametrize("fam", FAMILY_NAMES)
def test_model_matches_core(fam):
    for c, (root, _) in zip(M.family(fam), M.modelled(fam)):
        leaves = M.leaves_of(c.hashes, c.sizes)
        assert root == C.merkle_root(leaves), c.name
        assert M.file_hash_of_root(root, len(leaves)) == C.file_hash(leaves), c.name
    c = M.family(fam)[-1]
    leaves = M.leaves_of(c.hashes, c.sizes)
    assert M.merkle_model(leaves, file_hash=True) == C.file_hash(leaves), c.name


@pytest.mark.parametrize("name", M.FLAGWORDS_LARGE_NAMES)
def test_model_matches_core_large(name):
    c, root, _ = M.modelled_large(name)
    leaves = M.leaves_of(c.hashes, c.sizes)
    assert root == C.merkle_root(leaves)
    assert M.file_hash_of_root(root, len(leaves)) == C.file_hash(leaves)


def test_empty_and_single():
    h = bytes(range(32))
    assert M.merkle_model([]) == bytes(32) == C.merkle_root([])
    assert M.merkle_model([], file_hash=True) == bytes(32) == C.file_hash([])
    assert M.merkle_model([(h, 5)]) == h
    assert M.merkle_model([(h, 5)], file_hash=True) == C.blake3_keyed(bytes(32), h) == C.file_hash([(h, 5)])


def test_model_refuses_a_sum_of_2_to_64():
    h = bytes(32)
    M.merkle_model([(h, 2 ** 64 - 1), (h, 0)])
    with pytest.raises(AssertionError):
        M.merkle_model([(h, 2 ** 64 - 1), (h, 1)])


@pytest.mark.parametrize("fam", FAMILY_NAMES)
def test_ops_cpu_path_agrees(fam):
    """ops.merkle_roots on CPU tensors, a sample of each family batched as jobs over one leaf array."""
    picks = list(zip(M.family(fam), M.modelled(fam)))[::7][:12]
    hs = np.concatenate([c.hashes for c, _ in picks])
    sz = np.concatenate([c.sizes for c, _ in picks])
    jobs, base = [], 0
    for c, _ in picks:
        jobs.append((base, len(c.sizes)))
        base += len(c.sizes)
    h_t, s_t = torch.from_numpy(hs.copy()), torch.from_numpy(sz.view(np.int64).copy())
    raw = ops.merkle_roots(h_t, s_t, jobs, file_hash=False).numpy()
    fh = ops.merkle_roots(h_t, s_t, jobs, file_hash=True).numpy()
    for j, (c, (root, _)) in enumerate(picks):
        assert raw[j].tobytes() == root, c.name
        assert fh[j].tobytes() == M.file_hash_of_root(root, len(c.sizes)), c.name


def test_anchor_hf_xet_file_hash(tmp_path):
    """End to end against xet-core's own binding: real chunk boundaries and chunk hashes, the tree
    and the file hash from the model."""
    hf_xet = pytest.importorskip("hf_xet")
    rng = np.random.default_rng(77)
    data = rng.integers(0, 256, 24 << 20, dtype=np.uint8).tobytes()
    ends = C.chunk_ends(data)
    assert 200 <= len(ends) <= 1000
    leaves, prev = [], 0
    for e in ends:
        leaves.append((C.chunk_hash(data[prev:e]), e - prev))
        prev = e
    p = tmp_path / "f"
    p.write_bytes(data)
    assert M.xet_hex(M.merkle_model(leaves, file_hash=True)) == hf_xet.hash_files([str(p)])[0].hash


# ---- b. each family reaches its path ----------------------------------------------------------------
def test_shape_paths():
    by = _by_name("shape")
    n = M.SHAPE_N
    lv = by["shape_none"][2]["levels"][0]
    assert lv["groups"] == {9: n // 9, n % 9: 1} and lv["B"] == 3 and lv["span3"] > 0
    assert by["shape_idx01"][2]["levels"][0]["groups"] == lv["groups"]  # flags at indices 0 and 1 are ignored
    assert by["shape_all"][2]["levels"][0]["groups"] == {3: n // 3, n % 3: 1}
    for period in range(3, 10):  # a flag every `period` leaves from phase period-1: groups of `period`
        g = by[f"shape_p{period}_{period - 1}"][2]["levels"][0]["groups"]
        assert g[period] == n // period, period
    seen = set()
    for _, _, st in by.values():
        seen |= set(st["levels"][0]["groups"])
    assert seen >= set(range(3, 10))
    # a single flag moves one boundary: at k < 2 none, at k >= 2 the first group closes after it
    assert by["shape_one_50_1"][2]["levels"][0]["groups"] == {9: 5, 5: 1}
    assert by["shape_one_50_2"][2]["levels"][0]["groups"] == {3: 1, 9: 5, 2: 1}
    assert by["shape_one_50_10"][2]["levels"][0]["groups"] == {9: 5, 5: 1}  # index 1 of the second group: ignored
    assert by["shape_one_50_49"][2]["levels"][0]["groups"] == {9: 5, 5: 1}


def test_tails_paths():
    by = _by_name("tails")
    depth = {len(st["levels"]) for _, _, st in by.values()}
    assert depth >= {0, 1, 2, 3}
    sizes, last = set(), set()
    for c, _, st in by.values():
        for lv in st["levels"]:
            sizes |= set(lv["groups"])
        if st["levels"]:
            lv = st["levels"][0]
            if lv["groups"].get(1):
                last.add(1)
            if lv["groups"].get(2):
                last.add(2)
    assert sizes == set(range(1, 10)) and last == {1, 2}
    assert by["tails_0_none"][1] == bytes(32)
    assert by["tails_1_none"][1] == by["tails_1_none"][0].hashes.tobytes()


def test_depths_0_to_8():
    depth = set()
    for fam in FAMILY_NAMES:
        depth |= {len(st["levels"]) for _, st in M.modelled(fam)}
    depth.add(len(M.modelled_large(M.FLAGWORDS_LARGE_NAMES[-1])[2]["levels"]))
    depth.add(len(M.modelled_large("flagwords_131071")[2]["levels"]))
    depth.add(len(M.modelled_large("flagwords_131073")[2]["levels"]))
    assert depth >= set(range(9)), depth


def test_blocks_paths():
    by = _by_name("blocks")
    entries, span3_B = set(), set()
    for c, _, st in by.values():
        lv = st["levels"][0]
        assert lv["B"] == -(-len(c.sizes) // 1024)
        if lv["B"] >= 2:
            entries |= lv["entries"]
            # groups of 3 line up with B = 3, groups of 9 with B = 9, and `edges` is `all` while B <= 5
            if c.name.endswith("_rand4") or (c.name.endswith("_none") and lv["B"] % 9):
                assert lv["straddle"] > 0, c.name
            if lv["span3"]:
                span3_B.add(lv["B"])
    assert entries == set(range(9))
    assert span3_B >= {2, 3, 4}
    assert by["blocks_1025_none"][2]["levels"][0]["active"] == 513
    assert by["blocks_2049_none"][2]["levels"][0]["active"] == 683
    assert by["blocks_20480_none"][2]["levels"][0]["B"] == 20
    # `none`: chains from different entries never merge inside a block, every entry offset occurs
    assert by["blocks_2048_none"][2]["levels"][0]["entries"] == set(range(9))
    # `edges`: only the positions around the block edges carry a flag
    for n in M.BLOCKS_N:
        c = by[f"blocks_{n}_edges"][0]
        B = -(-n // 1024)
        idx = np.flatnonzero((c.hashes[:, 24] & 3) == 0)
        assert len(idx) and all(min(i % B, B - i % B) <= 2 for i in idx), n
    # inner levels reach block lengths the leaf level does not
    inner = {lv["B"] for _, _, st in by.values() for lv in st["levels"][1:]}
    assert inner >= {1, 2, 3}


def test_flagwords_paths():
    small = _by_name("flagwords")
    assert {len(c.sizes) % 32 for c, _, _ in small.values()} >= {31, 0, 1}
    assert {-(-len(c.sizes) // 32) for c, _, _ in small.values()} >= {1, 2, 3, 128, 129}
    for n in M.FLAGWORDS_LARGE:
        st = M.modelled_large(f"flagwords_{n}")[2]
        assert st["levels"][0]["global_flags"] == (n > 131072), n
        assert not any(lv["global_flags"] for lv in st["levels"][1:])
    assert {n % 32 for n in M.FLAGWORDS_LARGE} >= {31, 0, 1}  # 131104 = 4097 full words, 131105 one bit more
    st = M.modelled_large(M.FLAGWORDS_LARGE_NAMES[-1])[2]
    assert st["levels"][0]["groups"] == {3: 131100} and st["levels"][1]["n"] == 131100
    assert st["levels"][1]["global_flags"] and not st["levels"][2]["global_flags"]
    assert len(st["levels"]) >= 8


def test_digits_paths():
    by = _by_name("digits")
    seen = set()
    for _, _, st in by.values():
        for lv in st["levels"]:
            seen |= lv["digits"]
    assert seen == set(range(1, 21))
    leaf_sizes = {int(s) for c, _, _ in by.values() for s in c.sizes}
    assert leaf_sizes >= set(M.DIGIT_EDGES)
    for kind in ("none", "all", "rand4"):
        lv = by[f"digits_cross_4e15_{kind}"][2]["levels"]
        assert lv[0]["digits"] == {16} and 17 in lv[1]["digits"] and 18 in lv[2]["digits"], kind
        lv = by[f"digits_cross_9_{kind}"][2]["levels"]
        assert lv[0]["digits"] == {1} and 2 in lv[1]["digits"] and 3 in lv[2]["digits"], kind
        lv = by[f"digits_cross_4e17_{kind}"][2]["levels"]
        assert lv[0]["digits"] == {18} and 19 in lv[1]["digits"], kind
    lv = by["digits_cross_4e18"][2]["levels"]
    assert lv[0]["digits"] == {1, 19} and lv[1]["digits"] == {1, 20}


def test_block64_paths():
    by = _by_name("block64")
    for lines, digits in M.BLOCK64_SHAPES:
        lv = by[f"block64_{lines}_{digits}"][2]["levels"][0]
        assert lv["groups"] == {lines: 5}
        assert (lines, digits) in lv["msg64"]
        assert lv["mod64"] >= {0, 63, 1}
        assert lv["tail_straddles"] >= 1
        alone = by[f"block64_{lines}_{digits}_alone"][2]["levels"]
        assert len(alone) == 1 and alone[0]["msg64"] == {(lines, digits)}


def test_random_family_is_mixed():
    by = _by_name("random")
    assert max(len(c.sizes) for c, _, _ in by.values()) > 10000
    digits = set()
    for _, _, st in by.values():
        digits |= st["levels"][0]["digits"]
    assert digits >= set(range(1, 15))


# ---- c. a wrong rule is caught by a named case ------------------------------------------------------
WRONG = [
    ("scan_from_1", "shape", "shape_idx01"),
    ("scan_from_1", "shape", "shape_all"),
    ("scan_from_1", "tails", "tails_5_all"),
    ("scan_from_1", "shape", "shape_one_50_1"),
    ("max8", "shape", "shape_none"),
    ("max8", "tails", "tails_9_none"),
    ("max8", "blocks", "blocks_2049_none"),
    ("max10", "shape", "shape_none"),
    ("max10", "tails", "tails_10_none"),
    ("max10", "blocks", "blocks_2049_edges"),
    ("flag_byte31", "shape", "shape_all"),
    ("flag_byte31", "blocks", "blocks_1025_none"),
    ("flag_byte0", "shape", "shape_all"),
    ("flag_byte0", "tails", "tails_12_none"),
    ("flag_be_word", "shape", "shape_none"),
    ("flag_be_word", "tails", "tails_12_all"),
    ("drop_digit17", "digits", "digits_d17"),
    ("drop_digit17", "digits", "digits_d20"),
    ("drop_digit17", "digits", "digits_cross_4e15_none"),
    ("drop_digit17", "digits", f"digits_{2 ** 64 - 1}_at28"),
    ("drop_digit17", "digits", "digits_ladder_up"),
] + [("early_flush64", "block64", f"block64_{lines}_{digits}{tag}") for lines, digits in M.BLOCK64_SHAPES
     for tag in ("", "_alone")]


@pytest.mark.parametrize("rule,fam,name", WRONG, ids=[f"{r}-{n}" for r, _, n in WRONG])
def test_wrong_rule_is_caught(rule, fam, name):
    assert _rule_root(fam, name, rule) != _by_name(fam)[name][1]


def _leaf_flags(c):
    return bytes(((c.hashes[:, 24] & 3) == 0).astype(np.uint8))


def test_chain_walk_equals_the_rule_and_a_wrong_entry_is_caught():
    """The parallel chain walk of level_starts, emulated on the host: with the right block entries
    it gives the boundaries of the plain rule on the steered patterns; with the entry taken from
    offset 1 of the composed map it does not, on `none`, `all` and `edges` -- while the random
    patterns, in which chains merge within a group or two, mostly do not notice."""
    by = _by_name("blocks")
    caught, missed = set(), set()
    for name, (c, _, st) in by.items():
        if len(c.sizes) > 4097 and name not in ("blocks_9216_none", "blocks_20480_all"):
            continue
        f = _leaf_flags(c)
        ref = M.group_starts(f)
        assert M.chain_walk_starts(f) == ref, name
        if st["levels"][0]["B"] >= 2:
            (caught if M.chain_walk_starts(f, entry_from=1) != ref else missed).add(name)
    assert caught >= {f"blocks_{n}_{k}" for n in (1025, 2047, 2048, 2049, 3072, 4096) for k in ("none", "all", "edges")}
    assert caught >= {"blocks_4097_none", "blocks_4097_all", "blocks_9216_none", "blocks_20480_all"}
    assert missed and all(n.endswith(("_rand4", "_edges")) for n in missed), missed


def test_every_rule_has_a_case():
    assert {r for r, _, _ in WRONG} == set(M.RULES)


def test_wrong_rules_are_narrow():
    """A wrong rule changes only what it is about: the sharpness above is not an accident of a rule
    that changes every tree."""
    assert _rule_root("digits", "digits_d16", "drop_digit17") == _by_name("digits")["digits_d16"][1]
    assert _rule_root("tails", "tails_8_none", "max8") == _by_name("tails")["tails_8_none"][1]
    assert _rule_root("tails", "tails_9_none", "max10") == _by_name("tails")["tails_9_none"][1]
    assert _rule_root("tails", "tails_2_all", "scan_from_1") == _by_name("tails")["tails_2_all"][1]
    by = _by_name("tails")
    name = next(n for n, (_, _, st) in by.items() if st["levels"] and not any(0 in lv["mod64"] for lv in st["levels"]))
    assert _rule_root("tails", name, "early_flush64") == by[name][1]
