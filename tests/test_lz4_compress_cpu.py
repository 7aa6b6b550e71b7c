"""The CPU model of the GPU LZ4 compressor (tests/lz4_compress_model.py): its frames pass the strict
validator and decode to their input, each input family reaches the path it is named for, and every
deliberately wrong parse (`mutate`) is caught by a named case -- so the GPU test that compares the
kernels with this model byte for byte (tests/test_gpu_lz4_compress.py) is sharp.  Nothing is
skipped or filtered: a chunk a family lists as stored must come out as a frame.
"""
from __future__ import annotations

import numpy as np
import pytest

import lz4_compress_model as M
import lz4_synth as S
from zest_amd import _core as C

FAMILY_NAMES = sorted(M.FAMILIES)


def _by_name(fam, bg4=False):
    return {c.name: (c, src, fr, st) for c, (src, fr, st) in zip(M.family(fam), M.modelled(fam, bg4))}


def _seqs(fam, name):
    c, src, fr, _ = _by_name(fam)[name]
    assert fr is not None, name
    return M.parse_frame(fr, len(src))[1]


def test_xxh32_short_matches_core():
    for d in (b"", b"\x60\x40", b"\x60\x50", b"abcde", bytes(range(15))):
        assert M.xxh32_short(d) == C.xxh32(d, 0), d
    assert M.header_checksum(0x40) == C.lz4_compress_frame(b"\0" * 16)[6]
    assert M.header_checksum(0x50) == C.lz4_compress_frame(b"\0" * 65537)[6]


def test_bg4_split_np_matches_core():
    rng = np.random.default_rng(3)
    for n in (0, 1, 2, 3, 4, 5, 6, 7, 1023, 20001, 20002, 20003, 131072):
        d = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        assert M.bg4_split_np(d) == C.bg4_split(d), n
        assert S.bg4_join_np(M.bg4_split_np(d)) == d, n


# ---- a. model frames are valid and decode correctly ---------------------------------------------
@pytest.mark.parametrize("bg4", [False, True], ids=["lz4", "bg4"])
@pytest.mark.parametrize("fam", FAMILY_NAMES)
def test_model_frames_are_strictly_valid(fam, bg4):
    scheme = 2 if bg4 else 1
    for c, (src, fr, st) in zip(M.family(fam), M.modelled(fam, bg4)):
        assert (fr is None) == (st["frame_len"] >= len(src)), c.name
        assert fr is None or len(fr) == st["frame_len"], c.name
        if not bg4:
            assert (fr is not None) == c.stored, (c.name, len(c.data), st["frame_len"])
        if fr is None:
            continue
        assert M.check_frame(fr, len(src)) == src, c.name
        assert C.decompress_chunk(scheme, fr, len(src)) == c.data, c.name


# ---- b. each family reaches its path ------------------------------------------------------------
def test_lengths_edges_present():
    by = _by_name("lengths")
    assert by["zeros_26"][2] is None and by["zeros_27"][2] is not None and len(by["zeros_27"][2]) == 26
    assert by["p3_28"][2] is None and by["p3_29"][2] is not None
    assert by["p7_32"][2] is None and by["p7_33"][2] is not None
    for n in (0, 11, 12, 13, 63, 64, 65):
        assert f"zeros_{n}" in by
    assert by["zeros_12"][3]["windows"] == 1 and by["zeros_12"][3]["sequences"] == 1  # one lane is ok, nothing to find
    assert by["zeros_13"][3]["near_hits"] == 1  # the first length at which the parse finds a match
    assert {len(c.data) for c in M.family("lengths")} >= {65535, 65536, 65537, 131071, 131072}
    assert by["p7_65536"][2][5] == 0x40 and by["p7_65537"][2][5] == 0x50
    assert by["zeros_131071"][3]["max_ml"] == 131071 - 6
    assert sum(len(c.data) > 65537 for c in M.family("lengths")) == 2


def test_distance_reaches_both_sides_of_65535():
    by = _by_name("distance")
    assert by["dist_65534"][3]["max_off"] == 65534 and by["dist_65534"][3]["far_hits"] == 1
    assert by["dist_65535"][3]["max_off"] == 65535 and by["dist_65535"][3]["far_hits"] == 1
    for d in (65536, 65537):
        st = by[f"dist_{d}"][3]
        assert st["too_far"] > 0 and st["far_hits"] == 0 and st["max_off"] == 1, d
        assert st["frame_len"] > by["dist_65535"][3]["frame_len"] + 55  # R went out as literals


def test_tag_collision_reaches_the_confirm():
    for c, (src, fr, st) in zip(M.family("tag_collision"), M.modelled("tag_collision", False)):
        assert st["tag_reject"] >= 1, c.name
    assert len({(16 + i) & 3 for i in range(len(M.TAG_SEEDS))}) == 4  # the candidate at every address & 3


def test_chains_lengths_appear():
    for nl in M.CHAIN_LITS:
        for ml in M.CHAIN_MLS:
            first = _seqs("chains", f"chain_l{nl}_m{ml}")[0]
            assert first[0] == nl and first[2] == ml, (nl, ml, first)


def test_staging_shapes_appear():
    by = _by_name("staging")
    for nl in M.STAGING_LITS:
        seqs = _seqs("staging", f"stage_lit{nl}")
        assert seqs[0][0] == nl and seqs[0][2] >= 4, (nl, seqs[:2])
    for total in M.STAGING_TOTALS:
        assert len(by[f"stage_total{total}"][2]) == total
    assert {2048 * k + d for k in (1, 2) for d in (-1, 0, 1)} <= set(M.STAGING_TOTALS)
    seqs = _seqs("staging", "stage_zeros_128k")
    assert seqs == [(1, 1, 131066), (5, 0, 0)]
    assert len(by["stage_zeros_128k"][2]) == 11 + (1 + 1 + 2 + 514) + 6 + 4  # a 514-byte chain: 513 x 255 + 232
    assert by["stage_bf16_grouped_16k"][3]["sequences"] > 1000


def test_windows_edges_reached():
    by = _by_name("windows")
    assert by["win_lane63"][3]["lane63_hits"] == 1
    for name in ("win_back_anchor", "win_back_anchor_64"):
        assert by[name][3]["back_stop_anchor"] == 1 and by[name][3]["back_stop_mc0"] == 0, name
    assert (0, 40, 80) in _seqs("windows", "win_back_anchor_64")  # 64 bytes backwards + 16 forwards
    assert by["win_back_anchor_64"][3]["too_far"] > 0 and by["win_back_anchor_64"][2][5] == 0x50
    assert by["win_back_mc0"][3]["back_stop_mc0"] == 1 and by["win_back_mc0"][3]["back_stop_anchor"] == 0
    for ml in M.WINDOW_MLS:
        assert _seqs("windows", f"win_fwd{ml}")[0] == (331, 331, ml), ml
    assert {4 + 64 * k + d for k in (1, 2, 3) for d in (-1, 0, 1)} | {4, 5} == set(M.WINDOW_MLS)
    assert by["win_repeat32"][3]["near_hits"] == 1 and by["win_repeat32"][3]["far_hits"] == 0
    assert by["win_repeat33"][3]["near_hits"] == 0 and by["win_repeat33"][3]["far_hits"] == 1
    for d in M.REPEAT_DISTANCES:
        assert _seqs("windows", f"win_repeat{d}")[0][:2] == (d, d), d
    assert (10, 136, 40) in _seqs("windows", "win_insert_passed")


def test_tail_sweep_has_accepted_and_refused_starts():
    by = _by_name("tail")
    for t in M.TAIL_T:
        c, src, fr, st = by[f"tail_t{t}"]
        pos, starts = 0, []
        for nl, off, ml in M.parse_frame(fr, len(src))[1]:
            pos += nl
            if ml:
                starts.append(pos)
            pos += ml
        assert (len(src) - t in starts) == (t >= 12), (t, starts)
        assert st["partial_windows"] >= 1
    assert set(M.TAIL_T) == set(range(5, 21))


def test_random_families_mix_paths():
    for seed in (1, 2, 3, 4):
        tot = dict.fromkeys(M.STAT_KEYS, 0)
        for c, (src, fr, st) in zip(M.family(f"random{seed}"), M.modelled(f"random{seed}", False)):
            assert len(src) <= 32 * 1024
            for k in tot:
                tot[k] += st[k]
        assert tot["far_hits"] > 20 and tot["near_hits"] > 20 and tot["back_ext"] > 5, (seed, tot)


# ---- c. the validator and the families are sharp ------------------------------------------------
# mutant -> [(family, case, how it is caught)]: "check" = check_frame raises, "decode" = check_frame
# returns other bytes, "identity" = a valid frame that differs from the model's
CATCHERS = {
    "dist65536": [("distance", "dist_65536", "check")],
    "mend4": [("lengths", "zeros_27", "check"), ("staging", "stage_zeros_128k", "check"), ("tail", "tail_t12", "check")],
    "ok11": [("tail", "tail_t11", "check")],
    "noconfirm": [("tag_collision", f"tag_{s}", "decode") for s in M.TAG_SEEDS],
    "insert_all": [("windows", "win_insert_passed", "identity")],
    "chain_drop0": [("chains", f"chain_l{nl}_m{ml}", "check") for nl, ml in
                    ((15, 18), (270, 18), (525, 18), (14, 19), (14, 274), (270, 274))],
    "noback": [("windows", "win_back_anchor", "identity"), ("windows", "win_back_anchor_64", "identity"),
               ("windows", "win_back_mc0", "identity")],
}


def _caught(src, good, mutant):
    bad = M.compress_model(src, None, mutant)
    if bad is None:
        return "identity" if good is not None else None
    try:
        if M.check_frame(bad, len(src)) != src:
            return "decode"
    except AssertionError:
        return "check"
    return "identity" if bad != good else None


@pytest.mark.parametrize("mutant", M.MUTANTS)
def test_mutant_is_caught(mutant):
    assert CATCHERS[mutant]
    for fam, name, how in CATCHERS[mutant]:
        c, src, fr, st = _by_name(fam)[name]
        assert _caught(src, fr, mutant) == how, (mutant, name)


def test_mutants_cover_the_issue_list():
    assert set(CATCHERS) == set(M.MUTANTS) and len(M.MUTANTS) == 7
    for m in ("dist65536", "mend4", "ok11", "noconfirm", "chain_drop0"):  # by the validator itself
        assert all(how in ("check", "decode") for _, _, how in CATCHERS[m]), m


# ---- d. the validator rejects bad frames --------------------------------------------------------
def _good_4k():
    rng = np.random.default_rng(7)
    lit = rng.integers(0, 256, 100, dtype=np.uint8).tobytes()
    return [(lit, 100, 4096 - 100 - 6), (b"abcdef", 0, 0)]


def test_validator_accepts_the_good_frame():
    blk, dec = S.build_block(_good_4k())
    assert len(dec) == 4096
    assert M.check_frame(S.frame([(blk, False)]), 4096) == dec


def test_validator_rejects_bad_frames():
    seqs = _good_4k()
    blk, dec = S.build_block(seqs)
    good = S.frame([(blk, False)])

    def bad(frame, n, rule):
        with pytest.raises(AssertionError, match=rule):
            M.check_frame(frame, n)

    bad(good + b"\0", 4096, "after the end mark")
    bad(good + b"\0\0\0\0", 4096, "after the end mark")
    bad(S.frame([(dec, True)]), 4096, "stored block")
    half, d1 = S.build_block([(seqs[0][0], 100, 1000), (b"abcdef", 0, 0)])
    bad(S.frame([(half, False), (half, False)]), 2 * len(d1), "more than one block")
    bad(S.frame([(blk, False)], hc_xor=1), 4096, "HC")
    bad(S.frame([(blk, False)], max_block=70000), 4096, "BD")
    bad(b"\x05" + good[1:], 4096, "magic")
    bad(S.frame([(blk, False)], content_size=4096), 4096, "FLG")
    bad(S.frame([(blk, False)], end_mark=False), 4096, "runs past the frame|end mark")
    b2, d2 = S.build_block([(seqs[0][0], 100, 4096 - 100 - 4), (b"abcd", 0, 0)])
    assert len(d2) == 4096 and C.decompress_chunk(1, S.frame([(b2, False)]), 4096) == d2  # the host takes it
    bad(S.frame([(b2, False)]), 4096, "match ends at 4092")
    b3, d3 = S.build_block([(b"abcd", 0, 0)])
    bad(S.frame([(b3, False)]), 4, "last sequence has 4 literals")
    b4, d4 = S.build_block([(seqs[0][0], 100, 4096 - 100 - 11), (b"x", 1, 4), (b"abcdef", 0, 0)])
    assert len(d4) == 4096
    bad(S.frame([(b4, False)]), 4096, "match starts at 4086")
    bad(S.frame([(blk[:-7], False)]), 4096, "token must stand")  # the block ends with the match
    bad(S.frame([(blk[:-6], False)]), 4096, "literals run past the block")
    bad(S.frame([(blk + b"\x10", False)]), 4096, "offset runs past the block")
    bad(S.frame([(S.encode_seq(b"abc", 4, 8) + S.encode_seq(b"abcdef", 0, 0, last=True), False)]), 17, "offset 4 at")
    bad(S.frame([(S.encode_seq(b"abc", 0, 8) + S.encode_seq(b"abcdef", 0, 0, last=True), False)]), 17, "offset 0 at")
    bad(good, 4097, "decoded 4096")
    lits, _ = S.build_block([(dec[:40], 0, 0)])
    bad(S.frame([(lits, False)]), 40, "no smaller than the chunk")


# ---- e. ratio sanity ----------------------------------------------------------------------------
def test_model_ratio_close_to_host_encoder():
    """The inputs and the bound of test_gpu_kernels.py::test_gpu_lz4_compress_roundtrip_host_decoder."""
    rng = np.random.default_rng(5)
    w = (rng.standard_normal(300_000).astype(np.float32) * 0.02)
    bf16 = (w.view(np.uint32) >> 16).astype(np.uint16).tobytes()
    parts = [bf16[:65536], bf16[65536:65536 + 131072], rng.integers(0, 8, 70_000, dtype=np.uint8).tobytes(),
             rng.integers(0, 256, 50_000, dtype=np.uint8).tobytes(), bytes(40_000), b"abc" * 9, b"x" * 12,
             bf16[200_000:200_000 + 8191]]
    for bg4, scheme in ((True, 2), (False, 1)):
        model_total = host_total = 0
        for i, p in enumerate(parts):
            src = M.bg4_split_np(p) if bg4 else p
            fr = M.compress_model(src)
            if fr is not None:
                assert M.check_frame(fr, len(p)) == src and C.decompress_chunk(scheme, fr, len(p)) == p, (bg4, i)
            model_total += len(p) if fr is None else len(fr)
            host_total += min(len(p), len(C.compress_chunk(p, "bg4" if bg4 else "lz4")[1]))
        assert model_total <= host_total * 1.15, (bg4, model_total, host_total)
