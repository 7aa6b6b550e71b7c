"""ops.dedup_chunks without a GPU: the CPU path against the plain-Python rule (publish_model.first_rows),
the documented table contract (ops.dedup_slots, home slot) and every host refusal."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import dedup_cases as C
import publish_model as M
from zest_amd import ops

CASES = C.cases()


@pytest.mark.parametrize("name,index,fresh", CASES, ids=[c[0] for c in CASES])
def test_cpu_path_matches_the_rule(name, index, fresh):
    want = M.first_rows(index, fresh)
    got = ops.dedup_chunks(torch.from_numpy(index), torch.from_numpy(fresh))
    assert got.dtype == torch.int64 and got.shape == (len(fresh),) and got.device.type == "cpu"
    assert np.array_equal(got.numpy(), want)
    m = len(index)
    own = m + np.arange(len(fresh))
    assert ((want < m) | (want <= own)).all()


def test_the_cases_hit_what_they_claim():
    by = {c[0]: c for c in CASES}
    _, idx, new = by["wrap_last_slot"]
    slots = ops.dedup_slots(len(idx) + len(new))
    homes = [M.home_slot(k, slots) for k in np.concatenate([idx, new])]
    # the chain of the last slot runs over the table's end into the keys whose home is slot 0
    assert homes.count(slots - 1) > 20 and homes.count(0) == 10
    _, _, chain = by["chain_300_last_dword"]
    assert len({bytes(k[:28]) for k in chain}) == 1 and len({bytes(k) for k in chain}) == 300
    assert len({M.home_slot(k, ops.dedup_slots(len(chain))) for k in chain}) == 1
    _, idx, new = by["byte0_only"]
    assert len({bytes(k[1:]) for k in np.concatenate([idx, new])}) == 1
    _, idx, new = by["index_beats_fresh"]
    want = M.first_rows(idx, new)
    assert list(want[[2, 4, 7]]) == [3, 3, 3] and want[3] == len(idx) + 0 and want[8] == len(idx) + 6
    _, idx, new = by["dups_in_index"]
    assert list(M.first_rows(idx, new)[:4]) == [7, 8, 0, 1]
    _, idx, new = by["identical_4096_in_index"]
    assert set(M.first_rows(idx, new)) == {5}
    assert set(M.first_rows(*by["identical_4096"][1:])) == {0}


def test_random_rows_with_duplicates_twice():
    idx, new = C.random_with_duplicates()
    want = M.first_rows(idx, new)
    assert 0.25 < (want != len(idx) + np.arange(len(new))).mean() < 0.35
    a = ops.dedup_chunks(torch.from_numpy(idx), torch.from_numpy(new))
    b = ops.dedup_chunks(torch.from_numpy(idx), torch.from_numpy(new))
    assert np.array_equal(a.numpy(), want) and torch.equal(a, b)


def test_empty_and_sliced_inputs():
    none = torch.empty((0, 32), dtype=torch.uint8)
    assert ops.dedup_chunks(none, none).shape == (0,)
    big = torch.from_numpy(np.random.default_rng(1).integers(0, 256, (40, 32), dtype=np.uint8))
    assert ops.dedup_chunks(big, none).shape == (0,) and ops.dedup_chunks(big, none).dtype == torch.int64
    idx = big[7:19]  # a non-zero-offset slice of a larger allocation: still contiguous rows
    got = ops.dedup_chunks(idx, big[:30])
    assert np.array_equal(got.numpy(), M.first_rows(idx.numpy(), big[:30].numpy()))


def test_slots_contract():
    assert [ops.dedup_slots(r) for r in (0, 1, 31, 32, 33, 64, 65, 1000)] == [64, 64, 64, 64, 128, 128, 256, 2048]
    for r in (1, 50, 4096, 4097, 2_200_000 * 2):
        s = ops.dedup_slots(r)
        assert s >= 64 and s & (s - 1) == 0 and s >= 2 * r and (s == 64 or s < 4 * r)
    with pytest.raises(ValueError, match="negative"):
        ops.dedup_slots(-1)


def test_refusals_name_what_is_wrong():
    ok = torch.zeros((4, 32), dtype=torch.uint8)
    with pytest.raises(ValueError, match=r"new_hashes must be a uint8 tensor.*int32"):
        ops.dedup_chunks(ok, ok.to(torch.int32))
    with pytest.raises(ValueError, match=r"index_hashes must be a uint8 tensor"):
        ops.dedup_chunks(ok.numpy(), ok)
    with pytest.raises(ValueError, match=r"index_hashes must have shape \[k, 32\].*\[4, 16\]"):
        ops.dedup_chunks(torch.zeros((4, 16), dtype=torch.uint8), ok)
    with pytest.raises(ValueError, match=r"new_hashes must have shape \[k, 32\]"):
        ops.dedup_chunks(ok, torch.zeros(128, dtype=torch.uint8))
    with pytest.raises(ValueError, match=r"new_hashes must be contiguous"):
        ops.dedup_chunks(ok, torch.zeros((4, 64), dtype=torch.uint8)[:, :32])
    with pytest.raises(ValueError, match=r"index_hashes must be contiguous"):
        ops.dedup_chunks(torch.zeros((8, 32), dtype=torch.uint8)[::2], ok)
    with pytest.raises(ValueError, match=r"index_hashes is on meta, new_hashes on cpu"):
        ops.dedup_chunks(torch.zeros((4, 32), dtype=torch.uint8, device="meta"), ok)
    huge = torch.zeros((1, 32), dtype=torch.uint8).expand(2**31 - 4, 32)  # no memory behind it; refused for contiguity
    with pytest.raises(ValueError, match=r"contiguous"):
        ops.dedup_chunks(ok, huge)
    meta = torch.empty((2**31 - 4, 32), dtype=torch.uint8, device="meta")
    with pytest.raises(ValueError, match=r"2147483644 \+ 4 rows.*2\*\*31"):
        ops.dedup_chunks(meta, torch.empty((4, 32), dtype=torch.uint8, device="meta"))
