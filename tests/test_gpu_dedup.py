"""GPU: the chunk-dedup kernel K13 (csrc/gpu/dedup.hip, ops.dedup_chunks) against the plain-Python rule
(publish_model.first_rows).  Every input is valid (bad ones are refused on the host, tests/test_dedup_cpu.py);
the raw launches write into sentinel-filled outputs with guard rows that are checked element by element."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import dedup_cases as C
import publish_model as M
from zest_amd import ops

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CASES = C.cases()
SENTINEL = -0x5A5A5A5A5A5A5A5B
GUARD = 64


def _raw(index: np.ndarray, fresh: np.ndarray) -> np.ndarray:
    """One zg_dedup_chunks call with guard rows around `first` and guard bytes after the table."""
    H = ops.hip()
    m, n = len(index), len(fresh)
    ix = torch.from_numpy(index).to(DEV)
    fr = torch.from_numpy(fresh).to(DEV)
    tb = H.dedup_table_bytes(m + n)
    assert tb == 4 * ops.dedup_slots(m + n) == 4 * H.dedup_slots(m + n)
    table = torch.full((tb + 256,), 0x5A, dtype=torch.uint8, device=DEV)
    first = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.int64, device=DEV)
    H.dedup_chunks(ix.data_ptr() if m else 0, m, fr.data_ptr(), n, table.data_ptr(), tb,
                   first.data_ptr() + 8 * GUARD, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    out = first.cpu().numpy()
    assert (out[:GUARD] == SENTINEL).all() and (out[GUARD + n:] == SENTINEL).all(), "wrote outside first[0, n)"
    assert (table[tb:].cpu().numpy() == 0x5A).all(), "wrote past the table"
    slots = table[:tb].cpu().numpy().view("<u4")
    used = slots[slots != 0xFFFFFFFF]
    keys = np.concatenate([index, fresh])
    assert len(used) == len({bytes(k) for k in keys}), "one slot per distinct key"
    assert (used < m + n).all()
    return out[GUARD:GUARD + n]


@pytest.mark.parametrize("name,index,fresh", CASES, ids=[c[0] for c in CASES])
def test_kernel_matches_the_rule(name, index, fresh):
    want = M.first_rows(index, fresh)
    got = _raw(index, fresh)
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:8]
    via = ops.dedup_chunks(torch.from_numpy(index).to(DEV), torch.from_numpy(fresh).to(DEV))
    assert via.dtype == torch.int64 and via.device == torch.device(DEV)
    assert np.array_equal(via.cpu().numpy(), want)


def test_random_rows_twice_bit_identical():
    idx, new = C.random_with_duplicates()
    want = M.first_rows(idx, new)
    ix, fr = torch.from_numpy(idx).to(DEV), torch.from_numpy(new).to(DEV)
    a = ops.dedup_chunks(ix, fr)
    b = ops.dedup_chunks(ix, fr)
    assert torch.equal(a, b)
    assert np.array_equal(a.cpu().numpy(), want)
    assert np.array_equal(_raw(idx, new), want)


def test_empty_sliced_and_side_stream():
    none = torch.empty((0, 32), dtype=torch.uint8, device=DEV)
    big = torch.from_numpy(np.random.default_rng(1).integers(0, 256, (4000, 32), dtype=np.uint8)).to(DEV)
    out = ops.dedup_chunks(big, none)
    assert out.shape == (0,) and out.dtype == torch.int64 and out.device == torch.device(DEV)
    idx = big[700:1900]  # a non-zero-offset slice of a larger allocation
    assert idx.storage_offset() > 0
    want = M.first_rows(idx.cpu().numpy(), big[:3000].cpu().numpy())
    assert np.array_equal(ops.dedup_chunks(idx, big[:3000]).cpu().numpy(), want)
    flat = torch.zeros(32 * 100 + 8, dtype=torch.uint8, device=DEV)
    flat[8:] = big[:100].reshape(-1)
    odd = flat[8:].view(100, 32)  # rows that start 8 bytes off a 16-byte boundary: the wrapper copies them
    assert odd.data_ptr() % 16 == 8
    assert np.array_equal(ops.dedup_chunks(odd, big[:200]).cpu().numpy(),
                          M.first_rows(big[:100].cpu().numpy(), big[:200].cpu().numpy()))
    s = torch.cuda.Stream(DEV)
    s.wait_stream(torch.cuda.current_stream())
    got = ops.dedup_chunks(idx, big[:3000], stream=s)
    s.synchronize()
    assert np.array_equal(got.cpu().numpy(), want)


def test_cpu_index_with_gpu_hashes_is_refused():
    a = torch.zeros((4, 32), dtype=torch.uint8)
    with pytest.raises(ValueError, match=r"index_hashes is on cpu, new_hashes on cuda:0"):
        ops.dedup_chunks(a, a.to(DEV))
