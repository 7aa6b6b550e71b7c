"""Inputs for the chunk-dedup tests (CPU path and kernel K13 alike): `cases()` returns
[(name, index uint8 [m, 32], fresh uint8 [n, 32])], each the smallest input that can still go wrong."""
from __future__ import annotations

import numpy as np

from zest_amd import ops


def _rand(rng, k: int) -> np.ndarray:
    return rng.integers(0, 256, (k, 32), dtype=np.uint8)


def _with_home(rng, k: int, slot: int, slots: int) -> np.ndarray:
    """k distinct random keys whose home slot in a table of `slots` is `slot`."""
    keys = _rand(rng, k)
    lo = keys[:, :8].copy().view("<u8").reshape(-1)
    lo = (lo & ~np.uint64(slots - 1)) | np.uint64(slot)
    keys[:, :8] = lo.view(np.uint8).reshape(k, 8)
    return keys


def cases(seed: int = 5):
    rng = np.random.default_rng(seed)
    none = np.zeros((0, 32), np.uint8)
    out = [("m0_n1", none, _rand(rng, 1)), ("m3_n1", _rand(rng, 3), _rand(rng, 1))]
    for k in (63, 64, 65, 255, 256, 257):  # wave and block tails, as fresh rows and as index rows
        a = _rand(rng, k)
        out.append((f"m0_n{k}", none, a))
        b = _rand(rng, k)
        b[::3] = a[(np.arange(k)[::3] * 7) % k]  # a third of the fresh rows are index rows
        out.append((f"m{k}_n{k}", a, b))
    one = _rand(rng, 1)
    out.append(("identical_4096", none, np.repeat(one, 4096, axis=0)))
    out.append(("identical_4096_in_index", np.concatenate([_rand(rng, 5), one, _rand(rng, 2), one]),
                np.repeat(one, 4096, axis=0)))
    chain = np.repeat(_rand(rng, 1), 300, axis=0)  # one home slot, a 300-long probe chain; only the last dword differs
    chain[:, 28:] = np.arange(300, dtype="<u4").view(np.uint8).reshape(300, 4)
    out.append(("chain_300_last_dword", none, np.concatenate([chain, chain[::-1]])))
    out.append(("chain_300_index", chain[:150], chain[::-1].copy()))
    b0 = np.repeat(_rand(rng, 1), 256, axis=0)
    b0[:, 0] = np.arange(256, dtype=np.uint8)
    out.append(("byte0_only", b0[:100], np.concatenate([b0[50:], b0[:60]])))
    # keys whose home is the last slot: the chain wraps to slot 0
    m, n = 10, 40
    slots = ops.dedup_slots(m + n)
    wrap = _with_home(rng, 30, slots - 1, slots)
    near = _with_home(rng, 10, slots - 2, slots)
    zero = _with_home(rng, 10, 0, slots)
    idx = np.concatenate([wrap[:5], near[:5]])
    new = np.concatenate([wrap[5:], zero, wrap[:3], near[5:7]])
    assert len(idx) == m and len(new) == n
    out.append(("wrap_last_slot", idx, new))
    # duplicates inside the index: the first index row wins
    a = _rand(rng, 20)
    idx = np.concatenate([a, a[5:10], a[:3]])
    out.append(("dups_in_index", idx, np.concatenate([a[7:9], a[:2], _rand(rng, 3), a[19:]])))
    # a fresh row equal to an index row and to an earlier fresh row: the index row wins
    a = _rand(rng, 8)
    f = _rand(rng, 4)
    out.append(("index_beats_fresh", a, np.concatenate([f[:2], a[3:4], f[:1], a[3:4], f[2:], a[3:4], f[3:]])))
    return out


def random_with_duplicates(seed: int = 9, rows: int = 50_000, dup: float = 0.3, m: int = 20_000):
    """(index [m, 32], fresh [rows - m, 32]): `rows` random rows of which `dup` repeat an earlier one."""
    rng = np.random.default_rng(seed)
    keys = _rand(rng, rows)
    again = np.flatnonzero(rng.random(rows) < dup)
    again = again[again > 0]
    orig = np.setdiff1d(np.arange(rows), again)  # row 0 is one; every copy takes an earlier original
    keys[again] = keys[orig[(rng.random(len(again)) * np.searchsorted(orig, again)).astype(np.int64)]]
    return keys[:m].copy(), keys[m:].copy()
