"""GPU: the peer gather (K8, k_peer_gather in csrc/gpu/xgmi.hip) against a byte-by-byte model
(peer_gather_child.py).  The geometry is the code's: a block moves 256 x 8 x 16 B = 32 KiB per pass of
its loop, a launch has 512 blocks in all (512 // nseg per segment) unless ZG_PEER_GATHER_BLOCKS says
otherwise, and at most 16 segments.  Every source differs from its destination by a multiple of 16 of
its own, the destination is canary-filled, and every byte of it is compared after every launch.  Source
and destination are local buffers: the xGMI path itself needs a second device."""
from __future__ import annotations

import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import peer_gather_child as G
from scatter_model import canary, place_source
from zest_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    ops.hip()  # must load: no silent fallback


def grid_sizes(a: int) -> list:
    return sorted({n for n in (0, 1, 2, 15 - a, 16 - a, 17 - a, 16, 17, 31, 32, 33, 48 + a) if n >= 0})


def grid_launches() -> list:
    """Every (dst & 15, n) of the grid as launches of 16 segments, each segment one or two canary
    bytes behind its predecessor (the last of a launch and the first of the next one too).  The order
    is greedy: the gap whose alignment has more sizes left, then the size after which more is left
    within reach.  Where an alignment has nothing left, one of its sizes is taken again as a bridge.
    Returns [[(destination offset, n)] * 16]."""
    left = {a: grid_sizes(a) for a in range(16)}
    pos, launches, chain = 16, [], []
    while any(left.values()):
        g = max((1, 2), key=lambda g: len(left[(pos + g) & 15]))
        pos += g
        here = left[pos & 15]
        after = lambda n: max(len(left[(pos + n + g) & 15]) - ((n + g) % 16 == 0) for g in (1, 2))  # noqa: E731
        n = max(here or grid_sizes(pos & 15), key=after)
        if here:
            here.remove(n)
        chain.append((pos, n))
        pos += n
        if len(chain) == 16:
            launches.append(chain)
            chain = []
    return launches + ([chain] if chain else [])


def test_alignment_and_length_grid():
    """src & 15 == dst & 15 == a for every a, with the lengths around the head (15 - a, 16 - a, 17 - a:
    the head alone, with one byte less, with one byte of tail), around one and two vectors, 0, 1, 2
    (head > n for most a) and 48 + a."""
    launches = grid_launches()
    flat = [s for chain in launches for s in chain]
    assert {(do & 15, n) for do, n in flat} == {(a, n) for a in range(16) for n in grid_sizes(a)}
    assert sum(n < (16 - (do & 15)) & 15 for do, n in flat) > 30  # the head is cut short
    assert all(1 <= b[0] - (a[0] + a[1]) <= 2 for a, b in zip(flat, flat[1:]))
    assert all(len(c) == 16 for c in launches[:-1]) and len(launches) <= 20
    segs = [(do + 16 * (1 + (5 * i) % 7), do, n) for i, (do, n) in enumerate(flat)]
    end = flat[-1][0] + flat[-1][1]
    idx = iter(range(len(flat)))
    out = G.check_gather(ops.hip(), DEV, segs, end + 16 * 8, end + 33,
                         launches=[[next(idx) for _ in chain] for chain in launches])
    assert out["ok"], out


def test_unroll_edges():
    """Bodies of 255, 256, 257 vectors (the first group of the 8-deep unroll partly filled, full, and a
    second one begun) and 2047, 2048, 2049 (the last group, a whole pass, the second block's first
    vector), each with an 11-byte head and a 7-byte tail; together and one by one."""
    sizes = [11 + 16 * body + 7 for body in (255, 256, 257, 2047, 2048, 2049)]
    segs, src_len, dst_len = G.lay_out(sizes, align=(5,))
    assert all(do & 15 == 5 for _, do, _ in segs)
    out = G.check_gather(ops.hip(), DEV, segs, src_len, dst_len, seed=2)
    assert out["ok"], out
    out = G.check_gather(ops.hip(), DEV, segs, src_len, dst_len, seed=3, launches=[[i] for i in range(len(segs))])
    assert out["ok"], out


def test_the_loop_runs_three_passes():
    """16 segments leave 32 blocks for each: 1 MiB per pass.  2 MiB + 5 * 4096 + 55 bytes is two whole
    passes and a third in which only the first blocks still have work; its launch mates are done after
    their first block, or have no vector at all."""
    big = (2 << 20) + 5 * 4096 + 55
    assert 2 * 32 * G.PASS < big < 2 * 32 * G.PASS + G.PASS
    sizes = [(0, 1, 100, 40_000)[i % 4] for i in range(16)]
    sizes[6] = big
    segs, src_len, dst_len = G.lay_out(sizes, align=(3, 0, 15, 8, 9))
    assert dst_len < 8 << 20
    out = G.check_gather(ops.hip(), DEV, segs, src_len, dst_len, seed=4)
    assert out["ok"], out


@pytest.mark.parametrize("blocks,per_segment,passes", [(1, 1, 10), (37, 7, 2)])
def test_the_loop_with_a_set_number_of_blocks(blocks, per_segment, passes):
    """ZG_PEER_GATHER_BLOCKS is read once per process: a child of its own, which compares every byte
    and prints its verdict."""
    nseg, longest = len(G.CHILD_SIZES), max(G.CHILD_SIZES)
    assert max(1, blocks // nseg) == per_segment < -(-longest // G.PASS)  # the cap binds
    assert -(-longest // (per_segment * G.PASS)) == passes
    env = dict(os.environ, ZG_PEER_GATHER_BLOCKS=str(blocks))
    r = subprocess.run([sys.executable, str(Path(G.__file__).resolve())], env=env, capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["ok"] and out["differ"] == 0 and out["blocks"] == str(blocks), out
    assert out["bytes"] == sum(G.CHILD_SIZES)


def _canary_pair(n: int = 256):
    hold, s = place_source(np.random.default_rng(6).integers(0, 256, n, dtype=np.uint8), DEV)
    d = torch.from_numpy(canary(n, 5)).to(DEV)
    return hold, s, d


def test_all_segments_empty():
    hold, s, d = _canary_pair()
    for nseg in (0, 1, 16):
        ops.hip().peer_gather([s.data_ptr() + 16 * i for i in range(nseg)], [d.data_ptr() + 16 * i for i in range(nseg)],
                              [0] * nseg, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert np.array_equal(d.cpu().numpy(), canary(256, 5))


def test_refusals_leave_the_destination_alone():
    hold, s, d = _canary_pair()
    H, st = ops.hip(), torch.cuda.current_stream().cuda_stream
    with pytest.raises(ValueError, match="at most 16"):
        H.peer_gather([s.data_ptr() + 4 * i for i in range(17)], [d.data_ptr() + 4 * i for i in range(17)], [4] * 17, st)
    with pytest.raises(ValueError, match="congruent"):
        H.peer_gather([s.data_ptr(), s.data_ptr() + 33], [d.data_ptr(), d.data_ptr() + 32], [8, 8], st)
    with pytest.raises(ValueError, match="equal-length"):
        H.peer_gather([s.data_ptr()], [d.data_ptr()], [8, 8], st)
    torch.cuda.synchronize()
    assert np.array_equal(d.cpu().numpy(), canary(256, 5))
    H.peer_gather([s.data_ptr() + 33], [d.data_ptr() + 17], [8], st)  # legal: 33 and 17 are both 1 mod 16
    assert d.cpu().numpy()[17:25].tolist() == s.cpu().numpy()[33:41].tolist()
