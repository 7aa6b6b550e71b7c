"""CPU: the serve-pack reference model against the host xorb decoder, the NumPy path of
ops.serve_pack against the model, and the resident-run planner (seed.plan_resident_runs)."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import serve_pack_model as M
from zest_amd import _core, ops
from zest_amd.seed import plan_resident_runs


@pytest.fixture(scope="module", params=sorted(M.FAMILIES))
def family(request):
    arena, offs, lens = M.FAMILIES[request.param]()
    t = torch.from_numpy(arena)
    chunks = M.chunks_of(arena, offs, lens)
    return request.param, t, offs, lens, chunks, M.serialize(chunks)


def test_model_matches_host_decoder(family):
    _, _, _, lens, chunks, ser = family
    idx = _core.index_chunks(np.frombuffer(ser, dtype=np.uint8))
    ends = M.ser_ends(chunks)
    assert [e[0] for e in idx] == [0] + ends[:-1]
    assert [e[1] for e in idx] == [int(n) for n in lens]
    data, _ = _core.extract_chunk_range(np.frombuffer(ser, dtype=np.uint8), 0, len(idx), True)
    assert bytes(data) == b"".join(chunks)


def test_cpu_path_equals_model(family):
    name, t, offs, lens, chunks, ser = family
    addrs = t.data_ptr() + np.asarray(offs, dtype=np.uint64)
    run = ops.ServeRun(addrs, lens, buffers=[t])
    assert run.total == len(ser)
    assert ops.serve_pack(run).numpy().tobytes() == ser
    ends = M.ser_ends(chunks)
    if name == "tiny":
        wins = [(a, b) for a in range(0, 257) for b in range(a, 257, 7)]
    else:
        wins = M.boundary_windows(ends[:8] + ends[-2:], len(ser))[::3]
    for lo, hi in wins:
        assert ops.serve_pack(run, lo=lo, hi=hi).numpy().tobytes() == ser[lo:hi], (lo, hi)
    # the one-call form, and an `out` buffer
    out = torch.full((64,), 0xA5, dtype=torch.uint8)
    got = ops.serve_pack(addrs, lens, 3, 40, out=out, buffers=[t])
    assert got.numpy().tobytes() == ser[3:40] and out[37:].eq(0xA5).all()


def test_cpu_path_validates():
    t = torch.zeros(100, dtype=torch.uint8)
    p = t.data_ptr()
    with pytest.raises(ValueError):
        ops.serve_pack([p + 90], [11], buffers=[t])       # one byte past the buffer
    with pytest.raises(ValueError):
        ops.serve_pack([p], [1 << 24], buffers=[t])        # does not fit a u24 header
    with pytest.raises(ValueError):
        ops.serve_pack([p], [10], 0, 19, buffers=[t])      # window past the stream (18 bytes)
    assert len(ops.serve_pack([p + 90], [10], buffers=[t])) == 18


# ---------------------------------------------------------------------------------------------
# plan_resident_runs
# ---------------------------------------------------------------------------------------------
def _lens(*v):
    return np.asarray(v, dtype="<u4").tobytes()


def _flat(plan):
    return {hx: [(f, a.tolist(), ln.tolist()) for f, a, ln in runs] for hx, runs in plan.items()}


def test_plan_one_term_per_xorb():
    plan = plan_resident_runs([(1000, _lens(10, 20, 30), [("aa", 0, 2), ("bb", 0, 1)])])
    assert _flat(plan) == {"aa": [(0, [1000, 1010], [10, 20])], "bb": [(0, [1030], [30])]}


def test_plan_xorb_split_over_two_terms_of_one_file():
    plan = plan_resident_runs([(1000, _lens(10, 20, 5, 30), [("aa", 0, 2), ("bb", 0, 1), ("aa", 2, 3)])])
    assert _flat(plan) == {"aa": [(0, [1000, 1010, 1035], [10, 20, 30])], "bb": [(0, [1030], [5])]}


def test_plan_xorb_split_over_two_files_merges():
    plan = plan_resident_runs([(1000, _lens(10, 20), [("aa", 0, 2)]),
                               (5000, np.asarray([7, 8], dtype=np.uint32), [("aa", 2, 4)])])
    assert _flat(plan) == {"aa": [(0, [1000, 1010, 5000, 5007], [10, 20, 7, 8])]}


def test_plan_gap_gives_two_runs():
    plan = plan_resident_runs([(1000, _lens(10, 20, 30), [("aa", 0, 2), ("aa", 3, 4)])])
    assert _flat(plan) == {"aa": [(0, [1000, 1010], [10, 20]), (3, [1030], [30])]}


def test_plan_duplicate_reference_first_wins():
    plan = plan_resident_runs([(1000, _lens(10, 20), [("aa", 0, 2)]),
                               (5000, _lens(20, 9), [("aa", 1, 3)])])
    assert _flat(plan) == {"aa": [(0, [1000, 1010, 5020], [10, 20, 9])]}
    # a pure duplicate adds no second run
    plan = plan_resident_runs([(1000, _lens(10, 20), [("aa", 0, 2)]), (5000, _lens(10, 20), [("aa", 0, 2)])])
    assert _flat(plan) == {"aa": [(0, [1000, 1010], [10, 20])]}


def test_plan_term_starting_at_nonzero_chunk():
    plan = plan_resident_runs([(1000, _lens(10, 20), [("aa", 5, 7)])])
    assert _flat(plan) == {"aa": [(5, [1000, 1010], [10, 20])]}


@pytest.mark.parametrize("lens, terms", [((10, 20), [("aa", 0, 3)]), ((10, 20, 30), [("aa", 0, 2)]),
                                         ((10,), [("aa", 2, 2)])])
def test_plan_mismatched_chunk_count_raises(lens, terms):
    with pytest.raises(ValueError):
        plan_resident_runs([(1000, _lens(*lens), terms)])
