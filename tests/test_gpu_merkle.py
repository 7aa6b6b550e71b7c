"""The GPU Merkle kernels (csrc/gpu/merkle.hip: k_merkle_starts, k_merkle_spread, k_merkle) against
the plain-Python tree model (tests/merkle_model.py) on its steered families: every root and file hash
equal to the model's, on scratch that starts dirty, with nothing written outside the scratch the
launch was promised or outside its rows of `roots`, each job independent of its neighbours and of the
job layout.  tests/test_merkle_model_cpu.py shows that the families reach the paths they are named
for and that a wrong rule is caught by them.  The expected value is always the model, never the kernel.

Marked `gpu`: runs on a real MI355X.
"""
import functools

import numpy as np
import pytest
import torch

import merkle_model as M
from zest_amd import ops

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FILLS = (0xFF, 0xA5)  # what the scratch holds before a launch
GUARD = 4096  # bytes behind the scratch that a launch must leave alone
GUARD_BYTE = 0xC3
ROW_SENTINEL = 0x77  # the rows of `roots` before and after the launch's own
FAMILY_NAMES = sorted(M.FAMILIES)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    ops.hip()  # must load: no silent fallback


class Leaves:
    """Leaf hashes and sizes on the device; sizes go up as uint64 bits viewed as int64."""

    def __init__(self, hashes: np.ndarray, sizes: np.ndarray):
        assert hashes.dtype == np.uint8 and sizes.dtype == np.uint64 and hashes.shape == (len(sizes), 32)
        self.n = len(sizes)
        self.hashes = torch.from_numpy(np.ascontiguousarray(hashes).copy()).to(DEV)
        self.sizes = torch.from_numpy(np.ascontiguousarray(sizes).view(np.int64).copy()).to(DEV)
        if self.n == 0:  # a valid pointer even for no leaves
            self.hashes = torch.zeros((1, 32), dtype=torch.uint8, device=DEV)
            self.sizes = torch.zeros(1, dtype=torch.int64, device=DEV)


def new_scratch(max_leaves: int, n_jobs: int, fill: int):
    """(buffer with a guard behind it, the scratch bytes the launch is told about)."""
    sb = ops.hip().merkle_scratch_bytes(max_leaves, n_jobs)
    buf = torch.full((sb + GUARD,), fill, dtype=torch.uint8, device=DEV)
    buf[sb:] = GUARD_BYTE
    return buf, sb


def run_raw(leaves: Leaves, jobs, fill=0xFF, scratch=None) -> np.ndarray:
    """One zg_merkle call through the raw binding.  jobs: [(leaf_base, n_leaves, want_file_hash)].
    Returns uint8 [n_jobs, 32]; checks the guard behind the scratch and the rows around roots."""
    nj = len(jobs)
    assert nj >= 1 and all(0 <= b and b + n <= leaves.n for b, n, _ in jobs)
    rec = np.zeros(nj, dtype=ops.MERKLE_JOB_DTYPE)
    rec["leaf_base"] = [b for b, _, _ in jobs]
    rec["n_leaves"] = [n for _, n, _ in jobs]
    rec["want_file_hash"] = [w for _, _, w in jobs]
    rec["pad"] = 0xDEADBEEF
    jobs_d = torch.from_numpy(rec.view(np.uint8).copy()).to(DEV)
    buf, sb = scratch or new_scratch(max(n for _, n, _ in jobs), nj, fill)
    roots = torch.full((nj + 2, 32), ROW_SENTINEL, dtype=torch.uint8, device=DEV)
    ops.hip().merkle(leaves.hashes.data_ptr(), leaves.sizes.data_ptr(), jobs_d.data_ptr(), nj,
                     roots.data_ptr() + 32, buf.data_ptr(), sb, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert bool((buf[sb:] == GUARD_BYTE).all()), "wrote behind the scratch"
    out = roots.cpu().numpy()
    assert (out[0] == ROW_SENTINEL).all() and (out[-1] == ROW_SENTINEL).all(), "wrote outside its rows of roots"
    return out[1:-1]


def expect(root: bytes, n: int, want: int) -> bytes:
    return M.file_hash_of_root(root, n) if want else root


@functools.lru_cache(maxsize=None)
def family_batch(fam: str):
    """All cases of a family over one leaf array: each case as a raw-root job and a file-hash job
    over the same leaves, a zero-leaf job after every third case.  (Leaves, jobs, expected, names)."""
    cases, models = M.family(fam), M.modelled(fam)
    hs = np.concatenate([c.hashes for c in cases])
    sz = np.concatenate([c.sizes for c in cases])
    jobs, want, names, base = [], [], [], 0
    for i, (c, (root, _)) in enumerate(zip(cases, models)):
        n = len(c.sizes)
        for w in ((0, 1) if i % 2 == 0 else (1, 0)):
            jobs.append((base, n, w))
            want.append(expect(root, n, w))
            names.append(f"{c.name}/{'file' if w else 'root'}")
        if i % 3 == 0:
            jobs.append((base + n // 2, 0, i % 2))
            want.append(bytes(32))
            names.append(f"empty_after_{c.name}")
        base += n
    return Leaves(hs, sz), jobs, want, names


def check(got: np.ndarray, want, names):
    bad = [names[j] for j in range(len(want)) if got[j].tobytes() != want[j]]
    assert not bad, (len(bad), bad[:12])


# ---- every family, batched: jobs are independent of their neighbours --------------------------------
@pytest.mark.parametrize("fill", FILLS, ids=["ff", "a5"])
@pytest.mark.parametrize("fam", FAMILY_NAMES)
def test_family_batched(fam, fill):
    leaves, jobs, want, names = family_batch(fam)
    check(run_raw(leaves, jobs, fill), want, names)


# ---- the large trees, one job per launch: 2048 node-hash workgroups for the one tree ----------------
@pytest.mark.parametrize("name", M.FLAGWORDS_LARGE_NAMES)
def test_flagwords_large_single_job(name):
    c, root, _ = M.modelled_large(name)
    leaves = Leaves(c.hashes, c.sizes)
    n = leaves.n
    for fill in FILLS:
        for w in (0, 1):
            got = run_raw(leaves, [(0, n, w)], fill)
            assert got[0].tobytes() == expect(root, n, w), (name, hex(fill), w)


@pytest.mark.parametrize("fam", FAMILY_NAMES)
def test_single_job_launch(fam):
    """One job per launch for a few cases of each family (the node hashes of a small tree spread
    over 2048 workgroups, nearly all of them idle)."""
    cases, models = M.family(fam), M.modelled(fam)
    for i in sorted({0, len(cases) // 2, len(cases) - 1}):
        c, (root, _) = cases[i], models[i]
        leaves = Leaves(c.hashes, c.sizes)
        for w, fill in ((0, FILLS[0]), (1, FILLS[1])):
            got = run_raw(leaves, [(0, leaves.n, w)], fill)
            assert got[0].tobytes() == expect(root, leaves.n, w), (c.name, w)


# ---- job layouts -----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def small_pool():
    """4000 random leaves (flag density 1/4, mixed sizes) that the layout tests cut jobs from."""
    rng = np.random.default_rng(4242)
    n = 4000
    hs, sz = M.steer(rng, rng.random(n) < 0.25)
    sz = sz.copy()
    sz[::5] = 0
    sz[1::97] = 10 ** 12 + 7
    return hs, sz, Leaves(hs, sz)


@functools.lru_cache(maxsize=None)
def pool_root(base: int, n: int) -> bytes:
    hs, sz, _ = small_pool()
    return M.merkle_model(M.leaves_of(hs[base:base + n], sz[base:base + n]))


def small_jobs(n_jobs: int, seed: int):
    """n_jobs jobs of 0..60 leaves at random (overlapping) places of the pool, 0 and 60 included."""
    rng = np.random.default_rng(seed)
    ns = rng.integers(0, 61, size=n_jobs)
    ns[:4] = (60, 0, 1, 2)
    ns[-2:] = (0, 59)
    jobs = [(int(rng.integers(0, 4000 - 60)), int(n), int(rng.integers(0, 2))) for n in ns]
    return jobs


@pytest.mark.parametrize("n_jobs", [1, 255, 256, 300, 2049])
def test_job_counts_around_the_spread_switch(n_jobs):
    """Node-hash workgroups per tree: ceil(2048 / n_jobs) below 256 jobs (9 at 255), 8 from 256 on
    (where the quotient would be 8 at 256, 7 at 300 and 1 at 2049)."""
    _, _, leaves = small_pool()
    jobs = small_jobs(n_jobs, n_jobs) if n_jobs > 1 else [(123, 60, 1)]
    want = [expect(pool_root(b, n), n, w) for b, n, w in jobs]
    names = [str(j) for j in jobs]
    for fill in FILLS:
        check(run_raw(leaves, jobs, fill), want, names)


def test_overlapping_ranges_and_leaf_base():
    """Nested, overlapping and repeated ranges with non-zero leaf_base, both kinds of result."""
    _, _, leaves = small_pool()
    jobs = [(0, 4000, 1), (1, 3999, 0), (1, 3998, 1), (1999, 2001, 0), (3999, 1, 0), (3999, 1, 1), (4000, 0, 1),
            (1000, 1025, 0), (1000, 1025, 1), (1001, 1024, 0), (7, 2049, 1), (7, 2049, 1), (3, 9, 0), (3, 10, 0)]
    want = [expect(pool_root(b, n), n, w) for b, n, w in jobs]
    assert want[10] == want[11] and want[4] != want[5]
    for fill in FILLS:
        check(run_raw(leaves, jobs, fill), want, [str(j) for j in jobs])


def test_one_large_job_among_tiny_ones():
    """140 000 leaves next to 299 tiny jobs: the per-job scratch stride comes from the largest job,
    and the large tree gets 8 node-hash workgroups like every other."""
    c, root, _ = M.modelled_large("flagwords_140000")
    hs, sz, _ = small_pool()
    leaves = Leaves(np.concatenate([hs, c.hashes]), np.concatenate([sz, c.sizes]))
    tiny = small_jobs(299, 7)
    jobs = tiny[:150] + [(4000, 140000, 1)] + tiny[150:]
    want = [expect(pool_root(b, n), n, w) for b, n, w in tiny]
    want.insert(150, expect(root, 140000, 1))
    for fill in FILLS:
        check(run_raw(leaves, jobs, fill), want, [str(j) for j in jobs])


def test_scratch_reuse_large_then_small():
    """One scratch buffer, poisoned once: 140 000 leaves, then 37, then 3, then none and one.  The
    smaller calls find the group counts, boundaries and nodes of the larger ones where theirs go."""
    c, root, _ = M.modelled_large("flagwords_140000")
    leaves = Leaves(c.hashes, c.sizes)
    scratch = new_scratch(140000, 1, 0xFF)
    got = run_raw(leaves, [(0, 140000, 1)], scratch=scratch)
    assert got[0].tobytes() == expect(root, 140000, 1)
    for base, n, w in ((1000, 37, 1), (500, 3, 0), (0, 0, 1), (77, 1, 0), (99, 2, 1), (1000, 37, 0)):
        sub = M.merkle_model(M.leaves_of(c.hashes[base:base + n], c.sizes[base:base + n]))
        got = run_raw(leaves, [(base, n, w)], scratch=scratch)
        assert got[0].tobytes() == expect(sub, n, w), (base, n, w)


# ---- through ops.merkle_roots ----------------------------------------------------------------------
@pytest.mark.parametrize("fam", FAMILY_NAMES)
def test_ops_merkle_roots_sample(fam):
    cases, models = M.family(fam), M.modelled(fam)
    picks = sorted({0, len(cases) // 3, len(cases) - 1})
    hs = np.concatenate([cases[i].hashes for i in picks])
    sz = np.concatenate([cases[i].sizes for i in picks])
    jobs, base = [], 0
    for i in picks:
        jobs.append((base, len(cases[i].sizes)))
        base += len(cases[i].sizes)
    leaves = Leaves(hs, sz)
    for fh in (False, True):
        got = ops.merkle_roots(leaves.hashes, leaves.sizes, jobs, file_hash=fh).cpu().numpy()
        assert got.shape == (len(picks), 32)
        for j, i in enumerate(picks):
            assert got[j].tobytes() == expect(models[i][0], len(cases[i].sizes), fh), (cases[i].name, fh)


def test_ops_merkle_roots_rejects_bad_jobs_and_takes_none():
    _, _, leaves = small_pool()
    for bad in ([(0, 4001)], [(4000, 1)], [(-1, 2)], [(0, -1)], [(0, 5), (3999, 2)]):
        with pytest.raises(ValueError):
            ops.merkle_roots(leaves.hashes, leaves.sizes, bad)
    out = ops.merkle_roots(leaves.hashes, leaves.sizes, [])
    assert out.shape == (0, 32) and out.dtype == torch.uint8 and out.device.type == "cuda"
