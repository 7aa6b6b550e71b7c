"""Both device header walks (csrc/gpu/ingest.hip: the serial k_index_terms and the parallel
k_hdr_scan + k_hdr_link) against the plain-Python model of walk_term (tests/index_model.py) on
synthesised runs: records byte for byte, the error word, nothing written outside a term's records,
and -- only where a case says so -- which path the parallel walk took.
tests/test_index_model_cpu.py pins the model and shows that the cases are what they are named for.

Marked `gpu`: runs on a real MI355X.
"""
import numpy as np
import pytest
import torch

import index_model as M
from zest_amd import ops

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENTINEL = 0xEE
FELL_BACK = 1 << 31  # k_hdr_link's mark in the scan's per-term candidate counts


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    ops.hip()  # must load: no silent fallback


_EXPECT = {}


def _expect(case):
    """The model's records (from a sentinel-filled array) and error words, once per case."""
    if case.name not in _EXPECT:
        start = np.full(case.n_records * M.CHUNK_DTYPE.itemsize, SENTINEL, dtype=np.uint8).view(M.CHUNK_DTYPE)
        _EXPECT[case.name] = M.index(case.src, case.terms, start)
    return _EXPECT[case.name]


def _launch(case, scan: bool, shift: int = 0, scratch_short: int = 0):
    """(records, error word, per-term fallback flags or None when the scratch was not touched) of
    one walk.  The source starts `shift` bytes behind a 16-byte boundary; the records and the
    scratch start out as SENTINEL bytes."""
    H = ops.hip()
    st = torch.cuda.current_stream().cuda_stream
    nt = len(case.terms)
    base = ops.padded_empty(len(case.src) + shift, DEV)
    assert base.data_ptr() % 16 == 0
    base.fill_(0x55)
    src = base[shift:]
    src.copy_(torch.frombuffer(bytearray(case.src), dtype=torch.uint8))
    tdev = torch.from_numpy(case.terms.view(np.uint8).copy()).to(DEV)
    chunks = torch.full((case.n_records * ops.CHUNK_DTYPE.itemsize,), SENTINEL, dtype=torch.uint8, device=DEV)
    err = torch.zeros(1, dtype=torch.int64, device=DEV)
    flags = None
    if scan:
        sb = H.index_scratch_bytes(nt)
        scr = torch.full((sb,), SENTINEL, dtype=torch.uint8, device=DEV)
        H.index_terms_scan(src.data_ptr(), src.numel(), tdev.data_ptr(), nt, chunks.data_ptr(), err.data_ptr(),
                           scr.data_ptr(), sb - scratch_short, st)
        torch.cuda.synchronize()
        cnt = scr[:4 * nt].cpu().numpy().view(np.uint32)
        if not (scr == SENTINEL).all():
            flags = [bool(int(c) & FELL_BACK) for c in cnt]
    else:
        H.index_terms(src.data_ptr(), tdev.data_ptr(), nt, chunks.data_ptr(), err.data_ptr(), st)
        torch.cuda.synchronize()
    return chunks.cpu().numpy().view(M.CHUNK_DTYPE), int(err.item()) & (2 ** 64 - 1), flags


def _check(case, routed_serial: bool = False, **kw):
    want, words = _expect(case)
    for scan in (False, True):
        walk = "parallel" if scan else "serial"
        got, word, flags = _launch(case, scan, **kw)
        bad = np.flatnonzero(got != want)
        assert not len(bad), (f"{case.name}, {walk} walk: {len(bad)} records differ, first at {bad[0]}: "
                              f"got {got[bad[0]]}, want {want[bad[0]]}; error word {word:#x}, "
                              f"the model's {sorted(map(hex, words))}")
        if len(words) <= 1:
            assert word == (min(words) if words else 0), (case.name, walk, hex(word), sorted(map(hex, words)))
        else:  # the device keeps whichever failing term reports first
            assert word in words, (case.name, walk, hex(word))
        if not scan:
            continue
        if routed_serial:
            assert flags is None, "the launch was to take the serial kernel and leave the scratch alone"
            continue
        assert flags is not None
        for t, fast in enumerate(case.fast):
            if fast is not None:
                assert flags[t] == (not fast), (f"{case.name}: term {t} " +
                                                ("fell back to the serial walk" if fast else "kept the fast path"))


@pytest.mark.parametrize("name", M.case_names("clean"))
def test_clean_runs_keep_the_fast_path(name):
    """Raw chunks of 1..4096 bytes mixed with framed ones, 1..64 terms at every residue mod 64,
    chunk_base above 0, header look-alikes in the gaps and in front, whole terms inside one scan
    thread's slice, ulen checked and not: the model's records, and no term falls back."""
    case = M.by_name("clean", name)
    assert all(case.fast)
    _check(case)


@pytest.mark.parametrize("name", M.case_names("seams"))
def test_headers_on_scan_seams(name):
    """A real header at every position across a scan thread's and a scan block's boundary, and the
    last header 9..12 bytes before the run's end: found, and no term falls back."""
    case = M.by_name("seams", name)
    assert all(case.fast)
    _check(case)


@pytest.mark.parametrize("n", M.SORT_SIZES)
def test_sort_slice_and_cap_sizes(n):
    """n candidates in one term: the bitonic sort at P = 1024..8192 and prefix slices of 1..8
    candidates on the fast path; 8193 is over the candidate cap and takes the serial walk."""
    _check(M.sort_case(n))


@pytest.mark.parametrize("shift", [1, 4, 8])
def test_unaligned_source_takes_the_serial_kernel(shift):
    _check(M.by_name("clean", "mixed_3_terms"), routed_serial=True, shift=shift)


def test_short_scratch_takes_the_serial_kernel():
    _check(M.by_name("clean", "mixed_7_terms"), routed_serial=True, scratch_short=1)


def test_descending_terms_fall_back():
    case = M.descending_case()
    assert case.fast == (False,) * 3
    _check(case)


@pytest.mark.parametrize("name", M.case_names("lookalikes"))
def test_lookalikes_on_a_well_formed_chain(name):
    """Planted raw-header look-alikes: lone ones (the fast path is kept), a chain of two, one that
    points at a real header, two that point at the run's end, and headers over a run's last bytes
    that reach into the gap (no candidates)."""
    _check(M.by_name("lookalikes", name))


@pytest.mark.parametrize("where", [0, 2, 4])
@pytest.mark.parametrize("kind", M.MALFORMED)
def test_one_malformed_term(kind, where):
    """One steered term among four healthy ones, first, in the middle and last: every error code
    with its word and zeroed tail, and the valid runs the scan cannot list."""
    _check(M.malformed_case(kind, where))


@pytest.mark.parametrize("name", M.case_names("branches"))
def test_short_chain_with_side_branch(name):
    """The true chain is shorter than planned and a look-alike outside the chosen set points at a
    side branch that makes up the count: COUNT and a zeroed tail, as walk_term says, not records
    with overlapping payloads and error 0."""
    _check(M.by_name("branches", name))


@pytest.mark.parametrize("launch", range(M.SWEEP_LAUNCHES))
def test_steered_sweep(launch):
    """50 small terms a launch with planted look-alikes, chains and side branches and n_chunks at
    true - 1 .. true + 2.  Several terms fail, so the word is one of the model's; terms whose extra
    candidates are all dead ends must keep the fast path."""
    _check(M.sweep_case(launch))
