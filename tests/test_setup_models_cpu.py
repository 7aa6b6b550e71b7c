"""The models of setup_models.py against independent witnesses, without a GPU: the host xorb builder,
a splitmix64 in Python integers, the NumPy generator of zest_amd.synthetic and hashlib."""
from __future__ import annotations

import numpy as np
import torch

import setup_models as SM
from zest_amd import _core as C
from zest_amd import ops, synthetic

MASK = (1 << 64) - 1


def _rand(n: int, seed: int) -> np.ndarray:
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)


def test_pack_model_equals_the_host_builder():
    data = _rand(20_000, 1)
    for lens in ([0, 1, 3, 0, 8193, 2, 0], [1], [0], [3, 3, 255, 256, 257, 4099, 1, 0, 5000]):
        assert sum(lens) <= len(data)
        b = C.XorbBuilder("none")
        starts, pos = [], 7
        for n in lens:
            starts.append(pos)
            b.add_chunk(data[pos:pos + n].tobytes())
            pos += n + 1  # the chunks are not neighbours in `data`
        body = b.serialize(False)
        assert len(body) == sum(lens) + 8 * len(lens)
        out_off = [0] + list(b.chunk_boundaries())[:-1]
        out = np.full(len(body) + 2, 0xEE, dtype=np.uint8)
        SM.pack_model(data, starts, lens, [o + 1 for o in out_off], out)
        assert out[1:-1].tobytes() == body and out[0] == 0xEE and out[-1] == 0xEE, lens


def _splitmix_int(x: int) -> int:
    x = (x + 0x9E3779B97F4A7C15) & MASK
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & MASK
    return x ^ (x >> 31)


def _byte_int(seed: int, pos: int) -> int:
    word = _splitmix_int((seed & MASK) ^ (((pos >> 3) * 0xD1B54A32D192ED03) & MASK))
    return word.to_bytes(8, "little")[pos & 7]


def test_fill_model_equals_python_integers():
    """4096 positions: 1024 each from offset 0, 2^32 - 3 (the word index crosses 2^29), 2^40 + 5 and
    2^64 - 512 (the position wraps), with seeds of every width."""
    for seed, off in ((0, 0), (42, 2 ** 32 - 3), (2 ** 64 - 1, 2 ** 40 + 5), (-1, 2 ** 64 - 512),
                      (0x0123456789ABCDEF, 12345)):
        want = [_byte_int(seed, (off + i) & MASK) for i in range(1024)]
        assert SM.fill_model(seed, off, 1024).tolist() == want, (seed, off)
    assert SM.fill_model(7, 99, 0).shape == (0,)
    assert SM.fill_model(-1, 5, 64).tolist() == SM.fill_model(2 ** 64 - 1, 5, 64).tolist()


def test_fill_model_equals_the_host_generator():
    for seed, n in ((42, 100_000), (0, 1), (2 ** 64 - 1, 4099), (7, 8), (7, 9)):
        out = np.zeros(n, dtype=np.uint8)
        synthetic._host_fill(out, seed, 0)
        assert np.array_equal(out, SM.fill_model(seed, 0, n)), (seed, n)


def test_bf16_rounding_of_the_model():
    v = np.array([0.0, 1.0, -1.0, 1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 1 + 2.0 ** -8 + 2.0 ** -40, 2 - 2.0 ** -8,
                  -0.02, 2.0 ** -60, 3.0e38])
    want = [0, 0x3F80, 0xBF80, 0x3F80, 0x3F82, 0x3F81, 0x4000, 0xBCA4, 0x2180, 0x7F62]
    assert SM.bf16_rne(v).tolist() == want
    z, bf = SM.fill_model_f64(7, 0, 1 << 16)
    back = SM.bf16_values(bf.view(np.uint8))
    assert np.all(np.abs(back - z) <= 2.0 ** -8 * np.abs(z))  # half an ulp of 8 significant bits, at most
    assert np.all(np.abs(z) <= SM.MODE1_MAX) and 0.0199 < z.std() < 0.0201 and abs(z.mean()) < 3e-4
    # mode 1 of fill_model: the same patterns, low byte first, from any byte offset
    raw = SM.fill_model(7, 0, 1 << 10, mode=1)
    assert np.array_equal(raw.view("<u2"), bf[:1 << 9])
    assert np.array_equal(SM.fill_model(7, 101, 300, mode=1), raw[101:401])


def test_info_hash_cpu_path_equals_hashlib_on_all_rows():
    rows = _rand(1000 * 32, 3).reshape(1000, 32)
    rows[0], rows[1] = 0, 0xFF
    for i in range(256):
        rows[2 + i] = 0
        rows[2 + i, i >> 3] = 1 << (i & 7)
    want = SM.info_hash_model(rows)
    assert want.shape == (1000, 20) and len({r.tobytes() for r in want}) == 1000
    got = ops.sha1_info_hash(torch.from_numpy(rows)).numpy()
    assert np.array_equal(got, want)
    assert ops.sha1_info_hash(torch.from_numpy(rows[:0])).shape == (0, 20)
    assert SM.info_hash_model(rows[:0]).shape == (0, 20)
