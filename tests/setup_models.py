"""Reference models of the set-up kernels: raw xorb packing (ops.pack_chunks, K7), the synthetic
content generator (ops.fill_synthetic) and the info-hash batch (ops.sha1_info_hash, K6).  Plain NumPy,
hashlib and Python integers: no arithmetic shared with the kernels, with the ops CPU paths or with
zest_amd.synthetic.

  pack_model(data, data_off, lens, out_off, out)   what a pack launch writes into `out`
  fill_model(seed, stream_off, n, mode=0)          bytes [stream_off, stream_off + n) of the stream
  fill_model_f64(seed, first_elem, count)          mode 1 elements in float64, and their bf16 patterns
  bf16_rne(values)                                 float64 -> bf16 pattern, round to nearest even
  info_hash_model(rows)                            SHA-1 of "zest-xet-v1:" + row
"""
from __future__ import annotations

import hashlib

import numpy as np

U = np.uint64
GOLDEN = 0x9E3779B97F4A7C15  # splitmix64: the increment and the two multipliers of its finaliser
MIX1, MIX2 = 0xBF58476D1CE4E5B9, 0x94D049BB133111EB
WORD_KEY = 0xD1B54A32D192ED03  # mode 0: multiplies the index of the 8-byte word
ELEM_KEY = 0xA24BAED4963EE407  # mode 1: multiplies the index of the bf16 element
SIGMA = 0.02


def pack_model(data, data_off, lens, out_off, out: np.ndarray) -> None:
    """Per chunk i at out[out_off[i]:]: version 0, the length as u24 LE, scheme 0, the length as
    u24 LE again, then the lens[i] payload bytes from data[data_off[i]:].  Writes into `out`."""
    for d, n, o in zip(data_off, lens, out_off):
        d, n, o = int(d), int(n), int(o)
        assert 0 <= n < 1 << 24
        u24 = [n % 256, n // 256 % 256, n // 65536]
        for j, b in enumerate([0] + u24 + [0] + u24):
            out[o + j] = b
        for j in range(n):
            out[o + 8 + j] = data[d + j]


def _splitmix(x: np.ndarray) -> np.ndarray:
    """splitmix64 of each uint64 (wrap-around arithmetic)."""
    with np.errstate(over="ignore"):
        z = x + U(GOLDEN)
        z = (z ^ (z >> U(30))) * U(MIX1)
        z = (z ^ (z >> U(27))) * U(MIX2)
        return z ^ (z >> U(31))


def _positions(first: int, n: int) -> np.ndarray:
    with np.errstate(over="ignore"):
        return U(first % (1 << 64)) + np.arange(n, dtype=U)


def fill_model(seed: int, stream_off: int, n: int, mode: int = 0) -> np.ndarray:
    """uint8 [n]: stream bytes stream_off .. stream_off + n - 1 for any 64-bit seed and offset.  Mode 0:
    byte pos is byte pos & 7 (little endian) of splitmix64(seed ^ (pos >> 3) * WORD_KEY).  Mode 1: byte
    pos & 1 of the bf16 pattern of element pos >> 1 (fill_model_f64; the device rounds a float32
    result, so its bytes need not be these)."""
    pos = _positions(stream_off, n)
    if mode == 1:
        bf = fill_model_f64(seed, 0, 0, elems=pos >> U(1))[1].astype(U)
        return ((bf >> (U(8) * (pos & U(1)))) & U(0xFF)).astype(np.uint8)
    assert mode == 0
    with np.errstate(over="ignore"):
        w = _splitmix(U(seed % (1 << 64)) ^ ((pos >> U(3)) * U(WORD_KEY)))
    return ((w >> (U(8) * (pos & U(7)))) & U(0xFF)).astype(np.uint8)


def bf16_rne(values: np.ndarray) -> np.ndarray:
    """uint16 bf16 patterns of finite float64 values that are zero or in bf16's normal range: the
    exponent is re-biased, the 52 stored significand bits are rounded to 7 once, ties to even, and a
    carry out of the significand steps the exponent."""
    bits = np.ascontiguousarray(values, dtype=np.float64).view(U)
    sign, e, m = bits >> U(63), (bits >> U(52)) & U(0x7FF), bits & U((1 << 52) - 1)
    zero = (e == U(0)) & (m == U(0))
    assert np.all(zero | ((e > U(1023 - 127)) & (e <= U(1023 + 127)))), "outside bf16's normal range"
    wide = ((e - U(1023 - 127)) << U(52)) | m
    q, rem, half = wide >> U(45), wide & U((1 << 45) - 1), U(1 << 44)
    q = q + ((rem > half) | ((rem == half) & ((q & U(1)) == U(1)))).astype(U)
    return np.where(zero, sign << U(15), (sign << U(15)) | q).astype(np.uint16)


def fill_model_f64(seed: int, first_elem: int, count: int, elems: np.ndarray | None = None):
    """Mode 1 elements first_elem .. first_elem + count - 1 (or the uint64 indices `elems`): from
    h = splitmix64(seed ^ e * ELEM_KEY), u1 = (bits 40..63 + 1/2) / 2^24 and u2 = bits 16..39 / 2^24,
    the value sqrt(-2 ln u1) cos(2 pi u2) * 0.02 in float64.  Returns (values, their bf16 patterns)."""
    e = _positions(first_elem, count) if elems is None else elems
    with np.errstate(over="ignore"):
        h = _splitmix(U(seed % (1 << 64)) ^ (e * U(ELEM_KEY)))
    u1 = (((h >> U(40)) & U(0xFFFFFF)).astype(np.float64) + 0.5) / 2.0 ** 24
    u2 = ((h >> U(16)) & U(0xFFFFFF)).astype(np.float64) / 2.0 ** 24
    z = np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2) * SIGMA
    return z, bf16_rne(z)


MODE1_MAX = SIGMA * float(np.sqrt(-2.0 * np.log(0.5 / 2.0 ** 24)))  # the smallest u1, |cos| = 1


def bf16_values(raw: np.ndarray) -> np.ndarray:
    """float64 values of little-endian bf16 bytes (an even number of them)."""
    u16 = np.ascontiguousarray(raw).view("<u2").astype(np.uint32)
    return (u16 << np.uint32(16)).view(np.float32).astype(np.float64)


def info_hash_model(rows) -> np.ndarray:
    """uint8 [n, 20]: per 32-byte row the SHA-1 digest of b"zest-xet-v1:" + row."""
    rows = np.asarray(rows, dtype=np.uint8).reshape(-1, 32)
    out = np.zeros((len(rows), 20), dtype=np.uint8)
    for i, r in enumerate(rows):
        out[i] = np.frombuffer(hashlib.sha1(b"zest-xet-v1:" + r.tobytes()).digest(), dtype=np.uint8)
    return out
