// K9 serve pack: serialise a byte window of a resident run straight from decoded chunk bytes (gfx950).
//
// A resident run is n chunks of one xorb described by two device tables that live as long as the
// seeder: src[i] (device address of chunk i's decoded bytes, any alignment, any order) and
// ser_end[i] (serialized end offset of chunk i relative to the run: sum over j <= i of len_j + 8).
// The serialized stream is the scheme-0 layout of core/xorb.cpp write_chunk_header / k_pack
// (synth.hip): per chunk [0][len LE24][0][len LE24] then len payload bytes.  zg_serve_pack writes
// bytes [lo, hi) of that stream to out[0, hi - lo): a request is one launch with scalars, no
// per-request tables.
//
// Output-centric: each lane owns aligned 16-byte output vectors (a wave stores 1 KiB contiguous), a
// workgroup owns a 16 KiB output tile.  The workgroup finds the tile's first chunk with a 256-ary
// search over ser_end and caches the next kCache boundaries and addresses in LDS; a lane finds its
// chunk by binary search there (boundaries past the cache are read from memory).  A vector wholly
// inside one payload is two aligned 16-byte loads funnelled with alignbyte into one 16-byte store;
// a vector that touches a header, crosses chunks or is the window's partial tail is assembled byte
// by byte (byte stores for the tail).  Every full store is aligned and 16 bytes wide, so `out` may
// be pinned host memory; no byte outside out[0, hi - lo) is written, and a source load is widened
// only to the aligned 16-byte blocks that hold at least one byte of the chunk being read.
#include <hip/hip_runtime.h>

#include "zgpu.h"

namespace {

constexpr uint32_t kThreads = 256;
constexpr uint32_t kVecPerLane = 4;
constexpr uint32_t kTile = kThreads * kVecPerLane * 16;  // output bytes per workgroup
constexpr uint32_t kCache = 256;                         // chunk boundaries cached in LDS per tile

// Byte h (0..7) of the scheme-0 header of a chunk of `len` bytes.
__device__ __forceinline__ uint32_t hdr_byte(uint32_t len, uint32_t h) {
  const uint32_t k = h & 3;
  return k ? (len >> (8 * (k - 1))) & 0xFF : 0;
}

__global__ void __launch_bounds__(kThreads) k_serve_pack(const uint64_t* __restrict__ src,
                                                         const uint64_t* __restrict__ ser_end, uint32_t n,
                                                         uint64_t lo, uint64_t hi, uint8_t* __restrict__ out) {
  __shared__ uint64_t s_end[kCache];
  __shared__ uint64_t s_src[kCache];
  const uint32_t tid = threadIdx.x;
  const uint64_t t0 = lo + uint64_t(blockIdx.x) * kTile;  // stream position of the tile's first byte

  // c0 = first chunk with ser_end > t0 (n: none), 256 probes per round; a, b stay block-uniform.
  uint32_t a = 0, b = n;
  while (b - a > kThreads) {
    const uint32_t step = (b - a + kThreads - 1) / kThreads;
    const uint64_t idx = uint64_t(a) + uint64_t(tid) * step;
    const uint32_t cnt = uint32_t(__syncthreads_count(idx < b && ser_end[idx] <= t0));
    if (cnt == 0) {
      b = a;
    } else {
      const uint64_t f = uint64_t(a) + uint64_t(cnt - 1) * step;  // last probe at or below t0
      b = uint32_t(f + step < b ? f + step : b);
      a = uint32_t(f + 1);
    }
  }
  const uint32_t c0 = a + uint32_t(__syncthreads_count(a + tid < b && ser_end[a + tid] <= t0));
  const uint32_t m = n - c0 < kCache ? n - c0 : kCache;  // cached chunks c0 .. c0 + m
  if (m == 0) return;                                    // window starts past the run: nothing to serve
  if (tid < m) {
    s_end[tid] = ser_end[c0 + tid];
    s_src[tid] = src[c0 + tid];
  }
  const uint64_t start0 = c0 ? ser_end[c0 - 1] : 0;
  __syncthreads();
  const uint64_t cached_end = s_end[m - 1];
  const uint64_t total = ser_end[n - 1];

#pragma unroll
  for (uint32_t j = 0; j < kVecPerLane; ++j) {
    const uint64_t p = t0 + (uint64_t(j) * kThreads + tid) * 16;  // stream position of this vector
    if (p >= hi || p >= total) break;
    // the chunk holding p: index c, serialized [cs, ce)
    uint32_t c;
    uint64_t cs, ce;
    if (p < cached_end) {
      uint32_t l = 0, r = m - 1;
      while (l < r) {
        const uint32_t mid = (l + r) >> 1;
        if (s_end[mid] > p) r = mid; else l = mid + 1;
      }
      c = c0 + l;
      ce = s_end[l];
      cs = l ? s_end[l - 1] : start0;
    } else {  // more boundaries in the tile than the cache holds
      uint32_t l = c0 + m, r = n - 1;
      while (l < r) {
        const uint32_t mid = l + ((r - l) >> 1);
        if (ser_end[mid] > p) r = mid; else l = mid + 1;
      }
      c = l;
      ce = ser_end[l];
      cs = ser_end[l - 1];
    }
    uint8_t* o = out + (p - lo);
    if (p >= cs + 8 && p + 16 <= ce && p + 16 <= hi) {
      // fast path: 16 payload bytes of one chunk
      const uint64_t base = c - c0 < m ? s_src[c - c0] : src[c];
      const uint64_t sa = base + (p - cs - 8);
      const uint32_t k = uint32_t(sa & 15);
      const uint4* q = reinterpret_cast<const uint4*>(sa - k);
      const uint4 x = q[0];
      const uint4 y = k ? q[1] : make_uint4(0, 0, 0, 0);  // q[1] holds chunk bytes only when k > 0
      uint32_t t[5];
      switch (k >> 2) {
        case 0: t[0] = x.x; t[1] = x.y; t[2] = x.z; t[3] = x.w; t[4] = y.x; break;
        case 1: t[0] = x.y; t[1] = x.z; t[2] = x.w; t[3] = y.x; t[4] = y.y; break;
        case 2: t[0] = x.z; t[1] = x.w; t[2] = y.x; t[3] = y.y; t[4] = y.z; break;
        default: t[0] = x.w; t[1] = y.x; t[2] = y.y; t[3] = y.z; t[4] = y.w; break;
      }
      const uint32_t kb = k & 3;
      *reinterpret_cast<uint4*>(o) =
          make_uint4(__builtin_amdgcn_alignbyte(t[1], t[0], kb), __builtin_amdgcn_alignbyte(t[2], t[1], kb),
                     __builtin_amdgcn_alignbyte(t[3], t[2], kb), __builtin_amdgcn_alignbyte(t[4], t[3], kb));
      continue;
    }
    // slow path: header bytes, chunk crossings, the window's tail
    const uint32_t nb = hi - p < 16 ? uint32_t(hi - p) : 16u;
    uint32_t w[4] = {0, 0, 0, 0};
    uint64_t qpos = p;
    bool live = true;
#pragma unroll
    for (uint32_t i = 0; i < 16; ++i, ++qpos) {
      if (i >= nb || !live) continue;
      while (qpos >= ce) {  // next chunk (ser_end is strictly increasing: each step adds >= 8)
        if (++c >= n) {
          live = false;
          break;
        }
        cs = ce;
        ce = c - c0 < m ? s_end[c - c0] : ser_end[c];
      }
      if (!live) continue;
      const uint64_t rel = qpos - cs;
      uint32_t v;
      if (rel < 8) {
        v = hdr_byte(uint32_t(ce - cs - 8), uint32_t(rel));
      } else {
        const uint64_t base = c - c0 < m ? s_src[c - c0] : src[c];
        v = reinterpret_cast<const uint8_t*>(base)[rel - 8];
      }
      w[i >> 2] |= v << (8 * (i & 3));
    }
    if (nb == 16) {
      *reinterpret_cast<uint4*>(o) = make_uint4(w[0], w[1], w[2], w[3]);
    } else {
#pragma unroll
      for (uint32_t i = 0; i < 16; ++i)
        if (i < nb) o[i] = uint8_t(w[i >> 2] >> (8 * (i & 3)));
    }
  }
}

}  // namespace

extern "C" hipError_t zg_serve_pack(const uint64_t* src, const uint64_t* ser_end, uint32_t n, uint64_t lo, uint64_t hi,
                                    uint8_t* out, hipStream_t stream) {
  if (hi <= lo) return hipSuccess;
  if (!src || !ser_end || !out || n == 0 || (reinterpret_cast<uintptr_t>(out) & 15)) return hipErrorInvalidValue;
  const uint64_t blocks = (hi - lo + kTile - 1) / kTile;
  if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_serve_pack, dim3(uint32_t(blocks)), dim3(kThreads), 0, stream, src, ser_end, n, lo, hi, out);
  return hipGetLastError();
}
