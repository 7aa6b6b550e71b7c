// K5 GearHash CDC candidates, K14 the same over a segment list, K7 xorb packing, and
// synthetic-content generators (gfx950).
//
// CDC: the Xet gear hash only depends on the last 64 bytes (h = (h << 1) + G[b]), so every
// position's hash is recomputable from a 63-byte warm-up: each lane scans its own 256-byte
// segment independently and appends the END offsets (i + 1) whose hash has (h & mask) == 0.
// Chunk selection (min 8 KiB / max 128 KiB rule) runs on the host over the sparse candidates.
#include <hip/hip_runtime.h>

#include "../core/gear_table.h"
#include "zgpu.h"

namespace {

__constant__ uint64_t kGearDev[256] = ZEST_GEAR_TABLE_INIT;

// CDC: one lane per 2 KiB segment (warm-up overhead 128/2048), read with 16-byte loads from a
// 16-byte-aligned view of the buffer (the old lane-per-256-B dword reader made every load touch 64
// cache lines for 4 useful bytes each and thrashed L1, 274 GB/s).  The candidate test is folded
// into a per-step "any hit" flag; a hit (rare: 1 in 2^16 positions for the Xet mask) re-scans
// the step's bytes on a slow path that emits the offsets.
constexpr uint32_t kSeg = 2048;
constexpr uint32_t kStep = 128;  // bytes per lane per step: one full 128-byte line

template <bool kHiOnly>
__device__ __forceinline__ bool gear_zero(uint64_t h, uint64_t mask) {
  if (kHiOnly) return (uint32_t(h >> 32) & uint32_t(mask >> 32)) == 0;
  return (h & mask) == 0;
}

template <bool kHiOnly>
__global__ void __launch_bounds__(256) k_cdc_candidates(const uint8_t* __restrict__ data, uint64_t n, uint64_t mask,
                                                        uint64_t* __restrict__ out, unsigned long long* count,
                                                        uint64_t cap) {
  __shared__ uint64_t gear[256];
  gear[threadIdx.x] = kGearDev[threadIdx.x];
  __syncthreads();
  const uint64_t a0 = reinterpret_cast<uintptr_t>(data);
  const uint32_t shift = uint32_t(a0 & 15);
  const uint4* base = reinterpret_cast<const uint4*>(a0 - shift);  // virtual position v = index + shift
  const uint64_t vend = n + shift;
  const uint64_t vs = (uint64_t(blockIdx.x) * blockDim.x + threadIdx.x) * kSeg;
  if (vs >= vend) return;
  const uint64_t ve = vs + kSeg < vend ? vs + kSeg : vend;
  uint64_t h = 0;
  // 128 bytes per step: eight 16-byte loads issued together cover one whole line, so each line is
  // fetched once even though lanes are 2 KiB apart (L1 cannot hold a line per lane across steps).
  // The first step is the warm-up over the bytes before the segment (h depends on the last 64).
  for (uint64_t q = vs >= kStep ? vs - kStep : vs; q < ve; q += kStep) {
    uint32_t w[kStep / 4];
#pragma unroll
    for (int k = 0; k < int(kStep / 16); ++k) {
      const uint4 x = q + 16 * k < vend ? base[(q >> 4) + k] : make_uint4(0, 0, 0, 0);
      w[4 * k] = x.x;
      w[4 * k + 1] = x.y;
      w[4 * k + 2] = x.z;
      w[4 * k + 3] = x.w;
    }
    const bool warm = q < vs;
    const uint64_t h0 = h;
    bool any = false;
    if (q >= shift && q + kStep <= vend) {
#pragma unroll
      for (int j = 0; j < int(kStep); ++j) {
        h = (h << 1) + gear[(w[j >> 2] >> (8 * (j & 3))) & 0xFF];
        any |= gear_zero<kHiOnly>(h, mask);
      }
    } else {
      for (int j = 0; j < int(kStep); ++j) {
        if (q + j < shift || q + j >= vend) continue;
        h = (h << 1) + gear[(w[j >> 2] >> (8 * (j & 3))) & 0xFF];
        any |= gear_zero<kHiOnly>(h, mask);
      }
    }
    if (any && !warm) {  // rare: replay the step's bytes and emit END offsets (index + 1)
      uint64_t g = h0;
      for (int j = 0; j < int(kStep); ++j) {
        const uint64_t v = q + j;
        if (v < shift || v >= vend) continue;
        g = (g << 1) + gear[(w[j >> 2] >> (8 * (j & 3))) & 0xFF];
        if (gear_zero<kHiOnly>(g, mask)) {
          const unsigned long long k = atomicAdd(count, 1ull);
          if (k < cap) out[k] = v - shift + 1;
        }
      }
    }
  }
}

// K14: K5 over a file that is a list of segments (loose tensors, published where they lie).
//
// The work item is K5's: a lane owns one 2 KiB window of a segment's aligned address space, clipped
// to the segment, and steps through it 128 bytes at a time.  The window -> (segment, window in
// segment) map is implicit: the host uploads the prefix count of windows per segment (a few hundred
// entries for a 70B model, where a per-window table would be over 1 GB); a wave binary-searches it
// once, with scalar loads, for its first lane and the lanes walk forward from there (a wave spans
// at most 64 segments, and almost always one).  Windows 1.. of a segment warm up from the 128 bytes
// before them, which lie in the same segment (a window starts at a multiple of 2048 of the aligned
// space, at least 2033 bytes into the segment).  Window 0 starts with the segment: its history is
// the end of the previous segments, which k_seg_lead gathered into the segment's 64-byte lead-in
// row; the first segment has none, and h starts from 0 as the scalar scan of the file does.
__global__ void __launch_bounds__(64) k_seg_lead(const ZgSeg* __restrict__ segs, uint8_t* __restrict__ lead) {
  const uint32_t s = blockIdx.x, j = threadIdx.x;
  const uint64_t vstart = segs[s].vstart;
  const uint64_t L = vstart < 64 ? vstart : 64;  // file bytes before the segment, at most the gear window
  if (j >= L) return;
  const uint64_t p = vstart - L + j;  // lies in a segment before s
  uint32_t lo = 0, hi = s - 1;        // L > 0, so s >= 1
  while (lo < hi) {
    const uint32_t mid = (lo + hi + 1) >> 1;
    if (segs[mid].vstart <= p) lo = mid;
    else hi = mid - 1;
  }
  lead[64 * uint64_t(s) + j] = reinterpret_cast<const uint8_t*>(uintptr_t(segs[lo].addr))[p - segs[lo].vstart];
}

template <bool kHiOnly>
__global__ void __launch_bounds__(256) k_cdc_candidates_segs(const ZgSeg* __restrict__ segs,
                                                             const uint64_t* __restrict__ wpre, uint32_t nseg,
                                                             const uint8_t* __restrict__ lead, uint64_t mask,
                                                             uint64_t* __restrict__ out, unsigned long long* count,
                                                             uint64_t cap) {
  __shared__ uint64_t gear[256];
  gear[threadIdx.x] = kGearDev[threadIdx.x];
  __syncthreads();
  const uint64_t W = wpre[nseg];
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint64_t t0 = (uint64_t(blockIdx.x) * 4 + wave) * 64;  // the wave's first window: uniform
  if (t0 >= W) return;
  uint32_t lo = 0, hi = nseg - 1;  // the segment of window t0: the last s with wpre[s] <= t0
  while (lo < hi) {
    const uint32_t mid = (lo + hi + 1) >> 1;
    if (wpre[mid] <= t0) lo = mid;
    else hi = mid - 1;
  }
  const uint64_t t = t0 + (threadIdx.x & 63);
  if (t >= W) return;
  uint32_t s = lo;
  while (t >= wpre[s + 1]) ++s;  // every segment has a window, and t < W = wpre[nseg]
  const ZgSeg sg = segs[s];
  const uint64_t win = t - wpre[s];
  const uint32_t shift = uint32_t(sg.addr & 15);
  const uint4* base = reinterpret_cast<const uint4*>(uintptr_t(sg.addr - shift));  // position v = index + shift
  const uint64_t vend = sg.len + shift;
  const uint64_t vs = win * kSeg;  // < vend by the window count
  const uint64_t ve = vs + kSeg < vend ? vs + kSeg : vend;
  uint64_t h = 0;
  if (win == 0) {  // the history before the segment, oldest byte first
    const uint32_t L = sg.vstart < 64 ? uint32_t(sg.vstart) : 64u;
    const uint8_t* lp = lead + 64 * uint64_t(s);
    for (uint32_t j = 0; j < L; ++j) h = (h << 1) + gear[lp[j]];
  }
  // from here on K5's loop; a block [16 m, 16 m + 16) is loaded only when 16 m < vend, and such a
  // block holds a byte of the segment (m >= 1: byte 16 m >= shift; m = 0: byte shift, as len >= 1)
  for (uint64_t q = win ? vs - kStep : vs; q < ve; q += kStep) {
    uint32_t w[kStep / 4];
#pragma unroll
    for (int k = 0; k < int(kStep / 16); ++k) {
      const uint4 x = q + 16 * k < vend ? base[(q >> 4) + k] : make_uint4(0, 0, 0, 0);
      w[4 * k] = x.x;
      w[4 * k + 1] = x.y;
      w[4 * k + 2] = x.z;
      w[4 * k + 3] = x.w;
    }
    const bool warm = q < vs;
    const uint64_t h0 = h;
    bool any = false;
    if (q >= shift && q + kStep <= vend) {
#pragma unroll
      for (int j = 0; j < int(kStep); ++j) {
        h = (h << 1) + gear[(w[j >> 2] >> (8 * (j & 3))) & 0xFF];
        any |= gear_zero<kHiOnly>(h, mask);
      }
    } else {
      for (int j = 0; j < int(kStep); ++j) {
        if (q + j < shift || q + j >= vend) continue;
        h = (h << 1) + gear[(w[j >> 2] >> (8 * (j & 3))) & 0xFF];
        any |= gear_zero<kHiOnly>(h, mask);
      }
    }
    if (any && !warm) {  // rare: replay the step's bytes and emit END offsets in file coordinates
      uint64_t g = h0;
      for (int j = 0; j < int(kStep); ++j) {
        const uint64_t v = q + j;
        if (v < shift || v >= vend) continue;
        g = (g << 1) + gear[(w[j >> 2] >> (8 * (j & 3))) & 0xFF];
        if (gear_zero<kHiOnly>(g, mask)) {
          const unsigned long long k = atomicAdd(count, 1ull);
          if (k < cap) out[k] = sg.vstart + (v - shift) + 1;
        }
      }
    }
  }
}

__device__ __forceinline__ uint64_t splitmix64(uint64_t x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

// Byte `pos` of the synthetic stream.
__device__ __forceinline__ uint32_t synth_byte(uint64_t seed, uint64_t pos, int mode) {
  if (mode == 0) {
    const uint64_t w = splitmix64(seed ^ ((pos >> 3) * 0xD1B54A32D192ED03ull));
    return uint32_t(w >> (8 * (pos & 7))) & 0xFF;
  }
  // bf16 ~ N(0, 0.02) element e = pos >> 1 (Box-Muller on one hashed uniform pair)
  const uint64_t e = pos >> 1;
  const uint64_t h = splitmix64(seed ^ (e * 0xA24BAED4963EE407ull));
  const float u1 = (float((h >> 40) & 0xFFFFFF) + 0.5f) * (1.0f / 16777216.0f);
  const float u2 = float((h >> 16) & 0xFFFFFF) * (1.0f / 16777216.0f);
  const float z = sqrtf(-2.0f * __logf(u1)) * __cosf(6.28318530718f * u2) * 0.02f;
  const uint32_t bits = __float_as_uint(z);
  const uint32_t bf = (bits + 0x7FFFu + ((bits >> 16) & 1u)) >> 16;  // RNE (no NaNs possible here)
  return (pos & 1) ? (bf >> 8) & 0xFF : bf & 0xFF;
}

__global__ void __launch_bounds__(256) k_fill(uint8_t* __restrict__ dst, uint64_t n, uint64_t seed, uint64_t stream_off,
                                              int mode) {
  // Each thread produces 16 destination-aligned bytes.
  const uint64_t da = reinterpret_cast<uintptr_t>(dst);
  const uint64_t lead = (16 - (da & 15)) & 15;  // bytes before the first aligned vector
  const uint64_t t = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (t == 0) {
    for (uint64_t i = 0; i < lead && i < n; ++i) dst[i] = uint8_t(synth_byte(seed, stream_off + i, mode));
  }
  if (n <= lead) return;
  const uint64_t body = n - lead;
  const uint64_t nvec = body >> 4;
  for (uint64_t v = t; v < nvec; v += uint64_t(gridDim.x) * blockDim.x) {
    const uint64_t pos = stream_off + lead + 16 * v;
    uint32_t w[4];
    if (mode == 0 && (pos & 7) == 0) {
      const uint64_t a = splitmix64(seed ^ ((pos >> 3) * 0xD1B54A32D192ED03ull));
      const uint64_t b = splitmix64(seed ^ (((pos >> 3) + 1) * 0xD1B54A32D192ED03ull));
      w[0] = uint32_t(a);
      w[1] = uint32_t(a >> 32);
      w[2] = uint32_t(b);
      w[3] = uint32_t(b >> 32);
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        w[k] = synth_byte(seed, pos + 4 * k, mode) | (synth_byte(seed, pos + 4 * k + 1, mode) << 8) |
               (synth_byte(seed, pos + 4 * k + 2, mode) << 16) | (synth_byte(seed, pos + 4 * k + 3, mode) << 24);
      }
    }
    reinterpret_cast<uint4*>(dst + lead)[v] = make_uint4(w[0], w[1], w[2], w[3]);
  }
  if (t == 0) {
    for (uint64_t i = lead + 16 * nvec; i < n; ++i) dst[i] = uint8_t(synth_byte(seed, stream_off + i, mode));
  }
}

// Pack: one wave per chunk writes [header | payload] (scheme 0) at out + out_off[i].
__global__ void __launch_bounds__(256) k_pack(const uint8_t* __restrict__ data, const uint64_t* __restrict__ data_off,
                                              const uint32_t* __restrict__ lens, const uint64_t* __restrict__ out_off,
                                              int n, uint8_t* __restrict__ out) {
  const int c = __builtin_amdgcn_readfirstlane(int(blockIdx.x * 4 + (threadIdx.x >> 6)));
  if (c >= n) return;
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t len = lens[c];
  uint8_t* o = out + out_off[c];
  if (lane < 8) {
    uint32_t b;
    switch (lane) {
      case 0: b = 0; break;                       // version
      case 1: b = len & 0xFF; break;              // compressed len (LE u24)
      case 2: b = (len >> 8) & 0xFF; break;
      case 3: b = (len >> 16) & 0xFF; break;
      case 4: b = 0; break;                       // scheme: none
      case 5: b = len & 0xFF; break;              // uncompressed len
      case 6: b = (len >> 8) & 0xFF; break;
      default: b = (len >> 16) & 0xFF; break;
    }
    o[lane] = uint8_t(b);
  }
  // payload copy (dst arbitrary alignment): simple strided 4-byte funnel copy
  const uint8_t* s = data + data_off[c];
  uint8_t* d = o + 8;
  const uintptr_t dAddr = reinterpret_cast<uintptr_t>(d);
  uint32_t head = uint32_t((4 - (dAddr & 3)) & 3);
  if (head > len) head = len;
  if (lane < head) d[lane] = s[lane];
  const uint32_t nw = (len - head) >> 2;
  const uint8_t* s2 = s + head;
  const uintptr_t sa = reinterpret_cast<uintptr_t>(s2);
  const uint32_t k = uint32_t(sa & 3);
  const uint32_t* sw = reinterpret_cast<const uint32_t*>(sa & ~uintptr_t(3));
  uint32_t* dw = reinterpret_cast<uint32_t*>(d + head);
  for (uint32_t w = lane; w < nw; w += 64) {
    const uint32_t a = sw[w];
    dw[w] = k ? __builtin_amdgcn_alignbyte(sw[w + 1], a, k) : a;
  }
  const uint32_t done = head + 4 * nw;
  if (lane < len - done) d[done + lane] = s[done + lane];
}

}  // namespace

extern "C" {

hipError_t zg_cdc_candidates(const uint8_t* data, uint64_t n, uint64_t mask, uint64_t* out,
                             unsigned long long* count, uint64_t capacity, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  const uint64_t segs = (n + 15 + kSeg - 1) / kSeg;
  if ((mask & 0xFFFFFFFFull) == 0)
    hipLaunchKernelGGL(k_cdc_candidates<true>, dim3(uint32_t((segs + 255) / 256)), dim3(256), 0, stream, data, n, mask,
                       out, count, capacity);
  else
    hipLaunchKernelGGL(k_cdc_candidates<false>, dim3(uint32_t((segs + 255) / 256)), dim3(256), 0, stream, data, n,
                       mask, out, count, capacity);
  return hipGetLastError();
}

hipError_t zg_cdc_candidates_segs(const ZgSeg* segs, const uint64_t* win_prefix, uint32_t n_segs, uint64_t n_windows,
                                  uint8_t* lead, uint64_t mask, uint64_t* out, unsigned long long* count,
                                  uint64_t capacity, hipStream_t stream) {
  if (n_segs == 0 || n_windows == 0) return hipSuccess;
  const uint64_t blocks = (n_windows + 255) / 256;
  if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_seg_lead, dim3(n_segs), dim3(64), 0, stream, segs, lead);
  if ((mask & 0xFFFFFFFFull) == 0)
    hipLaunchKernelGGL(k_cdc_candidates_segs<true>, dim3(uint32_t(blocks)), dim3(256), 0, stream, segs, win_prefix,
                       n_segs, lead, mask, out, count, capacity);
  else
    hipLaunchKernelGGL(k_cdc_candidates_segs<false>, dim3(uint32_t(blocks)), dim3(256), 0, stream, segs, win_prefix,
                       n_segs, lead, mask, out, count, capacity);
  return hipGetLastError();
}

hipError_t zg_fill_synthetic(uint8_t* dst, uint64_t n, uint64_t seed, uint64_t stream_offset, int mode,
                             hipStream_t stream) {
  if (n == 0) return hipSuccess;
  uint64_t vecs = n / 16 + 1;
  uint64_t blocks = (vecs + 255) / 256;
  if (blocks > 65536) blocks = 65536;
  hipLaunchKernelGGL(k_fill, dim3(uint32_t(blocks)), dim3(256), 0, stream, dst, n, seed, stream_offset, mode);
  return hipGetLastError();
}

hipError_t zg_pack_chunks(const uint8_t* data, const uint64_t* data_off, const uint32_t* lens, const uint64_t* out_off,
                          int n, uint8_t* out, hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_pack, dim3((n + 3) / 4), dim3(256), 0, stream, data, data_off, lens, out_off, n, out);
  return hipGetLastError();
}

}  // extern "C"
