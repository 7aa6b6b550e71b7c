// K10 slice gather: copy the kept slices of many tensors out of one source buffer (a verified
// safetensors file) into one compact arena (gfx950).  Bytes only: dtype is the caller's business.
//
// Tensor i is n_runs[i] runs of run_bytes[i] bytes, run r starting at src + src_off[i] +
// r * src_stride[i]; its output is the runs laid end to end at dst + dst_off[i].  The table is six
// device arrays of n uint64 (ZG_SLICE_* rows of one [6][n] block), sorted by dst_off, outputs
// disjoint, dst_end[i] = dst_off[i] + n_runs[i] * run_bytes[i]; dst_end is therefore non-decreasing
// and doubles as the search key.  Zero-size entries (run_bytes == 0 or n_runs == 0) are legal and
// cost nothing: no output byte maps to them.
//
// Output-centric, as serve.hip: each lane owns aligned 16-byte output vectors (a wave stores 1 KiB
// contiguous), a workgroup owns a 16 KiB tile of the arena.  The workgroup finds the tile's first
// tensor with a 256-ary search over dst_end and caches the next kCache ends in LDS, with the fields
// of those tensors that can start inside the tile; a lane finds its tensor by binary search there
// (ends and fields past the cache are read from memory).  dst and every dst_off are 16-byte aligned,
// so a vector holds bytes of at most one tensor.  A vector wholly inside one run is two aligned
// 16-byte loads funnelled with alignbyte into one 16-byte store; a vector that crosses a run boundary
// or holds the tensor's last bytes is assembled byte by byte (byte stores when it is partial).  The
// lane's vectors are resolved first, then their bulk loads issued together, then stored, so four
// loads per lane are in flight instead of one.  Only output bytes of tensors are written: padding
// between tensors and everything past the last tensor stay untouched.  A source load is widened only
// to the aligned 16-byte blocks that hold at least one byte of the run being read.
#include <hip/hip_runtime.h>

#include "zgpu.h"

namespace {

constexpr uint32_t kThreads = 256;
constexpr uint32_t kVecPerLane = 4;
constexpr uint32_t kTile = kThreads * kVecPerLane * 16;  // arena bytes per workgroup
constexpr uint32_t kCache = 256;                         // tensor ends cached in LDS per tile

__global__ void __launch_bounds__(kThreads) k_slice_gather(const uint8_t* __restrict__ src,
                                                           const uint64_t* __restrict__ tab, uint32_t n,
                                                           uint8_t* __restrict__ dst) {
  __shared__ uint64_t s_end[kCache];
  __shared__ uint64_t s_fld[4][kCache];  // src_off, run_bytes, src_stride, dst_off of the cached tensors
  const uint64_t* __restrict__ t_end = tab + uint64_t(ZG_SLICE_DST_END) * n;
  const uint32_t tid = threadIdx.x;
  const uint64_t t0 = uint64_t(blockIdx.x) * kTile;  // arena offset of the tile's first byte

  // c0 = first tensor with dst_end > t0 (n: none), 256 probes per round; a, b stay block-uniform.
  uint32_t a = 0, b = n;
  while (b - a > kThreads) {
    const uint32_t step = (b - a + kThreads - 1) / kThreads;
    const uint64_t idx = uint64_t(a) + uint64_t(tid) * step;
    const uint32_t cnt = uint32_t(__syncthreads_count(idx < b && t_end[idx] <= t0));
    if (cnt == 0) {
      b = a;
    } else {
      const uint64_t f = uint64_t(a) + uint64_t(cnt - 1) * step;  // last probe at or below t0
      b = uint32_t(f + step < b ? f + step : b);
      a = uint32_t(f + 1);
    }
  }
  const uint32_t c0 = a + uint32_t(__syncthreads_count(a + tid < b && t_end[a + tid] <= t0));
  const uint32_t m = n - c0 < kCache ? n - c0 : kCache;  // cached tensors c0 .. c0 + m
  if (m == 0) return;                                    // tile past the last tensor
  if (tid < m) s_end[tid] = t_end[c0 + tid];
  __syncthreads();
  // A vector of this tile can only map to a cached tensor whose predecessor ends inside the tile:
  // the fields of the others are never looked up and are not fetched.
  if (tid < m && (tid == 0 || s_end[tid - 1] < t0 + kTile)) {
    s_fld[0][tid] = tab[uint64_t(ZG_SLICE_SRC_OFF) * n + c0 + tid];
    s_fld[1][tid] = tab[uint64_t(ZG_SLICE_RUN_BYTES) * n + c0 + tid];
    s_fld[2][tid] = tab[uint64_t(ZG_SLICE_SRC_STRIDE) * n + c0 + tid];
    s_fld[3][tid] = tab[uint64_t(ZG_SLICE_DST_OFF) * n + c0 + tid];
  }
  __syncthreads();
  const uint64_t cached_end = s_end[m - 1];
  const uint64_t total = t_end[n - 1];

  // Pass 1: where each of the lane's vectors reads.  kind 0: nothing to write (padding, or past the
  // last tensor); 1: 16 bytes of one run (bulk); 2: a run crossing or the tensor's tail (edge).
  const uint8_t* sp[kVecPerLane];
  uint64_t left[kVecPerLane], rbs[kVecPerLane], skip[kVecPerLane];  // bytes left in the run at sp; run_bytes;
                                                                    // src_stride - run_bytes (run end -> next run)
  uint32_t nbs[kVecPerLane], kind[kVecPerLane];
#pragma unroll
  for (uint32_t j = 0; j < kVecPerLane; ++j) {
    const uint64_t p = t0 + (uint64_t(j) * kThreads + tid) * 16;  // arena offset of this vector
    kind[j] = 0;
    if (p >= total) continue;
    // the first tensor ending after p: index c, output [ds, de)
    uint64_t de, ds, rb, stride, so;
    if (p < cached_end) {
      uint32_t l = 0, r = m - 1;
      while (l < r) {
        const uint32_t mid = (l + r) >> 1;
        if (s_end[mid] > p) r = mid; else l = mid + 1;
      }
      de = s_end[l];
      so = s_fld[0][l];
      rb = s_fld[1][l];
      stride = s_fld[2][l];
      ds = s_fld[3][l];
    } else {  // more tensors in the tile than the cache holds
      uint32_t l = c0 + m, r = n - 1;
      while (l < r) {
        const uint32_t mid = l + ((r - l) >> 1);
        if (t_end[mid] > p) r = mid; else l = mid + 1;
      }
      de = t_end[l];
      so = tab[uint64_t(ZG_SLICE_SRC_OFF) * n + l];
      rb = tab[uint64_t(ZG_SLICE_RUN_BYTES) * n + l];
      stride = tab[uint64_t(ZG_SLICE_SRC_STRIDE) * n + l];
      ds = tab[uint64_t(ZG_SLICE_DST_OFF) * n + l];
    }
    if (ds > p) continue;  // padding: ds is 16-byte aligned, so the tensor starts at p + 16 or later
    const uint64_t q = p - ds;  // output byte index within the tensor
    uint64_t run, within;
    if (de - ds <= rb) {  // one run (a tensor kept whole, or a slice of its outermost dim)
      run = 0;
      within = q;
    } else if (de - ds <= 0xFFFFFFFFull) {
      run = uint32_t(q) / uint32_t(rb);
      within = uint32_t(q) - uint32_t(run) * uint32_t(rb);
    } else {
      run = q / rb;
      within = q - run * rb;
    }
    sp[j] = src + so + run * stride + within;  // source of output byte p
    nbs[j] = de - p < 16 ? uint32_t(de - p) : 16u;
    left[j] = rb - within;  // >= 1
    rbs[j] = rb;
    skip[j] = stride - rb;
    kind[j] = nbs[j] == 16 && left[j] >= 16 ? 1 : 2;
  }

  // Pass 2: every bulk vector's two aligned loads, issued together.
  uint4 x[kVecPerLane], y[kVecPerLane];
#pragma unroll
  for (uint32_t j = 0; j < kVecPerLane; ++j) {
    if (kind[j] != 1) continue;
    const uint64_t sa = reinterpret_cast<uint64_t>(sp[j]);
    const uint32_t k = uint32_t(sa & 15);
    const uint4* v = reinterpret_cast<const uint4*>(sa - k);
    x[j] = v[0];
    y[j] = k ? v[1] : make_uint4(0, 0, 0, 0);  // v[1] holds bytes of the run only when k > 0
  }

  // Pass 3: funnel and store; edge vectors byte by byte.
#pragma unroll
  for (uint32_t j = 0; j < kVecPerLane; ++j) {
    if (kind[j] == 0) continue;
    uint8_t* o = dst + t0 + (uint64_t(j) * kThreads + tid) * 16;
    if (kind[j] == 1) {
      const uint32_t k = uint32_t(reinterpret_cast<uint64_t>(sp[j]) & 15);
      const uint4 xx = x[j], yy = y[j];
      uint32_t t[5];
      switch (k >> 2) {
        case 0: t[0] = xx.x; t[1] = xx.y; t[2] = xx.z; t[3] = xx.w; t[4] = yy.x; break;
        case 1: t[0] = xx.y; t[1] = xx.z; t[2] = xx.w; t[3] = yy.x; t[4] = yy.y; break;
        case 2: t[0] = xx.z; t[1] = xx.w; t[2] = yy.x; t[3] = yy.y; t[4] = yy.z; break;
        default: t[0] = xx.w; t[1] = yy.x; t[2] = yy.y; t[3] = yy.z; t[4] = yy.w; break;
      }
      const uint32_t kb = k & 3;
      *reinterpret_cast<uint4*>(o) =
          make_uint4(__builtin_amdgcn_alignbyte(t[1], t[0], kb), __builtin_amdgcn_alignbyte(t[2], t[1], kb),
                     __builtin_amdgcn_alignbyte(t[3], t[2], kb), __builtin_amdgcn_alignbyte(t[4], t[3], kb));
      continue;
    }
    const uint8_t* s = sp[j];
    const uint32_t nb = nbs[j];
    uint64_t lf = left[j];
    uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
    for (uint32_t i = 0; i < 16; ++i) {
      if (i >= nb) continue;
      if (lf == 0) {  // next run
        s += skip[j];
        lf = rbs[j];
      }
      w[i >> 2] |= uint32_t(*s) << (8 * (i & 3));
      ++s;
      --lf;
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

extern "C" hipError_t zg_slice_gather(const uint8_t* src, const uint64_t* table, uint32_t n, uint64_t dst_total,
                                      uint8_t* dst, hipStream_t stream) {
  if (n == 0 || dst_total == 0) return hipSuccess;
  if (!src || !table || !dst || (reinterpret_cast<uintptr_t>(dst) & 15)) return hipErrorInvalidValue;
  const uint64_t blocks = (dst_total + kTile - 1) / kTile;
  if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_slice_gather, dim3(uint32_t(blocks)), dim3(kThreads), 0, stream, src, table, n, dst);
  return hipGetLastError();
}
