// K15 slice scatter: copy the kept slices of many tensors out of one source buffer (a verified
// safetensors file) to absolute device addresses that the caller owns (gfx950).  The receiving twin
// of K10 (shard.hip): the same runs, but no arena.  Bytes only: dtype is the caller's business.
//
// Entry i is n_runs[i] runs of run_bytes[i] bytes, run r starting at src + src_off[i] +
// r * src_stride[i]; its output is the runs laid end to end at the address dst_addr[i], which may
// have any alignment and lie in any allocation.  The table is six device arrays of n uint64
// (ZG_SCATTER_* rows of one [6][n] block).  Outputs are disjoint from each other and from src.
// Zero-size entries (run_bytes == 0 or n_runs == 0) are legal and cost nothing.
//
// Output-centric, as K10 and K9: the index space is the concatenation of every entry's aligned
// 16-byte destination blocks, entry i covering blocks floor(dst / 16) .. ceil((dst + size) / 16), and
// blk_end[i] (the inclusive prefix sum of the block counts, built by the host) is the search key, as
// dst_end is K10's.  Each lane owns blocks of that space (a wave stores up to 1 KiB contiguous), a
// workgroup owns a tile of 1024 of them.  The workgroup finds the tile's first entry with a 256-ary
// search over blk_end and caches the next kCache ends in LDS with the fields of the entries that can
// start inside the tile; a lane finds its entry by binary search there (ends and fields past the
// cache are read from memory).  A block that two entries share appears once per entry, and each
// instance writes only its own bytes.
//
// Exact writes: a 16-byte store goes only to an aligned block that lies wholly inside one entry's
// output; heads, tails and shared blocks are written with byte stores.  No destination byte is ever
// read, so a block is never read and written back: another lane of the same launch may own the
// neighbouring bytes.  A block wholly inside one run is two aligned 16-byte loads funnelled with
// alignbyte into the one store; a block that crosses a run boundary or is partial is assembled byte
// by byte.  A source load is widened only to the aligned 16-byte blocks that hold at least one byte
// of the run being read.  The lane's blocks are resolved first, then their bulk loads issued
// together, then stored, so four loads per lane are in flight instead of one.
#include <hip/hip_runtime.h>

#include "zgpu.h"

namespace {

constexpr uint32_t kThreads = 256;
constexpr uint32_t kVecPerLane = 4;
constexpr uint32_t kTileBlocks = kThreads * kVecPerLane;  // 16-byte destination blocks per workgroup
constexpr uint32_t kCache = 256;                          // entry ends cached in LDS per tile

__global__ void __launch_bounds__(kThreads) k_slice_scatter(const uint8_t* __restrict__ src,
                                                            const uint64_t* __restrict__ tab, uint32_t n) {
  __shared__ uint64_t s_end[kCache];
  __shared__ uint64_t s_fld[5][kCache];  // src_off, run_bytes, src_stride, dst_addr, output end of the cached entries
  const uint64_t* __restrict__ t_end = tab + uint64_t(ZG_SCATTER_BLK_END) * n;
  const uint32_t tid = threadIdx.x;
  const uint64_t t0 = uint64_t(blockIdx.x) * kTileBlocks;  // index of the tile's first block

  // c0 = first entry with blk_end > t0 (n: none), 256 probes per round; a, b stay block-uniform.
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
  const uint32_t m = n - c0 < kCache ? n - c0 : kCache;  // cached entries c0 .. c0 + m
  if (m == 0) return;                                    // tile past the last entry
  if (tid < m) s_end[tid] = t_end[c0 + tid];
  __syncthreads();
  // A block of this tile can only map to a cached entry whose predecessor ends inside the tile: the
  // fields of the others are never looked up and are not fetched.
  if (tid < m && (tid == 0 || s_end[tid - 1] < t0 + kTileBlocks)) {
    s_fld[0][tid] = tab[uint64_t(ZG_SCATTER_SRC_OFF) * n + c0 + tid];
    s_fld[1][tid] = tab[uint64_t(ZG_SCATTER_RUN_BYTES) * n + c0 + tid];
    s_fld[2][tid] = tab[uint64_t(ZG_SCATTER_SRC_STRIDE) * n + c0 + tid];
    s_fld[3][tid] = tab[uint64_t(ZG_SCATTER_DST_ADDR) * n + c0 + tid];
    s_fld[4][tid] = s_fld[3][tid] + s_fld[1][tid] * tab[uint64_t(ZG_SCATTER_N_RUNS) * n + c0 + tid];  // output end
  }
  __syncthreads();
  const uint64_t cached_end = s_end[m - 1];
  const uint64_t total = t_end[n - 1];

  // Pass 1: where each of the lane's blocks reads and writes.  kind 0: past the last entry; 1: an
  // aligned block of 16 output bytes of one run (bulk); 1 + nb: nb output bytes of a run crossing, a
  // head, a tail or a shared block (edge).
  const uint8_t* sp[kVecPerLane];
  uint8_t* op[kVecPerLane];  // address of the block's first output byte
  uint64_t left[kVecPerLane], rbs[kVecPerLane], skip[kVecPerLane];  // bytes left in the run at sp; run_bytes;
                                                                    // src_stride - run_bytes (run end -> next run)
  uint32_t kind[kVecPerLane];
#pragma unroll
  for (uint32_t j = 0; j < kVecPerLane; ++j) {
    const uint64_t v = t0 + uint64_t(j) * kThreads + tid;  // index of this block
    kind[j] = 0;
    if (v >= total) continue;
    // the first entry ending after v: output [ds, de), its blocks end at index be
    uint64_t be, ds, de, rb, stride, so;
    if (v < cached_end) {
      uint32_t l = 0, r = m - 1;
      while (l < r) {
        const uint32_t mid = (l + r) >> 1;
        if (s_end[mid] > v) r = mid; else l = mid + 1;
      }
      be = s_end[l];
      so = s_fld[0][l];
      rb = s_fld[1][l];
      stride = s_fld[2][l];
      ds = s_fld[3][l];
      de = s_fld[4][l];
    } else {  // more entries in the tile than the cache holds
      uint32_t l = c0 + m, r = n - 1;
      while (l < r) {
        const uint32_t mid = l + ((r - l) >> 1);
        if (t_end[mid] > v) r = mid; else l = mid + 1;
      }
      be = t_end[l];
      so = tab[uint64_t(ZG_SCATTER_SRC_OFF) * n + l];
      rb = tab[uint64_t(ZG_SCATTER_RUN_BYTES) * n + l];
      stride = tab[uint64_t(ZG_SCATTER_SRC_STRIDE) * n + l];
      ds = tab[uint64_t(ZG_SCATTER_DST_ADDR) * n + l];
      de = ds + rb * tab[uint64_t(ZG_SCATTER_N_RUNS) * n + l];
    }
    // The entry's last block ends at de rounded up; this one is be - v blocks before that.
    const uint64_t p = ((de + 15) & ~uint64_t(15)) - (be - v) * 16;  // aligned address of this block
    const uint64_t lo = p > ds ? p : ds;                             // its output bytes: [lo, hi)
    const uint64_t hi = p + 16 < de ? p + 16 : de;
    const uint64_t q = lo - ds;  // output byte index within the entry
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
    sp[j] = src + so + run * stride + within;  // source of output byte lo
    op[j] = reinterpret_cast<uint8_t*>(lo);
    const uint32_t nb = uint32_t(hi - lo);  // 1 .. 16
    left[j] = rb - within;                  // >= 1
    rbs[j] = rb;
    skip[j] = stride - rb;
    kind[j] = nb == 16 && left[j] >= 16 ? 1 : 1 + nb;  // 16 output bytes: lo == p, the block is whole
  }

  // Pass 2: every bulk block's two aligned loads, issued together.
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

  // Pass 3: funnel and store; edge blocks byte by byte.
#pragma unroll
  for (uint32_t j = 0; j < kVecPerLane; ++j) {
    if (kind[j] == 0) continue;
    uint8_t* o = op[j];
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
    const uint32_t nb = kind[j] - 1;
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
    if (nb == 16) {  // a whole aligned block that crosses a run boundary
      *reinterpret_cast<uint4*>(o) = make_uint4(w[0], w[1], w[2], w[3]);
    } else {  // a head, a tail or a shared block: its own bytes only
#pragma unroll
      for (uint32_t i = 0; i < 16; ++i)
        if (i < nb) o[i] = uint8_t(w[i >> 2] >> (8 * (i & 3)));
    }
  }
}

}  // namespace

extern "C" hipError_t zg_slice_scatter(const uint8_t* src, const uint64_t* table, uint32_t n, uint64_t total_blocks,
                                       hipStream_t stream) {
  if (n == 0 || total_blocks == 0) return hipSuccess;
  if (!src || !table) return hipErrorInvalidValue;
  const uint64_t blocks = (total_blocks + kTileBlocks - 1) / kTileBlocks;
  if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_slice_scatter, dim3(uint32_t(blocks)), dim3(kThreads), 0, stream, src, table, n);
  return hipGetLastError();
}
