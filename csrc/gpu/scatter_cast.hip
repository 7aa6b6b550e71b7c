// K16 converting slice scatter: K15 (scatter.hip) with a float conversion on the way (gfx950).  The
// kept slices of many tensors go out of one source buffer (a verified safetensors file, in its stored
// dtype) to absolute device addresses that the caller owns, in the destinations' own dtype.
//
// Geometry is K15's: entry i is n_runs[i] runs of run_bytes[i] SOURCE bytes, run r starting at src +
// src_off[i] + r * src_stride[i]; the converted elements are laid end to end at dst_addr[i].  kind[i]
// (ZG_CAST_*) names the conversion, so an entry writes run_bytes * n_runs / src_item * dst_item bytes.
// dst_addr is a multiple of the destination item and run_bytes of the source item (the host checks
// both); src_off and src_stride are arbitrary, so a source element may sit at any byte address.
// Entries of different kinds mix freely in one launch and may share a 16-byte destination block.
//
// Output-centric, as K15: the index space is the concatenation of every entry's aligned 16-byte
// destination blocks with blk_end (their inclusive prefix sum) as the search key, a lane owns blocks
// of it, a workgroup a tile of 1024.  The tile search is K15's: 256-ary over blk_end, the next kCache
// ends and the fields of the entries that can start inside the tile cached in LDS, memory past that.
//
// A block of 16 output bytes is 8, 16 or 32 source bytes.  When those lie inside one run they are
// read as the one to three aligned 16-byte blocks that hold them (so a load is widened only to
// aligned blocks holding at least one byte of the run being read), funnelled with alignbyte,
// converted and written with one 16-byte store.  Such a store goes only to an aligned block wholly
// inside one entry's output.  Heads, tails, shared blocks and blocks that cross a run boundary are
// written element by element with 2- or 4-byte stores of the entry's own elements, their source read
// byte by byte.  No destination byte is ever read.  The lane's blocks are resolved first, then their
// bulk loads issued together, then converted and stored.
//
// Arithmetic: round to nearest, ties to even, one rounding (a 16-bit source is widened to f32
// exactly, then rounded once); overflow gives infinity, signed zeros and subnormals are kept, a NaN
// stays a NaN (sign and payload unspecified).  bf16 is integer bit arithmetic; f16 uses the
// hardware converts (v_cvt_f16_f32, v_cvt_f32_f16), which keep subnormals in the default mode.
#include <hip/hip_runtime.h>

#include "zgpu.h"

namespace {

constexpr uint32_t kThreads = 256;
constexpr uint32_t kVecPerLane = 4;
constexpr uint32_t kTileBlocks = kThreads * kVecPerLane;  // 16-byte destination blocks per workgroup
constexpr uint32_t kCache = 256;                          // entry ends cached in LDS per tile

__host__ __device__ inline uint32_t f32_to_bf16(uint32_t x) {
  if ((x & 0x7FFFFFFFu) > 0x7F800000u) return (x >> 16) | 0x40u;  // NaN: keep it one
  return (x + 0x7FFFu + ((x >> 16) & 1u)) >> 16;                  // ties to even; carries into inf
}
__host__ __device__ inline uint32_t f32_to_f16(uint32_t x) {
  return __builtin_bit_cast(uint16_t, static_cast<_Float16>(__builtin_bit_cast(float, x)));
}
__host__ __device__ inline uint32_t f16_to_f32(uint32_t h) {
  return __builtin_bit_cast(uint32_t, static_cast<float>(__builtin_bit_cast(_Float16, uint16_t(h))));
}
// One element: v holds the source item in its low bits, the result is the destination item.
__host__ __device__ inline uint32_t convert_one(uint32_t kind, uint32_t v) {
  switch (kind) {
    case ZG_CAST_F32_BF16: return f32_to_bf16(v);
    case ZG_CAST_F32_F16: return f32_to_f16(v);
    case ZG_CAST_BF16_F32: return v << 16;
    case ZG_CAST_F16_F32: return f16_to_f32(v);
    case ZG_CAST_BF16_F16: return f32_to_f16(v << 16);
    default: return f32_to_bf16(f16_to_f32(v));  // ZG_CAST_F16_BF16
  }
}
__host__ __device__ inline uint32_t src_shift(uint32_t kind) { return kind <= ZG_CAST_F32_F16 ? 2 : 1; }  // log2 item
__host__ __device__ inline uint32_t dst_shift(uint32_t kind) {
  return kind == ZG_CAST_BF16_F32 || kind == ZG_CAST_F16_F32 ? 2 : 1;
}

__global__ void __launch_bounds__(kThreads) k_slice_scatter_cast(const uint8_t* __restrict__ src,
                                                                 const uint64_t* __restrict__ tab, uint32_t n) {
  __shared__ uint64_t s_end[kCache];
  __shared__ uint64_t s_fld[6][kCache];  // src_off, run_bytes, src_stride, dst_addr, output end, kind of the cached entries
  const uint64_t* __restrict__ t_end = tab + uint64_t(ZG_CAST_BLK_END) * n;
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
    const uint64_t rb = tab[uint64_t(ZG_CAST_RUN_BYTES) * n + c0 + tid];
    const uint64_t da = tab[uint64_t(ZG_CAST_DST_ADDR) * n + c0 + tid];
    const uint32_t kd = uint32_t(tab[uint64_t(ZG_CAST_KIND) * n + c0 + tid]);
    s_fld[0][tid] = tab[uint64_t(ZG_CAST_SRC_OFF) * n + c0 + tid];
    s_fld[1][tid] = rb;
    s_fld[2][tid] = tab[uint64_t(ZG_CAST_SRC_STRIDE) * n + c0 + tid];
    s_fld[3][tid] = da;
    s_fld[4][tid] = da + ((rb * tab[uint64_t(ZG_CAST_N_RUNS) * n + c0 + tid]) >> src_shift(kd) << dst_shift(kd));
    s_fld[5][tid] = kd;
  }
  __syncthreads();
  const uint64_t cached_end = s_end[m - 1];
  const uint64_t total = t_end[n - 1];

  // Pass 1: where each of the lane's blocks reads and writes.  what 0: past the last entry; 1: an
  // aligned block of 16 output bytes whose source lies in one run (bulk); 1 + ne: ne output elements
  // of a run crossing, a head, a tail or a shared block (edge).
  const uint8_t* sp[kVecPerLane];
  uint8_t* op[kVecPerLane];  // address of the block's first output byte
  uint64_t left[kVecPerLane], rbs[kVecPerLane], skip[kVecPerLane];  // bytes left in the run at sp; run_bytes;
                                                                    // src_stride - run_bytes (run end -> next run)
  uint32_t what[kVecPerLane], kinds[kVecPerLane];
#pragma unroll
  for (uint32_t j = 0; j < kVecPerLane; ++j) {
    const uint64_t v = t0 + uint64_t(j) * kThreads + tid;  // index of this block
    what[j] = 0;
    kinds[j] = 0;
    if (v >= total) continue;
    // the first entry ending after v: output [ds, de), its blocks end at index be
    uint64_t be, ds, de, rb, stride, so;
    uint32_t kd;
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
      kd = uint32_t(s_fld[5][l]);
    } else {  // more entries in the tile than the cache holds
      uint32_t l = c0 + m, r = n - 1;
      while (l < r) {
        const uint32_t mid = l + ((r - l) >> 1);
        if (t_end[mid] > v) r = mid; else l = mid + 1;
      }
      be = t_end[l];
      so = tab[uint64_t(ZG_CAST_SRC_OFF) * n + l];
      rb = tab[uint64_t(ZG_CAST_RUN_BYTES) * n + l];
      stride = tab[uint64_t(ZG_CAST_SRC_STRIDE) * n + l];
      ds = tab[uint64_t(ZG_CAST_DST_ADDR) * n + l];
      kd = uint32_t(tab[uint64_t(ZG_CAST_KIND) * n + l]);
      de = ds + ((rb * tab[uint64_t(ZG_CAST_N_RUNS) * n + l]) >> src_shift(kd) << dst_shift(kd));
    }
    const uint32_t ss = src_shift(kd), dsh = dst_shift(kd);
    // The entry's last block ends at de rounded up; this one is be - v blocks before that.
    const uint64_t p = ((de + 15) & ~uint64_t(15)) - (be - v) * 16;  // aligned address of this block
    const uint64_t lo = p > ds ? p : ds;                             // its output bytes: [lo, hi)
    const uint64_t hi = p + 16 < de ? p + 16 : de;
    const uint64_t q = (lo - ds) >> dsh << ss;        // source byte index within the entry's runs
    const uint64_t all = (de - ds) >> dsh << ss;      // source bytes of the entry
    uint64_t run, within;
    if (all <= rb) {  // one run (a tensor kept whole, or a slice of its outermost dim)
      run = 0;
      within = q;
    } else if (all <= 0xFFFFFFFFull) {
      run = uint32_t(q) / uint32_t(rb);
      within = uint32_t(q) - uint32_t(run) * uint32_t(rb);
    } else {
      run = q / rb;
      within = q - run * rb;
    }
    sp[j] = src + so + run * stride + within;  // source of the output element at lo
    op[j] = reinterpret_cast<uint8_t*>(lo);
    const uint32_t nb = uint32_t(hi - lo);  // 2 .. 16
    left[j] = rb - within;                  // >= one source item
    rbs[j] = rb;
    skip[j] = stride - rb;
    kinds[j] = kd;
    // 16 output bytes: lo == p, the block is whole; its source is 16 >> dsh << ss bytes
    what[j] = nb == 16 && left[j] >= (16u >> dsh << ss) ? 1 : 1 + (nb >> dsh);
  }

  // Pass 2: every bulk block's one to three aligned loads, issued together.
  uint4 x[kVecPerLane], y[kVecPerLane], z[kVecPerLane];
#pragma unroll
  for (uint32_t j = 0; j < kVecPerLane; ++j) {
    if (what[j] != 1) continue;
    const uint64_t sa = reinterpret_cast<uint64_t>(sp[j]);
    const uint32_t k = uint32_t(sa & 15);
    const uint32_t last = (k + (16u >> dst_shift(kinds[j]) << src_shift(kinds[j])) - 1) >> 4;  // block of the last byte
    const uint4* v = reinterpret_cast<const uint4*>(sa - k);
    x[j] = v[0];
    y[j] = last >= 1 ? v[1] : make_uint4(0, 0, 0, 0);  // v[1], v[2] are read only when they hold bytes of the run
    z[j] = last >= 2 ? v[2] : make_uint4(0, 0, 0, 0);
  }

  // Pass 3: funnel, convert and store; edge blocks element by element.
#pragma unroll
  for (uint32_t j = 0; j < kVecPerLane; ++j) {
    if (what[j] == 0) continue;
    uint8_t* o = op[j];
    const uint32_t kd = kinds[j];
    if (what[j] == 1) {
      const uint32_t k = uint32_t(reinterpret_cast<uint64_t>(sp[j]) & 15);
      const uint4 xx = x[j], yy = y[j], zz = z[j];
      uint32_t t[9];
      switch (k >> 2) {
        case 0: t[0] = xx.x; t[1] = xx.y; t[2] = xx.z; t[3] = xx.w; t[4] = yy.x; t[5] = yy.y; t[6] = yy.z; t[7] = yy.w; t[8] = zz.x; break;
        case 1: t[0] = xx.y; t[1] = xx.z; t[2] = xx.w; t[3] = yy.x; t[4] = yy.y; t[5] = yy.z; t[6] = yy.w; t[7] = zz.x; t[8] = zz.y; break;
        case 2: t[0] = xx.z; t[1] = xx.w; t[2] = yy.x; t[3] = yy.y; t[4] = yy.z; t[5] = yy.w; t[6] = zz.x; t[7] = zz.y; t[8] = zz.z; break;
        default: t[0] = xx.w; t[1] = yy.x; t[2] = yy.y; t[3] = yy.z; t[4] = yy.w; t[5] = zz.x; t[6] = zz.y; t[7] = zz.z; t[8] = zz.w; break;
      }
      const uint32_t kb = k & 3;
      uint32_t w[8];  // the source bytes of the block, from its first
#pragma unroll
      for (uint32_t i = 0; i < 8; ++i) w[i] = __builtin_amdgcn_alignbyte(t[i + 1], t[i], kb);
      uint32_t r[4];
      if (src_shift(kd) == 2) {  // 8 f32 -> 8 halves
#pragma unroll
        for (uint32_t i = 0; i < 4; ++i)
          r[i] = kd == ZG_CAST_F32_BF16 ? f32_to_bf16(w[2 * i]) | f32_to_bf16(w[2 * i + 1]) << 16
                                        : f32_to_f16(w[2 * i]) | f32_to_f16(w[2 * i + 1]) << 16;
      } else if (dst_shift(kd) == 2) {  // 4 halves -> 4 f32
#pragma unroll
        for (uint32_t i = 0; i < 4; ++i) {
          const uint32_t h = (w[i >> 1] >> (16 * (i & 1))) & 0xFFFFu;
          r[i] = kd == ZG_CAST_BF16_F32 ? h << 16 : f16_to_f32(h);
        }
      } else {  // 8 halves -> 8 halves
#pragma unroll
        for (uint32_t i = 0; i < 4; ++i)
          r[i] = kd == ZG_CAST_BF16_F16 ? f32_to_f16(w[i] << 16) | f32_to_f16(w[i] & 0xFFFF0000u) << 16
                                        : f32_to_bf16(f16_to_f32(w[i] & 0xFFFFu)) | f32_to_bf16(f16_to_f32(w[i] >> 16)) << 16;
      }
      *reinterpret_cast<uint4*>(o) = make_uint4(r[0], r[1], r[2], r[3]);
      continue;
    }
    const uint8_t* s = sp[j];
    const uint32_t ne = what[j] - 1;  // elements: 1 .. 8 halves or 1 .. 4 f32
    const bool wide_src = src_shift(kd) == 2, wide_dst = dst_shift(kd) == 2;
    uint64_t lf = left[j];
#pragma unroll
    for (uint32_t i = 0; i < 8; ++i) {
      if (i >= ne) continue;
      if (lf == 0) {  // next run: run_bytes is a multiple of the source item, so no element straddles two
        s += skip[j];
        lf = rbs[j];
      }
      uint32_t e = uint32_t(s[0]) | uint32_t(s[1]) << 8;
      if (wide_src) e |= uint32_t(s[2]) << 16 | uint32_t(s[3]) << 24;
      const uint32_t step = wide_src ? 4 : 2;
      s += step;
      lf -= step;
      const uint32_t c = convert_one(kd, e);
      if (wide_dst) *reinterpret_cast<uint32_t*>(o + 4 * i) = c;
      else *reinterpret_cast<uint16_t*>(o + 2 * i) = uint16_t(c);
    }
  }
}

}  // namespace

extern "C" hipError_t zg_slice_scatter_cast(const uint8_t* src, const uint64_t* table, uint32_t n,
                                            uint64_t total_blocks, hipStream_t stream) {
  if (n == 0 || total_blocks == 0) return hipSuccess;
  if (!src || !table) return hipErrorInvalidValue;
  const uint64_t blocks = (total_blocks + kTileBlocks - 1) / kTileBlocks;
  if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_slice_scatter_cast, dim3(uint32_t(blocks)), dim3(kThreads), 0, stream, src, table, n);
  return hipGetLastError();
}
