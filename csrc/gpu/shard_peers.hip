// K11 slice gather from several sources: K10 (shard.hip) with up to kZgMaxPeerSegs source buffers,
// for the collective sharded pull (zest_amd/parallel/shard_pull.py).  In a round every rank copies
// its kept slices out of the owners' scratches (its own, and its peers' mapped by map_peer_arenas)
// into one compact arena.  Bytes only.
//
// The table is K10's six rows plus ZG_SLICE_SRC, the source index of each entry; src_off is relative
// to that source's base (passed by value in ZgSliceSrcs, as K8's ZgPeerSegs).  Entries are sorted by
// dst_off, outputs disjoint and 16-byte aligned, and the entries of one source are contiguous, so
// source s owns one arena range [lo[s], hi[s]) (first dst_off .. last dst_end of its entries with
// output; lo == hi: no entries).  Per entry the semantics are exactly K10's: only output bytes of
// entries are written, padding between entries and between sources keeps its bytes, and a source
// load is widened only to the aligned 16-byte blocks that hold a byte of the run being read.
//
// Scheduling, as K8 (xgmi.hip): one launch serves every source; neighbouring blocks serve different
// sources and a block loops over the 16 KiB tiles of its source's arena range, so all peers' links
// are read at once instead of one after the other (K10's tiles walk the arena in order: launched
// per source, all running workgroups would read one peer).  Block b is the (b / nseg)-th block of
// source (b % nseg + b / nseg) % nseg.  K8's plain b % nseg, with workgroups dealt round-robin over
// the 8 XCDs, gives each of 8 sources to one XCD, and the largest source then sets the time: the
// Llama-70B shard table cut into 8 sources took 0.51 ms that way with the grid cap lifted, against
// 0.36 ms cut into 7 (profiles/shard_collective/).  The rotation spreads every source over all
// XCDs (0.45 ms for the 8).  The default grid is K8's 512 blocks: the gather runs beside the next
// round's decode kernels, which are occupancy-bound (see xgmi.hip).  A tile that holds the boundary
// between two sources is visited by a block of each; a vector is written only by the block whose
// source the vector's entry names.
//
// Memory: bulk loads and all stores are non-temporal, as K8's (a slice is written once and not
// re-read; a scratch is read once per round).  Per lane 4 output vectors are resolved, then loaded
// together: 8 x 16 B in flight when the source is misaligned to the output (two loads per vector),
// 4 x 16 B when it is aligned.  K8 keeps 8 always; this kernel stays at 4 vectors because each
// carries its run state (pointer, bytes left, run size, stride) through the loads: at 4 it takes 116
// VGPRs (4 waves per SIMD, no scratch), and 8 vectors were not tried.  Under the default cap
// 512 blocks x 256 lanes x 64 B = 8 MiB are still in flight in the aligned case, above the
// bandwidth-delay product of 7 links (~350 GB/s x a few us = a few MB); whether that suffices on
// real links is unmeasured.
//
// Visibility: there is no hand-off inside the kernel.  A scratch is written by the owner's pull
// kernels, the owner synchronises its device, the ranks meet in a host barrier, and only then is
// this kernel launched; the owner overwrites its scratch only after a second host barrier that
// follows every reader's stream synchronise.  Data crosses between devices at kernel boundaries
// only.  No run across two devices has checked this kernel: it has run with every source on one
// GPU (ranks sharing a device); shard_pull's cross_check compares it with the send path.
#include <hip/hip_runtime.h>

#include "zgpu.h"

namespace {

typedef uint32_t v4u __attribute__((ext_vector_type(4)));

constexpr uint32_t kThreads = 256;
constexpr uint32_t kVecPerLane = 4;
constexpr uint32_t kTile = kThreads * kVecPerLane * 16;  // arena bytes per tile
constexpr uint32_t kCache = 256;                         // entry ends cached in LDS per tile
constexpr uint32_t kDefaultBlocks = 512;                 // K8's default grid

__global__ void __launch_bounds__(kThreads) k_slice_gather_peers(ZgSliceSrcs s, const uint64_t* __restrict__ tab,
                                                                 uint32_t n, uint8_t* __restrict__ dst,
                                                                 uint32_t blocks_per_seg) {
  __shared__ uint64_t s_end[kCache];
  __shared__ uint64_t s_fld[5][kCache];  // src_off, run_bytes, src_stride, dst_off, source of the cached entries
  const uint64_t* __restrict__ t_end = tab + uint64_t(ZG_SLICE_DST_END) * n;
  const uint32_t tid = threadIdx.x;
  const uint32_t sb = blockIdx.x / uint32_t(s.nseg);
  const uint32_t seg = (blockIdx.x % uint32_t(s.nseg) + sb) % uint32_t(s.nseg);  // rotated: see the header
  const uint64_t lo = s.lo[seg], hi = s.hi[seg];
  if (hi <= lo) return;  // a source without output
  const uint8_t* __restrict__ src = reinterpret_cast<const uint8_t*>(s.src[seg]);

  for (uint64_t tile = lo / kTile + sb; tile * kTile < hi; tile += blocks_per_seg) {
    const uint64_t t0 = tile * kTile;  // arena offset of the tile's first byte
    // c0 = first entry with dst_end > t0 (n: none), 256 probes per round; a, b stay block-uniform.
    // Every iteration passes at least one barrier here before it rewrites the LDS cache.
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
    if (m == 0) break;                                     // past the last entry (not reached: t0 < hi)
    if (tid < m) s_end[tid] = t_end[c0 + tid];
    __syncthreads();
    // A vector of this tile can only map to a cached entry whose predecessor ends inside the tile.
    if (tid < m && (tid == 0 || s_end[tid - 1] < t0 + kTile)) {
      s_fld[0][tid] = tab[uint64_t(ZG_SLICE_SRC_OFF) * n + c0 + tid];
      s_fld[1][tid] = tab[uint64_t(ZG_SLICE_RUN_BYTES) * n + c0 + tid];
      s_fld[2][tid] = tab[uint64_t(ZG_SLICE_SRC_STRIDE) * n + c0 + tid];
      s_fld[3][tid] = tab[uint64_t(ZG_SLICE_DST_OFF) * n + c0 + tid];
      s_fld[4][tid] = tab[uint64_t(ZG_SLICE_SRC) * n + c0 + tid];
    }
    __syncthreads();
    const uint64_t cached_end = s_end[m - 1];

    // Pass 1: where each of the lane's vectors reads.  kind 0: nothing to write (padding, another
    // source's entry, or outside this source's range); 1: 16 bytes of one run (bulk); 2: a run
    // crossing or the entry's tail (edge).
    const uint8_t* sp[kVecPerLane];
    uint64_t left[kVecPerLane], rbs[kVecPerLane], skip[kVecPerLane];
    uint32_t nbs[kVecPerLane], kind[kVecPerLane];
#pragma unroll
    for (uint32_t j = 0; j < kVecPerLane; ++j) {
      const uint64_t p = t0 + (uint64_t(j) * kThreads + tid) * 16;  // arena offset of this vector
      kind[j] = 0;
      if (p >= hi) continue;
      uint64_t de, ds, rb, stride, so, who;
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
        who = s_fld[4][l];
      } else {  // more entries in the tile than the cache holds; p < hi <= dst_end[n - 1]
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
        who = tab[uint64_t(ZG_SLICE_SRC) * n + l];
      }
      if (ds > p || who != seg) continue;  // padding, or the neighbouring source's side of a shared tile
      const uint64_t q = p - ds;           // output byte index within the entry
      uint64_t run, within;
      if (de - ds <= rb) {
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

    // Pass 2: every bulk vector's aligned loads, issued together.
    v4u x[kVecPerLane], y[kVecPerLane];
#pragma unroll
    for (uint32_t j = 0; j < kVecPerLane; ++j) {
      if (kind[j] != 1) continue;
      const uint64_t sa = reinterpret_cast<uint64_t>(sp[j]);
      const uint32_t k = uint32_t(sa & 15);
      const v4u* v = reinterpret_cast<const v4u*>(sa - k);
      x[j] = __builtin_nontemporal_load(v);
      y[j] = x[j];
      if (k) y[j] = __builtin_nontemporal_load(v + 1);  // v[1] holds bytes of the run only when k > 0
    }

    // Pass 3: funnel and store; edge vectors byte by byte.
#pragma unroll
    for (uint32_t j = 0; j < kVecPerLane; ++j) {
      if (kind[j] == 0) continue;
      uint8_t* o = dst + t0 + (uint64_t(j) * kThreads + tid) * 16;
      if (kind[j] == 1) {
        const uint32_t k = uint32_t(reinterpret_cast<uint64_t>(sp[j]) & 15);
        const v4u xx = x[j], yy = y[j];
        uint32_t t[5];
        switch (k >> 2) {
          case 0: t[0] = xx.x; t[1] = xx.y; t[2] = xx.z; t[3] = xx.w; t[4] = yy.x; break;
          case 1: t[0] = xx.y; t[1] = xx.z; t[2] = xx.w; t[3] = yy.x; t[4] = yy.y; break;
          case 2: t[0] = xx.z; t[1] = xx.w; t[2] = yy.x; t[3] = yy.y; t[4] = yy.z; break;
          default: t[0] = xx.w; t[1] = yy.x; t[2] = yy.y; t[3] = yy.z; t[4] = yy.w; break;
        }
        const uint32_t kb = k & 3;
        v4u w;
        w.x = __builtin_amdgcn_alignbyte(t[1], t[0], kb);
        w.y = __builtin_amdgcn_alignbyte(t[2], t[1], kb);
        w.z = __builtin_amdgcn_alignbyte(t[3], t[2], kb);
        w.w = __builtin_amdgcn_alignbyte(t[4], t[3], kb);
        __builtin_nontemporal_store(w, reinterpret_cast<v4u*>(o));
        continue;
      }
      const uint8_t* e = sp[j];
      const uint32_t nb = nbs[j];
      uint64_t lf = left[j];
      uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
      for (uint32_t i = 0; i < 16; ++i) {
        if (i >= nb) continue;
        if (lf == 0) {  // next run
          e += skip[j];
          lf = rbs[j];
        }
        w[i >> 2] |= uint32_t(__builtin_nontemporal_load(e)) << (8 * (i & 3));
        ++e;
        --lf;
      }
      if (nb == 16) {
        v4u ww;
        ww.x = w[0]; ww.y = w[1]; ww.z = w[2]; ww.w = w[3];
        __builtin_nontemporal_store(ww, reinterpret_cast<v4u*>(o));
      } else {
#pragma unroll
        for (uint32_t i = 0; i < 16; ++i)
          if (i < nb) __builtin_nontemporal_store(uint8_t(w[i >> 2] >> (8 * (i & 3))), o + i);
      }
    }
  }
}

}  // namespace

extern "C" hipError_t zg_slice_gather_peers(const ZgSliceSrcs* srcs, const uint64_t* table, uint32_t n,
                                            uint64_t dst_total, uint8_t* dst, uint32_t max_blocks, hipStream_t stream) {
  if (n == 0 || dst_total == 0 || srcs->nseg <= 0) return hipSuccess;
  if (srcs->nseg > kZgMaxPeerSegs || !table || !dst || (reinterpret_cast<uintptr_t>(dst) & 15))
    return hipErrorInvalidValue;
  uint64_t max_tiles = 0;
  for (int i = 0; i < srcs->nseg; ++i) {
    const uint64_t lo = srcs->lo[i], hi = srcs->hi[i];
    if (hi <= lo) continue;
    if (hi > dst_total || !srcs->src[i]) return hipErrorInvalidValue;
    const uint64_t tiles = (hi + kTile - 1) / kTile - lo / kTile;
    if (tiles > max_tiles) max_tiles = tiles;
  }
  if (max_tiles == 0) return hipSuccess;
  // K8's grid rule: at most max_blocks blocks in all (default 512, about 2 per CU), at least one
  // per source; a block loops over its source's tiles.
  const uint64_t total = max_blocks ? max_blocks : kDefaultBlocks;
  uint64_t bps = max_tiles;
  const uint64_t cap = total / uint64_t(srcs->nseg);
  if (bps > cap) bps = cap;
  if (bps < 1) bps = 1;
  if (bps * uint64_t(srcs->nseg) > 0x7FFFFFFFull) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_slice_gather_peers, dim3(uint32_t(bps) * uint32_t(srcs->nseg)), dim3(kThreads), 0, stream,
                     *srcs, table, n, dst, uint32_t(bps));
  return hipGetLastError();
}
