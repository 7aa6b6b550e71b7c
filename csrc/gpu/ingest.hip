// Xorb ingest kernels for MI355X (gfx950, CDNA4, wave64): index -> place (copy / LZ4 decode)
// -> hash.  SURVEY §2.G K1 (BLAKE3 chunk hashes), K3 (LZ4/BG4 decode), K4 (header walk + fused
// ingest).  Host oracle: csrc/core/{xorb,lz4,blake3}.cpp.
//
// Buffers handed to these kernels must be padded by >= 4 KiB past their logical end: the
// alignment-fixing loads read whole aligned dwords (and the LZ4 parse reads 8 bytes at a time).
#include <hip/hip_runtime.h>

#include "blake3_dev.h"
#include "wave64.h"
#include "zgpu.h"

namespace {

constexpr int kWave = 64;
constexpr int kWavesPerBlock = 4;
using zwv::kMaxChunk;
using zwv::lane_id;
using zwv::report;

__device__ __forceinline__ int wave_uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }

// Load 8 bytes at an arbitrary address as two little-endian words (reads aligned dwords).
__device__ __forceinline__ void load8(const uint8_t* p, uint32_t& lo, uint32_t& hi) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(p);
  const uint32_t k = uint32_t(a & 3);
  const uint32_t* w = reinterpret_cast<const uint32_t*>(a & ~uintptr_t(3));
  const uint32_t w0 = w[0], w1 = w[1];
  if (k == 0) {
    lo = w0;
    hi = w1;
  } else {
    const uint32_t w2 = w[2];
    lo = __builtin_amdgcn_alignbyte(w1, w0, k);
    hi = __builtin_amdgcn_alignbyte(w2, w1, k);
  }
}

// --------------------------------------------------------------------------------------------
// K4a: header walk.  One thread per fetched run; sequential by construction (chunk i+1's header
// position depends on chunk i's compressed length), parallel across runs.
// --------------------------------------------------------------------------------------------
// The walk of one run: `hdr(off, lo, hi)` yields the 8 header bytes at run offset `off` (a global
// load, or a lookup in a table the scan below built).  On any error the remaining descriptors of
// the term are written as empty no-ops so later kernels never dereference garbage.
template <class Hdr>
__device__ __forceinline__ void walk_term(const ZgTerm& tm, int t, ZgChunk* __restrict__ chunks, unsigned long long* err,
                                          const Hdr& hdr) {
  uint64_t off = 0, uoff = 0;
  auto fail = [&](uint32_t code, uint32_t from) {
    report(err, code, uint32_t(t));
    ZgChunk z{0, 0, 0, 0, 0, uint32_t(t)};
    for (uint32_t k = from; k < tm.n_chunks; ++k) chunks[tm.chunk_base + k] = z;
  };
  for (uint32_t c = 0; c < tm.n_chunks; ++c) {
    if (off + 8 > tm.src_len) {
      fail(ZG_ERR_COUNT, c);
      return;
    }
    uint32_t lo, hi;
    hdr(off, lo, hi);
    const uint32_t version = lo & 0xFF;
    const uint32_t clen = lo >> 8;
    const uint32_t scheme = hi & 0xFF;
    const uint32_t ulen = hi >> 8;
    if (version != 0 || scheme > 2 || (scheme == 0 && clen != ulen)) {
      fail(ZG_ERR_HEADER, c);
      return;
    }
    if (off + 8 + clen > tm.src_len || (tm.ulen != 0 && uoff + ulen > tm.ulen)) {
      fail(ZG_ERR_RANGE, c);
      return;
    }
    if (ulen > kMaxChunk) {
      fail(ZG_ERR_CAPACITY, c);
      return;
    }
    ZgChunk ch;
    ch.src = tm.src + off + 8;
    ch.dst = tm.dst + uoff;
    ch.clen = clen;
    ch.ulen = ulen;
    ch.scheme = scheme;
    ch.term = uint32_t(t);
    chunks[tm.chunk_base + c] = ch;
    off += 8 + clen;
    uoff += ulen;
  }
  if (off != tm.src_len || (tm.ulen != 0 && uoff != tm.ulen)) report(err, ZG_ERR_COUNT, uint32_t(t));
}

struct GlobalHdr {
  const uint8_t* p;
  __device__ __forceinline__ void operator()(uint64_t off, uint32_t& lo, uint32_t& hi) const { load8(p + off, lo, hi); }
};

__global__ void k_index_terms(const uint8_t* __restrict__ src, const ZgTerm* __restrict__ terms, int n_terms,
                              ZgChunk* __restrict__ chunks, unsigned long long* err) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_terms) return;
  const ZgTerm tm = terms[t];
  walk_term(tm, t, chunks, err, GlobalHdr{src + tm.src});
}

// K4a': parallel header walk ("scan, sort, link").  The walk above is one dependent HBM load per
// chunk: ~1000 chained loads per 64 MiB xorb run, ~0.6 ms whatever the GPU's width.  Here:
//   scan   every byte position of the span is tested in parallel for a plausible chunk header
//          (version 0, scheme <= 2, 1 <= ulen <= 128 KiB, clen >= 1, raw => clen == ulen, payload
//          inside its run, a compressed payload starting with the LZ4 frame magic); candidates
//          (one per chunk, plus a few look-alikes per 256 MiB) are appended to their term's list.
//   link   one workgroup per term sorts its candidates in LDS (bitonic), picks the chain from
//          offset 0 to the run's end out of them (successor lookups, see k_hdr_link) and checks
//          it has n_chunks links; block prefix sums give every chunk's index and output offset and
//          the records are written in parallel.
// Anything else -- a list over capacity, a broken, ambiguous or short chain -- falls back to the
// serial walk for that term, so records and error codes are exactly walk_term's.
constexpr int kScanThreads = 256;
// 64 positions per thread from 80 loaded bytes (5 x 16 B): 1.25 loads per position byte instead of
// 2 with 16 positions from 32 bytes
constexpr uint32_t kScanBytesPerThread = 64;
constexpr uint32_t kScanWords = (kScanBytesPerThread + 16) / 4;
constexpr uint32_t kCandCap = 8192;  // chunks of a 64 MiB xorb at the 8 KiB CDC minimum
constexpr int kLinkThreads = 1024;

// `pay`: the 4 bytes after the header.  A compressed chunk's payload is an LZ4 frame, so it starts
// with the frame magic: without that test the LZ4 streams of BG4 bf16 weights (zero bytes every few
// bytes) produced millions of header-like candidates and the scan lost to the serial walk.
constexpr uint32_t kLz4Magic = 0x184D2204u;
__device__ __forceinline__ bool plausible_header(uint32_t lo, uint32_t hi, uint32_t pay, uint64_t rel,
                                                 uint64_t run_len) {
  const uint32_t clen = lo >> 8, scheme = hi & 0xFF, ulen = hi >> 8;
  return (lo & 0xFF) == 0 && scheme <= 2 && ulen >= 1 && ulen <= kMaxChunk && clen >= 1 &&
         (scheme == 0 ? clen == ulen : pay == kLz4Magic) && rel + 8 + clen <= run_len;
}

// terms must be sorted by src (else the fast path finds no chain and the serial walk runs)
__global__ void __launch_bounds__(kScanThreads) k_hdr_scan(const uint8_t* __restrict__ src, uint64_t src_n,
                                                          const ZgTerm* __restrict__ terms, int n_terms,
                                                          uint32_t* __restrict__ counts, uint32_t* __restrict__ cands) {
  const uint64_t q = (uint64_t(blockIdx.x) * kScanThreads + threadIdx.x) * kScanBytesPerThread;
  if (q >= src_n) return;
  // the last term starting at or before q (binary search; terms are few)
  int lo_t = 0, hi_t = n_terms - 1, t = -1;
  while (lo_t <= hi_t) {
    const int mid = (lo_t + hi_t) >> 1;
    if (terms[mid].src <= q) {
      t = mid;
      lo_t = mid + 1;
    } else {
      hi_t = mid - 1;
    }
  }
  if (t < 0) {
    t = 0;  // q lies before the first term: positions below terms[0].src are skipped
  }
  uint64_t t0 = terms[t].src, t1 = t0 + terms[t].src_len;
  uint64_t nx = t + 1 < n_terms ? terms[t + 1].src : ~uint64_t(0);
  uint32_t w[kScanWords];
#pragma unroll
  for (uint32_t i = 0; i < kScanWords / 4; ++i) {  // padded buffers: safe past the end
    const uint4 v = *reinterpret_cast<const uint4*>(src + q + 16 * i);
    w[4 * i] = v.x;
    w[4 * i + 1] = v.y;
    w[4 * i + 2] = v.z;
    w[4 * i + 3] = v.w;
  }
#pragma unroll
  for (uint32_t k = 0; k < kScanBytesPerThread; ++k) {
    const uint64_t p = q + k;
    while (p >= nx) {  // crossed into the next term (wave-divergent, rare)
      ++t;
      t0 = terms[t].src;
      t1 = t0 + terms[t].src_len;
      nx = t + 1 < n_terms ? terms[t + 1].src : ~uint64_t(0);
    }
    if (p < t0 || p + 8 > t1) continue;
    const uint32_t j = k >> 2, sh = k & 3;
    const uint32_t lo = sh ? __builtin_amdgcn_alignbyte(w[j + 1], w[j], sh) : w[j];
    const uint32_t hi = sh ? __builtin_amdgcn_alignbyte(w[j + 2], w[j + 1], sh) : w[j + 1];
    const uint32_t pay = sh ? __builtin_amdgcn_alignbyte(w[j + 3], w[j + 2], sh) : w[j + 2];
    if (plausible_header(lo, hi, pay, p - t0, t1 - t0)) {
      const uint32_t i = atomicAdd(&counts[t], 1u);
      if (i < kCandCap) cands[uint64_t(t) * kCandCap + i] = uint32_t(p - t0);
    }
  }
}

// Link.  The candidates are sorted, then every candidate's successor (its offset + 8 + clen) is
// looked up among them.  False candidates do occur: LZ4 streams of BG4 bf16 weights hold a few
// raw-header look-alikes ([00 x y z 00 x y z], clen == ulen) per 256 MiB, so demanding exactly
// n_chunks candidates sent every term of a 256 MiB batch back to the serial walk.  The chain is
// instead picked out of the candidate set G' = {candidates with a successor (a candidate, or the
// run's end) that sit at offset 0 or are some candidate's successor}.  G' is accepted when
//   (a) it contains offset 0,
//   (b) it is closed under the successor (a member's successor is a member, or the run's end),
//   (c) every member other than offset 0 is the successor of a MEMBER (kChain), and
//   (d) it has n_chunks members whose sizes add up to the term's ulen (when that is given).
// Then G' is exactly the chain from offset 0: a successor lies strictly behind its candidate, so by
// (c) every member leads back through members at ever smaller offsets, which can only stop at
// offset 0; a candidate has one successor, so the forward path from 0 is unique and every member
// lies on it; and by (a) and (b) that path stays in G' until it hits the run's end.  (Without (c) a
// look-alike outside G' could put its successor Y into G': Y is pointed at, though not from the
// chain, and made up the count of a run one chunk short of the plan.)  Every member passed
// plausible_header, which implies walk_term's header, range and capacity checks, so with (d) the
// serial walk would write these very records and report nothing.  Otherwise -- and for a chain
// holding a chunk the scan does not list, such as a raw chunk of zero bytes -- the serial walk
// decides: records and error codes are walk_term's in every case.
constexpr uint32_t kEnd = 0xFFFFFFFEu, kNone = 0xFFFFFFFFu;
// flags in cs[] above clen (24 bits) and the scheme (2 bits)
constexpr uint32_t kPointed = 1u << 31, kGood = 1u << 30, kChain = 1u << 29;
constexpr uint32_t kFellBack = 1u << 31;  // in counts[t] after the link: term t took the serial walk

__device__ __forceinline__ uint32_t lds_find(const uint32_t* key, uint32_t n, uint32_t v) {
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (key[mid] < v) lo = mid + 1;
    else hi = mid;
  }
  return lo < n && key[lo] == v ? lo : kNone;
}

__global__ void __launch_bounds__(kLinkThreads) k_hdr_link(const uint8_t* __restrict__ src,
                                                          const ZgTerm* __restrict__ terms,
                                                          uint32_t* __restrict__ counts,  // kFellBack marks a serial-walk term
                                                          const uint32_t* __restrict__ cands,
                                                          ZgChunk* __restrict__ chunks, unsigned long long* err) {
  __shared__ uint32_t key[kCandCap];   // candidate offsets, sorted
  __shared__ uint32_t ul[kCandCap];    // uncompressed sizes
  __shared__ uint32_t cs[kCandCap];    // clen | scheme << 24 | kPointed | kGood
  __shared__ uint32_t nx[kCandCap];    // index of the successor candidate, kEnd or kNone
  __shared__ uint32_t part_n[kLinkThreads / kWave];
  __shared__ uint32_t part_u[kLinkThreads / kWave];
  __shared__ int ok;
  const int t = blockIdx.x;
  const ZgTerm tm = terms[t];
  const uint32_t n = counts[t];
  const int tid = threadIdx.x;
  // the fast path needs at least one candidate per planned chunk (terms of at most 4 GiB)
  if (n < tm.n_chunks || n == 0 || n > kCandCap || tm.src_len >= (uint64_t(1) << 32)) {
    if (tid == 0) {
      counts[t] = n | kFellBack;
      walk_term(tm, t, chunks, err, GlobalHdr{src + tm.src});
    }
    return;
  }
  uint32_t P = 1;
  while (P < n) P <<= 1;
  for (uint32_t i = tid; i < P; i += kLinkThreads) key[i] = i < n ? cands[uint64_t(t) * kCandCap + i] : 0xFFFFFFFFu;
  if (tid == 0) ok = 1;
  __syncthreads();
  for (uint32_t k = 2; k <= P; k <<= 1) {  // bitonic sort, ascending
    for (uint32_t jj = k >> 1; jj > 0; jj >>= 1) {
      for (uint32_t i = tid; i < P; i += kLinkThreads) {
        const uint32_t l = i ^ jj;
        if (l > i) {
          const uint32_t a = key[i], b = key[l];
          if (((i & k) == 0) == (a > b)) {
            key[i] = b;
            key[l] = a;
          }
        }
      }
      __syncthreads();
    }
  }
  // successors
  const uint8_t* run = src + tm.src;
  for (uint32_t i = tid; i < n; i += kLinkThreads) {
    uint32_t lo, hi;
    load8(run + key[i], lo, hi);
    const uint32_t clen = lo >> 8;
    const uint64_t end = uint64_t(key[i]) + 8 + clen;
    nx[i] = end == tm.src_len ? kEnd : end < tm.src_len ? lds_find(key, n, uint32_t(end)) : kNone;
    ul[i] = hi >> 8;
    cs[i] = clen | (hi & 0xFF) << 24;
  }
  __syncthreads();
  for (uint32_t i = tid; i < n; i += kLinkThreads)
    if (nx[i] < n) atomicOr(&cs[nx[i]], kPointed);
  __syncthreads();
  for (uint32_t i = tid; i < n; i += kLinkThreads)
    if (nx[i] != kNone && (key[i] == 0 || (cs[i] & kPointed))) atomicOr(&cs[i], kGood);
  __syncthreads();
  for (uint32_t i = tid; i < n; i += kLinkThreads)  // successors of members
    if ((cs[i] & kGood) && nx[i] < n) atomicOr(&cs[nx[i]], kChain);
  __syncthreads();
  for (uint32_t i = tid; i < n; i += kLinkThreads) {
    if (!(cs[i] & kGood)) continue;
    if (nx[i] != kEnd && !(cs[nx[i]] & kGood)) ok = 0;  // closed under the successor
    if (key[i] != 0 && !(cs[i] & kChain)) ok = 0;       // reached from a member
  }
  if (tid == 0 && (key[0] != 0 || !(cs[0] & kGood))) ok = 0;
  // exclusive prefix sums (chunk count, uncompressed bytes) over the chain members: each thread
  // owns a contiguous slice, then a wave scan and the wave totals
  const uint32_t per = (n + kLinkThreads - 1) / kLinkThreads;
  const uint32_t a = min(n, tid * per), b = min(n, a + per);
  uint32_t cnt = 0, sum = 0;
  for (uint32_t i = a; i < b; ++i)
    if (cs[i] & kGood) {
      ++cnt;
      sum += ul[i];
    }
  uint32_t inc_n = cnt, inc_u = sum;
#pragma unroll
  for (int d = 1; d < kWave; d <<= 1) {
    const uint32_t yn = __shfl_up(inc_n, d, kWave), yu = __shfl_up(inc_u, d, kWave);
    if (int(lane_id()) >= d) {
      inc_n += yn;
      inc_u += yu;
    }
  }
  const int wv = tid / kWave;
  if (lane_id() == kWave - 1) {
    part_n[wv] = inc_n;
    part_u[wv] = inc_u;
  }
  __syncthreads();
  if (tid == 0) {
    uint32_t rn = 0, ru = 0;
    for (int k = 0; k < kLinkThreads / kWave; ++k) {
      const uint32_t xn = part_n[k], xu = part_u[k];
      part_n[k] = rn;
      part_u[k] = ru;
      rn += xn;
      ru += xu;
    }
    if (rn != tm.n_chunks || (tm.ulen != 0 && ru != tm.ulen)) ok = 0;
  }
  __syncthreads();
  if (!ok) {  // a broken or ambiguous chain: the serial walk decides
    if (tid == 0) {
      counts[t] = n | kFellBack;
      walk_term(tm, t, chunks, err, GlobalHdr{src + tm.src});
    }
    return;
  }
  uint32_t c = part_n[wv] + inc_n - cnt;  // this slice's first chunk index
  uint32_t off = part_u[wv] + inc_u - sum;
  for (uint32_t i = a; i < b; ++i) {
    if (!(cs[i] & kGood)) continue;
    ZgChunk ch;
    ch.src = tm.src + key[i] + 8;
    ch.dst = tm.dst + off;
    ch.clen = cs[i] & 0xFFFFFF;
    ch.ulen = ul[i];
    ch.scheme = (cs[i] >> 24) & 0x3;
    ch.term = uint32_t(t);
    chunks[tm.chunk_base + c] = ch;
    ++c;
    off += ul[i];
  }
}

using zwv::wave_copy;  // wave64.h

// K3a: place uncompressed chunks (scheme 0): one wave per chunk, clipped to [clip_lo, clip_hi).
__global__ void __launch_bounds__(256) k_place_raw(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                   const ZgChunk* __restrict__ chunks, int n_chunks,
                                                   uint64_t clip_lo, uint64_t clip_hi, uint64_t src_n,
                                                   uint64_t dst_n) {
  const int c = wave_uniform(blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6));
  if (c >= n_chunks) return;
  const ZgChunk ch = chunks[c];
  if (ch.scheme != 0) return;
  if (ch.src + ch.ulen > src_n || ch.dst + ch.ulen > dst_n) return;
  const uint64_t lo = ch.dst > clip_lo ? ch.dst : clip_lo;
  const uint64_t end = ch.dst + ch.ulen;
  const uint64_t hi = end < clip_hi ? end : clip_hi;
  if (lo >= hi) return;
  wave_copy(dst + lo, src + ch.src + (lo - ch.dst), hi - lo, lane_id());
}

// --------------------------------------------------------------------------------------------
// K1: keyed BLAKE3 chunk hashes, latency path (launches without scratch; the leaf-flat pipeline
// in blake3_flat.hip is the throughput path).  One wave per Xet chunk (4 per 256-thread block);
// lane l owns BLAKE3 chunks l, l+64 (<= 128 for a 128 KiB Xet chunk); chaining values are merged
// pairwise in LDS (pairwise-with-carry == BLAKE3's left-complete tree).
// --------------------------------------------------------------------------------------------
using zg::store_hash;
using zg::wave_hash;

__global__ void __launch_bounds__(256) k_hash_chunks(const uint8_t* __restrict__ dst, const ZgChunk* __restrict__ chunks,
                                                     int n_chunks, uint8_t* __restrict__ hashes,
                                                     uint64_t* __restrict__ sizes, uint32_t hash_index_base,
                                                     uint64_t dst_n) {
  __shared__ uint32_t cvs_all[kWavesPerBlock][128 * 8];
  const int wid = threadIdx.x >> 6;
  const int c = wave_uniform(blockIdx.x * kWavesPerBlock + wid);
  if (c >= n_chunks) return;
  const uint32_t lane = lane_id();
  ZgChunk ch = chunks[c];
  if (ch.dst + ch.ulen > dst_n || ch.ulen > kMaxChunk) ch.ulen = 0, ch.dst = 0;
  uint32_t h[8];
  wave_hash(dst + ch.dst, ch.ulen, zg::kDataKeyW, zg::KEYED_HASH, cvs_all[wid], lane, h);
  const uint64_t idx = uint64_t(hash_index_base) + uint64_t(c);
  store_hash(hashes + 32 * idx, h, lane);
  if (sizes && lane == 0) sizes[idx] = ch.ulen;
}

__global__ void __launch_bounds__(256) k_hash_ranges(const uint8_t* __restrict__ buf, const uint64_t* __restrict__ offs,
                                                     const uint32_t* __restrict__ lens, int n, uint8_t* __restrict__ out,
                                                     int key_mode) {
  __shared__ uint32_t cvs_all[kWavesPerBlock][128 * 8];
  const int wid = threadIdx.x >> 6;
  const int c = wave_uniform(blockIdx.x * kWavesPerBlock + wid);
  if (c >= n) return;
  const uint32_t lane = lane_id();
  const uint32_t len = lens[c];
  uint32_t h[8];
  if (len > 128u * 1024u) {
    if (lane < 8) reinterpret_cast<uint32_t*>(out + 32 * size_t(c))[lane] = 0xFFFFFFFFu;
    return;
  }
  const zg::Key8& key = key_mode == 0 ? zg::kDataKeyW : key_mode == 1 ? zg::kNodeKeyW : key_mode == 2 ? zg::kIVW : zg::kZeroW;
  const uint32_t mode = key_mode == 2 ? 0u : zg::KEYED_HASH;
  wave_hash(buf + offs[c], len, key, mode, cvs_all[wid], lane, h);
  store_hash(out + 32 * size_t(c), h, lane);
}

__global__ void k_compare(const uint8_t* __restrict__ got, const uint8_t* __restrict__ want, int n,
                          unsigned long long* err) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint4* a = reinterpret_cast<const uint4*>(got + 32 * size_t(i));
  const uint4* b = reinterpret_cast<const uint4*>(want + 32 * size_t(i));
  const uint4 a0 = a[0], a1 = a[1], b0 = b[0], b1 = b[1];
  if (a0.x != b0.x || a0.y != b0.y || a0.z != b0.z || a0.w != b0.w || a1.x != b1.x || a1.y != b1.y ||
      a1.z != b1.z || a1.w != b1.w)
    report(err, ZG_ERR_HASH, uint32_t(i));
}

}  // namespace

extern "C" {

hipError_t zg_index_terms(const uint8_t* src, const ZgTerm* terms, int n_terms, ZgChunk* chunks,
                          unsigned long long* err, hipStream_t stream) {
  if (n_terms <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_index_terms, dim3((n_terms + 63) / 64), dim3(64), 0, stream, src, terms, n_terms, chunks, err);
  return hipGetLastError();
}

size_t zg_index_scratch_bytes(int n_terms) {
  return (size_t(n_terms) * 4 + 255) / 256 * 256 + size_t(n_terms) * kCandCap * 4;
}

hipError_t zg_index_terms_scan(const uint8_t* src, uint64_t src_n, const ZgTerm* terms, int n_terms, ZgChunk* chunks,
                               unsigned long long* err, uint8_t* scratch, size_t scratch_bytes, hipStream_t stream) {
  if (n_terms <= 0) return hipSuccess;
  if (scratch == nullptr || scratch_bytes < zg_index_scratch_bytes(n_terms) || (reinterpret_cast<uintptr_t>(src) & 15))
    return zg_index_terms(src, terms, n_terms, chunks, err, stream);
  uint32_t* counts = reinterpret_cast<uint32_t*>(scratch);
  uint32_t* cands = reinterpret_cast<uint32_t*>(scratch + (size_t(n_terms) * 4 + 255) / 256 * 256);
  hipError_t e = hipMemsetAsync(counts, 0, size_t(n_terms) * 4, stream);
  if (e != hipSuccess) return e;
  const uint64_t per_block = uint64_t(kScanThreads) * kScanBytesPerThread;
  const uint64_t blocks = (src_n + per_block - 1) / per_block;
  if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_hdr_scan, dim3(uint32_t(blocks ? blocks : 1)), dim3(kScanThreads), 0, stream, src, src_n, terms,
                     n_terms, counts, cands);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_hdr_link, dim3(n_terms), dim3(kLinkThreads), 0, stream, src, terms, counts, cands, chunks, err);
  return hipGetLastError();
}

hipError_t zg_place_chunks(const uint8_t* src, uint64_t src_n, uint8_t* dst, uint64_t dst_n, const ZgChunk* chunks,
                           int n_chunks, uint64_t clip_lo, uint64_t clip_hi, uint8_t* clip_scratch,
                           unsigned long long* err, hipStream_t stream) {
  if (n_chunks <= 0) return hipSuccess;
  const bool clipped = clip_lo > 0 || clip_hi < dst_n;
  if (clipped && clip_scratch == nullptr) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_place_raw, dim3((n_chunks + kWavesPerBlock - 1) / kWavesPerBlock), dim3(256), 0, stream, src,
                     dst, chunks, n_chunks, clip_lo, clip_hi, src_n, dst_n);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  if (!clipped) return zg_lz4_batched_decode(src, src_n, dst, dst_n, chunks, n_chunks, err, stream);
  return zg_lz4_decode_clipped(src, src_n, dst, dst_n, chunks, n_chunks, clip_lo, clip_hi, clip_scratch, err, stream);
}

hipError_t zg_hash_chunks(const uint8_t* dst, uint64_t dst_n, const ZgChunk* chunks, int n_chunks, uint8_t* hashes,
                          uint64_t* sizes, uint32_t hash_index_base, uint8_t* scratch, size_t scratch_bytes,
                          hipStream_t stream) {
  if (n_chunks <= 0) return hipSuccess;
  if (scratch)
    return zg_hash_chunks_flat(dst, dst_n, chunks, n_chunks, hashes + 32 * uint64_t(hash_index_base),
                               sizes ? sizes + hash_index_base : nullptr, scratch, scratch_bytes, stream);
  hipLaunchKernelGGL(k_hash_chunks, dim3((n_chunks + kWavesPerBlock - 1) / kWavesPerBlock), dim3(256), 0, stream, dst,
                     chunks, n_chunks, hashes, sizes, hash_index_base, dst_n);
  return hipGetLastError();
}

hipError_t zg_ingest_chunks(const uint8_t* src, uint64_t src_n, uint8_t* dst, uint64_t dst_n, const ZgChunk* chunks,
                            int n_chunks, int has_compressed, unsigned long long* err, uint8_t* hashes,
                            uint64_t* sizes, uint32_t hash_index_base, uint8_t* scratch, size_t scratch_bytes,
                            hipStream_t stream) {
  if (n_chunks <= 0) return hipSuccess;
  if (!scratch) return hipErrorInvalidValue;
  uint8_t* h = hashes + 32 * uint64_t(hash_index_base);
  uint64_t* sz = sizes ? sizes + hash_index_base : nullptr;
  int hashed = 0;  // the decoder hashed the compressed chunks itself (zg_lz4_decode_ingest)
  if (has_compressed) {
    // the hash scratch doubles as the BG4 staging of the decoder (which finishes before the place/hash
    // pass below uses it: one stream); zg_ingest_scratch_bytes sizes it for both
    const hipError_t e = zg_lz4_decode_ingest(src, src_n, dst, dst_n, chunks, n_chunks, err, h, sz, &hashed, scratch,
                                              scratch_bytes, stream);
    if (e != hipSuccess) return e;
  }
  if (hashed)
    return zg_place_hash_flat_raw(src, src_n, dst, dst_n, chunks, n_chunks, err, h, sz, scratch, scratch_bytes, stream);
  return zg_place_hash_flat(src, src_n, dst, dst_n, chunks, n_chunks, err, h, sz, scratch, scratch_bytes, stream);
}

hipError_t zg_hash_ranges(const uint8_t* buf, const uint64_t* offsets, const uint32_t* lens, int n, uint8_t* hashes,
                          int key_mode, uint8_t* scratch, size_t scratch_bytes, hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  if (scratch) return zg_hash_ranges_flat(buf, offsets, lens, n, hashes, key_mode, scratch, scratch_bytes, stream);
  hipLaunchKernelGGL(k_hash_ranges, dim3((n + kWavesPerBlock - 1) / kWavesPerBlock), dim3(256), 0, stream, buf, offsets,
                     lens, n, hashes, key_mode);
  return hipGetLastError();
}

hipError_t zg_compare_hashes(const uint8_t* got, const uint8_t* want, int n, unsigned long long* err,
                             hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_compare, dim3((n + 255) / 256), dim3(256), 0, stream, got, want, n, err);
  return hipGetLastError();
}

int zg_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

}  // extern "C"
