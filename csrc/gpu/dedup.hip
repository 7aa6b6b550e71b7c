// K13 chunk dedup: a hash join over 32-byte chunk hashes that already sit in device memory (gfx950).
//
// Rows 0 .. m are the index's hashes (what the swarm already has), rows m .. m + n the fresh ones of
// the files being published; the two arrive as two pointers, so a persistent index is never
// concatenated.  first[j] = the smallest row r' <= m + j whose 32 bytes equal fresh row j's: a value
// below m names an index row, the value m + j says fresh row j is the first of its kind.  The result
// is a pure function of the keys.
//
// The table is open addressing with linear probing over uint32 row ids in caller-owned memory:
// zg_dedup_slots(rows) slots, the next power of two >= 2 * rows and at least 64 (load factor <= 0.5,
// so every probe walk ends at an empty slot or at its key).  A row's home slot is the little-endian
// u64 of key bytes 0 .. 8 masked to the table: the keys are BLAKE3 outputs and need no mixing.  Both
// are part of the contract (tests steer collisions with them).
//
// Three launches on one stream, no grid barrier, no fence:
//   fill   every slot = kEmpty.
//   build  one lane per row.  CAS the row id into the slot if it is empty; if it is occupied, compare
//          all 32 bytes with the occupant's key: equal -> atomicMin the row id into the slot and stop,
//          different -> next slot.  A slot's key never changes once claimed (only its row id falls,
//          and only to rows with the same key), and a claimed slot is never vacated, so comparing
//          with whichever occupant the lane reads is safe, and every lane of one key stops at the
//          same slot: the first one on their common walk that was not taken by another key.
//   probe  one lane per fresh row: walk to the slot whose occupant's key equals the row's and write
//          that slot's row id, by then the minimum over the key's rows.
// The table holds row ids only; keys are read from the inputs, which no launch writes, so relaxed
// agent-scope atomics suffice: nothing is published through the table but the ids themselves.
#include <hip/hip_runtime.h>

#include "zgpu.h"

namespace {

constexpr uint32_t kThreads = 256;
constexpr uint32_t kEmpty = 0xFFFFFFFFu;  // no row id: rows < 2^31

struct Key {
  uint4 lo, hi;
};

// Row r of the concatenation (index rows, then fresh rows): two 16-byte loads.
__device__ __forceinline__ Key load_key(const uint4* __restrict__ index, const uint4* __restrict__ fresh, uint32_t m,
                                        uint32_t r) {
  const uint4* p = r < m ? index + 2 * uint64_t(r) : fresh + 2 * uint64_t(r - m);
  return Key{p[0], p[1]};
}

__device__ __forceinline__ bool same(const Key& a, const Key& b) {
  return ((a.lo.x ^ b.lo.x) | (a.lo.y ^ b.lo.y) | (a.lo.z ^ b.lo.z) | (a.lo.w ^ b.lo.w) | (a.hi.x ^ b.hi.x) |
          (a.hi.y ^ b.hi.y) | (a.hi.z ^ b.hi.z) | (a.hi.w ^ b.hi.w)) == 0;
}

__device__ __forceinline__ uint32_t home_slot(const Key& k, uint32_t mask) {
  return uint32_t((uint64_t(k.lo.y) << 32 | k.lo.x) & mask);  // slots <= 2^32: the mask keeps low bits only
}

__global__ void __launch_bounds__(kThreads) k_dedup_fill(uint4* __restrict__ table, uint64_t n_vec) {
  const uint64_t i = uint64_t(blockIdx.x) * kThreads + threadIdx.x;
  if (i < n_vec) table[i] = make_uint4(kEmpty, kEmpty, kEmpty, kEmpty);
}

__global__ void __launch_bounds__(kThreads) k_dedup_build(const uint4* __restrict__ index,
                                                          const uint4* __restrict__ fresh, uint32_t m, uint32_t rows,
                                                          uint32_t* __restrict__ table, uint32_t mask) {
  const uint64_t g = uint64_t(blockIdx.x) * kThreads + threadIdx.x;
  if (g >= rows) return;
  const uint32_t r = uint32_t(g);
  const Key k = load_key(index, fresh, m, r);
  uint32_t s = home_slot(k, mask);
  for (;;) {
    uint32_t cur = __hip_atomic_load(table + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (cur == kEmpty) {
      if (__hip_atomic_compare_exchange_strong(table + s, &cur, r, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                               __HIP_MEMORY_SCOPE_AGENT))
        return;  // claimed; on failure cur is the row that won the slot
    }
    if (same(k, load_key(index, fresh, m, cur))) {
      if (r < cur) __hip_atomic_fetch_min(table + s, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      return;
    }
    s = (s + 1) & mask;
  }
}

__global__ void __launch_bounds__(kThreads) k_dedup_probe(const uint4* __restrict__ index,
                                                          const uint4* __restrict__ fresh, uint32_t m, uint32_t n,
                                                          const uint32_t* __restrict__ table, uint32_t mask,
                                                          int64_t* __restrict__ first) {
  const uint64_t g = uint64_t(blockIdx.x) * kThreads + threadIdx.x;
  if (g >= n) return;
  const uint32_t r = m + uint32_t(g);
  const Key k = load_key(index, fresh, m, r);
  uint32_t s = home_slot(k, mask);
  for (;;) {
    const uint32_t cur = table[s];
    // cur == kEmpty cannot happen after a build over the same rows; stop instead of reading row 2^32 - 1
    if (cur == r || cur == kEmpty || same(k, load_key(index, fresh, m, cur))) {
      first[g] = cur == kEmpty ? int64_t(r) : int64_t(cur);
      return;
    }
    s = (s + 1) & mask;
  }
}

}  // namespace

extern "C" uint64_t zg_dedup_slots(uint64_t rows) {
  uint64_t s = 64;
  while (s < 2 * rows) s <<= 1;
  return s;
}

extern "C" size_t zg_dedup_table_bytes(uint64_t rows) { return size_t(zg_dedup_slots(rows)) * sizeof(uint32_t); }

extern "C" hipError_t zg_dedup_chunks(const uint8_t* index, uint32_t m, const uint8_t* fresh, uint32_t n,
                                      uint32_t* table, size_t table_bytes, int64_t* first, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  const uint64_t rows = uint64_t(m) + n;
  if (rows >= (1ull << 31)) return hipErrorInvalidValue;
  if (!fresh || !table || !first || (m && !index)) return hipErrorInvalidValue;
  const auto addr = [](const void* p) { return reinterpret_cast<uintptr_t>(p); };
  if ((addr(index) | addr(fresh) | addr(table)) & 15) return hipErrorInvalidValue;
  if (addr(first) & 7) return hipErrorInvalidValue;
  const uint64_t slots = zg_dedup_slots(rows);
  if (table_bytes < slots * sizeof(uint32_t)) return hipErrorInvalidValue;
  const uint32_t mask = uint32_t(slots - 1);
  const uint64_t n_vec = slots / 4;  // slots is a multiple of 64
  const uint4* ix = reinterpret_cast<const uint4*>(index);
  const uint4* fr = reinterpret_cast<const uint4*>(fresh);
  hipLaunchKernelGGL(k_dedup_fill, dim3(uint32_t((n_vec + kThreads - 1) / kThreads)), dim3(kThreads), 0, stream,
                     reinterpret_cast<uint4*>(table), n_vec);
  hipLaunchKernelGGL(k_dedup_build, dim3(uint32_t((rows + kThreads - 1) / kThreads)), dim3(kThreads), 0, stream, ix,
                     fr, m, uint32_t(rows), table, mask);
  hipLaunchKernelGGL(k_dedup_probe, dim3(uint32_t((uint64_t(n) + kThreads - 1) / kThreads)), dim3(kThreads), 0,
                     stream, ix, fr, m, n, table, mask, first);
  return hipGetLastError();
}
