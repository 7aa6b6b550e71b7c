// Device-side descriptors and the C ABI of the zest HIP/CDNA4 kernel library (gfx950).
//
// Pipeline for one batch of fetched xorb ranges ("terms"):
//   zg_index_terms   one thread per term walks the 8-byte chunk headers -> ChunkDesc[]   (K4)
//   zg_place_chunks  one wave per chunk: scheme 0 -> aligned copy, LZ4/BG4 -> LDS decode (K3)
//   zg_hash_chunks   keyed BLAKE3 of the placed bytes -> chunk hashes (K1; lane per 1 KiB leaf)
//   zg_merkle_files  one workgroup per file: Xet Merkle tree -> root -> file hash compare (K2)
// plus zg_cdc_candidates (K5), zg_pack_xorbs (K7), zg_serve_pack (K9, seeding from decoded bytes) and
// synthetic data generators.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

// A fetched byte run holding whole chunks [chunk 0 .. n_chunks) of one xorb range.
typedef struct ZgTerm {
  uint64_t src;         // byte offset of the first chunk header in the src (staging) buffer
  uint64_t src_len;     // bytes in the run
  uint64_t dst;         // byte offset of the first chunk's output in the dst (arena) buffer
  uint32_t chunk_base;  // index of the first chunk in the ChunkDesc / hash arrays
  uint32_t n_chunks;    // chunks the run must contain
  uint64_t ulen;        // expected total uncompressed bytes (0 = don't check)
} ZgTerm;

typedef struct ZgChunk {
  uint64_t src;     // payload offset in src buffer (after the 8-byte header)
  uint64_t dst;     // output offset in dst buffer
  uint32_t clen;    // compressed payload length
  uint32_t ulen;    // uncompressed length
  uint32_t scheme;  // 0 none, 1 LZ4 frame, 2 BG4+LZ4 frame
  uint32_t term;    // owning term (for error reports)
} ZgChunk;

// One Merkle job: n leaves (hash[32] + size) -> root; optional expected file hash compare.
typedef struct ZgMerkleJob {
  uint64_t leaf_base;  // index of the first leaf in the hash/size arrays
  uint64_t n_leaves;
  uint32_t want_file_hash;  // 1: result = file hash (keyed zero-salt of root); 0: raw root
  uint32_t pad;
} ZgMerkleJob;

// Error word layout written by kernels (first error wins via atomicCAS):
//   code << 32 | index.  Codes:
enum {
  ZG_OK = 0,
  ZG_ERR_HEADER = 1,       // bad chunk header (version/scheme)
  ZG_ERR_RANGE = 2,        // chunk extends past its run
  ZG_ERR_COUNT = 3,        // run has a different chunk count / size than planned
  ZG_ERR_LZ4 = 4,          // malformed LZ4 frame / block
  ZG_ERR_SIZE = 5,         // decoded size != header ulen
  ZG_ERR_HASH = 6,         // hash mismatch
  ZG_ERR_CAPACITY = 7,     // chunk larger than kernel capacity
};

// All launchers return hipError_t of the launch and never synchronize.
hipError_t zg_index_terms(const uint8_t* src, const ZgTerm* terms, int n_terms, ZgChunk* chunks,
                          unsigned long long* err, hipStream_t stream);
// Descriptors are bounds-checked in-kernel against src_n / dst_n (bytes).  A clip window narrower
// than [0, dst_n) needs `clip_scratch` (ZG_CLIP_SCRATCH_BYTES of device memory owned by the caller,
// one per concurrently running launch): compressed chunks that straddle the window decode there
// before their clipped part is copied out.  Without it such a launch returns hipErrorInvalidValue.
#define ZG_CLIP_SCRATCH_BYTES (2u * (128u * 1024u + 256u))
// LZ4 chunks decode with the batched decoder (lz4seq.hip: scalar parse into lane registers +
// lane-parallel execute): unclipped launches by zg_lz4_batched_decode, clipped ones by the one-wave
// kernel's clipped instantiation (zg_lz4_decode_clipped).
// K4 parallel header walk: candidate scan over the span [0, src_n) of src + per-term sort/link in
// LDS; a term whose candidates are not exactly its chunk chain takes the serial walk (same records
// and errors as zg_index_terms).  Terms sorted by src.  scratch: zg_index_scratch_bytes(n_terms)
// of device memory, private to the stream (null / too small: zg_index_terms).
size_t zg_index_scratch_bytes(int n_terms);
hipError_t zg_index_terms_scan(const uint8_t* src, uint64_t src_n, const ZgTerm* terms, int n_terms, ZgChunk* chunks,
                               unsigned long long* err, uint8_t* scratch, size_t scratch_bytes, hipStream_t stream);
hipError_t zg_place_chunks(const uint8_t* src, uint64_t src_n, uint8_t* dst, uint64_t dst_n,
                           const ZgChunk* chunks, int n_chunks, uint64_t clip_lo, uint64_t clip_hi,
                           uint8_t* clip_scratch, unsigned long long* err, hipStream_t stream);
hipError_t zg_lz4_batched_decode(const uint8_t* src, uint64_t src_n, uint8_t* dst, uint64_t dst_n,
                                 const ZgChunk* chunks, int n_chunks, unsigned long long* err, hipStream_t stream);
// Two-kernel decode (lane-per-chunk parse into records, wave-per-chunk execute) with a caller-owned
// scratch of zg_lz4_rec_scratch_bytes(n_chunks, src_n) bytes (one per concurrently running
// launch); a null or short scratch runs zg_lz4_batched_decode instead.
size_t zg_lz4_rec_scratch_bytes(int n_chunks, uint64_t src_n);
hipError_t zg_lz4_decode_records(const uint8_t* src, uint64_t src_n, uint8_t* dst, uint64_t dst_n,
                                 const ZgChunk* chunks, int n_chunks, unsigned long long* err, uint8_t* scratch,
                                 size_t scratch_bytes, hipStream_t stream);
// Producer/consumer decode: two waves per chunk (scalar parse -> LDS batch ring -> lane-parallel
// execute), for launches with fewer chunks than resident waves.  grid_cap: pairs (0 = 4096).
hipError_t zg_lz4_pair_decode(const uint8_t* src, uint64_t src_n, uint8_t* dst, uint64_t dst_n, const ZgChunk* chunks,
                              int n_chunks, unsigned long long* err, int grid_cap, hipStream_t stream);
// Same with an explicit persistent-grid cap in blocks of 4 waves (0 = default 2048).
hipError_t zg_lz4_batched_decode_grid(const uint8_t* src, uint64_t src_n, uint8_t* dst, uint64_t dst_n,
                                      const ZgChunk* chunks, int n_chunks, unsigned long long* err, int grid_cap,
                                      hipStream_t stream);
// The LZ4/BG4 half of a clipped zg_place_chunks: the one-wave decoder writing only dst bytes
// [clip_lo, clip_hi); clip_scratch as for zg_place_chunks (null: hipErrorInvalidValue).
hipError_t zg_lz4_decode_clipped(const uint8_t* src, uint64_t src_n, uint8_t* dst, uint64_t dst_n,
                                 const ZgChunk* chunks, int n_chunks, uint64_t clip_lo, uint64_t clip_hi,
                                 uint8_t* clip_scratch, unsigned long long* err, hipStream_t stream);
// K1 keyed BLAKE3 of placed chunks (hashes[hash_index_base + c], sizes likewise when non-null) or of
// raw (offset, len) messages (key_mode 0 Xet data key, 1 node key, 2 plain, 3 zero key; a message
// over 128 KiB gets an all-ones hash).  With `scratch` (>= zg_hash_scratch_bytes(n, total message
// bytes) of device memory owned by the caller, one per concurrently running launch) the leaf-flat
// pipeline of blake3_flat.hip runs; without it, one wave per message (ingest.hip).
size_t zg_hash_scratch_bytes(int n, uint64_t total_bytes);
// Scratch of one zg_ingest_chunks launch (hash scratch + the decoder's BG4 staging, which share it).
size_t zg_ingest_scratch_bytes(int n, uint64_t total_bytes);
hipError_t zg_hash_chunks(const uint8_t* dst, uint64_t dst_n, const ZgChunk* chunks, int n_chunks,
                          uint8_t* hashes, uint64_t* sizes, uint32_t hash_index_base, uint8_t* scratch,
                          size_t scratch_bytes, hipStream_t stream);
hipError_t zg_hash_ranges(const uint8_t* buf, const uint64_t* offsets, const uint32_t* lens, int n,
                          uint8_t* hashes, int key_mode, uint8_t* scratch, size_t scratch_bytes, hipStream_t stream);
hipError_t zg_hash_chunks_flat(const uint8_t* dst, uint64_t dst_n, const ZgChunk* chunks, int n_chunks,
                               uint8_t* hashes, uint64_t* sizes, uint8_t* scratch, size_t scratch_bytes,
                               hipStream_t stream);
hipError_t zg_hash_ranges_flat(const uint8_t* buf, const uint64_t* offsets, const uint32_t* lens, int n,
                               uint8_t* hashes, int key_mode, uint8_t* scratch, size_t scratch_bytes,
                               hipStream_t stream);
// Decode of an unclipped ingest launch; *hashed = 1 when the decoder also hashed every compressed
// chunk (hashes[c], sizes[c]: the pair decoder with ZG_FUSED_HASH not 0), else 0.
// `stage` (>= zg_lz4_stage_bytes(n) of device memory, or null): BG4 chunks decode their grouped
// stream there and are written to dst once, whole lines at a time (ZG_BG4_STAGE=0 turns it off).
hipError_t zg_lz4_decode_ingest(const uint8_t* src, uint64_t src_n, uint8_t* dst, uint64_t dst_n, const ZgChunk* chunks,
                                int n_chunks, unsigned long long* err, uint8_t* hashes, uint64_t* sizes, int* hashed,
                                uint8_t* stage, size_t stage_bytes, hipStream_t stream);
size_t zg_lz4_stage_bytes(int n_chunks);
// Fused K3a + K1: uncompressed chunks are copied src -> dst by the hashing waves themselves (and
// hashed from src); compressed ones must already be decoded into dst (_raw: and hashed, so they are
// skipped).  Descriptors out of bounds are not placed, hash over empty leaves (never their real
// hash) and set ZG_ERR_RANGE (chunk index) in `err` (may be null).
hipError_t zg_place_hash_flat_raw(const uint8_t* src, uint64_t src_n, uint8_t* dst, uint64_t dst_n,
                                  const ZgChunk* chunks, int n_chunks, unsigned long long* err, uint8_t* hashes,
                                  uint64_t* sizes, uint8_t* scratch, size_t scratch_bytes, hipStream_t stream);
hipError_t zg_place_hash_flat(const uint8_t* src, uint64_t src_n, uint8_t* dst, uint64_t dst_n, const ZgChunk* chunks,
                              int n_chunks, unsigned long long* err, uint8_t* hashes, uint64_t* sizes, uint8_t* scratch,
                              size_t scratch_bytes, hipStream_t stream);
// One ingest launch sequence for an unclipped batch: LZ4/BG4 decode of the compressed chunks (only
// when `has_compressed`), then the fused place + hash (hashes[hash_index_base + c]).  Replaces
// zg_place_chunks + zg_hash_chunks (2 passes over the arena) with one pass; `scratch` is required.
hipError_t zg_ingest_chunks(const uint8_t* src, uint64_t src_n, uint8_t* dst, uint64_t dst_n, const ZgChunk* chunks,
                            int n_chunks, int has_compressed, unsigned long long* err, uint8_t* hashes,
                            uint64_t* sizes, uint32_t hash_index_base, uint8_t* scratch, size_t scratch_bytes,
                            hipStream_t stream);
hipError_t zg_merkle(const uint8_t* leaf_hashes, const uint64_t* leaf_sizes, const ZgMerkleJob* jobs,
                     int n_jobs, uint8_t* roots, uint8_t* scratch, uint64_t scratch_bytes,
                     hipStream_t stream);
size_t zg_merkle_scratch_bytes(uint64_t max_leaves_per_job, int n_jobs);
hipError_t zg_compare_hashes(const uint8_t* got, const uint8_t* want, int n, unsigned long long* err,
                             hipStream_t stream);
// CDC: candidate END offsets (i+1) where the full-window gear hash has (h & mask) == 0.
hipError_t zg_cdc_candidates(const uint8_t* data, uint64_t n, uint64_t mask, uint64_t* out,
                             unsigned long long* count, uint64_t capacity, hipStream_t stream);
// Synthetic content.  mode 0: uniform random bytes; mode 1: bf16 ~ N(0, 0.02).
hipError_t zg_fill_synthetic(uint8_t* dst, uint64_t n, uint64_t seed, uint64_t stream_offset, int mode,
                             hipStream_t stream);
// K7b: compress chunks (optional BG4 grouping into `scratch`, slot `in_slot` bytes per chunk) into
// LZ4 frames at out + c * out_slot; out_len[c] = frame bytes, or 0 when the chunk does not compress.
// hc64 / hc256: frame header checksum bytes for the 64 KiB / 256 KiB block-size descriptors.
hipError_t zg_compress_chunks(const uint8_t* data, const uint64_t* offs, const uint32_t* lens, int n, int bg4,
                              uint8_t* scratch, uint64_t in_slot, uint8_t* out, uint64_t out_slot, uint32_t* out_len,
                              uint32_t hc64, uint32_t hc256, hipStream_t stream);
// Serialize chunks (header + payload copied from per-chunk device addresses) into xorb bodies.
hipError_t zg_pack_frames(const uint64_t* src, const uint32_t* clen, const uint32_t* ulen, const uint8_t* scheme,
                          const uint64_t* out_off, int n, uint8_t* out, hipStream_t stream);

// Pack uncompressed chunks into serialized xorb bodies: header (version 0, scheme 0) + payload.
hipError_t zg_pack_chunks(const uint8_t* data, const uint64_t* data_off, const uint32_t* lens,
                          const uint64_t* out_off, int n, uint8_t* out, hipStream_t stream);

// K9 (serve.hip): write bytes [lo, hi) of a resident run's scheme-0 serialized stream to
// out[0, hi - lo).  src[i]: device address of chunk i's decoded bytes (any alignment); ser_end[i]:
// serialized end offset of chunk i relative to the run (sum of len + 8); both tables stay on the
// device, so a request is a launch with scalars.  out: 16-byte aligned, device or device-visible
// pinned host memory; nothing outside out[0, hi - lo) is written.  The caller vouches for the
// tables and for hi <= ser_end[n - 1].
hipError_t zg_serve_pack(const uint64_t* src, const uint64_t* ser_end, uint32_t n, uint64_t lo, uint64_t hi,
                         uint8_t* out, hipStream_t stream);

// K10 (shard.hip): gather the kept slices of n tensors from src into a compact arena at dst.  table:
// device block of ZG_SLICE_ROWS rows of n uint64 each.  Tensor i is n_runs[i] runs of run_bytes[i]
// bytes, run r read at src + src_off[i] + r * src_stride[i] (any alignment, src_stride >= run_bytes),
// laid end to end at dst + dst_off[i]; dst_end[i] = dst_off[i] + n_runs[i] * run_bytes[i].  Entries
// are sorted by dst_off with disjoint outputs; dst and every dst_off are 16-byte aligned; zero-size
// entries are legal.  dst_total = dst_end[n - 1].  Only the tensors' output bytes are written.  The
// caller vouches for the table: nothing is checked on the device.
enum {
  ZG_SLICE_SRC_OFF = 0,
  ZG_SLICE_RUN_BYTES = 1,
  ZG_SLICE_SRC_STRIDE = 2,
  ZG_SLICE_N_RUNS = 3,
  ZG_SLICE_DST_OFF = 4,
  ZG_SLICE_DST_END = 5,
  ZG_SLICE_ROWS = 6
};
hipError_t zg_slice_gather(const uint8_t* src, const uint64_t* table, uint32_t n, uint64_t dst_total, uint8_t* dst,
                           hipStream_t stream);

// K15 (scatter.hip): K10 with the destination at any address.  table: device block of
// ZG_SCATTER_ROWS rows of n uint64 each.  Entry i is n_runs[i] runs of run_bytes[i] bytes, run r read
// at src + src_off[i] + r * src_stride[i] (any alignment, src_stride >= run_bytes), laid end to end at
// the absolute device address dst_addr[i] (any alignment, any allocation).  blk_end[i] is the
// inclusive prefix sum of the entries' aligned 16-byte destination block counts,
// ceil((dst_addr + size) / 16) - floor(dst_addr / 16) for size = n_runs * run_bytes > 0 and 0
// otherwise; total_blocks = blk_end[n - 1].  Outputs are disjoint from each other and from src;
// entries should be sorted by dst_addr (locality only); zero-size entries are legal.  Only output
// bytes are stored, 16 bytes at a time only to aligned blocks wholly inside one output, and no
// destination byte is read.  The caller vouches for the table: nothing is checked on the device.
enum {
  ZG_SCATTER_SRC_OFF = 0,
  ZG_SCATTER_RUN_BYTES = 1,
  ZG_SCATTER_SRC_STRIDE = 2,
  ZG_SCATTER_N_RUNS = 3,
  ZG_SCATTER_DST_ADDR = 4,
  ZG_SCATTER_BLK_END = 5,
  ZG_SCATTER_ROWS = 6
};
hipError_t zg_slice_scatter(const uint8_t* src, const uint64_t* table, uint32_t n, uint64_t total_blocks,
                            hipStream_t stream);

// K16 (scatter_cast.hip): K15 with a float conversion on the way.  table: device block of
// ZG_CAST_ROWS rows of n uint64 each: K15's five fields, kind[i] (one of ZG_CAST_F32_BF16 ..
// ZG_CAST_F16_BF16), then blk_end.  run_bytes, src_off and src_stride count SOURCE bytes; entry i
// writes size = n_runs * run_bytes / src_item * dst_item bytes at dst_addr[i], and blk_end is K15's
// prefix sum over those output sizes.  dst_addr[i] is a multiple of the destination item, run_bytes[i]
// of the source item; src_off and src_stride are arbitrary (a source element may sit at any byte
// address).  Round to nearest even, one rounding, overflow to infinity, subnormals and signed zeros
// kept, NaN stays NaN (sign and payload unspecified).  Stores as K15, with 2- or 4-byte element stores
// for its byte stores; no destination byte is read.  The caller vouches for the table.
enum {
  ZG_CAST_SRC_OFF = 0,
  ZG_CAST_RUN_BYTES = 1,
  ZG_CAST_SRC_STRIDE = 2,
  ZG_CAST_N_RUNS = 3,
  ZG_CAST_DST_ADDR = 4,
  ZG_CAST_KIND = 5,
  ZG_CAST_BLK_END = 6,
  ZG_CAST_ROWS = 7
};
enum {
  ZG_CAST_F32_BF16 = 0,
  ZG_CAST_F32_F16 = 1,
  ZG_CAST_BF16_F32 = 2,
  ZG_CAST_F16_F32 = 3,
  ZG_CAST_BF16_F16 = 4,
  ZG_CAST_F16_BF16 = 5,
  ZG_CAST_KINDS = 6
};
hipError_t zg_slice_scatter_cast(const uint8_t* src, const uint64_t* table, uint32_t n, uint64_t total_blocks,
                                 hipStream_t stream);

// K8: pull each segment's bytes from a peer's IPC-mapped arena (xGMI) into this GPU's arena;
// every segment is read concurrently.  src[i] and dst[i] must be congruent mod 16.
enum { kZgMaxPeerSegs = 16 };
typedef struct ZgPeerSegs {
  uint64_t src[kZgMaxPeerSegs];
  uint64_t dst[kZgMaxPeerSegs];
  uint64_t n[kZgMaxPeerSegs];
  int nseg;
} ZgPeerSegs;
hipError_t zg_peer_gather(const ZgPeerSegs* segs, hipStream_t stream);

// K11 (shard_peers.hip): K10 over up to kZgMaxPeerSegs source buffers in one launch.  table: K10's
// rows plus row ZG_SLICE_SRC, the source index of each entry (ZG_SLICE_PEER_ROWS rows of n uint64);
// src_off is relative to src[that index].  Beyond K10's preconditions the entries of one source are
// contiguous in the table; [lo[s], hi[s]) is the arena range from the first dst_off to the last
// dst_end of source s's entries with output (lo == hi: none).  Neighbouring blocks serve
// different sources and a block loops over its source's tiles; max_blocks caps the grid (0: 512, as K8; at least one block per
// source).  Nothing is checked on the device beyond hi <= dst_total.
enum { ZG_SLICE_SRC = 6, ZG_SLICE_PEER_ROWS = 7 };
typedef struct ZgSliceSrcs {
  uint64_t src[kZgMaxPeerSegs];
  uint64_t lo[kZgMaxPeerSegs];
  uint64_t hi[kZgMaxPeerSegs];
  int nseg;
} ZgSliceSrcs;
hipError_t zg_slice_gather_peers(const ZgSliceSrcs* srcs, const uint64_t* table, uint32_t n, uint64_t dst_total,
                                 uint8_t* dst, uint32_t max_blocks, hipStream_t stream);

// K12 (blake3_flat.hip): reuse chunks that are resident on this device under another revision.
// Record i copies `len` bytes from the absolute device address `src` (any alignment, any allocation)
// to dst + `dst`, writes their Xet chunk hash (keyed, DATA_KEY) to hashes + 32 * `index` and, when
// sizes is non-null, `len` to sizes[`index`].  Rows of hashes / sizes that no record names keep their
// bytes, and no byte of dst outside the records' outputs is written.  len == 0 is legal (the empty
// hash, nothing copied); len > 128 KiB must be refused by the caller (such a record is not copied and
// hashes as empty).  Source loads are widened at most to the aligned dwords that hold a byte of the
// chunk.  scratch: zg_hash_scratch_bytes(n, sum of len) of device memory, one per concurrently
// running launch.  The caller vouches for every record: nothing is checked on the device.
typedef struct ZgReuse {
  uint64_t src;    // device address of the chunk's bytes
  uint64_t dst;    // output offset in dst
  uint32_t len;    // bytes (<= 128 KiB)
  uint32_t index;  // row of hashes / sizes
} ZgReuse;
hipError_t zg_reuse_chunks(const ZgReuse* recs, int n, uint8_t* dst, uint8_t* hashes, uint64_t* sizes,
                           uint8_t* scratch, size_t scratch_bytes, hipStream_t stream);

// K13 (dedup.hip): chunk dedup, a hash join over 32-byte keys.  Rows 0 .. m are `index`, rows
// m .. m + n are `fresh` (two pointers: a persistent index is never concatenated); both are
// contiguous rows of 32 bytes, 16-byte aligned.  first[j] (j < n) = the smallest row r' <= m + j whose
// 32 bytes equal fresh row j's: below m an index row, m + j when fresh row j is the first of its
// kind.  A pure function of the keys.  table: caller-owned scratch of zg_dedup_table_bytes(m + n)
// bytes, 16-byte aligned, overwritten by every call: open addressing with linear probing over
// uint32 row ids in zg_dedup_slots(m + n) slots (the next power of two >= 2 * rows, at least 64);
// a row's home slot is (little-endian u64 of key bytes 0 .. 8) & (slots - 1).  Size and slot
// function are part of the contract.  m + n < 2^31; n == 0 launches nothing.  Three launches on
// `stream` (fill, build, probe).
uint64_t zg_dedup_slots(uint64_t rows);
size_t zg_dedup_table_bytes(uint64_t rows);
hipError_t zg_dedup_chunks(const uint8_t* index, uint32_t m, const uint8_t* fresh, uint32_t n, uint32_t* table,
                           size_t table_bytes, int64_t* first, hipStream_t stream);

// K14 (synth.hip): K5 over a file that exists only as a list of segments.  segs[i] = `len` > 0 bytes
// at the absolute device address `addr` (any alignment) that are bytes [vstart, vstart + len) of the
// file; the table is sorted and covers [0, n) without gaps.  A lane owns one 2 KiB window of a
// segment's 16-byte-aligned address space; win_prefix[i] (n_segs + 1 entries) = windows of the
// segments before i, window count of segment i = ceil(((addr & 15) + len) / 2048), n_windows =
// win_prefix[n_segs].  lead: 64 * n_segs bytes of scratch; a pre-pass launch fills row i with the
// min(64, vstart) file bytes before segment i, from which the segment's first window warms up (at
// the start of the file there is no history).  out / count / capacity as zg_cdc_candidates: unsorted
// END offsets (i + 1) in file coordinates, *count may exceed capacity (retry with more).  The set
// equals zg_cdc_candidates' over the concatenated bytes.  Loads touch only aligned 16-byte blocks
// that hold a byte of a segment: no pad behind a segment is assumed.  The caller vouches for the
// table: nothing is checked on the device.  Two launches whatever n_segs is.
typedef struct ZgSeg {
  uint64_t addr;
  uint64_t len;
  uint64_t vstart;
} ZgSeg;
hipError_t zg_cdc_candidates_segs(const ZgSeg* segs, const uint64_t* win_prefix, uint32_t n_segs, uint64_t n_windows,
                                  uint8_t* lead, uint64_t mask, uint64_t* out, unsigned long long* count,
                                  uint64_t capacity, hipStream_t stream);

// Chunk hashes at absolute addresses (blake3_flat.hip): K12 without the copy.  Record i hashes `len`
// bytes at the device address `src` (any alignment, any allocation) and writes the Xet chunk hash to
// hashes + 32 * `index` and, when sizes is non-null, `len` to sizes[`index`].  Rows no record names
// keep their bytes; nothing but the two tables (and scratch) is stored.  Loads stay inside the
// aligned dwords that hold a byte of the chunk.  len == 0 gives the empty hash; len > 128 KiB must be
// refused by the caller (it hashes as empty).  scratch: zg_hash_scratch_bytes(n, sum of len).  The
// caller vouches for every record.
typedef struct ZgHashAt {
  uint64_t src;    // device address of the chunk's bytes
  uint32_t len;    // bytes (<= 128 KiB)
  uint32_t index;  // row of hashes / sizes
} ZgHashAt;
hipError_t zg_hash_chunks_at(const ZgHashAt* recs, int n, uint8_t* hashes, uint64_t* sizes, uint8_t* scratch,
                             size_t scratch_bytes, hipStream_t stream);

int zg_device_count(void);
// K6: out[i] (20 B) = SHA1("zest-xet-v1:" || hashes[i] (32 B)); out must be 4-byte aligned.
hipError_t zg_sha1_info_hash(const uint8_t* hashes, int n, uint8_t* out, hipStream_t stream);

#ifdef __cplusplus
}
#endif
