// vbf_kernels.hpp -- internal launch interface between the C ABI (vbf_api.hip) and the kernels.
#pragma once

// Ablation builds (timing experiments, tools/ablate*.py): compiled with -DVBF_ABLATION_BUILD=1 and
// loaded through VBF_LIB, they honour VBF_ABLATE, which skips phases and so gives WRONG
// results.  The product library is built without it and ignores VBF_ABLATE.
#ifndef VBF_ABLATION_BUILD
#define VBF_ABLATION_BUILD 0
#endif
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace vbf {

// A batch of keys resident in device memory.
//   offsets == nullptr : key j = keys[j*stride .. j*stride + stride)
//   offsets != nullptr : key j = keys[offsets[j]-off_base .. offsets[j+1]-off_base)
struct KeyBatch {
    const uint8_t* keys;
    const uint64_t* offsets;
    uint64_t off_base;
    uint64_t stride;
    uint64_t n;
    bool len_prefix;  // prepend LE64(len) (Rust `Hash for [u8]`)
};

hipError_t launch_build(const KeyBatch& kb, uint32_t m, uint32_t k, uint32_t* words, hipStream_t s);

// Optional per-phase timing (vbf_profile_*): HIP events recorded on the launch stream.
enum Phase { kPhaseTileSort = 0, kPhaseTranspose = 1, kPhaseSegOr = 2, kPhaseAtomicBuild = 3,
             kPhaseProbe = 4, kPhaseSstWalk = 5, kPhaseSstScan = 6, kPhaseSstEmit = 7,
             kPhaseMergeLevels = 8, kPhaseFold = 9, kPhaseSelect = 10, kPhaseProbePack = 11,
             kPhaseProbeSeg = 12, kPhaseProbeOut = 13, kPhaseEncTile = 14, kPhaseEncScan = 15,
             kPhaseEncIndex = 16, kPhaseEncData = 17, kPhaseTableOpen = 18, kPhaseTableGet = 19,
             kPhaseScanRank = 20, kPhaseScanEmit = 21, kPhaseVlogSizes = 22, kPhaseVlogCopy = 23,
             kPhaseVlogEncode = 24, kPhaseMemSort = 25, kPhaseMemMerge = 26, kPhaseFilterInsert = 27,
             kPhaseGcJudge = 28, kPhaseGcEmit = 29, kPhaseMemGet = 30, kNumPhases = 31 };
void phase_begin(int phase, hipStream_t s);
void phase_end(int phase, hipStream_t s);

// Partitioned build (vbf_partition.hip).  Key batches are processed in chunks of at most
// kBuildChunkIdx (build) / kPartChunkIdx (probe) bit indices; the workspace holds one chunk's
// sorted tiles + offset tables (build: 2.5 B per index, ~10.7 GB at 2^32; probe: 4 B per index).
// Each build chunk re-reads and re-writes the whole filter in k_seg_or, so build chunks are big:
// 2^32 holds config 5's 1B keys x k = 4 in one chunk (26.9 -> 26.5 ms: one k_seg_or pass over
// the 512 MiB filter instead of two, and that one fresh; profiles/r05/ab_cfg5_single_chunk.txt).
constexpr uint64_t kPartChunkIdx = 1ull << 30;
constexpr uint64_t kBuildChunkIdx = 1ull << 32;
bool partition_supported(uint32_t m, uint32_t k);
// chunk_idx: bit indices per build chunk (0: kBuildChunkIdx or VBF_BUILD_CHUNK_LOG2); the C ABI
// halves it when the workspace for the default chunk cannot be allocated (2^32
// indices take ~10.7 GB)
uint64_t build_chunk_default();
uint64_t partition_workspace_bytes(uint64_t n, uint32_t m, uint32_t k, uint64_t chunk_idx = 0);
// Partitioned probe (vbf_partition.hip): out (answer bytes) or count (hits), one of them.
bool probe_partition_supported(uint32_t m, uint32_t k);
uint64_t probe_workspace_bytes(uint64_t n, uint32_t m, uint32_t k);
hipError_t launch_probe_partitioned(const KeyBatch& kb, uint32_t m, uint32_t k, const uint32_t* words, uint8_t* out,
                                    unsigned long long* count, void* ws, uint64_t ws_bytes, hipStream_t s);
uint64_t probe_count_partials(uint64_t n, uint32_t m, uint32_t k);
// fresh: `words` holds no filter yet; the first chunk's segment pass writes every word without
// reading it (callers zero the words themselves where that pass cannot own every segment).
hipError_t launch_build_partitioned(const KeyBatch& kb, uint32_t m, uint32_t k, uint32_t* words,
                                    void* ws, uint64_t ws_bytes, bool atomic_merge, hipStream_t s,
                                    bool fresh = false, uint64_t chunk_idx = 0);
// Whether a fresh build of n keys can skip the zero fill (one chunk, one workgroup per segment).
bool partition_fresh_ok(uint64_t n, uint32_t m, uint32_t k, uint64_t chunk_idx = 0);
hipError_t launch_probe(const KeyBatch& kb, uint32_t m, uint32_t k, const uint32_t* words,
                        uint8_t* out, hipStream_t s);
// Count: `partial` holds count_partials(n) u32 of scratch; the hits are added to *count.
uint64_t count_partials(uint64_t n);
hipError_t launch_count(const KeyBatch& kb, uint32_t m, uint32_t k, const uint32_t* words,
                        unsigned long long* count, uint32_t* partial, hipStream_t s);
hipError_t launch_count_finish(const uint32_t* partial, uint64_t np, unsigned long long* count, hipStream_t s);
hipError_t launch_hashes(const KeyBatch& kb, uint32_t k, uint64_t* out, hipStream_t s);
hipError_t launch_or_words(uint32_t* dst, const uint32_t* src, uint64_t nwords, hipStream_t s);
hipError_t launch_popcount(const uint32_t* words, uint64_t nwords, unsigned long long* out,
                           hipStream_t s);
hipError_t launch_gen_fixed(uint64_t seed, uint64_t base, uint64_t n, uint32_t len, uint8_t* out,
                            hipStream_t s);
hipError_t launch_gen_var(uint64_t seed, uint64_t base, uint64_t n, const uint64_t* offsets,
                          uint8_t* out, hipStream_t s);


// SST data.db decode (vbf_sst.hip).  Output arrays may be NULL.
struct SstArgs {
    const uint8_t* data;
    uint64_t len;
    const uint32_t* blocks;  // block start offsets (index.db)
    uint64_t nblocks;
    uint32_t* counts;        // [nblocks + 1] entry counts (walk pass)
    uint16_t* pos;           // [nblocks * 256] entry starts within each block (walk pass)
    uint32_t* lmin;          // [nblocks] shortest / longest key per block (walk pass)
    uint32_t* lmax;
    const uint64_t* ebase;   // [nblocks + 1] exclusive scan of counts (emit pass)
    uint8_t* keys;
    uint64_t* offsets;       // [n + 1] absolute positions in keys
    uint32_t* val_off;
    uint64_t* created;
    uint8_t* tomb;
    uint32_t* err;           // [0] error bits, [1] first bad block, [2]/[3] min/max key length
    uint32_t ablate;         // timing experiments only (VBF_ABLATE 11-14, ablation builds)
    uint32_t walk_v;         // 1: vector-register entry walk (default), 0: scalar (VBF_SST_WALK)
};
hipError_t sst_count(const SstArgs& a, hipStream_t s);
hipError_t sst_emit(const SstArgs& a, hipStream_t s);
uint64_t sst_pos_bytes(uint64_t nblocks);
hipError_t sst_len_range(const uint32_t* lmin, const uint32_t* lmax, uint64_t nblocks, uint32_t* out2, void* tmp,
                         size_t* tmp_bytes, hipStream_t s);
hipError_t sst_scan(const uint32_t* counts, uint64_t* ebase, uint64_t nblocks, void* tmp, size_t* tmp_bytes,
                    hipStream_t s);
// SST data.db / index.db encode (vbf_sst_write.hip).  Entry j = key j plus val_off / created / tomb
// (each may be NULL: zeros).  With offsets the blocks come from the tile-table segmentation
// (sst_enc_segment, then an exclusive scan of tsum into tbase); with a fixed stride they are
// closed-form and only sst_enc_emit runs.
constexpr uint32_t kEncTile = 1024;   // entries per tile
constexpr uint32_t kEncReach = 240;   // entries a block can hold at most (4096 / 17)
constexpr uint32_t kEncGroup = 128;   // tiles per group
enum : uint32_t { kEncErrOrder = 1, kEncErrBig = 2 };
struct SstEncArgs {
    const uint8_t* keys;
    const uint64_t* offsets;  // n + 1 absolute positions, or NULL for `stride`
    uint64_t stride, n;
    const uint32_t* val_off;
    const int64_t* created;
    const uint8_t* tomb;
    uint64_t ntiles, ngroups;
    uint8_t* delta;         // [n] entries in the block that would start at entry e
    uint8_t* tab;           // [ngroups * kEncGroup][kEncReach] tile transfer tables
    uint8_t* gtab;          // [ngroups][kEncReach] group transfer tables
    uint8_t* gep;           // [ngroups] entry point of each group's first tile
    uint8_t* ep;            // [ngroups * kEncGroup] entry point of each tile
    uint64_t* tsum;         // [ntiles + 1] per tile: blocks << 40 | index.db bytes
    const uint64_t* tbase;  // [ntiles + 1] exclusive scan of tsum
    uint32_t* err;          // [0] kEncErr bits, [1] first bad entry
    uint8_t* data;          // outputs, each may be NULL
    uint8_t* index;
    uint32_t* blocks;
};
hipError_t sst_enc_segment(const SstEncArgs& a, hipStream_t s);
hipError_t sst_enc_emit(const SstEncArgs& a, hipStream_t s);
// Point lookups in SST tables (vbf_table.hip).  A table as the lookup kernel sees it: the three
// file buffers plus the side tables built at open.
struct TableDesc {
    const uint8_t* data;
    const uint8_t* index;
    const uint32_t* blocks;   // [nblocks] block starts in data
    const uint32_t* counts;   // [nblocks] entries per block (<= 256)
    const uint16_t* pos;      // [nblocks * 256] entry starts within each block
    const uint64_t* kpos;     // [nblocks + 1] start of index record b in index; [nblocks] = index_len
    const uint64_t* ebase;    // [nblocks + 1] entries before block b; [nblocks] = the table's entries
    uint64_t nblocks;
};
enum : uint32_t { kTabErrBig = 1, kTabErrDense = 2, kTabErrOrder = 4, kTabErrIndexLen = 8, kTabErrIndexRec = 16 };
struct TableOpenArgs {
    const uint8_t* data;
    uint64_t len;
    const uint8_t* index;
    uint64_t index_len;
    const uint32_t* blocks;
    uint64_t nblocks;
    const uint32_t* counts;     // the walk pass's outputs (SstArgs)
    const uint16_t* pos_walk;
    const uint32_t* lmin;
    const uint32_t* lmax;
    const uint64_t* ebase;
    uint16_t* pos;              // [nblocks * 256] the handle's entry starts (fill pass)
    uint64_t* reclen;           // [nblocks + 1] bytes of index record b (fill pass); [nblocks] = 0
    const uint64_t* kpos;       // [nblocks + 1] exclusive scan of reclen (check pass)
    uint32_t* err;              // [0] kTabErr bits, [1] first bad block, [2] first bad entry
};
struct TableGetArgs {
    const uint8_t* keys;
    const uint64_t* offsets;  // n + 1 absolute positions, or NULL for `stride`
    uint64_t stride, n;
    uint32_t nsst;
    const TableDesc* tab;     // device, nsst entries, in the caller's table order
    const uint8_t* cand;      // device n * nsst, or NULL: every table
    uint8_t* found;           // outputs, each may be NULL
    uint32_t* table_idx;
    uint32_t* val_off;
    uint64_t* created;
};
hipError_t table_fill(const TableOpenArgs& a, hipStream_t s);
hipError_t table_check(const TableOpenArgs& a, hipStream_t s);
hipError_t table_get(const TableGetArgs& a, hipStream_t s);
// Range scans over open tables (vbf_table_scan.hip).  P = nranges * nsst (range, table) pairs in
// range-major order; `total` candidate entries (the sum of cnt), one merged slot each.
enum : uint32_t { kScanKeepTombstones = 1, kScanEndExclusive = 2 };
enum : uint32_t { kScanErrBounds = 1, kScanErrRank = 2 };
struct TableScanArgs {
    const uint8_t* bounds;      // device; lo_r / hi_r as in MultiSst
    const uint64_t* bounds_off; // device, 2 * nranges + 1 absolute positions
    uint64_t nranges;
    uint32_t nsst, flags;
    const TableDesc* tab;       // device, nsst entries, in the caller's table order
    uint64_t* first;            // [P] rank of the pair's first candidate in its table (bounds pass)
    uint64_t* cnt;              // [P + 1] candidates of the pair (bounds pass); [P] = 0
    const uint64_t* cbase;      // [P + 1] exclusive scan of cnt; [P] = total
    uint64_t total;
    uint32_t* m_table;          // [total] merged slot -> table, -> entry start in data.db (rank pass)
    uint32_t* m_pos;
    uint64_t* m_keep;           // [total + 1] 1 when the slot's entry is listed, its key length then
    uint64_t* m_len;            //             (rank pass; [total] = 0)
    const uint64_t* opos;       // [total + 1] exclusive scans of m_keep / m_len
    const uint64_t* kofs;
    uint32_t* err;              // [0] kScanErr bits
    uint64_t* range_off;        // outputs, each may be NULL (emit / keys passes)
    uint8_t* keys;
    uint64_t* key_off;
    uint32_t* table_idx;
    uint32_t* val_off;
    uint64_t* created;
    uint8_t* tomb;
};
hipError_t table_scan_bounds(const TableScanArgs& a, hipStream_t s);
hipError_t table_scan_rank(const TableScanArgs& a, hipStream_t s);
hipError_t table_scan_emit(const TableScanArgs& a, hipStream_t s);
hipError_t table_scan_keys(const TableScanArgs& a, hipStream_t s);
// Value-log reads and appends (vbf_vlog.hip).  The copies divide their work by output bytes: one
// workgroup per kVlogSlice bytes of the destination (a power of two between 1 KiB and 128 KiB).
constexpr uint32_t kVlogSlice = 16384;
enum : uint8_t { kVlogSkipped = 0, kVlogValue = 1, kVlogTombstone = 2, kVlogNone = 3, kVlogBad = 4,
                 kVlogKeyMismatch = 5 };
struct VlogGetArgs {
    const uint8_t* bytes;         // the log's bytes [base, base + len)
    uint64_t len, base;
    const uint32_t* val_offsets;  // [n] file positions
    const uint8_t* found;         // [n] or NULL: item j is fetched only when found[j] == 1
    uint64_t n;
    const uint8_t* keys;          // NULL: no key check; else the layout of every entry point
    const uint64_t* offsets;
    uint64_t stride;
    uint8_t* status;              // [n] kVlog* (sizes pass)
    uint64_t* vlen;               // [n + 1] value length, 0 unless status == kVlogValue; [n] = 0
    uint64_t* src;                // [n] the value's position in `bytes`
    const uint64_t* voff;         // [n + 1] exclusive scan of vlen; [n] = total
    uint64_t total;
    uint8_t* values;              // output of the copy pass
};
hipError_t vlog_sizes(const VlogGetArgs& a, hipStream_t s);
hipError_t vlog_copy(const VlogGetArgs& a, hipStream_t s);
enum : uint32_t { kVlogEncErrOrder = 1, kVlogEncErrLong = 2 };
struct VlogEncArgs {
    const uint8_t* keys;
    const uint64_t* offsets;      // n + 1 absolute positions, or NULL for `stride`
    uint64_t stride, n;
    const uint8_t* values;
    const uint64_t* value_off;    // n + 1 absolute positions in values
    const int64_t* created;       // NULL: zeros
    const uint8_t* tomb;          // NULL: zeros
    uint64_t base;                // the file's size before the append
    uint64_t k0, v0;              // offsets[0] (0 with a stride), value_off[0]
    uint64_t k_end, v_end;        // offsets[n] (n * stride), value_off[n]: no byte at or past them is read
    uint64_t total;               // bytes appended
    uint32_t* err;                // check pass: [0] kVlogEncErr bits, [1] first bad entry
    uint8_t* out;                 // outputs, each may be NULL
    uint32_t* val_offsets;
};
hipError_t vlog_enc_check(const VlogEncArgs& a, hipStream_t s);
hipError_t vlog_encode(const VlogEncArgs& a, hipStream_t s);
// The walk of the value log (vbf_vlog_walk.hip).  The window is walked in segments of at most
// kWalkSegment bytes, a segment in tiles of kWalkTile bytes, the tiles in groups of kWalkGroup.
// Positions inside a segment are u32 relative to its first byte, kWalkOut = none / outside.
constexpr uint32_t kWalkTile = 4096;
constexpr uint32_t kWalkGroup = 32;
constexpr uint32_t kWalkSegment = 8u << 20;
constexpr uint32_t kWalkSlots = 256;  // entry slots per tile (at most kWalkTile / 17 + 1 = 241 are used)
constexpr uint32_t kWalkOut = 0xFFFFFFFFu;
static_assert(kWalkSegment % (kWalkTile * kWalkGroup) == 0, "whole groups per segment");
struct WalkRes {           // one segment's result, read back by the host
    uint64_t n, kbytes, vbytes;  // entries, key bytes, value bytes
    uint64_t end;                // window position where the walk left the segment's last entered tile
    uint64_t last_entry;         // window position of the last entry (n > 0)
    uint32_t torn, last_tile;    // the entry at `end` is cut by the window's end; the last tile entered
};
struct WalkArgs {
    const uint8_t* bytes;  // the log's bytes [base, base + len)
    uint64_t len, base;
    uint64_t seg0;         // window position of the segment's first byte (a multiple of kWalkTile)
    uint32_t ntiles, q0;   // tiles of the segment; the entry position, relative to seg0, in tile 0
    uint64_t cap;          // successors at or beyond it leave the segment: min(segment end, len, lim)
    uint64_t lim;          // entries start below it (the budget rule, in window positions)
    uint32_t* exit;        // [ntiles * kWalkTile] (hop pass)
    uint32_t* gexit;       // [groups * kWalkTile] (group pass)
    uint32_t* tentry;      // [ntiles] entry position of each tile, kWalkOut: not entered (entry pass)
    uint16_t* pos;         // [ntiles * kWalkSlots] entry starts within the tile (mark pass)
    uint16_t* kpre;        // [ntiles * kWalkSlots] key bytes of the tile's entries before this one
    uint64_t* cnt;         // [ntiles + 1] per tile: entries, key bytes, value bytes; [ntiles] = 0
    uint64_t* ksum;
    uint64_t* vsum;
    uint64_t* tend;        // [ntiles] where the tile's walk stopped, [ntiles] whether on a torn entry
    uint32_t* ttorn;
    uint64_t* cbase;       // [ntiles + 1] exclusive scans of cnt / ksum / vsum
    uint64_t* kbase;
    uint64_t* vbase;
    uint64_t* ko;          // [entries + 1] per entry of the segment: the key's place in the segment's
    uint64_t* ks;          // key bytes and its position in the window; the same for the value (emit)
    uint64_t* vo;
    uint64_t* vs;
    WalkRes* res;
};
struct WalkOut {           // the caller's arrays (each may be NULL) and the segment's place in them
    uint64_t* entry_off;
    uint32_t* val_offsets;
    uint8_t* keys;
    uint64_t* key_off;
    uint8_t* values;
    uint64_t* value_off;
    int64_t* created;
    uint8_t* tomb;
    uint64_t j0, k0, v0;            // entries, key bytes and value bytes of the segments before
    uint64_t n_seg, kb_seg, vb_seg; // this segment's
};
// hop, group, entry, mark, the three scans and the result, queued on s; scan_tmp: scan_u64's scratch
// for ntiles + 1 items.
hipError_t walk_passes(const WalkArgs& a, void* scan_tmp, size_t scan_bytes, hipStream_t s);
hipError_t walk_emit(const WalkArgs& a, const WalkOut& o, hipStream_t s);
hipError_t walk_tail(const WalkOut& o, uint64_t n, uint64_t end_off, uint64_t kb, uint64_t vb, hipStream_t s);
// The GC's data step (vbf_gc.hip): every entry of a walked chunk judged against its most recent
// entry, then the `tail` entry and the surviving entries written from the window into the bytes to
// append.  Per chunk entry i: its file position, and the lookup's answer (found / val_off / wcreated:
// vbf_table_get_*'s arrays, which the overlay pass overrides where the overlay holds the key).
enum : uint8_t { kGcValid = 0, kGcAbsent = 1, kGcDeleted = 2, kGcLogNone = 3, kGcLogTombstone = 4, kGcOlder = 5,
                 kGcStar = 6, kGcBad = 0xFF };
constexpr uint32_t kGcNoEntry = 0xFFFFFFFFu;  // put_ids[0]: the `tail` put comes from no chunk entry
constexpr uint64_t kGcTailSize = 17 + 4 + 8;  // the `tail` entry: header, "tail", LE64(new tail)
struct GcRes {               // read back by the host after the judge
    uint64_t n_invalid;
    uint64_t bad;            // the first chunk entry whose most recent entry is BAD, ~0: none
    uint64_t last_valid;     // 1 + the last valid chunk entry, 0: none
};
struct GcArgs {
    const uint8_t* bytes;    // the log's bytes [base, base + len)
    uint64_t len, base;
    uint64_t n;              // chunk entries
    const uint64_t* entry_off;   // [n] file positions (the walk's)
    const uint8_t* ov_keys;      // the overlay: ov_n strictly ascending keys, key k = ov_keys[ov_off[k] .. ov_off[k+1])
    const uint64_t* ov_off;
    const uint32_t* ov_val;
    const int64_t* ov_created;
    const uint8_t* ov_tomb;
    uint64_t ov_n;
    uint8_t* found;          // [n] 0 nowhere, 1 live, 2 tombstone
    uint32_t* val_off;       // [n] the winner's file position
    uint64_t* wcreated;      // [n] the winner's created_at
    uint8_t* verdict;        // [n] kGc* (judge)
    uint8_t* keep;           // [n] 1 for a valid entry
    uint32_t* ids;           // [n] i, the select's input
    uint64_t* size;          // [n + 2] bytes appended for item 0 (the `tail` put) and for entry i at [i + 1]; [n + 1] = 0
    uint64_t* ksrc;          // [n] valid entries: window positions of the own key and of the most recent value
    uint64_t* vsrc;
    uint32_t* klen;          // [n] and their lengths
    uint32_t* vlen;
    GcRes* res;
    const uint64_t* pos;     // [n + 2] exclusive scan of size; [n + 1] = the bytes appended
    const uint32_t* put_ids; // [n_puts] put j's chunk entry, kGcNoEntry for put 0 (the select's output behind it)
    uint64_t n_puts, total;
    uint64_t log_size, new_tail;
    int64_t now_ms;
    uint8_t* append;         // emit's outputs
    uint32_t* put_val_offsets;
    uint8_t* put_tombstones;
};
hipError_t gc_overlay(const GcArgs& a, hipStream_t s);
hipError_t gc_judge(const GcArgs& a, hipStream_t s);
hipError_t gc_emit(const GcArgs& a, hipStream_t s);
// Memtable lookups and the whole get (vbf_memget.hip).  A MemDesc is an open vbf_memtable: n distinct
// keys ascending, key e = keys[off[e] .. off[e + 1]), pfx[e] its zero-padded big-endian 8-byte prefix.
struct MemDesc {
    const uint8_t* keys;
    const uint64_t* off;
    const uint64_t* pfx;
    const uint32_t* val;
    const int64_t* created;
    const uint8_t* tomb;
    uint64_t n;
};
struct MemGetArgs {
    const uint8_t* keys;
    const uint64_t* offsets;  // n + 1 absolute positions, or NULL for `stride`
    uint64_t stride, n;
    const MemDesc* layers;    // device, 2 + nro entries: the gc table, the active memtable (n = 0 when
    uint32_t nro;             // absent), then the read-only memtables in the caller's order
    const uint8_t* log;       // the log window, read only for hits in layer 0
    uint64_t log_len, log_base;
    uint8_t* found;           // outputs, each may be NULL
    uint32_t* layer;
    uint32_t* val_off;
    uint64_t* created;
};
struct StoreMergeArgs {
    uint64_t n;
    uint8_t* found;           // the memtables' answers, merged in place
    uint32_t* layer;
    uint32_t* val_off;
    uint64_t* created;
    const uint8_t* t_found;   // the tables' answers, NULL without tables
    const uint32_t* t_idx;
    const uint32_t* t_val;
    const uint64_t* t_created;
    uint32_t* table_idx;      // out: the winning table, 0xFFFFFFFF when no table answered
};
hipError_t mem_prefixes(const uint8_t* keys, const uint64_t* off, uint64_t n, uint64_t* pfx, hipStream_t s);
hipError_t mem_get(const MemGetArgs& a, bool sampled, hipStream_t s);
hipError_t store_cand(const uint8_t* found, uint64_t n, uint32_t nsst, uint8_t* cand, hipStream_t s);
hipError_t store_merge(const StoreMergeArgs& a, hipStream_t s);
// Range scans over the whole store (vbf_store_scan.hip).  nl = nmem + nsst layers in DataStore::get's
// order: the gc table, the active memtable (n = 0 when absent), the read-only memtables, the tables.
// P = nranges * nl (range, layer) pairs in range-major order; `total` candidate entries, one merged
// slot each.  Flags and error bits are the table scan's (kScan*).
struct StoreScanArgs {
    const uint8_t* bounds;      // device; lo_r / hi_r as in TableScanArgs
    const uint64_t* bounds_off; // device, 2 * nranges + 1 absolute positions
    uint64_t nranges;
    uint32_t nmem, nsst, flags; // nmem = 2 + nro
    const MemDesc* mem;         // device, nmem entries
    const TableDesc* tab;       // device, nsst entries, in the caller's table order
    const uint8_t* log;         // the log window, read only for hits in layer 0
    uint64_t log_len, log_base;
    uint64_t* first;            // [P] rank of the pair's first candidate in its layer (bounds pass)
    uint64_t* cnt;              // [P + 1] candidates of the pair (bounds pass); [P] = 0
    const uint64_t* cbase;      // [P + 1] exclusive scan of cnt; [P] = total
    uint64_t total;
    uint64_t* m_keep;           // [total + 1] 1 when the slot's key is listed, its key length then
    uint64_t* m_len;            //             (rank pass; [total] = 0)
    const uint8_t** m_src;      // [total] listed slots: the key's bytes in its first layer,
    uint64_t* m_created;        //         and the get's answer for it (rank pass)
    uint32_t* m_layer;
    uint32_t* m_tidx;
    uint32_t* m_val;
    uint8_t* m_found;
    const uint64_t* opos;       // [total + 1] exclusive scans of m_keep / m_len
    const uint64_t* kofs;
    uint32_t* err;              // [0] kScanErr bits
    uint64_t* range_off;        // outputs, each may be NULL (emit / keys passes)
    uint8_t* keys;
    uint64_t* key_off;
    uint8_t* tomb;
    uint32_t* layer;
    uint32_t* table_idx;
    uint32_t* val_off;
    uint64_t* created;
    uint8_t* found;             // 1 live / 2 tombstone per listed entry: the value fetch's `found`
};
hipError_t store_scan_bounds(const StoreScanArgs& a, hipStream_t s);
hipError_t store_scan_rank(const StoreScanArgs& a, hipStream_t s);
hipError_t store_scan_emit(const StoreScanArgs& a, hipStream_t s);
hipError_t store_scan_keys(const StoreScanArgs& a, hipStream_t s);
// Batched probe across SSTs (vbf_multi.hip).
struct MultiSst {
    const uint32_t* words;
    uint64_t m, mu;
    uint32_t k, col;                          // col: the SST's column in `out`
    uint64_t lo_beg, lo_end, hi_beg, hi_end;  // smallest / biggest key in `bounds`
};
struct MultiArgs {
    const uint8_t* keys;
    const uint64_t* offsets;
    uint64_t off_base, stride, n;
    uint32_t nsst;          // table entries
    const MultiSst* tab;    // device table, nsst entries
    const uint8_t* bounds;  // device, NULL = no key-range test
    uint8_t* out;           // n rows of out_stride bytes
    uint32_t* err;          // device word: set to 1 when a key reaches a filter with m == 0 < k
    uint32_t out_stride;    // all SSTs of the call
};
hipError_t launch_multi_probe(const MultiArgs& a, bool len_prefix, hipStream_t s);
// Interleaved groups (vbf_multi_part.hip): G <= 8 filters of one (m, k) probed together, their bits
// interleaved into one byte per position; a partitioned probe tests all G per entry.
constexpr uint32_t kMaxGroup = 8;
struct MultiGroup {
    const uint32_t* words[kMaxGroup];
    uint32_t G, k;
    uint64_t m;
    uint32_t col[kMaxGroup];
    uint64_t lo_beg[kMaxGroup], lo_end[kMaxGroup], hi_beg[kMaxGroup], hi_end[kMaxGroup];
};
bool multi_group_supported(uint64_t m, uint32_t k);
uint64_t multi_group_workspace_bytes(uint64_t n, uint64_t m, uint32_t k);
hipError_t launch_multi_probe_group(const KeyBatch& kb, const MultiGroup& g, const uint8_t* bounds, uint8_t* out,
                                    uint32_t out_stride, void* ws, uint64_t ws_bytes, hipStream_t s);
// Compaction merge (vbf_compact.hip).
struct CompactArgs {
    const uint8_t* keys;
    const uint64_t* offsets;  // arena: entry e = keys[offsets[e] .. offsets[e+1])
    const int64_t* created;   // ms
    const uint8_t* tomb;
    const uint64_t* run_off;  // device, nruns + 1 entry boundaries (run_off[0] = 0)
    uint32_t nruns;
    const uint8_t* map_keys;  // tombstone map: sorted unique keys
    const uint64_t* map_off;
    const int64_t* map_time;
    uint64_t map_n;
    int use_ttl;
    uint64_t entry_ttl_ms, tomb_ttl_ms, now_ms;
    uint64_t run_off_host_total;  // entries in all runs (host side)
};
struct GatherArgs {
    const uint8_t* keys;
    const uint64_t* offsets;
    const int64_t* created;
    const uint8_t* tomb;
    const uint32_t* val;
    const uint32_t* ids;
    uint64_t n;
    uint8_t* out_keys;
    const uint64_t* out_off;
    int64_t* out_created;
    uint8_t* out_tomb;
    uint32_t* out_val;
};
hipError_t launch_iota_u32(uint32_t* out, uint64_t n, hipStream_t s);
hipError_t compact_check_sorted(const CompactArgs& a, uint32_t* err, hipStream_t s);
hipError_t compact_merge_levels(const CompactArgs& a, const uint64_t* d_bnd_all, const uint64_t* d_tiles_all,
                                const uint32_t* nseg_per_level, const uint64_t* ntiles_per_level, uint32_t nlevels,
                                uint32_t* ping, uint32_t* pong, uint64_t* pping, uint64_t* ppong, uint64_t* split,
                                uint32_t** result, uint64_t** presult, hipStream_t s);
hipError_t merge_levels_from(const CompactArgs& a, const uint64_t* d_bnd_all, const uint64_t* d_tiles_all,
                             const uint32_t* nseg_per_level, const uint64_t* ntiles_per_level, uint32_t nlevels,
                             uint32_t* ping, uint32_t* pong, uint64_t* pping, uint64_t* ppong, uint64_t* split,
                             uint32_t** result, uint64_t** presult, hipStream_t s);
uint32_t compact_tile();
hipError_t compact_fold(const CompactArgs& a, const uint32_t* order, const uint64_t* opfx, uint64_t total,
                        uint8_t* keep, uint32_t* sel, uint8_t* upd, int64_t* upd_time, hipStream_t s);
hipError_t select_u32(void* tmp, size_t* bytes, const uint32_t* in, const uint8_t* flags, uint32_t* out,
                      uint64_t* nsel, uint64_t n, hipStream_t s);
hipError_t select_i64(void* tmp, size_t* bytes, const int64_t* in, const uint8_t* flags, int64_t* out,
                      uint64_t* nsel, uint64_t n, hipStream_t s);
hipError_t gather_lens(const uint64_t* offsets, const uint32_t* ids, uint64_t n, uint64_t* lens, hipStream_t s);
hipError_t scan_u64(void* tmp, size_t* bytes, const uint64_t* in, uint64_t* out, uint64_t n, hipStream_t s);
hipError_t gather(const GatherArgs& g, hipStream_t s);
// Memtable flush (vbf_memtable.hip).  The sort works on `soff`, its own copy of the offsets (n + 1;
// generated from the stride without offsets, every key empty when *err reports descending offsets),
// which CompactArgs::offsets then names for the tile sort, the merge levels and the keep pass.
uint32_t memtable_tile();  // == compact_tile()
hipError_t memtable_prefixes(const uint8_t* keys, const uint64_t* offsets, uint64_t stride, uint64_t n, uint32_t* err,
                             uint64_t* soff, uint32_t* ids, uint64_t* pfx, hipStream_t s);
hipError_t memtable_tile_sort(const CompactArgs& a, uint64_t n, uint32_t* ids, uint64_t* pfx, hipStream_t s);
hipError_t memtable_keep(const CompactArgs& a, const uint32_t* order, const uint64_t* opfx, uint64_t n, uint8_t* keep,
                         hipStream_t s);
// The memtable's `if !contains(key) { set(key) }` count: `first` holds m u32, `partial`
// filter_insert_partials(n) u32; the keys not contained at their turn are added to *count.
uint64_t filter_insert_partials(uint64_t n);
hipError_t filter_insert_count(const KeyBatch& kb, uint32_t m, uint32_t k, const uint32_t* words, uint32_t* first,
                               uint32_t* partial, unsigned long long* count, hipStream_t s);
hipError_t gen_sst_fixed(uint64_t seed, uint64_t base, uint64_t n, uint32_t len, uint8_t* data, uint32_t* blocks,
                         hipStream_t s);
}  // namespace vbf
