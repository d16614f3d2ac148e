/*
 * vbf.h -- C ABI of the MI355X (gfx950) Bloom-filter engine behind velarixdb's src/filter.
 *
 * This is the drop-in boundary.  Every entry point takes plain pointers and sizes, never
 * aborts or throws across the ABI, and returns an int status (VBF_OK = 0) unless noted.
 * The message of the last failure on the calling thread is available from vbf_last_error().
 *
 * Reference interface replaced (velarixdb 0.0.17, /root/reference):
 *   BloomFilter struct                 src/filter/bf.rs:38-58      -> vbf_filter (opaque handle)
 *   BloomFilter::new                   src/filter/bf.rs:62-81      -> vbf_filter_new / vbf_size
 *   BloomFilter::set                   src/filter/bf.rs:84-92      -> vbf_filter_set_host / _dev
 *   BloomFilter::contains              src/filter/bf.rs:95-105     -> vbf_filter_contains_host / _dev
 *   BloomFilter::build_filter_from_entries src/filter/bf.rs:126-128 -> vbf_filter_set_host (batch)
 *                                                                     / vbf_filter_set_host_async
 *   BloomFilter::recover_meta          src/filter/bf.rs:135-150    -> vbf_filter_recover
 *   BloomFilter::serialize             src/filter/bf.rs:158-172    -> vbf_filter_serialize
 *   BloomFilter::write + recover_meta + lazy rebuild, bits persisted (bf.rs:114-150,
 *     range.rs:117-128)                                            -> vbf_filter_serialize_ext / _recover_ext
 *   FilterFileNode::recover            src/fs/mod.rs:768-796       -> vbf_meta_parse
 *   BloomFilter::clear                 src/filter/bf.rs:180-195    -> vbf_filter_clear
 *   num_elements / num_bits / num_of_hash_functions bf.rs:198-213  -> vbf_filter_num_*
 *   calculate_hash                     src/filter/bf.rs:222-227    -> vbf_hashes_dev (parity)
 *   calculate_no_of_bits               src/filter/bf.rs:230-233    -> vbf_num_bits
 *   calculate_no_of_hash_function      src/filter/bf.rs:236-239    -> vbf_num_hash_functions
 *   Clone (shares the bit array)       src/filter/bf.rs:242-254    -> vbf_filter_clone
 *   Default                            src/filter/bf.rs:256-267    -> vbf_filter_default
 *   DataFileNode::load_entries         src/fs/mod.rs:275-332       -> vbf_sst_decode_dev / _host
 *   index.db block offsets             src/index/indexer.rs:151-170 -> vbf_sst_index_blocks
 *   lazy filter rebuild                src/key_range/range.rs:117-128 -> vbf_filter_rebuild_from_sst_*
 *   KeyRange::filter_sstables_by_key_range src/key_range/range.rs:91-147 -> vbf_multi_probe_* (batch)
 *   SizedTierRunner::merge_ssts_in_buckets src/compactors/sized.rs:170-320 -> vbf_compact_merge_*
 *   Table::write_to_file               src/sst/table.rs:287-324    -> vbf_sst_encode_dev / _host
 *   one bucket, merge to files + filter src/compactors/sized.rs:170-200 -> vbf_compact_write_host
 *   Index::get                         src/index/indexer.rs:170-172 -> vbf_table_get_* (index step)
 *   IndexFileNode::get_from_index      src/fs/mod.rs:667-710       -> vbf_table_get_* (index step)
 *   Table::get                         src/sst/table.rs:184-193    -> vbf_table_get_* (block step)
 *   DataFileNode::find_entry           src/fs/mod.rs:334-389       -> vbf_table_get_* (block step)
 *   DataStore::search_key_in_sstables  src/db/store.rs:579-612     -> vbf_table_open_* + vbf_table_get_*
 *   DataStore::seek (a stub there)     src/range/range_iterator.rs:47-60 -> vbf_table_scan_* (the key side)
 *   ValueLog::get                      src/vlog/v_log.rs:205-207   -> vbf_vlog_open_* + vbf_vlog_get_*
 *   VLogFileNode::get                  src/fs/mod.rs:470-518       -> vbf_vlog_get_* (header, key skip, value)
 *   DataStore::get_value_from_vlog     src/db/store.rs:628-641     -> vbf_vlog_get_* (tombstone -> no value)
 *   ValueLog::append                   src/vlog/v_log.rs:173-196   -> vbf_vlog_encode_* (val_offsets)
 *   ValueLogEntry::serialize           src/vlog/v_log.rs:291-309   -> vbf_vlog_encode_* (the bytes)
 *   ValueLog::recover                  src/fs/mod.rs:520-577       -> vbf_vlog_walk_* (budget UINT64_MAX)
 *   read_chunk_to_garbage_collect      src/fs/mod.rs:579-651       -> vbf_vlog_walk_* (budget = bytes)
 *   MemTable::insert (the SkipMap)     src/memtable/mem.rs:207-221 -> vbf_memtable_sort_* (last put wins)
 *   MemTable::insert (contains, set)   src/memtable/mem.rs:209-211 -> vbf_filter_insert_host / _dev
 *   Flusher::flush                     src/flush/flusher.rs:37-64  -> vbf_flush_write_host
 *   Table::write_to_file (a memtable)  src/sst/table.rs:258-326    -> vbf_flush_write_host
 *   DataStore::put (log, then insert)  src/db/store.rs:215-243     -> vbf_vlog_encode_* + vbf_flush_write_host
 *   GC::gc_handler                     src/gc/garbage_collector.rs:168-262 -> vbf_gc_collect_host
 *   GC::get                            src/gc/garbage_collector.rs:429-469 -> vbf_gc_collect_host (overlay, tables, log)
 *   write_tail_to_disk                 src/gc/garbage_collector.rs:265-275 -> vbf_gc_collect_host (put 0 of `append`)
 *   write_valid_entries_to_vlog        src/gc/garbage_collector.rs:304-317 -> vbf_gc_collect_host (the rest of `append`)
 *   GC::put                            src/gc/garbage_collector.rs:404-419 -> vbf_gc_collect_host (put_val_offsets,
 *                                                                             put_tombstones)
 *   MemTable (an immutable one)        src/memtable/mem.rs:207-221 -> vbf_memtable_open_* (a batch of inserts)
 *   MemTable::get                      src/memtable/mem.rs:223-230 -> vbf_memtable_get_* (per layer)
 *   DataStore::search_gc_entries       src/db/store.rs:489-501     -> vbf_memtable_get_* (the gc layer)
 *   DataStore::get                     src/db/store.rs:442-481     -> vbf_memtable_get_* (steps 0-2),
 *                                                                     vbf_store_get_host (the whole get)
 *
 * Key batches.  `keys` holds the key bytes back to back.  When `offsets` is non-NULL it has
 * n+1 nondecreasing entries and key j is keys[offsets[j] .. offsets[j+1]) (positions are
 * absolute in `keys`; offsets[0] need not be 0); otherwise key j is
 * keys[j*stride .. (j+1)*stride).  Offsets live where the keys live (device or host).  `len_prefix` = 1 hashes LE64(len) || key, which is
 * Rust's `Hash for [u8]` / `Vec<u8>` (every production call site: memtable/mem.rs:209-210,224,
 * key_range/range.rs:130,136,171, filter/bf.rs:127).  len_prefix = 0 hashes the bytes as given,
 * for callers that pre-encode other Hash impls (usize -> 8 LE bytes, as bf.rs's tests use).
 *
 * Filter words.  ceil(m/32) uint32 words, bit i = words[i/32] bit (i%32): the storage of
 * bit-vec 0.6.3 `BitVec<u32>` (Cargo.toml:19).  Builds OR into existing bits, never clear.
 *
 * Threads.  Every `_host` entry point and every call on a handle (vbf_filter_*, vbf_table_*,
 * vbf_vlog_*) may be made from any number of threads at once, on the same or on different devices,
 * with the answers a single caller gets.  Calls on one filter are ordered by the filter's lock, as
 * the reference's Mutex<BitVec> orders them; a vbf_table, a vbf_vlog and a vbf_memtable are immutable once opened,
 * so any number of gets and scans may read them together.  Per device the library serialises what
 * shares its staging: vbf_build_host, vbf_probe_host and the filters' set_host / contains_host /
 * words copies take turns on the device's two staging streams, and the other `_host` entry points
 * (sst_decode, sst_encode, rebuild_from_sst, multi_probe, compact_merge, compact_write,
 * table_open, table_get, table_scan, vlog_open, vlog_get, vlog_encode, vlog_walk, memtable_sort,
 * flush_write, gc_collect, memtable_open, memtable_export, memtable_encode, memtable_get, store_get,
 * and filter_insert_host on a device-resident filter) take turns on its shared
 * stream, each from its first upload to its last download; the two groups overlap each other, and
 * devices never wait for each other.  A call that spans several devices (vbf_multi_probe_host over filters on several GPUs)
 * holds one device at a time.  Locks are taken filters first (in address order), then the device.
 * The `_dev` entry points take no device lock: their workspace is cached per stream and belongs
 * to the caller's stream, so two threads must not drive one stream through the library at the
 * same time (different streams are independent).  vbf_release_workspaces waits for the `_host`
 * calls in flight and keeps new ones out while it frees; no `_dev` call may be in flight then.
 */
#ifndef VBF_H
#define VBF_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VBF_OK 0
#define VBF_EINVAL (-1)   /* bad argument (where the reference asserts: bf.rs:63-67)    */
#define VBF_EHIP (-2)     /* HIP runtime / launch failure                               */
#define VBF_ENOMEM (-3)   /* device or pinned-host allocation failed                    */
#define VBF_ENODEV (-4)   /* no usable gfx950 device                                    */
#define VBF_EDIVZERO (-5) /* m == 0 with k > 0: the reference panics (`% 0`, bf.rs:88)   */

/* `device` of a filter whose bits live in host memory (see "Residency" below). */
#define VBF_DEVICE_HOST (-1)
/* `device` for vbf_filter_new, _new_sized, _default, _recover, _recover_ext and _migrate: the library places the filter,
 * round-robin over the visible devices (successive filters land on different GPUs). */
#define VBF_DEVICE_AUTO (-2)

const char* vbf_version(void);
const char* vbf_last_error(void); /* thread-local; "" when the last call succeeded */
int vbf_device_count(int* count);

/* Kernel-phase timing with hipEvents on the launch streams (for bench.py's roofline):
 * phases 0 tile-sort, 1 transpose, 2 segment-OR (partitioned build), 3 atomic build, 4 probe,
 * 5 data.db walk, 6 data.db scan, 7 data.db emit, 8 compaction merge levels, 9 fold, 10 select,
 * 11 partitioned-probe pack, 12 probe segment test, 13 probe answers, 14 SST-encode tile tables,
 * 15 encode table scan + block count, 16 index.db emit, 17 data.db emit, 18 table open (side
 * tables + validation), 19 table get, 20 table scan bounds + rank (with their scans), 21 table scan
 * emit + key copy, 22 value-log fetch sizes + scan, 23 value-log fetch copy, 24 value-log encode
 * (its check and its copy), 25 memtable tile sort (with its prefix pass), 26 memtable merge levels
 * + keep flags + select, 27 filter insert (count passes and the build), 28 GC judge (with its overlay
 * search, scan and select), 29 GC emit, 30 memtable get.
 * vbf_profile_read synchronizes, returns per-phase summed ms and launch counts, and resets; it
 * fills the first `nphases` phases, so a caller built against a shorter list keeps working (the
 * later phases' records are dropped). */
int vbf_profile_enable(int on);
int vbf_profile_read(double* ms, uint64_t* launches, int nphases);

/* ---- sizing (host arithmetic, glibc log, Rust `as u32` saturation) ---- */
uint32_t vbf_num_bits(uint64_t n, double p);              /* bf.rs:230-233 */
uint32_t vbf_num_hash_functions(uint32_t m, uint32_t n);  /* bf.rs:236-239 */
/* bf.rs:62-70: asserts p >= 0 and n > 0 (-> VBF_EINVAL), m = num_bits(n, p),
 * k = num_hash_functions(m, n as u32). */
int vbf_size(double p, uint64_t n, uint32_t* m, uint32_t* k);

/* ---- filter.db metadata: u32 k | u32 n | f64 p, little-endian, 16 bytes ---- */
void vbf_meta_serialize(uint32_t k, uint32_t n, double p, uint8_t out[16]); /* bf.rs:158-172 */
int vbf_meta_parse(const uint8_t* in, size_t len, uint32_t* k, uint32_t* n, double* p); /* fs/mod.rs:768-796 */

/* ---- stateless kernels on device-resident buffers; `stream` is a hipStream_t (NULL = the
 *      legacy default stream).  Calls are asynchronous on that stream. ---- */
int vbf_build_dev(const uint8_t* keys, const uint64_t* offsets, uint64_t stride, uint64_t n,
                  int len_prefix, uint32_t m, uint32_t k, uint32_t* words, void* stream);
int vbf_probe_dev(const uint8_t* keys, const uint64_t* offsets, uint64_t stride, uint64_t n,
                  int len_prefix, uint32_t m, uint32_t k, const uint32_t* words, uint8_t* out,
                  void* stream);
/* Build strategies.  ATOMIC: one lane per key, k global atomicOr's per key.  PARTITIONED:
 * hash + per-tile LDS sort by 2^20-bit segment, then one workgroup ORs each segment in LDS
 * (no global atomics; needs 1 <= k <= 32 and a device workspace the library caches per
 * stream).  AUTO picks PARTITIONED for batches of >= 2^22 bit indices.  Results are
 * bit-identical.  vbf_build_dev/_ex expect stream-ordered exclusive use of `words` (the
 * partitioned path rewrites whole segments); the host and handle APIs merge atomically. */
#define VBF_BUILD_AUTO 0
#define VBF_BUILD_ATOMIC 1
#define VBF_BUILD_PARTITIONED 2
/* OR into a build strategy: `words` holds no filter yet -- BloomFilter::new (bf.rs:62-81, an
 * all-zero BitVec) fused with build_filter_from_entries (bf.rs:126-128), as flush and compaction
 * call them.  Every one of the ceil(m/32) words is written (prior contents ignored, the bits of
 * keys set, all others 0), with no separate zero fill: the partitioned build's segment pass
 * writes its segments without reading them first.  Without the flag a build ORs into `words`. */
#define VBF_BUILD_FRESH 0x100
int vbf_build_dev_ex(const uint8_t* keys, const uint64_t* offsets, uint64_t stride, uint64_t n,
                     int len_prefix, uint32_t m, uint32_t k, uint32_t* words, int strategy,
                     void* stream);
/* Device bytes the partitioned build of n keys needs as workspace (0 if unsupported): the tile
 * image (~2.6 bytes per bit index) and the run ends of one build chunk of up to 2^32 bit indices
 * -- about 11 GB for a chunk of 2^32 indices (config 5's 1B keys at k = 4), kept per stream until
 * vbf_release_workspaces.  When that allocation fails the build retries with half the chunk, down
 * to 2^28 indices (VBF_WS_MAX_BYTES caps the workspace the same way). */
uint64_t vbf_build_workspace_bytes(uint64_t n, uint32_t m, uint32_t k);
/* Free every cached workspace (synchronizes the streams that own them).  Safe beside `_host` and
 * handle calls on other threads: it waits for those in flight on every device and holds new ones
 * back until the buffers are gone (they allocate again).  The `_dev` workspaces belong to the
 * callers' streams: no `_dev` call may be running, or be started, while this runs. */
int vbf_release_workspaces(void);
/* Adds the number of keys the filter answers "present" for to *count_dev (device u64). */
int vbf_probe_count_dev(const uint8_t* keys, const uint64_t* offsets, uint64_t stride, uint64_t n,
                        int len_prefix, uint32_t m, uint32_t k, const uint32_t* words,
                        unsigned long long* count_dev, void* stream);

/* Same with an explicit strategy: VBF_BUILD_ATOMIC (one lane per key, early exit on the first
 * clear bit, random filter loads), VBF_BUILD_PARTITIONED (keys hashed in tiles, entries sorted by
 * 2^20-bit filter segment, every bit test against a segment staged in LDS; all k hashes per key),
 * VBF_BUILD_AUTO (the calls above): for batches of >= 2^24 bit tests against filters of >= 2^26
 * bits it probes the first 65 536 keys by gather, reads their hit count back (one stream
 * synchronisation) and goes partitioned when >= 35 % hit (positive sweeps), gather otherwise.
 * Identical answers either way. */
int vbf_probe_dev_ex(const uint8_t* keys, const uint64_t* offsets, uint64_t stride, uint64_t n,
                     int len_prefix, uint32_t m, uint32_t k, const uint32_t* words, uint8_t* out,
                     int strategy, void* stream);
int vbf_probe_count_dev_ex(const uint8_t* keys, const uint64_t* offsets, uint64_t stride,
                           uint64_t n, int len_prefix, uint32_t m, uint32_t k,
                           const uint32_t* words, unsigned long long* count_dev, int strategy,
                           void* stream);
/* out[j*k + i] = calculate_hash(key_j, i) (bf.rs:222-227). */
int vbf_hashes_dev(const uint8_t* keys, const uint64_t* offsets, uint64_t stride, uint64_t n,
                   int len_prefix, uint32_t k, uint64_t* out, void* stream);
/* dst |= src over nwords (16-byte aligned): merging partial filters of one key set. */
int vbf_or_words_dev(uint32_t* dst, const uint32_t* src, uint64_t nwords, void* stream);
/* dst[i] = OR over p < nparts of src[p * part_stride + i], i < nwords, in one pass (the fold of the
 * multi-GPU OR all-reduce: every rank's copy of one bit range, received back to back; the bitwise
 * OR that merges partial filters of one key set, bf.rs:89).  16-byte aligned pointers, part_stride
 * a multiple of 4 words and >= nwords; dst may be src (part 0) itself. */
int vbf_or_fold_dev(uint32_t* dst, const uint32_t* src, uint64_t nwords, uint32_t nparts, uint64_t part_stride,
                    void* stream);
/* *count_dev += popcount(words[0..nwords)). */
int vbf_popcount_dev(const uint32_t* words, uint64_t nwords, unsigned long long* count_dev,
                     void* stream);

/* ---- synthetic key sets (benchmarks/tests; definitions in DESIGN.md, section Workloads) ---- */
int vbf_gen_fixed_dev(uint64_t seed, uint64_t base, uint64_t n, uint32_t len, uint8_t* out,
                      void* stream);
int vbf_gen_var_dev(uint64_t seed, uint64_t base, uint64_t n, const uint64_t* offsets,
                    uint8_t* out, void* stream);

/* ---- one-shot host-pointer variants: keys/words in host memory, chunked H2D through pinned
 *      staging on `device`, synchronous.  Build ORs into `words` (nwords = ceil(m/32)). ---- */
int vbf_build_host(const uint8_t* keys, const uint64_t* offsets, uint64_t stride, uint64_t n,
                   int len_prefix, uint32_t m, uint32_t k, uint32_t* words, uint64_t nwords,
                   int device);
int vbf_probe_host(const uint8_t* keys, const uint64_t* offsets, uint64_t stride, uint64_t n,
                   int len_prefix, uint32_t m, uint32_t k, const uint32_t* words, uint64_t nwords,
                   uint8_t* out, int device);

/* Compaction fan-in (src/compactors/sized.rs:170-200 builds one filter per merged SSTable, each
 * from its own entries): independent builds spread over devices[0..ndevices), shard s on
 * devices[s % ndevices], one host thread and its own staging streams per device, shards of one
 * device in order.  Each shard is a vbf_build_host call: host keys, ORed into its host words.
 * Per-shard status lands in shards[s].status; the return value is the first failure's (the
 * message is this thread's vbf_last_error). */
typedef struct vbf_shard {
    const uint8_t* keys;
    const uint64_t* offsets; /* n+1 host offsets, or NULL for fixed `stride` */
    uint64_t stride;
    uint64_t n;
    int len_prefix;
    uint32_t m, k;
    uint32_t* words;         /* host, ceil(m/32) words, OR-accumulated */
    uint64_t nwords;
    int status;              /* out */
} vbf_shard;
int vbf_build_shards_host(vbf_shard* shards, uint64_t nshards, const int* devices, int ndevices);

/* ---- BloomFilter handle: the bit array lives in HBM on `device` ----
 *
 * Residency.  A filter created on a device keeps its bits in that GPU's HBM: batch builds and
 * probes run as kernels, and every call on the filter is ordered after the filter's previous
 * one whatever stream either ran on (the reference's Mutex<BitVec>, bf.rs:85,96): a _dev call
 * is queued behind the last asynchronous operation on the filter, a host call waits for it.
 * A filter created with device = VBF_DEVICE_HOST keeps its bits in host memory and runs
 * set/contains on the CPU inside this library (same SipHash-1-3 rounds, Rust's `hash % m`):
 * the memtable's filter, one contains + set per put (memtable/mem.rs:207-221) and one contains
 * per get (:223-230), where a kernel launch per key would cost two PCIe round trips.  Such a
 * filter needs no GPU; the _dev, rebuild and multi-probe entry points reject it (VBF_EINVAL).
 * vbf_filter_migrate moves a filter's bits between host and devices in place (clones follow).
 *
 * Element count.  no_of_elements (bf.rs:46) lives in the handle only: set_host / set_dev /
 * rebuild add the number of keys, recover loads the stored n, clones copy it (bf.rs:248), and
 * vbf_filter_set_num_elements assigns it (bf.rs:143).  A binding keeps no second counter. */
typedef struct vbf_filter vbf_filter;

int vbf_filter_new(double p, uint64_t no_of_elements, int device, vbf_filter** out); /* bf.rs:62-81 */
int vbf_filter_default(int device, vbf_filter** out);                               /* bf.rs:256-267 */
/* A filter of exactly m bits and k hash functions (the struct's pub fields set directly,
 * bf.rs:38-58), no elements, false_positive_rate p. */
int vbf_filter_new_sized(uint32_t m, uint32_t k, double p, int device, vbf_filter** out);
/* recover_meta (bf.rs:135-150): k and n from the 16-byte metadata, m recomputed from n, bits 0. */
int vbf_filter_recover(const uint8_t* meta, size_t len, int device, vbf_filter** out);
int vbf_filter_clone(const vbf_filter* f, vbf_filter** out); /* shares the bit array, bf.rs:242-254 */
void vbf_filter_free(vbf_filter* f);

/* set over a batch (bf.rs:84-92 per key; build_filter_from_entries bf.rs:126-128).
 * no_of_elements += n (u32, wrapping like AtomicU32::fetch_add).  _host takes host keys (any
 * residency: a host-resident filter hashes them on the CPU, a device-resident one streams them
 * to its GPU); _dev takes device keys and a stream (device-resident filters only). */
int vbf_filter_set_host(vbf_filter* f, const uint8_t* keys, const uint64_t* offsets,
                        uint64_t stride, uint64_t n, int len_prefix);
int vbf_filter_set_dev(vbf_filter* f, const uint8_t* keys, const uint64_t* offsets, uint64_t stride,
                       uint64_t n, int len_prefix, void* stream);
/* set over host keys, returning before the work is done (build_filter_from_entries for a
 * device-resident filter, bf.rs:126-128, without blocking the caller).  The batch is queued on
 * its device's worker thread, which streams it to the GPU exactly as vbf_filter_set_host does;
 * no_of_elements += n at once.  Every later call on the filter (or a clone) first waits for the
 * queued sets, so results are those of the synchronous call; a failure is returned by the next
 * call on the filter.  With `release` NULL the library copies the keys before returning (the
 * caller may reuse its buffers); otherwise it reads the caller's buffers and calls
 * release(release_ctx) from its worker once it no longer needs them (a Rust caller hands over
 * its packed Vec and drops it there).  Host-resident filters set synchronously (then release). */
int vbf_filter_set_host_async(vbf_filter* f, const uint8_t* keys, const uint64_t* offsets, uint64_t stride,
                              uint64_t n, int len_prefix, void (*release)(void*), void* release_ctx);
/* Wait until every queued or in-flight operation on the filter has finished (returns a queued
 * set's failure).  vbf_filter_busy: 1 while such work is outstanding, 0 when idle, < 0 error. */
int vbf_filter_sync(vbf_filter* f);
int vbf_filter_busy(const vbf_filter* f);
/* Writers of the bits through vbf_filter_words_dev (an OR/merge kernel on the caller's stream)
 * bracket their work: vbf_filter_stream_wait makes `stream` wait for the filter's previous
 * operations, vbf_filter_stream_record makes the work queued on `stream` so far the filter's
 * last operation (later calls are ordered after it; the host mirror is refreshed behind it).
 * Every write through the pointer must be declared with vbf_filter_stream_record: once
 * vbf_filter_words_dev has handed the pointer out, the library no longer trusts its host mirror
 * (host reads copy the words from the GPU each time, and migrate copies instead of assuming the
 * words are zero) until the next vbf_filter_stream_record; a write made after that record and
 * not recorded itself may be missed by host-side reads.  A writer that skips stream_wait must
 * synchronize its stream before the next call on the filter.
 * A failed asynchronous set is returned once, by the next call on the filter that waits for
 * the queue (every call but vbf_filter_busy and the accessors).  `release` runs after the job
 * counts as done, so it may call back into the library.  A child forked while a set is queued
 * does not run it: the child's next call on that filter returns VBF_EINVAL.  More generally, HIP
 * does not survive fork(): in a child of a process that used the GPU through the library, every
 * call on a device-resident filter (and creating one) and every stateless device-pointer entry
 * point returns VBF_EINVAL before any HIP call, and freeing a handle there releases no device
 * memory (it is the parent's); host-resident filters work as usual. */
int vbf_filter_stream_wait(const vbf_filter* f, void* stream);
int vbf_filter_stream_record(vbf_filter* f, void* stream);
/* contains over a batch (bf.rs:95-105): out[j] = 1 when every one of the k bits is set.
 * Host mirror: a device-resident filter keeps a pinned host copy of its bits, refreshed after
 * device writes, and vbf_filter_contains_host / vbf_multi_probe_host batches of at most
 * VBF_MIRROR_MAX_KEYS (env, default 256) keys answer from it on the CPU -- the read path's one
 * contains per SST per get (key_range/range.rs:130,136,171) costs what it costs on a
 * host-resident filter instead of a PCIe round trip.  Larger batches run on the GPU. */
int vbf_filter_contains_host(const vbf_filter* f, const uint8_t* keys, const uint64_t* offsets,
                             uint64_t stride, uint64_t n, int len_prefix, uint8_t* out);
int vbf_filter_contains_dev(const vbf_filter* f, const uint8_t* keys, const uint64_t* offsets,
                            uint64_t stride, uint64_t n, int len_prefix, uint8_t* out, void* stream);

uint32_t vbf_filter_num_bits(const vbf_filter* f);           /* bf.rs:204-207 */
uint32_t vbf_filter_num_elements(const vbf_filter* f);       /* bf.rs:198-201 */
uint32_t vbf_filter_num_hash_functions(const vbf_filter* f); /* bf.rs:210-213 */
double vbf_filter_false_positive_rate(const vbf_filter* f);  /* bf.rs:54 */
int vbf_filter_device(const vbf_filter* f);          /* a device id or VBF_DEVICE_HOST */
/* Bytes of host memory the filter's bits hold: the host-resident words (allocated on their first
 * use, so a filter created on the host and migrated to a GPU before any set -- the compaction
 * filter of compactors/sized.rs:192-193 -- holds none) plus a device filter's pinned host mirror. */
uint64_t vbf_filter_host_bytes(const vbf_filter* f);
uint32_t* vbf_filter_words_dev(const vbf_filter* f); /* device pointer to the bit array (NULL if host) */
/* Read-only device pointer to the bit array (NULL if host-resident), e.g. the source of an OR
 * merge: unlike vbf_filter_words_dev it does not mark the bits externally written, so the host
 * mirror stays trusted.  Readers order themselves with vbf_filter_stream_wait. */
const uint32_t* vbf_filter_words_dev_read(const vbf_filter* f);
/* no_of_elements = n (bf.rs:143 assigns it on recover_meta). */
int vbf_filter_set_num_elements(vbf_filter* f, uint32_t n);
/* Binding bookkeeping kept in the handle, so a binding's BloomFilter struct needs no private
 * fields: velarixdb builds `BloomFilter { file_path: Some(..), ..Default::default() }` outside
 * filter::bf (db/recovery.rs:143-146, tests/workload.rs:309-312), which a private field would
 * forbid.  Both are per handle and copied by vbf_filter_clone, like the struct's plain fields
 * (bf.rs:242-254).
 * sst entries: the entry count of the SST this filter was batch-built from
 * (build_filter_from_entries), VBF_EXT_NONE until set; the binding's write() passes it to
 * vbf_filter_serialize_ext.  restored: vbf_filter_recover_ext loaded persisted bits;
 * vbf_filter_take_restored returns 1 once (and clears it), so the build_filter_from_entries that
 * follows recover_meta on the lazy-rebuild path (range.rs:117-128) can skip the rebuild. */
int vbf_filter_set_sst_entries(vbf_filter* f, uint64_t entries);
uint64_t vbf_filter_sst_entries(const vbf_filter* f);
int vbf_filter_take_restored(vbf_filter* f); /* 1 or 0; < 0 on error */
/* Move the (shared) bit array to `device` or to host memory (VBF_DEVICE_HOST), in place. */
int vbf_filter_migrate(vbf_filter* f, int device);
int vbf_filter_serialize(const vbf_filter* f, uint8_t out[16]); /* bf.rs:158-172 */
/* clear (bf.rs:180-195): zero this filter's (shared) bits and return a fresh empty filter with
 * the same m, k and p. */
int vbf_filter_clear(vbf_filter* f, vbf_filter** out);
/* Bit-array persistence: copy the ceil(m/32) words out / in. */
int vbf_filter_words_to_host(const vbf_filter* f, uint32_t* out, uint64_t nwords);
int vbf_filter_words_from_host(vbf_filter* f, const uint32_t* in, uint64_t nwords);

/* Host mirror mode (see contains above): OFF frees it and sends every contains to the GPU;
 * LAZY (default, env VBF_MIRROR) fills it with one D2H on the first small contains after a
 * device write; EAGER queues that D2H behind every device write, off the read path. */
#define VBF_MIRROR_OFF 0
#define VBF_MIRROR_LAZY 1
#define VBF_MIRROR_EAGER 2
int vbf_filter_set_mirror(vbf_filter* f, int mode);

/* filter.db with the bit array persisted after the reference's 16 bytes.
 * Layout (little-endian): the 16-byte header of vbf_filter_serialize (bf.rs:158-172), then
 *   u32 magic "VBFW" | u32 version 2 | u32 m | u32 nwords | u64 entries | u64 checksum | words
 * The reference reads exactly 16 bytes (fs/mod.rs:768-796), so the file stays readable by it.
 * The words are those recover_meta + build_filter_from_entries (range.rs:117-128) would rebuild:
 * a filter of m = num_bits(n_stored, p) bits (bf.rs:144-147) holding the SST's `entries` keys.
 *
 * vbf_filter_serialize_ext: `entries` = the SST's data.db entry count, or VBF_EXT_NONE for the
 * reference's 16 bytes alone.  When the filter's own m equals that recovery m (a compaction-built
 * filter, sized from its table's entries: sized.rs:192-193) its words are written; otherwise
 * (a memtable-born filter, sized from the write-buffer capacity: mem.rs:188-191) the recovery-
 * shaped words are built from `keys` (the SST's `entries` keys, layout as for set; on the CPU for
 * a host-resident filter, on its GPU otherwise), and with no keys only the 16 bytes are written.
 * *len = bytes needed; buf NULL is a size query; cap < *len is VBF_EINVAL.
 * vbf_filter_recover_ext: vbf_filter_recover, then, when the extension is present, intact
 * (checksum) and of the recovered m, loads its words and sets no_of_elements = n + entries
 * (what the rebuild leaves), *restored = 1: the caller skips the rebuild.  Otherwise
 * *restored = 0 and the caller rebuilds as the reference does. */
#define VBF_EXT_NONE UINT64_MAX
int vbf_filter_serialize_ext(const vbf_filter* f, const uint8_t* keys, const uint64_t* offsets, uint64_t stride,
                             uint64_t entries, int len_prefix, uint8_t* buf, uint64_t cap, uint64_t* len);
int vbf_filter_recover_ext(const uint8_t* bytes, uint64_t len, int device, vbf_filter** out, int* restored);

/* Synthetic data.db (bench / tests): n entries whose keys are vbf_gen_fixed_dev's, value offset
 * (u32)j, created_at 1720785462000 + j ms, tombstone j % 97 == 0, blocked as
 * Table::write_to_file blocks them (src/sst/table.rs:295-324): floor(4096 / (len + 17)) entries
 * per block.  data: n * (len + 17) bytes; blocks: ceil(n / per_block) u32 start offsets. */
int vbf_gen_sst_fixed_dev(uint64_t seed, uint64_t base, uint64_t n, uint32_t len, uint8_t* data,
                          uint32_t* blocks, void* stream);

/* ---- SST data.db decode ----
 * data.db = blocks of whole entries, entry = u32 key_len | key | u32 value offset | i64
 * created_at ms | u8 tombstone (src/block/block_manager.rs:168-190), each block <= 4096 bytes
 * (:121-125); index.db holds one u32 key_len | key | u32 block offset record per block
 * (src/index/indexer.rs:151-170).  The decode is block-parallel, so it needs the block offsets. */

/* index.db bytes -> block start offsets.  Writes min(cap, count) offsets (offsets may be NULL)
 * and the count to *nblocks; VBF_EINVAL on a truncated record.  Host-only. */
int vbf_sst_index_blocks(const uint8_t* index, uint64_t len, uint32_t* offsets, uint64_t cap,
                         uint64_t* nblocks);

/* DataFileNode::load_entries (src/fs/mod.rs:275-332) on the device.  data/blocks are device
 * pointers; outputs are device pointers, each may be NULL: keys (packed key bytes, 4-byte aligned,
 * keys_cap >= len - 17 n), offsets (n+1 absolute positions in keys: the build's key layout),
 * val_offsets, created_ms, tombstones (1 iff the byte is 1, as the reference reads it),
 * entries_cap >= n (+1 for offsets).  *n_out = entry count, also when the outputs are too small
 * (VBF_EINVAL) so a first call with NULL outputs sizes them.  Synchronizes the stream once (the
 * entry count); the output pass is left queued on it.  A malformed file (entry crossing its block,
 * offsets out of order) is VBF_EINVAL, where the reference reports UnexpectedEof. */
int vbf_sst_decode_dev(const uint8_t* data, uint64_t len, const uint32_t* blocks, uint64_t nblocks,
                       uint8_t* keys, uint64_t keys_cap, uint64_t* offsets, uint32_t* val_offsets,
                       uint64_t* created_ms, uint8_t* tombstones, uint64_t entries_cap,
                       uint64_t* n_out, void* stream);

/* Same from host buffers (the data.db and index.db file contents) to host outputs; decoded on
 * `device`.  Synchronous. */
int vbf_sst_decode_host(const uint8_t* data, uint64_t len, const uint8_t* index, uint64_t index_len,
                        uint8_t* keys, uint64_t keys_cap, uint64_t* offsets, uint32_t* val_offsets,
                        uint64_t* created_ms, uint8_t* tombstones, uint64_t entries_cap,
                        uint64_t* n_out, int device);

/* ---- SST data.db / index.db encode ----
 * Table::write_to_file (src/sst/table.rs:287-324) on the device, the inverse of vbf_sst_decode_*:
 * entries laid back to back, entry = u32 key_len | key | u32 value offset | i64 created_at ms | u8
 * tombstone (Block::serialize, src/block/block_manager.rs:176-193), cut into blocks greedily -- a
 * block takes the next entry unless size + (L + 17) > 4096 (Block::is_full, :159-161) -- and one
 * index.db record per block, u32 key_len | key | u32 block_start with the block's LAST key
 * (write_block, table.rs:333-340; Index::serialize_entry, src/index/indexer.rs:151-170).
 * Keys in the layout of every entry point (offsets: n+1 absolute positions, offsets[0] need not be
 * 0; or NULL with a fixed stride).  val_offsets / created_ms / tombstones may each be NULL (zeros
 * are written); a tombstone byte != 0 is written as 1.  Key order is not checked.
 * Outputs: data, index and blocks (the u32 block start offsets, what vbf_sst_decode_dev takes) may
 * each be NULL; all three NULL is the size query.  *data_len, *index_len and *nblocks are always
 * written, also when a capacity is too small (VBF_EINVAL, nothing written to the outputs).
 * Capacities that always suffice: key bytes + 17 n, key bytes + 8 n, n.
 * Synchronizes the stream once (the sizes; never with a fixed stride, whose blocks are closed-form);
 * the output passes are left queued on it.  n == 0 is VBF_OK with zero sizes and no device work.
 * VBF_EINVAL: a key longer than 4079 bytes (the reference fails the flush with BlockIsFull,
 * block_manager.rs:121-125), descending offsets, or a data.db of 2^32 bytes or more (index.db's
 * u32 block_start could not address it; the reference would truncate silently). */
int vbf_sst_encode_dev(const uint8_t* keys, const uint64_t* offsets, uint64_t stride, uint64_t n,
                       const uint32_t* val_offsets, const int64_t* created_ms, const uint8_t* tombstones,
                       uint8_t* data, uint64_t data_cap, uint64_t* data_len,
                       uint8_t* index, uint64_t index_cap, uint64_t* index_len,
                       uint32_t* blocks, uint64_t blocks_cap, uint64_t* nblocks, void* stream);
/* Same with every array in host memory, encoded on `device`.  Synchronous. */
int vbf_sst_encode_host(const uint8_t* keys, const uint64_t* offsets, uint64_t stride, uint64_t n,
                        const uint32_t* val_offsets, const int64_t* created_ms, const uint8_t* tombstones,
                        uint8_t* data, uint64_t data_cap, uint64_t* data_len,
                        uint8_t* index, uint64_t index_cap, uint64_t* index_len,
                        uint32_t* blocks, uint64_t blocks_cap, uint64_t* nblocks, int device);

/* The lazy rebuild of src/key_range/range.rs:117-128 (load_entries_from_file then
 * build_filter_from_entries): decode data.db on the filter's device and OR every key into its
 * bits (len_prefix = 1), no_of_elements += n.  *n_out (may be NULL) = entries decoded.
 * _dev: device data/blocks, queued on `stream` after one count readback.  _host: file bytes. */
int vbf_filter_rebuild_from_sst_dev(vbf_filter* f, const uint8_t* data, uint64_t len,
                                    const uint32_t* blocks, uint64_t nblocks, uint64_t* n_out,
                                    void* stream);
int vbf_filter_rebuild_from_sst_host(vbf_filter* f, const uint8_t* data, uint64_t len,
                                     const uint8_t* index, uint64_t index_len, uint64_t* n_out);

/* ---- batched read-path probe across SSTs ----
 * For n keys and nsst filters: out[j * nsst + s] = 1 iff SST s is a candidate for key j, i.e.
 * the key lies in [smallest_s, biggest_s] (Vec<u8> order; skipped when bounds_off is NULL) and
 * filters[s]->contains(key) -- the test KeyRange::filter_sstables_by_key_range applies per key
 * (src/key_range/range.rs:118,136).  Each key is hashed once for all filters.
 * filters: host array of handles, all on one device.  bounds / bounds_off (host): smallest_s =
 * bounds[bounds_off[2s] .. bounds_off[2s+1]), biggest_s = bounds[bounds_off[2s+1] ..
 * bounds_off[2s+2]).  A key reaching a filter with m == 0 and k > 0 is VBF_EDIVZERO (bf.rs:100):
 * without bounds every key reaches every filter, with bounds only the keys inside that SST's
 * range do (one extra readback when such a filter is present).  Host-resident filters are
 * rejected (vbf_filter_migrate them to the device first).
 * _dev: keys / offsets / out on that device, queued on `stream` after one synchronisation of it (the
 * upload of the filters' table and of the bounds, whose host sources are the caller's).  _host: host
 * buffers, synchronous. */
int vbf_multi_probe_dev(const uint8_t* keys, const uint64_t* offsets, uint64_t stride, uint64_t n,
                        int len_prefix, uint32_t nsst, const vbf_filter* const* filters,
                        const uint8_t* bounds, const uint64_t* bounds_off, uint8_t* out, void* stream);
int vbf_multi_probe_host(const uint8_t* keys, const uint64_t* offsets, uint64_t stride, uint64_t n,
                         int len_prefix, uint32_t nsst, const vbf_filter* const* filters,
                         const uint8_t* bounds, const uint64_t* bounds_off, uint8_t* out);
/* vbf_multi_probe_host's path for filters on several GPUs, with the split given: group[i] names
 * filter i's group, each group is probed on its first filter's device (all of a group's filters
 * must share it) and its answer columns are scattered back.  vbf_multi_probe_host calls it with
 * group[i] = the filter's device; a one-GPU host can exercise the split with any grouping. */
int vbf_multi_probe_host_grouped(const uint8_t* keys, const uint64_t* offsets, uint64_t stride, uint64_t n,
                                 int len_prefix, uint32_t nsst, const vbf_filter* const* filters,
                                 const uint8_t* bounds, const uint64_t* bounds_off, const int* group,
                                 uint8_t* out);

/* ---- compaction merge ----
 * One bucket of SizedTierRunner::merge_ssts_in_buckets (src/compactors/sized.rs:170-200): the
 * pairwise fold merged = tables[0], merged = merge_sstables(merged, t) (:207-283) with
 * tombstone_check (:286-320) at every pairwise merge.  Input: an arena of all tables' entries,
 * table r = entries run_off[r] .. run_off[r+1] (host array, run_off[0] = 0), each table strictly
 * increasing by key (a SkipMap; VBF_EINVAL otherwise); entry e = keys[offsets[e] ..
 * offsets[e+1]), created_ms[e] (i64 ms), tombstones[e] (0/1).  The compactor's tombstone map
 * enters as sorted unique keys (map_keys/map_off, map_n + 1 offsets) with times map_time;
 * map_n = 0 for an empty map.  TTLs as Config (use_ttl, entry_ttl, tombstone_ttl in ms) and
 * `now_ms` for Entry::has_expired (memtable/mem.rs:149-153: now > created + ttl).
 * Output: the merged table's entry ids in key order (out_ids, capacity = all entries), *n_out;
 * and, when upd_ids/upd_time are non-NULL, the keys whose map value changed (an entry id holding
 * the key) with their new time, *n_upd (capacity = all entries).  Synchronous on the stream.
 * Limits and checks: at most 2^31 - 1 entries in all (run_off[nruns] <= 0x7FFFFFFF; the device
 * selects count in that range), VBF_EINVAL "too many entries" otherwise.  Every argument check
 * (NULL pointers, run_off not starting at 0 or decreasing, the entry limit, a map without its
 * arrays) runs on the host before any device work, the same in _dev, _host and
 * vbf_compact_write_host; no tables (nruns = 0) or only empty ones give VBF_OK with *n_out = 0
 * and need no device.
 * Times are i64 and TTLs u64 over their whole range.  has_expired's created + ttl is computed in
 * u64 and wraps (a negative `created` counts as a large u64): that is this library's and its
 * oracle's reading of mem.rs:149-153 outside the range of real clocks, not a claim about what
 * the Rust reference does there (its arithmetic may panic on overflow). */
int vbf_compact_merge_dev(const uint8_t* keys, const uint64_t* offsets, const int64_t* created_ms,
                          const uint8_t* tombstones, const uint64_t* run_off, uint32_t nruns,
                          const uint8_t* map_keys, const uint64_t* map_off, const int64_t* map_time,
                          uint64_t map_n, int use_ttl, uint64_t entry_ttl_ms, uint64_t tombstone_ttl_ms,
                          uint64_t now_ms, uint32_t* out_ids, uint64_t* n_out, uint32_t* upd_ids,
                          int64_t* upd_time, uint64_t* n_upd, void* stream);
/* Same with every array in host memory, merged on `device`. */
int vbf_compact_merge_host(const uint8_t* keys, const uint64_t* offsets, const int64_t* created_ms,
                           const uint8_t* tombstones, const uint64_t* run_off, uint32_t nruns,
                           const uint8_t* map_keys, const uint64_t* map_off, const int64_t* map_time,
                           uint64_t map_n, int use_ttl, uint64_t entry_ttl_ms,
                           uint64_t tombstone_ttl_ms, uint64_t now_ms, uint32_t* out_ids,
                           uint64_t* n_out, uint32_t* upd_ids, int64_t* upd_time, uint64_t* n_upd,
                           int device);
/* ids -> the build's key layout: out_keys packed (capacity out_keys_cap), out_offsets n+1 (from 0),
 * and optionally the per-entry arrays (each needs its input).  *key_bytes (may be NULL) = packed
 * size.  Device pointers; one readback of the size.  n <= 2^31 - 2 (the offsets' scan runs over
 * n + 1 items), VBF_EINVAL "too many entries" otherwise, checked before any device work. */
int vbf_gather_entries_dev(const uint8_t* keys, const uint64_t* offsets, const int64_t* created_ms,
                           const uint8_t* tombstones, const uint32_t* val_offsets, const uint32_t* ids,
                           uint64_t n, uint8_t* out_keys, uint64_t out_keys_cap, uint64_t* out_offsets,
                           int64_t* out_created_ms, uint8_t* out_tombstones, uint32_t* out_val_offsets,
                           uint64_t* key_bytes, void* stream);

/* One bucket of merge_ssts_in_buckets (src/compactors/sized.rs:170-200) carried through to what
 * Table::write_to_file writes (src/sst/table.rs:287-324): the arena (every input of
 * vbf_compact_merge_host, plus the entries' value offsets, NULL = zeros) goes up once; the merge,
 * the gather of the merged entries with their three per-entry arrays, the data.db / index.db
 * encode and BloomFilter::new(false_positive, n) + build_filter_from_entries (sized.rs:192-193)
 * all run on `device` with nothing returned to the host in between.  The two files (data / index
 * may be NULL; capacities that always suffice: input key bytes + 17 entries and + 8 entries) and
 * the tombstone-map updates come down; the filter stays device-resident in *filter_out (the
 * caller frees it).  *n_out = merged entries.  An empty merge is VBF_EINVAL with *n_out = 0 and
 * the map updates written: BloomFilter::new(p, 0) asserts (bf.rs:67).  Synchronous. */
int vbf_compact_write_host(const uint8_t* keys, const uint64_t* offsets, const int64_t* created_ms,
                           const uint8_t* tombstones, const uint64_t* run_off, uint32_t nruns,
                           const uint8_t* map_keys, const uint64_t* map_off, const int64_t* map_time,
                           uint64_t map_n, int use_ttl, uint64_t entry_ttl_ms, uint64_t tombstone_ttl_ms,
                           uint64_t now_ms, const uint32_t* val_offsets, double false_positive,
                           vbf_filter** filter_out, uint8_t* data, uint64_t data_cap, uint64_t* data_len,
                           uint8_t* index, uint64_t index_cap, uint64_t* index_len, uint64_t* n_out,
                           uint32_t* upd_ids, int64_t* upd_time, uint64_t* n_upd, int device);

/* ---- memtable flush: a batch of puts in arrival order -> an SST's files ----
 *
 * DataStore::put appends to the value log and calls MemTable::insert (src/db/store.rs:215-243,
 * src/memtable/mem.rs:207-221); Flusher::flush hands the memtable's SkipMap to
 * Table::write_to_file (src/flush/flusher.rs:37-64, src/sst/table.rs:258-326).  These entry points
 * are that data transformation for a whole batch -- a bulk load, or the replay of a recovered value
 * log (src/db/recovery.rs:245-286).  Cutting a put stream into memtables by capacity (is_full,
 * mem.rs:277-279), the `head` entry of migrate_memtable_to_read_only (store.rs:250-263; a caller
 * appends it to the batch), summary.db and file I/O stay with the caller.
 *
 * vbf_memtable_sort_*: the outcome of SkipMap::insert(key_j, ..) for j = 0 .. n-1 in order.
 * crossbeam-skiplist 0.1.3 removes an entry of the same key before it inserts, so the last insert
 * of a key wins whatever its created_at.  out_ids (capacity n) receives the distinct keys in
 * ascending `Ord for [u8]` order (unsigned bytes, a proper prefix first, the empty key first of
 * all), each represented by the largest j that holds it; *n_out = their number.  n == 0 is VBF_OK
 * with *n_out = 0 and no device work; n > 2^31 - 1 is VBF_EINVAL ("too many entries") before any.
 * Descending offsets are VBF_EINVAL: _host finds them on the host, _dev after its first pass (no
 * later pass reads a key of such a batch).  _dev synchronises the stream once, to read the count;
 * its workspace (33 bytes per entry) is cached per stream. */
int vbf_memtable_sort_dev(const uint8_t* keys, const uint64_t* offsets, uint64_t stride, uint64_t n,
                          uint32_t* out_ids, uint64_t* n_out, void* stream);
int vbf_memtable_sort_host(const uint8_t* keys, const uint64_t* offsets, uint64_t stride, uint64_t n,
                           uint32_t* out_ids, uint64_t* n_out, int device);

/* MemTable::insert's filter step, `if !contains(key) { set(key) }` (mem.rs:209-211), replayed over
 * the batch in order against the filter's current bits.  The bits end as a set of every key would
 * leave them (a skipped set would have changed nothing); no_of_elements grows only by the keys
 * that were not contained when their turn came (u32, wrapping), and that number is returned in
 * *n_new (may be NULL).  It is the count filter.db stores for a flushed SST, from which recovery
 * recomputes m (bf.rs:144-147).  k == 0: every key is contained, *n_new = 0.  m == 0 with k > 0 is
 * VBF_EDIVZERO.  n <= 2^32 - 2.  A device-resident filter takes one u32 of scratch per bit, so
 * m <= 2^30 bits (VBF_EINVAL beyond, whatever the residency, before any work).  _host runs the
 * literal loop on the CPU for a host-resident filter; _dev needs a device-resident one and
 * synchronises the stream once, for the count.  Ordered by the filter's lock like set_host /
 * set_dev. */
int vbf_filter_insert_host(vbf_filter* f, const uint8_t* keys, const uint64_t* offsets, uint64_t stride,
                           uint64_t n, int len_prefix, uint64_t* n_new);
int vbf_filter_insert_dev(vbf_filter* f, const uint8_t* keys, const uint64_t* offsets, uint64_t stride,
                          uint64_t n, int len_prefix, uint64_t* n_new, void* stream);

/* One batch of puts carried through to what Table::write_to_file writes, the counterpart of
 * vbf_compact_write_host: one upload, vbf_memtable_sort, the gather of the surviving entries with
 * their per-entry arrays (val_offsets / created_ms / tombstones, each may be NULL: zeros), the
 * data.db / index.db encode and, when `filter` is non-NULL, vbf_filter_insert over all n keys in
 * input order (len_prefix = 1), with nothing returned to the host in between.  `filter` must be
 * device-resident on `device` (a caller flushing a real memtable owns its host filter and passes
 * NULL); it is touched only when everything before it succeeded.  out_ids (may be NULL, capacity
 * n) receives the sort's ids: keys[out_ids[0]] is the summary's smallest key and
 * keys[out_ids[*n_out - 1]] its biggest (table.rs:270-274).  *data_len / *index_len / *n_out are
 * always written; data / index may be NULL (a size query), and a capacity that is too small is
 * VBF_EINVAL with the sizes written and no output touched.  Key bytes + 17 n and + 8 n always
 * suffice.  n == 0 is VBF_EINVAL with zero sizes ("Cannot flush an empty table",
 * flusher.rs:40-44); a key of more than 4079 bytes is the encoder's VBF_EINVAL.  Synchronous. */
int vbf_flush_write_host(const uint8_t* keys, const uint64_t* offsets, uint64_t stride, uint64_t n,
                         const uint32_t* val_offsets, const int64_t* created_ms, const uint8_t* tombstones,
                         vbf_filter* filter, uint8_t* data, uint64_t data_cap, uint64_t* data_len,
                         uint8_t* index, uint64_t index_cap, uint64_t* index_len, uint32_t* out_ids,
                         uint64_t* n_out, int device);

/* ---- batched point lookups in SST tables ----
 * The read path after the filters: per key and candidate SST the reference scans index.db for the
 * first record whose key is >= the searched key (Index::get, src/index/indexer.rs:170-172;
 * IndexFileNode::get_from_index, src/fs/mod.rs:667-710), scans data.db from that block's offset for
 * an equal key (Table::get, src/sst/table.rs:184-193; DataFileNode::find_entry, src/fs/mod.rs:334-389)
 * and keeps the strictly newest hit over the SSTs (DataStore::search_key_in_sstables,
 * src/db/store.rs:579-612).  Here a table is opened once on the device and a batch of keys is
 * looked up in every table in one launch; the value-log read that follows is vbf_vlog_get_* below.
 *
 * A vbf_table holds data.db, index.db and the block starts on the device plus side tables built at
 * open (every block's entry starts and count, the entries before every block, the start of every
 * index record).  Open validates the files once; VBF_EINVAL, with the first offending block or entry in vbf_last_error(), for
 *   - what the decoder rejects: an entry crossing its block, block offsets out of order;
 *   - keys not strictly increasing over the whole file (the writer emits a SkipMap; the same demand
 *     as vbf_compact_merge_*);
 *   - an index record that is not (last key of its block, start of its block), or index.db not
 *     exactly one record per block;
 *   - a block longer than 4096 bytes or of more than 256 entries (the reference's writer produces
 *     neither: block_manager.rs:121-125).
 * On a table that passed, find_entry's scan to the end of the file finds a key iff it is in the block
 * the index step chose (every later key is greater), so both scans are run as binary searches.
 * An empty table (data_len == 0, nblocks == 0, index_len == 0) opens and holds nothing.  A
 * zero-length key is an ordinary key (the reference's reader reports UnexpectedEof on one,
 * fs/mod.rs:355-358). */
typedef struct vbf_table vbf_table;

/* Borrows the caller's device buffers (exactly vbf_sst_encode_dev's three outputs, or an uploaded
 * file + its vbf_sst_index_blocks offsets) on the current device; allocates only the side tables.
 * The buffers must outlive the handle.  Synchronizes `stream` (the validation's verdict). */
int vbf_table_open_dev(const uint8_t* data, uint64_t data_len, const uint8_t* index, uint64_t index_len,
                       const uint32_t* blocks, uint64_t nblocks, void* stream, vbf_table** out);
/* File bytes from the host: uploads them to `device` into buffers the handle owns, parses the block
 * starts from index.db (vbf_sst_index_blocks), then the same path. */
int vbf_table_open_host(const uint8_t* data, uint64_t data_len, const uint8_t* index, uint64_t index_len,
                        int device, vbf_table** out);
void vbf_table_free(vbf_table* t);
uint64_t vbf_table_entries(const vbf_table* t);
uint64_t vbf_table_blocks(const vbf_table* t);
int vbf_table_device(const vbf_table* t);
/* smallest = the first entry's key, biggest = the last index record's key (what KeyRange stores,
 * src/key_range/range.rs:91-147); both empty for an empty table.  *slen / *blen are always written;
 * NULL buffers make it a size query, a too-small capacity is VBF_EINVAL. */
int vbf_table_key_range(const vbf_table* t, uint8_t* smallest, uint64_t scap, uint64_t* slen,
                        uint8_t* biggest, uint64_t bcap, uint64_t* blen);

/* For key j (layout as every entry point: offsets or stride) and tables[0..nsst) in the given order,
 * DataStore::search_key_in_sstables (src/db/store.rs:579-612):
 *   found[j]       0 = no table holds it, 1 = the winning entry is live, 2 = it is a tombstone
 *                  (tombstone byte == 1; any other value is live)
 *   table_idx[j]   index of the winning table in `tables`, 0xFFFFFFFF when found[j] == 0
 *   val_offsets[j], created_ms[j]   the winning entry's fields, 0 when found[j] == 0
 * Per table: get_from_index yields the first index record with key >= key j -- none (the key is
 * greater than every index key: the reference never reassigns its block_offset, fs/mod.rs:667-710)
 * skips the table -- and find_entry an equal key in that block.  The fold starts at
 * default_datetime() (0 ms) and a hit replaces the winner only when its created_at (u64 ms, as
 * stored) is strictly greater: on a tie the earlier table of `tables` wins, and an entry with
 * created_at == 0 never wins (found_in_table, store.rs:616-618).
 * cand (device, n * nsst bytes, vbf_multi_probe_dev's `out`) restricts key j to the tables with
 * cand[j * nsst + s] != 0; NULL = every table.  A filter built from a table's keys has no false
 * negatives, so cand only prunes work.  Any output may be NULL.  All tables on one device
 * (VBF_EINVAL otherwise).  n == 0 is VBF_OK with nothing done; nsst == 0 fills every output
 * (table_idx too) with zeros.  Queued on `stream` after one synchronisation of it (the table
 * descriptors' upload). */
int vbf_table_get_dev(const uint8_t* keys, const uint64_t* offsets, uint64_t stride, uint64_t n,
                      uint32_t nsst, const vbf_table* const* tables, const uint8_t* cand,
                      uint8_t* found, uint32_t* table_idx, uint32_t* val_offsets, uint64_t* created_ms,
                      void* stream);
/* Host keys and host outputs, synchronous.  filters NULL: every table is searched.  filters
 * non-NULL (nsst device-resident handles on the tables' device, hashed with len_prefix = 1):
 * vbf_multi_probe_dev with the tables' own key ranges as bounds makes `cand` first --
 * filter_sstables_by_key_range (src/key_range/range.rs:91-147) then search_key_in_sstables, keys
 * uploaded once. */
int vbf_table_get_host(const uint8_t* keys, const uint64_t* offsets, uint64_t stride, uint64_t n,
                       uint32_t nsst, const vbf_table* const* tables, const vbf_filter* const* filters,
                       uint8_t* found, uint32_t* table_idx, uint32_t* val_offsets, uint64_t* created_ms);

/* ---- batched range scans over open tables ----
 * The key side of DataStore::seek(start, end) (src/range/range_iterator.rs:47-60, a stub in the
 * reference; Range Query is on its TODO list): the merged, newest-wins entries of every table whose
 * key lies in the range -- what a `seek` binding hands to RangeIterator.keys before it fetches the
 * values from the value log.  The scan has no semantics of its own: for range r and
 * tables[0..nsst) in the given order, let U_r be the distinct keys k held by some table with
 * lo_r <= k <= hi_r (Rust's `Ord for [u8]`, both ends inclusive as KeyRange tests,
 * src/key_range/range.rs:101-113).  The scan of r lists, in ascending key order, every k of U_r
 * for which vbf_table_get_* over the same tables in the same order reports found != 0, with exactly
 * that call's table_idx, val_offsets and created_ms.  So, as there: the strictly newest created_at
 * wins, on a tie the earlier table of `tables`, an entry with created_at == 0 never wins (a key
 * whose copies are all at time 0 is absent), a tombstone is byte == 1.
 * flags (an unknown bit is VBF_EINVAL):
 *   VBF_SCAN_KEEP_TOMBSTONES  keys whose winner is a tombstone are listed with tombstones[i] = 1;
 *                             without it they are omitted.  Either way a newer tombstone hides an
 *                             older live entry of another table.
 *   VBF_SCAN_END_EXCLUSIVE    lo_r <= k < hi_r.
 * lo_r > hi_r is an empty range, not an error; so is lo_r == hi_r with END_EXCLUSIVE.  A zero-length
 * lo_r starts at the first key; a zero-length key is an ordinary key.
 * bounds / bounds_off: vbf_multi_probe_*'s layout -- lo_r = bounds[bounds_off[2r] ..
 * bounds_off[2r+1]), hi_r = bounds[bounds_off[2r+1] .. bounds_off[2r+2]); 2 * nranges + 1
 * nondecreasing entries, bounds_off[0] need not be 0 -- on the tables' device in _dev, in host
 * memory in _host.
 * Outputs (device arrays in _dev, host arrays in _host): output i belongs to range r when
 * range_off[r] <= i < range_off[r+1] (nranges + 1 entries, from 0, not subject to entries_cap); its
 * key is keys[key_off[i] .. key_off[i+1]) (key_off: n_out + 1 entries, from 0, so entries_cap + 1
 * slots); table_idx / val_offsets / created_ms / tombstones hold entries_cap items.  Every output
 * array may be NULL; all of them NULL is the size query.  *n_out (listed entries) and *key_bytes
 * are always written; a capacity that is too small (entries_cap < *n_out with a per-entry array
 * given, keys_cap < *key_bytes with keys given) is VBF_EINVAL with the sizes written and nothing
 * written to the outputs (the encoder's convention).
 * nranges == 0 is VBF_OK with zero sizes and no device work (_dev then writes no output; _host
 * writes range_off[0] = key_off[0] = 0).  nsst == 0, or only empty tables, gives empty ranges.
 * All tables on one device.  Every argument check (NULL pointers, unknown flags, a table on another
 * device; in _host also a descending bounds_off, which _dev reports after its first pass) runs on
 * the host before any HIP call.  The candidate entries -- the sum, over ranges and tables, of the
 * table's entries inside the range -- are limited to 2^31 - 1, VBF_EINVAL "too many entries"
 * beyond, like the compaction merge.
 * Work is O(candidates x nsst x log(entries per table)) key comparisons: every candidate searches
 * its key in every other table.  That suits short and medium ranges; it is not a merge-path scan.
 * Workspace (cached per stream like every other): 40 bytes per candidate + 24 per (range, table)
 * pair, plus the scans' scratch.  It belongs to the caller's stream, so two threads must not drive
 * one stream through the library at the same time ("Threads" above); _host callers need no care.
 * _dev synchronises `stream` three times (the table descriptors' upload, the candidate total, the
 * two sizes); the output passes stay queued on it.  _host is synchronous. */
#define VBF_SCAN_KEEP_TOMBSTONES 1u
#define VBF_SCAN_END_EXCLUSIVE 2u
int vbf_table_scan_dev(const uint8_t* bounds, const uint64_t* bounds_off, uint64_t nranges, uint32_t nsst,
                       const vbf_table* const* tables, uint32_t flags, uint64_t* range_off, uint8_t* keys,
                       uint64_t keys_cap, uint64_t* key_off, uint32_t* table_idx, uint32_t* val_offsets,
                       uint64_t* created_ms, uint8_t* tombstones, uint64_t entries_cap, uint64_t* n_out,
                       uint64_t* key_bytes, void* stream);
int vbf_table_scan_host(const uint8_t* bounds, const uint64_t* bounds_off, uint64_t nranges, uint32_t nsst,
                        const vbf_table* const* tables, uint32_t flags, uint64_t* range_off, uint8_t* keys,
                        uint64_t keys_cap, uint64_t* key_off, uint32_t* table_idx, uint32_t* val_offsets,
                        uint64_t* created_ms, uint8_t* tombstones, uint64_t entries_cap, uint64_t* n_out,
                        uint64_t* key_bytes);

/* ---- batched value-log reads and appends ----
 * The last step of a get and the first of a put.  The value log (src/vlog/v_log.rs) is one file of
 * entries laid back to back, little-endian, no padding and no index (ValueLogEntry::serialize,
 * v_log.rs:291-309):
 *     u32 key_len | u32 val_len | u64 created_at ms | u8 tombstone | key | value
 * The header is 17 bytes; an entry's offset is the file position of its first byte, and data.db
 * stores it as u32 (block_manager.rs:91,183).  ValueLog::get (v_log.rs:205-207) -> VLogFileNode::get
 * (fs/mod.rs:470-518): an offset at or past the end of the file is Ok(None); otherwise one header is
 * read, the key skipped and the value returned, with no check of the key or of created_at;
 * DataStore::get_value_from_vlog (db/store.rs:628-641) turns a tombstone (byte == 1, any other byte
 * is live) into None.  ValueLog::append (v_log.rs:173-196) writes the entry at the file's size and
 * returns that position.
 * Two readings of this library's: a zero-length value is an ordinary value, and so is a zero-length
 * key (the reference's load_buffer! treats a 0-byte read as UnexpectedEof, so its get of either
 * fails); an entry whose header or body runs past the end of the log is reported as bad, per item
 * (the reference's single read would return a short buffer there; no short value is returned here).
 * ValueLog::recover and the GC's chunk read, the serial walks of the unindexed file, are
 * vbf_vlog_walk_* below.  Out of scope: hole punching, file I/O.
 *
 * A vbf_vlog is a window of the log on a device: bytes[0..len) are the file's bytes
 * [base, base + len).  `base` is the log's tail: the GC punches the front of the file away, so a
 * caller uploads only what is live.  Open parses nothing (there is no index to validate against);
 * len == 0 opens and holds nothing; base + len must not wrap.  The handle is immutable, like
 * vbf_table. */
typedef struct vbf_vlog vbf_vlog;
/* Borrows the caller's device buffer on the current device; it must outlive the handle. */
int vbf_vlog_open_dev(const uint8_t* bytes, uint64_t len, uint64_t base, vbf_vlog** out);
/* Uploads host bytes to `device` into a buffer the handle owns. */
int vbf_vlog_open_host(const uint8_t* bytes, uint64_t len, uint64_t base, int device, vbf_vlog** out);
void vbf_vlog_free(vbf_vlog* v);
uint64_t vbf_vlog_bytes(const vbf_vlog* v);
uint64_t vbf_vlog_base(const vbf_vlog* v);
int vbf_vlog_device(const vbf_vlog* v);

/* The batched fetch.  Item j reads the entry at file position val_offsets[j]; `found`
 * (vbf_table_get_*'s output, passed straight through) restricts the fetch to the items with
 * found[j] == 1, NULL fetches every item.  keys / offsets / stride: the layout of every entry point;
 * keys == NULL means no check, otherwise the entry's key must equal key j in length and in bytes.
 * status[j]: */
#define VBF_VLOG_SKIPPED 0       /* the `found` mask excluded item j                               */
#define VBF_VLOG_VALUE 1         /* the value was fetched                                          */
#define VBF_VLOG_TOMBSTONE 2     /* the entry's byte is 1: no value is returned                    */
#define VBF_VLOG_NONE 3          /* offset >= base + len: the reference's Ok(None)                 */
#define VBF_VLOG_BAD 4           /* offset < base, or the header or the body crosses base + len    */
                                 /* (computed in 64 bits: key_len = val_len = 0xFFFFFFFF is BAD)   */
#define VBF_VLOG_KEY_MISMATCH 5  /* a key was given and it differs from the entry's key            */
/* The checks run in that order of precedence: SKIPPED, NONE, BAD, KEY_MISMATCH (also for a
 * tombstone of another key), TOMBSTONE, VALUE.
 * Only status 1 has a value: item j's is values[value_off[j] .. value_off[j+1]); value_off has
 * n + 1 entries, starts at 0 and gives zero length to every other status.  Values are in item
 * order; duplicated offsets give duplicated values.  A bad item never fails the call.
 * *value_bytes (= value_off[n]) is always written.  values == NULL is the size query: status and
 * value_off, where given, are still filled.  values given with values_cap < *value_bytes is
 * VBF_EINVAL with the size written and no output array touched (the encoder's convention).
 * n == 0 is VBF_OK with no device work (_host then writes value_off[0] = 0).  At most 2^31 - 2 items.
 * Every argument check (NULL handle, NULL val_offsets with n > 0, NULL value_bytes, the item limit;
 * in _host also a descending `offsets`) runs on the host before any HIP call.  _dev runs on the
 * current device, which must be the handle's (VBF_EINVAL otherwise, checked first of the device
 * work).  _dev synchronises `stream` once, to read the byte total; the copy stays queued.
 * Workspace (cached per stream like every other, so the "Threads" rule for `_dev` holds): 25 bytes
 * per item plus the scan's scratch.  _host: every array in host memory, synchronous, on the
 * handle's device. */
int vbf_vlog_get_dev(const vbf_vlog* v, const uint32_t* val_offsets, const uint8_t* found, uint64_t n,
                     const uint8_t* keys, const uint64_t* offsets, uint64_t stride,
                     uint8_t* status, uint8_t* values, uint64_t values_cap, uint64_t* value_off,
                     uint64_t* value_bytes, void* stream);
int vbf_vlog_get_host(const vbf_vlog* v, const uint32_t* val_offsets, const uint8_t* found, uint64_t n,
                      const uint8_t* keys, const uint64_t* offsets, uint64_t stride,
                      uint8_t* status, uint8_t* values, uint64_t values_cap, uint64_t* value_off,
                      uint64_t* value_bytes);

/* The batched append.  Entry j = (key j, values[value_off[j] .. value_off[j+1]), created_ms[j],
 * tombstones[j]) is serialised at base + the sum of the earlier entries' sizes, as ValueLog::append
 * places it when the file's size is `base`; val_offsets[j] is that position, exactly what
 * vbf_sst_encode_* takes.  Keys in the layout of every entry point; value_off has n + 1
 * nondecreasing absolute positions in `values` and need not start at 0, like `offsets`.
 * created_ms / tombstones may be NULL (zeros); a tombstone byte != 0 is written as 1.
 * *out_len (the bytes appended) is always written.  out == NULL && val_offsets == NULL is the size
 * query; either may be NULL on its own.  out given with out_cap < *out_len is VBF_EINVAL with
 * *out_len written and nothing else.  n == 0 is VBF_OK with *out_len = 0 and no device work.
 * VBF_EINVAL: an entry that would start at 2^32 or beyond (data.db could not address it; where
 * base + 17 (n - 1) already reaches 2^32 this is decided before any device work), descending
 * offsets or value_off, a key or value longer than 2^32 - 1 bytes.  _dev (device arrays) checks the
 * two offset arrays in a first pass and synchronises the stream once (their ends and that pass's
 * verdict); the copy stays queued.  _host (host arrays, encoded on `device`, synchronous) checks
 * everything on the host before any HIP call, and its size query needs no device. */
int vbf_vlog_encode_dev(const uint8_t* keys, const uint64_t* offsets, uint64_t stride, uint64_t n,
                        const uint8_t* values, const uint64_t* value_off,
                        const int64_t* created_ms, const uint8_t* tombstones, uint64_t base,
                        uint8_t* out, uint64_t out_cap, uint64_t* out_len, uint32_t* val_offsets, void* stream);
int vbf_vlog_encode_host(const uint8_t* keys, const uint64_t* offsets, uint64_t stride, uint64_t n,
                         const uint8_t* values, const uint64_t* value_off,
                         const int64_t* created_ms, const uint8_t* tombstones, uint64_t base,
                         uint8_t* out, uint64_t out_cap, uint64_t* out_len, uint32_t* val_offsets, int device);

/* ---- the walk of the value log: crash recovery and the GC's chunk read ----
 * ValueLog::recover(head) is VLogFileNode::recover (fs/mod.rs:520-577): seek to the head offset
 * (:524) and read entry after entry -- the four header fields (:529-556), the key (:557-558), the
 * value (:563-564) -- until a read returns 0 bytes at an entry's first field (:531-533).
 * recover_memtable (db/recovery.rs:245-286) turns the entries into memtable inserts; the first one
 * is already in an SST and is skipped (recovery.rs:261-264).  read_chunk_to_garbage_collect(bytes,
 * tail) (fs/mod.rs:579-651) is the same loop from the tail (:587) that also adds up the bytes read
 * (:594-633) and returns after the entry that brought them to `bytes` or more (:646-649);
 * GC::gc_handler (gc/garbage_collector.rs:168-262) looks every key up and re-appends the live ones.
 *
 * The walk runs over an open vbf_vlog, from file position `start`, following
 * p -> p + 17 + key_len(p) + val_len(p).  It stops with *stop = */
#define VBF_WALK_END 0     /* the chain reached base + len exactly (fs/mod.rs:531-533, :595-597)      */
#define VBF_WALK_BUDGET 1  /* after the entry that brought the bytes read to >= budget (:646-649)     */
#define VBF_WALK_TORN 2    /* the entry at *end_off has a header or a body that crosses base + len    */
/* Budget: the test `bytes read >= budget` runs after each whole entry (fs/mod.rs:646-649), so
 * budget = 0 yields exactly one entry when one exists, and it wins over END when the same entry
 * also ends the log; budget = UINT64_MAX is recover.  Bytes read = *end_off - start.
 * Start: start == base + len is VBF_OK with no entry and VBF_WALK_END; start outside
 * [base, base + len] is VBF_EINVAL.  `start` must be an entry's first byte, as the reference's
 * head and tail offsets are: the walk has no way to tell.
 * Torn tail, this library's reading: a log cut by a crash ends in a partial entry.  That is its
 * normal state, not an error: the entries before it are returned, *end_off is the torn entry's
 * position and *stop = VBF_WALK_TORN (the reference's short read would return an entry of garbage
 * there, :558-575; as with vbf_vlog_get_*, no short entry is returned here).  Hops are computed in
 * 64 bits: key_len = val_len = 0xFFFFFFFF is torn and never wraps.
 * Fields: tombstones[i] is 1 iff the byte is 1 (:556); created_ms[i] is the stored 8 bytes (:549);
 * zero-length keys and values are ordinary entries, as above.  Entry i lies at entry_off[i], its
 * key is keys[key_off[i] .. key_off[i+1]), its value values[value_off[i] .. value_off[i+1]) -- the
 * entry's own value, tombstone or not.  entry_off, key_off and value_off have n + 1 entries;
 * entry_off[n] = *end_off, key_off and value_off start at 0.  val_offsets[i] is entry_off[i] as u32,
 * what vbf_sst_encode_*, vbf_flush_write_host and vbf_vlog_get_* take; val_offsets given while an
 * entry lies at or beyond 2^32 is VBF_EINVAL.
 * Outputs: every array may be NULL; all of them NULL is the size query; the five scalars (*n_out,
 * *key_bytes, *value_bytes, *end_off, *stop) are always written.  A capacity that is too small
 * (entries_cap < n with any per-entry array given -- the n + 1 arrays need entries_cap + 1
 * elements --, keys_cap, values_cap) is VBF_EINVAL with the sizes written and no array touched.  At
 * most 2^31 - 2 entries.  Every argument check (NULL scalars, NULL handle, start outside the window)
 * runs on the host before any HIP call.  _dev runs on the current device, which must be the
 * handle's (VBF_EINVAL otherwise).
 * Cost: the window is walked in segments of 8 MiB, in order, and the walk ends with the segment in
 * which the budget is met or the chain stops: a GC chunk costs its own bytes, not the window's.  No
 * lane follows the chain entry by entry: per segment the dependent steps of any lane are bounded by
 * the segment's groups (64) + the tiles of a group (32) + the entries of a tile (241); see
 * csrc/vbf_vlog_walk.hip.  _dev synchronises `stream` once per segment (the segment's sizes and
 * where the chain left it); the emit and copy passes stay queued.  With outputs and more than one
 * segment the segments' passes run a second time, without synchronising.  Workspace (cached per
 * stream like every other): about 4.4 bytes per byte of the largest segment walked plus 32 bytes
 * per possible entry of it (242 per tile), 51 MiB for a full segment, whatever the window's length.  _host: every
 * array in host memory, synchronous, on the handle's device. */
int vbf_vlog_walk_dev(const vbf_vlog* v, uint64_t start, uint64_t budget, uint64_t* entry_off,
                      uint32_t* val_offsets, uint8_t* keys, uint64_t keys_cap, uint64_t* key_off, uint8_t* values,
                      uint64_t values_cap, uint64_t* value_off, int64_t* created_ms, uint8_t* tombstones,
                      uint64_t entries_cap, uint64_t* n_out, uint64_t* key_bytes, uint64_t* value_bytes,
                      uint64_t* end_off, int* stop, void* stream);
int vbf_vlog_walk_host(const vbf_vlog* v, uint64_t start, uint64_t budget, uint64_t* entry_off,
                       uint32_t* val_offsets, uint8_t* keys, uint64_t keys_cap, uint64_t* key_off, uint8_t* values,
                       uint64_t values_cap, uint64_t* value_off, int64_t* created_ms, uint8_t* tombstones,
                       uint64_t entries_cap, uint64_t* n_out, uint64_t* key_bytes, uint64_t* value_bytes,
                       uint64_t* end_off, int* stop);

/* ---- the garbage collector's handler over one chunk, in one device pass ----
 * GC::gc_handler (gc/garbage_collector.rs:168-262) reads a chunk of the log from its tail (:176-179),
 * looks every entry's key up (GC::get, :429-469), sorts the entries into valid and invalid (:203-214)
 * and, when any is invalid, appends a `tail` entry (write_tail_to_disk, :265-275) and the valid
 * entries (write_valid_entries_to_vlog, :304-317) to the log and puts them into the GC table
 * (:245-251, GC::put :404-419).  vbf_gc_collect_host does the data side of that over an open vbf_vlog
 * and open tables: the log window and the tables are already on the device, so only the overlay goes
 * up and only the verdicts, the bytes to append and the puts come down.  The chunk's own values are
 * never materialised: a valid entry carries the MOST RECENT value (:210), which is copied from its
 * place in the window straight into `append`.
 *
 * Chunk: vbf_vlog_walk_* from `tail` with budget `chunk_bytes`; *n_chunk, *end_off and *stop are the
 * walk's, the total bytes read (the punch hole's length, :257) is *end_off - tail.  A torn tail ends
 * the chunk as it ends the walk; the entries before it are judged.  tail == base + len is VBF_OK with
 * every count 0 and no device work.
 * Lookup: chunk entry i's key is first searched in the overlay -- ov_n strictly ascending keys
 * (`Ord for [u8]`), key k = ov_keys[ov_off[k] .. ov_off[k+1]) (the layout of the compaction's
 * tombstone map: ov_off has ov_n + 1 absolute positions), with ov_val_offsets[k], ov_created_ms[k],
 * ov_tombstones[k].  It stands for steps 1 and 2 of GC::get (:440-463), the GC table and the
 * read-only memtables, which the caller folds (the active table first, else the most recent of the
 * read-only ones); a hit decides the entry whatever its time.  Otherwise vbf_table_get_* over
 * `tables` decides (step 3), the candidates first cut by `filters` when given (one per table, or
 * NULL), exactly as in vbf_table_get_host.
 * verdict[i] is the first of these tests that applies, in this order: */
#define VBF_GC_VALID 0          /* kept: re-appended with its most recent value (:210)                 */
#define VBF_GC_ABSENT 1         /* neither the overlay nor any table holds the key (NotFoundInDB)      */
#define VBF_GC_DELETED 2        /* the winner (overlay or table) is a tombstone (:442-444, :459, :505) */
#define VBF_GC_LOG_NONE 3       /* the winner's offset is >= base + len: Ok(None) (:524-537)           */
#define VBF_GC_LOG_TOMBSTONE 4  /* the most recent log entry's byte is 1 (:531-533)                    */
#define VBF_GC_OLDER 5          /* entry.created_at < the winner's creation time (:205)                */
#define VBF_GC_STAR 6           /* the most recent value is "*" (:206)                                 */
/* The window checks on the most recent entry are vbf_vlog_get_*'s.  created_at on both sides is
 * compared as the signed 64-bit value the reference's DateTime holds; equal times are valid.  A most
 * recent entry that is BAD (before base, or its header or body crosses base + len) fails the call
 * with VBF_EINVAL, the message naming the first such chunk entry and its offset; no output array is
 * touched.  *n_invalid counts the entries whose verdict is not VBF_GC_VALID.
 * Nothing to collect: *n_invalid == 0 is VBF_OK with *n_puts = *append_len = 0 (:228-230); verdict
 * is still filled.
 * Appended bytes (*n_invalid > 0): `append` holds exactly what vbf_vlog_encode_* with base = log_size
 * produces for the puts: every created_at is now_ms and every tombstone byte 0 (:265-275, :304-317).
 * Put 0 has key "tail" and value LE64(tail + total bytes read) (:231-238); after it come the valid
 * entries in chunk order (this library's reading: the reference's tasks push them in no fixed order,
 * :185-217), each with its own key and the most recent value.  put_val_offsets[j] is put j's
 * position (u32), put_tombstones[j] is 1 iff its value is empty (GC::put :411), put_ids[j] the chunk
 * index of put j and 0xFFFFFFFF for put 0; *n_puts = 1 + the valid entries.  The puts' keys are not
 * returned apart: put j's key lies in `append` at put_val_offsets[j] - log_size + 17, its length in
 * the 4 bytes at put_val_offsets[j] - log_size.
 * Sizes: the six scalars (*n_chunk, *n_invalid, *n_puts, *append_len, *end_off, *stop) are always
 * written.  Every output array may be NULL; all of them NULL is the size query.  A capacity that is
 * too small -- entries_cap < *n_chunk with verdict given, puts_cap < *n_puts with a put array given,
 * append_cap < *append_len with append given -- is VBF_EINVAL with the sizes written and no array
 * touched.  An appended entry that would start at 2^32 or beyond is VBF_EINVAL, as in
 * vbf_vlog_encode_*; log_size + 25 > 2^32, where no entry can follow the 29-byte `tail` entry below
 * 2^32, is rejected before any device work.  At most 2^31 - 2 chunk entries and overlay keys.
 * Checks that run on the host before any HIP call and before any handle is followed: a NULL scalar
 * (nothing is written then); after the scalars are written, a NULL log, nsst > 0 with NULL tables or
 * a NULL element, a NULL filters[i], ov_n > 0 with an overlay array missing, a descending ov_off,
 * overlay keys not strictly ascending, the log_size rule.  Once the handles are read: `tail` outside
 * [base, base + len], tables or filters not on the log's device (VBF_EINVAL).
 * Cost: the walk's passes, one lookup, then three kernels (csrc/vbf_gc.hip) -- the overlay search and
 * the judge, one lane per chunk entry, and the emit, which divides the bytes to append among the
 * workgroups as vbf_vlog_get_*'s copy does.  Workspace: 79 bytes per chunk entry plus its key (and
 * nsst with filters), 1 byte per appended byte and 5 per put, next to the walk's and the lookup's.
 * Stream synchronisations: the walk's one per 8 MiB segment, the lookup's (its descriptors, and the
 * filters' table), one for the judge's result, one at the end.  Synchronous, on the log's device;
 * locks as vbf_table_get_host takes them (the filters first, then the device). */
int vbf_gc_collect_host(const vbf_vlog* v, uint64_t tail, uint64_t chunk_bytes, uint64_t log_size, int64_t now_ms,
                        uint32_t nsst, const vbf_table* const* tables, const vbf_filter* const* filters,
                        const uint8_t* ov_keys, const uint64_t* ov_off, const uint32_t* ov_val_offsets,
                        const int64_t* ov_created_ms, const uint8_t* ov_tombstones, uint64_t ov_n,
                        uint8_t* verdict, uint64_t entries_cap,
                        uint8_t* append, uint64_t append_cap,
                        uint32_t* put_ids, uint32_t* put_val_offsets, uint8_t* put_tombstones, uint64_t puts_cap,
                        uint64_t* n_chunk, uint64_t* n_invalid, uint64_t* n_puts, uint64_t* append_len,
                        uint64_t* end_off, int* stop);

/* ---- device-resident memtables and the whole get ----
 * DataStore::get (src/db/store.rs:442-481) asks four places in order -- the GC's not-yet-synced
 * entries (search_gc_entries, :489-501), the active memtable (:452-456), the read-only memtables
 * (:458-472), the SSTs (:474-478) -- and then reads the value log (get_value_from_vlog, :628-641).
 * vbf_table_get_* and vbf_vlog_get_* are the last two; these entry points are the first three and
 * the join of all five.
 *
 * A vbf_memtable is an immutable memtable on a device: the outcome of MemTable::insert
 * (memtable/mem.rs:207-221) for a batch of puts in arrival order, i.e. vbf_memtable_sort (the last
 * put of a key wins) and the gather of the survivors.  The handle owns the sorted keys, their
 * offsets, the three per-entry arrays and the lookup's side table (pfx: every key's first 8 bytes as
 * a big-endian word, zero-padded; 8 bytes per entry).  A mutable memtable is a sequence of such
 * handles: a caller that keeps putting opens the active table again from its puts.
 * open_*: vbf_flush_write_host's input convention -- val_offsets (u32) / created_ms (i64) /
 * tombstones may each be NULL and then mean zeros; a tombstone byte != 0 is a tombstone, as the
 * encoder writes it.  n == 0 opens an empty memtable (no device work).  n > 2^31 - 1 and descending
 * offsets are VBF_EINVAL, as in the sort.  _dev (device arrays, the current device) copies: the
 * gather writes new arrays anyway, so the caller's may go once it returns; it synchronises `stream`
 * for the sort's count (the key bytes' extent rides along), for the gathered key bytes, and once at
 * its end, so the handle is complete on return and any stream may read it.  _host uploads to
 * `device`; synchronous. */
typedef struct vbf_memtable vbf_memtable;
int vbf_memtable_open_host(const uint8_t* keys, const uint64_t* offsets, uint64_t stride, uint64_t n,
                           const uint32_t* val_offsets, const int64_t* created_ms, const uint8_t* tombstones,
                           int device, vbf_memtable** out);
int vbf_memtable_open_dev(const uint8_t* keys, const uint64_t* offsets, uint64_t stride, uint64_t n,
                          const uint32_t* val_offsets, const int64_t* created_ms, const uint8_t* tombstones,
                          void* stream, vbf_memtable** out);
void vbf_memtable_free(vbf_memtable* t);
uint64_t vbf_memtable_entries(const vbf_memtable* t);   /* distinct keys */
uint64_t vbf_memtable_key_bytes(const vbf_memtable* t); /* their bytes, back to back */
int vbf_memtable_device(const vbf_memtable* t);
/* The sorted entries, in host memory: key e = keys[key_off[e] .. key_off[e+1]), key_off has
 * entries + 1 positions from 0 (so entries_cap + 1 slots).  Exactly the layout of
 * vbf_gc_collect_host's overlay arrays; key 0 and the last key are the summary's two keys
 * (table.rs:270-274).  Every array may be NULL; all of them NULL is the size query through the
 * accessors above.  A capacity that is too small (keys_cap < key bytes with keys given, entries_cap
 * < entries with a per-entry array given) is VBF_EINVAL with nothing written. */
int vbf_memtable_export_host(const vbf_memtable* t, uint8_t* keys, uint64_t keys_cap, uint64_t* key_off,
                             uint32_t* val_offsets, int64_t* created_ms, uint8_t* tombstones,
                             uint64_t entries_cap);
/* Flusher::flush (src/flush/flusher.rs:37-64) of an open memtable: vbf_sst_encode_dev over the
 * handle's arrays, with vbf_flush_write_host's conventions -- *data_len / *index_len are always
 * written, data / index may be NULL (a size query), a capacity that is too small is VBF_EINVAL with
 * the sizes written and no output touched.  The bytes are those of vbf_flush_write_host over the same
 * puts.  An empty memtable is VBF_EINVAL ("Cannot flush an empty table", flusher.rs:40-44). */
int vbf_memtable_encode_host(const vbf_memtable* t, uint8_t* data, uint64_t data_cap, uint64_t* data_len,
                             uint8_t* index, uint64_t index_cap, uint64_t* index_len);

/* Steps 0-2 of DataStore::get for a batch of keys (layout as every entry point).  `gc` and `active`
 * may be NULL, nro may be 0; ro[0..nro) in the reference's iteration order.  MemTable::get
 * (memtable/mem.rs:223-230) tests its Bloom filter first; the filter has no false negatives, so a
 * memtable lookup is the map lookup.  Per key:
 *   gc (search_gc_entries, store.rs:489-501): a hit decides only when the entry is live AND the log
 *     holds a live value at its offset, by vbf_vlog_get_*'s window tests on the 17-byte header in
 *     `log`.  A tombstone entry (:494-496), a log status NONE and a log status TOMBSTONE
 *     (get_value_from_vlog's None, :628-641) all return Ok(None) there, so the lookup FALLS THROUGH
 *     to the active memtable (:445-447).  An offset that is BAD keeps the gc hit: the value fetch
 *     reports BAD for that item, where the reference's get fails.  The key in the log is not
 *     compared.  gc != NULL with log == NULL is VBF_EINVAL; without gc, log is not read.
 *   active (:452-456): a hit decides whatever its time, found = 2 for a tombstone (:453-455), else
 *     1.  There is no fall-through.
 *   read-only (:458-472): a fold over ro[] in the given order from default_datetime() (time 0).  A
 *     hit replaces the winner only when its created_at, compared as the signed 64-bit value the
 *     memtable's DateTime holds (as vbf_gc_collect_host reads it), is strictly greater (:461); on a
 *     tie the earlier table wins; an entry at time <= 0 never wins, and a key that only such entries
 *     hold is not found here (found_in_table, :468, :616-618): the SSTs get their turn.
 * found[j] is 0, 1 or 2 as in vbf_table_get_*; layer[j] is 0 for gc, 1 for active, 2 + r for
 * read-only table r, 0xFFFFFFFF for none; val_offsets[j] and created_ms[j] (the i64's bits) are the
 * winner's fields, 0 when not found.  Any output may be NULL.
 * All handles live on one device (VBF_EINVAL otherwise).  n == 0 is VBF_OK with no device work; at
 * most 2^31 - 2 keys.  Every argument check runs on the host before any HIP call.  _dev: keys and
 * outputs on the handles' device, queued on `stream` after one synchronisation of it (the layers'
 * descriptors' upload), as vbf_table_get_dev; with no handle at all the outputs are filled by memsets.
 * _host: host arrays, synchronous.
 * Kernel (csrc/vbf_memget.hip): a workgroup looks up 1024 keys, four per lane.  Per layer it stages
 * an evenly strided sample of pfx in LDS (at most 4096 words, 32 KiB; all of pfx up to 4096
 * entries); a lane takes its prefix's lower and upper bound in the sample, and the log2(entries /
 * 4096) steps inside them compare pfx[mid] first and the key bytes only on a prefix tie.
 * VBF_MEMGET=0 (environment, read per call) selects the plain kernel instead -- one binary search
 * over the keys per layer -- with identical results.  Workspace: 56 bytes per layer. */
int vbf_memtable_get_dev(const uint8_t* keys, const uint64_t* offsets, uint64_t stride, uint64_t n,
                         const vbf_memtable* gc, const vbf_memtable* active, uint32_t nro,
                         const vbf_memtable* const* ro, const vbf_vlog* log, uint8_t* found, uint32_t* layer,
                         uint32_t* val_offsets, uint64_t* created_ms, void* stream);
int vbf_memtable_get_host(const uint8_t* keys, const uint64_t* offsets, uint64_t stride, uint64_t n,
                          const vbf_memtable* gc, const vbf_memtable* active, uint32_t nro,
                          const vbf_memtable* const* ro, const vbf_vlog* log, uint8_t* found, uint32_t* layer,
                          uint32_t* val_offsets, uint64_t* created_ms);

/* DataStore::get (store.rs:442-481) for a batch, from key bytes to values in one device pass: the
 * keys go up once; vbf_memtable_get_* runs; for the keys it left undecided vbf_table_get_dev runs
 * over `tables` (search_key_in_sstables, :579-612) -- its candidate matrix made by
 * vbf_multi_probe_dev with the tables' own key ranges when `filters` is given, exactly as in
 * vbf_table_get_host (filter_sstables_by_key_range, :474), and the decided keys' rows zeroed --; the
 * two answers are merged on the device (a memtable's answer stands; otherwise the tables' stands
 * with layer[j] = 0x80000000 | table_idx[j]); vbf_vlog_get_dev fetches the values of the merged
 * found == 1 items, comparing the log entry's key with key j when check_keys != 0.
 * found / layer / val_offsets / created_ms: as above after the merge; table_idx[j] is the winning
 * table or 0xFFFFFFFF when no table answered.  status, values, values_cap, value_off and *value_bytes
 * are vbf_vlog_get_host's, with its conventions: values == NULL is the size query (every other
 * output is still filled), values given with values_cap < *value_bytes is VBF_EINVAL with the size
 * written and no output array touched, n == 0 writes value_off[0] = 0.  Any output but value_bytes
 * may be NULL.  `log` is required; gc, active, nro = 0, nsst = 0 and filters may be absent.
 * Everything on the log's device (VBF_EINVAL otherwise); every argument check runs on the host before
 * any HIP call.  validate_size (store.rs:443: an empty key is an error) stays with the caller: a
 * zero-length key is an ordinary key here.  Synchronous; locks as vbf_table_get_host takes them (the
 * filters first, then the device).  Workspace: the keys, 33 + nsst bytes per key, and the callees'.
 * Stream synchronisations: the layers' descriptors, the tables' (and with filters the filters'
 * table), the value bytes' total, one at the end. */
int vbf_store_get_host(const uint8_t* keys, const uint64_t* offsets, uint64_t stride, uint64_t n,
                       const vbf_memtable* gc, const vbf_memtable* active, uint32_t nro,
                       const vbf_memtable* const* ro, uint32_t nsst, const vbf_table* const* tables,
                       const vbf_filter* const* filters, const vbf_vlog* log, int check_keys,
                       uint8_t* found, uint32_t* layer, uint32_t* table_idx, uint32_t* val_offsets,
                       uint64_t* created_ms, uint8_t* status, uint8_t* values, uint64_t values_cap,
                       uint64_t* value_off, uint64_t* value_bytes);

/* DataStore::seek (src/range/range_iterator.rs:47-60, a stub in the reference) for a batch of ranges
 * over the whole store, from bounds to values in one device pass.  The scan has no semantics of its
 * own: for range r let U_r be the distinct keys k with lo_r <= k <= hi_r (Rust's `Ord for [u8]`;
 * lo_r <= k < hi_r with VBF_SCAN_END_EXCLUSIVE) held by any of gc, active, ro[0..nro) and
 * tables[0..nsst).  The scan of r lists, in ascending key order, every k of U_r for which
 * vbf_store_get_host over the same handles in the same order, with filters == NULL and the same
 * check_keys, reports found != 0, with exactly that call's layer, table_idx, val_offsets, created_ms,
 * status and value.  A key with found == 2 is listed with tombstones[i] = 1 only under
 * VBF_SCAN_KEEP_TOMBSTONES and omitted without it; either way the deciding tombstone hides everything
 * below it.  Every rule of the get carries over because the definition is the get: the gc layer's
 * fall-through on a tombstone entry or a NONE / TOMBSTONE log status, a BAD gc offset keeping its hit,
 * the active memtable with no fall-through, signed times and "time <= 0 never wins" for the read-only
 * memtables, created_at == 0 never winning in a table.  A key that only non-winning copies hold
 * belongs to U_r and is not listed.
 * bounds / bounds_off and the flags are vbf_table_scan_host's, and so are its rules for the ends:
 * lo_r > hi_r is an empty range, not an error, and so is lo_r == hi_r with END_EXCLUSIVE; a
 * zero-length lo_r starts at the first key, and a zero-length key is an ordinary key.
 * Outputs (host arrays): range_off, keys, key_off, table_idx, val_offsets, created_ms and tombstones
 * as vbf_table_scan_host writes them (table_idx[i] = 0xFFFFFFFF when a memtable answered); layer[i] as
 * vbf_store_get_host writes it; status, values and value_off as vbf_vlog_get_host over the listed
 * entries (the fetch runs for tombstones[i] == 0, the rest are SKIPPED; value_off has n_out + 1
 * entries, so entries_cap + 1 slots, as key_off).  *n_out, *key_bytes and *value_bytes are always
 * written.  Every output array may be NULL; all of them NULL is the size query.  A capacity that is
 * too small -- entries_cap < *n_out with any per-entry array given, keys_cap < *key_bytes with keys
 * given, values_cap < *value_bytes with values given -- is VBF_EINVAL with the three sizes written
 * and no output array touched.
 * nranges == 0 is VBF_OK with zero sizes and no device work, and writes range_off[0] = key_off[0] =
 * value_off[0] = 0.  `log` is required; gc, active, nro = 0 and nsst = 0 may all be absent, and with
 * no layer at all every range is empty, with no device work.  Everything lives on the log's device
 * (VBF_EINVAL otherwise).  Every argument check (NULL pointers, unknown flag bits, a handle on another
 * device, a descending bounds_off, gc without log) runs on the host before any HIP call.  The
 * candidate entries -- the sum, over ranges and layers, of the layer's entries inside the range --
 * are limited to 2^31 - 1, VBF_EINVAL "too many entries" beyond; so are the (range, layer) pairs.
 * Work is O(candidates x layers x log(entries per layer)) key comparisons: every candidate searches
 * its key in every other layer (csrc/vbf_store_scan.hip).  That suits short and medium ranges; it is
 * not a merge-path scan.
 * Synchronous; the device's lock as vbf_store_get_host takes it.  Workspace (cached per stream like
 * every other): the bounds, 64 bytes per layer, 24 per (range, layer) pair, 61 per candidate, 30 per
 * listed entry plus the listed keys, the scans' scratch, and vbf_vlog_get_host's for the listed
 * entries.  Stream synchronisations: the layers' descriptors, the candidate total, the entry and key
 * sizes, the value bytes' total, one at the end. */
int vbf_store_scan_host(const uint8_t* bounds, const uint64_t* bounds_off, uint64_t nranges,
                        const vbf_memtable* gc, const vbf_memtable* active, uint32_t nro,
                        const vbf_memtable* const* ro, uint32_t nsst, const vbf_table* const* tables,
                        const vbf_vlog* log, uint32_t flags, int check_keys,
                        uint64_t* range_off, uint8_t* keys, uint64_t keys_cap, uint64_t* key_off,
                        uint8_t* tombstones, uint32_t* layer, uint32_t* table_idx, uint32_t* val_offsets,
                        uint64_t* created_ms, uint8_t* status, uint64_t entries_cap,
                        uint8_t* values, uint64_t values_cap, uint64_t* value_off,
                        uint64_t* n_out, uint64_t* key_bytes, uint64_t* value_bytes);

#ifdef __cplusplus
}
#endif
#endif /* VBF_H */
