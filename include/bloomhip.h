/*
 * bloomhip.h — C ABI of the MI355X (gfx950) Bloom-filter engine.
 *
 * Drop-in for the set/test surface of jackdent/cs265-lsm-tree
 * src/bloom_filter.{h,cpp}:
 *
 *   class BloomFilter {                       src/bloom_filter.h:6-15
 *       boost::dynamic_bitset<> table;        src/bloom_filter.h:7
 *       uint64_t hash_1/2/3(KEY_t) const;     src/bloom_filter.h:8-10, .cpp:8-47
 *     public:
 *       BloomFilter(long length);             src/bloom_filter.h:12
 *       void set(KEY_t);                      src/bloom_filter.cpp:49-53
 *       bool is_set(KEY_t) const;             src/bloom_filter.cpp:55-59
 *   };
 *
 * and for its sizing in Run::Run (src/run.cpp:13-15).  Results are bit-exact
 * with the reference: the same bitmap (dynamic_bitset block layout, bit i in
 * 64-bit block i/64 at bit i%64) after the same keys are set, and the same
 * is_set booleans.  k = 3 with the reference's three fixed hashes.
 *
 * Conventions
 *   - Plain C types only; `void *stream` is a hipStream_t, NULL meaning HIP's
 *     default (null) stream as in every HIP API.  No HIP or torch headers are
 *     needed to bind this ABI.
 *   - Every entry point returns an int status: 0 on success, a negative
 *     errno-style code on failure; nothing throws across the ABI.  The
 *     reference has no error path at all (m == 0 is a SIGFPE there,
 *     src/bloom_filter.cpp:19); here m == 0 is rejected with BLOOMHIP_EINVAL.
 *   - A handle owns one device bitmap on one device.  Calls on a handle are
 *     ordered on the stream they are given; different handles may be driven
 *     from different host threads (one per GPU for per-run sharding).
 *   - Device-resident calls (keys_on_device = 1, out_on_device = 1) are
 *     asynchronous.  A call given any HOST buffer synchronises the stream
 *     before it returns, so host buffers may be reused immediately (the
 *     reference's calls are synchronous, src/run.cpp:93,162).
 *   - Keys are KEY_t = int32_t (src/types.h:4) read at `stride_bytes`
 *     (4 for a packed key vector, 8 for entry_t runs, src/types.h:14-22).
 */
#ifndef BLOOMHIP_H
#define BLOOMHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BLOOMHIP_ABI_VERSION 1

#define BLOOMHIP_OK 0
#define BLOOMHIP_EIO (-5)     /* HIP runtime error; see bloomhip_last_error() */
#define BLOOMHIP_ENOMEM (-12) /* device allocation failed */
#define BLOOMHIP_ENODEV (-19) /* no such device / no GPU */
#define BLOOMHIP_EINVAL (-22) /* bad argument (m == 0, NULL, bad stride...) */
#define BLOOMHIP_ERANGE (-34) /* size out of supported range */

/* Build strategies for bloomhip_set_batch (bloomhip_set_strategy). */
#define BLOOMHIP_BUILD_AUTO 0      /* pick by m and n (default) */
#define BLOOMHIP_BUILD_ATOMIC 1    /* one pass, global atomicOr per bit */
#define BLOOMHIP_BUILD_LDS 2       /* private LDS bitmap per workgroup (m/8 <= LDS) */
#define BLOOMHIP_BUILD_PARTITION 3 /* hash+bin pass, then LDS segment pass */

/* Probe strategies for bloomhip_test_batch (bloomhip_set_probe_strategy). */
#define BLOOMHIP_PROBE_AUTO 0      /* LDS for LDS-sized filters, gather up to 8 MiB, else partition */
#define BLOOMHIP_PROBE_GATHER 1    /* per-key gathers of the 3 bits */
#define BLOOMHIP_PROBE_PARTITION 2 /* bin positions by segment, test in LDS */
#define BLOOMHIP_PROBE_LDS 3       /* whole filter staged in each workgroup's LDS (m/8 <= 160 KiB) */
/* One partitioned pass for up to 8 filters whose sizes all divide the largest
 * one's (x % m_j == (x % m_max) % m_j): an LSM's stacked levels, where run
 * capacities grow by the fanout (src/lsm_tree.cpp:36-41).  AUTO picks it for
 * such groups when it beats probing the members one by one. */
#define BLOOMHIP_PROBE_STACKED 4

typedef struct bloomhip_filter bloomhip_filter;

int bloomhip_abi_version(void);
/* Digest of the kernel sources this library was compiled from (first 16 hex
 * digits of SHA-256 over csrc/bloom_kernels.hip, bloom_kernels.h,
 * bloom_math.h): measurement tools tie profiles to the kernels that ran. */
const char *bloomhip_kernel_sha(void);
const char *bloomhip_strerror(int status);
/* Text of the last HIP error seen by this host thread ("" if none). */
const char *bloomhip_last_error(void);
int bloomhip_device_count(int *count);

/* m = (long)((float)max_size * bits_per_entry): Run::Run's sizing of its
 * filter, evaluated in float exactly as src/run.cpp:13-15 does. */
int bloomhip_m_bits(int64_t max_size, float bits_per_entry, uint64_t *m_out);

/* BloomFilter(long length): an all-zero filter of m_bits bits on `device`.
 * src/bloom_filter.h:12.  m_bits must be >= 1. */
int bloomhip_create(int device, uint64_t m_bits, bloomhip_filter **out);
int bloomhip_destroy(bloomhip_filter *f);

/* table.size() (src/bloom_filter.cpp:19) and the number of 64-bit blocks. */
int bloomhip_size(const bloomhip_filter *f, uint64_t *m_out);
int bloomhip_nwords(const bloomhip_filter *f, uint64_t *nwords_out);
int bloomhip_device(const bloomhip_filter *f, int *device_out);
/* Device address of the bitmap (ceil(m/64) uint64 blocks), for zero-copy
 * interop.  Valid until bloomhip_destroy.  A deferred clear is issued on the
 * default stream first. */
int bloomhip_device_words(const bloomhip_filter *f, void **dptr_out);
/* A non-blocking stream owned by the handle, for callers that want the
 * filter's work off the default stream (pass it as `stream`). */
int bloomhip_stream(const bloomhip_filter *f, void **stream_out);

/* Reset every bit to 0.  The memset is deferred: a following partition
 * build overwrites every word anyway, and any other use of the bitmap issues
 * it first on that use's stream. */
int bloomhip_clear(bloomhip_filter *f, void *stream);

/* BloomFilter::set for keys[0..n): src/bloom_filter.cpp:49-53, as called per
 * written entry by Run::put (src/run.cpp:162) during a flush
 * (src/lsm_tree.cpp:127-129) or compaction (src/lsm_tree.cpp:81-88). */
int bloomhip_set_batch(bloomhip_filter *f, const void *keys, size_t n, size_t stride_bytes,
                       int keys_on_device, void *stream);

/* BloomFilter::is_set of every key against each of nf filters
 * (src/bloom_filter.cpp:55-59; Run::get's probe, src/run.cpp:93, over the
 * runs a GET visits, src/lsm_tree.cpp:180-212).  All filters must live on
 * one device.  Result bit i%64 of out_packed[j*ceil(n/64) + i/64] is
 * is_set(key i) for filters[j]; bits past n in the last word are 0. */
int bloomhip_test_batch(const bloomhip_filter *const *filters, int nf, const void *keys,
                        size_t n, size_t stride_bytes, int keys_on_device,
                        uint64_t *out_packed, int out_on_device, void *stream);

/* --- run metadata and batched GET routing ------
 *
 * bloomhip_set_batch_run: a whole run written at once (a flush,
 * src/lsm_tree.cpp:124-129, or a compaction's output, :74-88): set() of every
 * key as bloomhip_set_batch, plus the run's metadata that Run::put builds in
 * the same pass (src/run.cpp:158-174): a fence pointer = the key of every
 * entry whose index is a multiple of 4096 (getpagesize(), :164-166), and the
 * max key (:170; the reference leaves max_key uninitialised, src/run.h:13 —
 * here it starts at INT32_MIN).  Replaces the previous metadata. */
int bloomhip_set_batch_run(bloomhip_filter *f, const void *keys, size_t n, size_t stride_bytes,
                           int keys_on_device, void *stream);
/* Metadata of a run restored from disk (fences ascending).  Synchronous. */
int bloomhip_set_run_meta(bloomhip_filter *f, const int32_t *fences, size_t nfences,
                          int32_t max_key);
/* Metadata back to the host: *nfences_out always; fences (if non-NULL,
 * capacity cap) and *max_key_out.  Synchronous. */
int bloomhip_get_run_meta(const bloomhip_filter *f, int32_t *fences, size_t cap,
                          size_t *nfences_out, int32_t *max_key_out);

/* Batched GET routing over nruns <= 64 runs, runs[0] the newest
 * (LSMTree::get_run order, src/lsm_tree.cpp:141-151).  Run r is a candidate
 * for key i when Run::get would read a page for it (src/run.cpp:94-96):
 *     fence_r[0] <= key <= max_key_r  &&  is_set_r(key)
 * (a run without metadata is never a candidate).  Outputs, each optional
 * (NULL to skip):
 *   cand_packed  nruns x ceil(n/64) u64, bit i%64 of row r word i/64;
 *   first_run[i] the newest candidate (the run LSMTree::get settles on when
 *                the key is there, src/lsm_tree.cpp:195-201), -1 if none;
 *   page[i]      that run's page index, upper_bound(fences, key) - 1
 *                (src/run.cpp:97-99), -1 if none.
 * Reading the page and checking the key stays with the caller, or goes to
 * bloomhip_get_batch below. */
int bloomhip_route_gets(const bloomhip_filter *const *runs, int nruns, const void *keys,
                        size_t n, size_t stride_bytes, int keys_on_device,
                        uint64_t *cand_packed, int32_t *first_run, int32_t *page,
                        int out_on_device, void *stream);
/* The same routing with first_run and page packed into one u32 per GET, half
 * the output bytes of the two int32 arrays (the GET's whole answer for
 * Run::get, src/run.cpp:93-99, in one word):
 *   route[i] = first_run[i] << 28 | page[i]   when key i has a candidate run,
 *              BLOOMHIP_ROUTE_NONE            when it has none.
 * nruns <= 16.  cand_packed as above; each output optional (NULL to skip). */
#define BLOOMHIP_ROUTE_NONE 0xFFFFFFFFu
#define BLOOMHIP_ROUTE_PAGE_BITS 28
int bloomhip_route_gets_packed(const bloomhip_filter *const *runs, int nruns, const void *keys,
                               size_t n, size_t stride_bytes, int keys_on_device,
                               uint64_t *cand_packed, uint32_t *route, int out_on_device,
                               void *stream);

/* Batched GET, whole (LSMTree::get past the buffer, src/lsm_tree.cpp:173-215;
 * Run::get, src/run.cpp:85-113): routing as bloomhip_route_gets, then the
 * candidate runs are read on the device until one holds the key.  runs[0] is
 * the newest, nruns <= 64, all on one device.
 * entries[r]: run r's entry_t {int32 key; int32 val;} records, keys strictly
 * ascending (as a flush or bloomhip_compact writes them), nentries[r] of them,
 * on runs' device when entries_on_device (8-byte aligned); host entries are
 * staged to the device inside the call.
 * Per key i, newest run first: run r is read when it is a routing candidate
 * (fence_r[0] <= key <= max_key_r && is_set_r(key)); its page is
 * upper_bound(fences, key) - 1, and the entries searched are that fence
 * interval, [page * 4096, min((page + 1) * 4096, nentries[r])).  If the key
 * is there, found_run[i] = r and vals[i] = its value, VAL_TOMBSTONE
 * (INT32_MIN) included: a tombstone in a newer run hides older values
 * (src/lsm_tree.cpp:214).  If not, the read was a false positive and the next
 * candidate run is visited.  No run holds the key: found_run[i] = -1 and
 * vals[i] = INT32_MIN, so vals[i] != INT32_MIN is exactly "the reference
 * prints a value".
 * stats (optional, 2 * nruns u64, overwritten by every call; zeros when
 * n == 0): stats[2r] = page reads of run r, stats[2r + 1] = how many of those
 * did not hold the key.  vals and found_run are optional too (NULL to skip).
 * Outputs are all host or all device.  Asynchronous when keys, entries and
 * outputs are all device-resident; otherwise the stream is synchronised
 * before the call returns.
 * BLOOMHIP_EINVAL: NULLs where data is required, nentries[r] > 0 with
 * entries[r] NULL, or a run with fences whose entries do not fit them
 * (nfences != ceil(nentries[r] / 4096)); a run without fences is never a
 * candidate and may have any entries.  With that check and the kernel's
 * clamping of every entry index to [0, nentries[r]), entries that disagree
 * with a run's metadata give unspecified answers but no access outside them.
 * Deviation from the reference: Run::put places a fence every 4096 ENTRIES
 * (src/run.cpp:164) while Run::get reads 4096 BYTES at byte offset
 * page * 4096 (:101-103): 512 entries, at the wrong place for any page > 0,
 * slots past the run's size included.  Here the interval
 * the fences describe is searched; for runs of at most 512 entries the two
 * agree on every stored key. */
int bloomhip_get_batch(const bloomhip_filter *const *runs, const void *const *entries,
                       const size_t *nentries, int nruns, int entries_on_device,
                       const void *keys, size_t n, size_t stride_bytes, int keys_on_device,
                       int32_t *vals, int32_t *found_run, uint64_t *stats,
                       int out_on_device, void *stream);

/* --- persistence beside the run -------------------------
 * The reference keeps a run's entries in an mmap'd file (src/run.cpp:34-72)
 * and its filter only in memory (src/run.h:11).  bloomhip_save writes the
 * bitmap (dynamic_bitset blocks) and the run metadata to `path` (written to
 * path.tmp, then renamed); bloomhip_load creates a filter on `device` from
 * such a file (BLOOMHIP_EINVAL for a file that is not one, or is damaged:
 * the file ends with an FNV-1a 64 checksum).  bloomhip_build_from_run_file
 * maps a run file of entry_t {key, val} records (src/types.h:14-22), sizes
 * the filter as Run::Run does (m = (long)((float)max_size * bpe),
 * src/run.cpp:13-15) and builds it and the run metadata from its first
 * n_entries records.  All synchronous. */
int bloomhip_save(const bloomhip_filter *f, const char *path);
int bloomhip_load(const char *path, int device, bloomhip_filter **out);
int bloomhip_build_from_run_file(const char *path, uint64_t n_entries, int64_t max_size,
                                 float bits_per_entry, int device, bloomhip_filter **out);

/* --- compaction fused with the new run's filter build ----
 * LSMTree::merge_down (src/lsm_tree.cpp:48-95) through MergeContext
 * (src/merge.cpp:6-39): a k-way merge of nruns key-sorted runs of entry_t
 * {key, val} records (src/types.h:14-22), runs[0] the newest (precedence 0),
 * releasing for each distinct key only the newest run's entry; with
 * drop_tombstones (merging into the last level, src/lsm_tree.cpp:84-86)
 * entries whose val is VAL_TOMBSTONE (INT32_MIN) are dropped.  The merged run
 * (ascending keys) goes to out_entries (capacity: the sum of nentries; must
 * not alias an input) and its length to *n_out.  When f is not NULL the new
 * run's filter and metadata are built from the merged keys in the same call
 * (bloomhip_set_batch_run on the device copy).  Runs and output are host
 * buffers unless runs_on_device / out_on_device; everything runs on
 * `device` (f's device when given).  Synchronous (the output length is
 * returned). */
int bloomhip_compact(const void *const *runs, const size_t *nentries, int nruns,
                     int runs_on_device, int drop_tombstones, void *out_entries, size_t *n_out,
                     int out_on_device, bloomhip_filter *f, int device, void *stream);

/* --- batched RANGE: newest-wins range scans over the runs -------------------
 * LSMTree::range (src/lsm_tree.cpp:218-290) over Buffer::range and Run::range
 * (src/run.cpp:115-157), for nq queries at once.  Query q has the bounds
 * [starts[q], ends[q]), end exclusive as the reference's CLI.  Its answer is
 * the entries {key, val} with starts[q] <= key < ends[q], taken over all runs,
 * keys ascending; for a key held by several runs only the newest run's entry
 * counts (runs[0] is the newest), and that entry is dropped when its value is
 * VAL_TOMBSTONE (INT32_MIN): a tombstone in a newer run hides older live
 * values (src/lsm_tree.cpp:273-279; MergeContext precedence, src/merge.cpp).
 * ends[q] <= starts[q] answers nothing (:226-229); a key equal to INT32_MAX is
 * never returned, as in the reference.
 * The answer depends only on entries, starts and ends; run metadata only
 * speeds the search.  1 <= nruns <= 64.  runs[r] may be NULL or a handle
 * without metadata: that run is searched by plain binary search over its
 * entries, which is how the memtable (Buffer::range) is passed, as a sorted
 * runs[0].  Every non-NULL handle is on `device`; one that has fences must
 * have nfences == ceil(nentries[r] / 4096), as for bloomhip_get_batch.
 * entries[r]: entry_t records, keys strictly ascending, on `device` when
 * entries_on_device (8-byte aligned); host entries are staged inside the call.
 * starts, ends: packed int32[nq], on the device when bounds_on_device.
 * Outputs: offsets (required, nq + 1 u64) and out_entries, both host or both
 * device (out_on_device; 8-byte aligned there): query q's answer is
 * out_entries[offsets[q] .. offsets[q + 1]), offsets[0] = 0 and offsets[nq] =
 * *total_out (required, a host pointer).
 *   out_entries == NULL && out_capacity == 0: count only; offsets and
 *     *total_out are filled, BLOOMHIP_OK.
 *   *total_out > out_capacity otherwise: BLOOMHIP_ERANGE; offsets and
 *     *total_out are valid and no byte of out_entries is written.
 *   nq == 0: offsets[0] = 0, *total_out = 0.
 * Always synchronous (the total is returned).
 * BLOOMHIP_EINVAL (nothing is launched): NULLs where data is required,
 * nentries[r] > 0 with entries[r] NULL, misaligned entries or device outputs,
 * a fence / entry mismatch, a handle on another device, nruns out of range, a
 * bad device.  BLOOMHIP_ERANGE also for nq >= 2^32 - 1, and for a query with
 * more than BLOOMHIP's compaction limit of candidates (2^32 - 2 entries of
 * all runs inside its bounds), which is answered as a compaction of its
 * sub-ranges; offsets are not valid then.  Every entry index is clamped into
 * [0, nentries[r]]: entries that disagree with their fences, or are not
 * strictly ascending, give unspecified answers but no access outside them or
 * outside the query's slice of out_entries.
 * BLOOMHIP_RANGE_PATH = auto | compact (environment, read per call): compact
 * answers every non-empty query as a compaction (for tests).
 * Deviation from the reference, beside the one of bloomhip_get_batch:
 * Run::range maps num_pages * 4096 BYTES at byte offset page * 4096
 * (src/run.cpp:142-145) while the fences sit every 4096 ENTRIES (:164), so
 * for runs over 512 entries it scans the wrong place.  Here every entry of
 * the run inside the bounds is returned; for runs of at most 512 entries the
 * two agree. */
int bloomhip_range_batch(const bloomhip_filter *const *runs, const void *const *entries,
                         const size_t *nentries, int nruns, int entries_on_device,
                         const int32_t *starts, const int32_t *ends, size_t nq, int bounds_on_device,
                         uint64_t *offsets, void *out_entries, size_t out_capacity,
                         size_t *total_out, int out_on_device, int device, void *stream);

/* --- batched PUT: a batch of puts and deletes sorted into a run -------------
 * The write side up to a flush.  LSMTree::put (src/lsm_tree.cpp:104-139)
 * inserts into Buffer, a std::set<entry_t> ordered by key, where a second put
 * of a key replaces the first (src/buffer.cpp:37-58); del is a put of
 * VAL_TOMBSTONE (src/lsm_tree.cpp:292-294) and load a put per record of a
 * binary file (:296-309).  A flush walks the set in key order into a new
 * level-0 run (:124-131), Run::put setting filter bits and fences on the way.
 * ops: n entry_t {int32 key; int32 val;} records in arrival order, a delete
 * being a record whose val is INT32_MIN; host memory (4-byte aligned) unless
 * ops_on_device (8-byte aligned).  ops is not modified.
 * The answer is what iterating Buffer::entries gives after Buffer::put of
 * every op in order, with a buffer large enough never to refuse: one entry per
 * distinct key, keys strictly ascending as signed int32, each carrying the
 * value of the LAST op on its key.  With drop_tombstones (level 0 is the
 * tree's last level, as in bloomhip_compact) entries whose surviving value is
 * INT32_MIN are left out: a delete followed by a put of the key survives, a
 * put followed by a delete does not.
 * out_entries (capacity n entries; host, or on `device` when out_on_device;
 * aligned as ops; must not overlap ops) receives the run and *n_out its
 * length.  When f is not NULL the new run's filter and metadata are built
 * from the output keys in the same call (bloomhip_set_batch_run on the device
 * copy), exactly as bloomhip_compact does it.  Synchronous (the length is
 * returned).
 * n == 0: *n_out = 0; f, if given, is cleared and receives the metadata of a
 * run of no keys.
 * Checked before any HIP call, in this order: BLOOMHIP_EINVAL for n_out ==
 * NULL, for n > 0 with ops or out_entries NULL, for a misaligned ops or
 * out_entries, for f on another device than `device`; BLOOMHIP_ERANGE for
 * n >= 2^32 - 1 (32-bit offsets, bloomhip_compact's limit).  Then
 * BLOOMHIP_ENODEV without a GPU and BLOOMHIP_EINVAL for a bad device.
 * BLOOMHIP_FLUSH_PATH = auto | tiled (environment, read per call): a batch
 * that fits one workgroup's LDS is sorted and de-duplicated in one launch;
 * tiled sends it down the multi-launch radix sort instead (for tests).
 * Deviation from the reference: it decides the flush boundaries itself.
 * Buffer::put refuses once the buffer holds max_size distinct keys, even for
 * a key already in it (src/buffer.cpp:42), and the tree flushes then.  Here
 * the caller chooses the batch.  A larger batch gives the same GET and RANGE
 * answers (newest-wins is associative) but other run boundaries;
 * bloomhip_flush_cuts below finds the reference's own cut points in an op
 * stream, and bloomhip_tree_put_batch ingests a stream at them. */
int bloomhip_flush_batch(const void *ops, size_t n, int ops_on_device, int drop_tombstones,
                         void *out_entries, size_t *n_out, int out_on_device,
                         bloomhip_filter *f, int device, void *stream);

/* --- the reference's flush cut points in an op stream -----------------------
 * Where LSMTree::put flushes (src/lsm_tree.cpp:104-139): Buffer::put replaces
 * the value of a key the buffer holds and refuses every op, even one on a key
 * it holds, once it holds buffer_max_entries distinct keys (src/buffer.cpp:
 * 37-58); the tree then flushes and the refused op starts a new buffer.  A
 * segment therefore ends right after the op that brought its B-th distinct
 * key, and the cut is realised only if another op follows: a stream that ends
 * exactly there leaves a full buffer and no flush.
 * ops: n entry_t records in arrival order, as for bloomhip_flush_batch (host,
 * 4-byte aligned, or on `device`, 8-byte aligned); only the keys matter.
 * cuts[0..*ncuts_out): the realised cuts 0 < c_1 < c_2 < ... < n (host
 * memory): segment k is ops[c_{k-1}, c_k) with c_0 = 0, and the tail
 * ops[c_last, n) stays in the buffer.  *ncuts_out is always the true count;
 * when it exceeds cuts_cap the call returns BLOOMHIP_ERANGE and writes nothing
 * to cuts.  n <= buffer_max_entries has no cut and launches nothing.
 * Synchronous.
 * Checked before any HIP call, in this order: BLOOMHIP_EINVAL for ncuts_out ==
 * NULL, buffer_max_entries == 0, a NULL or misaligned ops with n > 0, cuts ==
 * NULL with cuts_cap > 0; BLOOMHIP_ERANGE for n >= 2^32 - 1.  Then
 * BLOOMHIP_ENODEV without a GPU and BLOOMHIP_EINVAL for a bad device. */
int bloomhip_flush_cuts(const void *ops, size_t n, int ops_on_device,
                        uint64_t buffer_max_entries, uint64_t *cuts, size_t cuts_cap,
                        size_t *ncuts_out, int device, void *stream);

/* --- the LSM tree handle ----------------------------------------------------
 * LSMTree (src/lsm_tree.cpp:28-139) with batched ingest.  After any sequence
 * of bloomhip_tree_put_batch calls the handle holds exactly the tree the
 * reference holds after the same ops put one by one: the same runs in the same
 * levels with the same entries, filter bits and fences, and the same buffer.
 * Level l holds up to `fanout` runs of capacity buffer_max_entries *
 * fanout^l; a run's filter has bloomhip_m_bits(that capacity, bits_per_entry)
 * bits (src/lsm_tree.cpp:28-42, src/run.cpp:13-15).  The cascade of flushes
 * and merge_downs (:44-102) is not replayed: every run the tree holds after a
 * batch is built once, from one contiguous slice of the op stream and the old
 * runs that end in it (newest-wins is associative).  Tombstones are kept by a
 * flush and dropped only by a merge into the last level (:84-86).
 * Calls on one tree serialise on a lock of the tree and are synchronous.
 *
 * bloomhip_tree_create: BLOOMHIP_EINVAL for out == NULL, buffer_max_entries ==
 * 0, depth < 1, fanout < 1 or bloomhip_m_bits(buffer_max_entries,
 * bits_per_entry) == 0 (the reference divides by zero there); BLOOMHIP_ERANGE
 * for depth * fanout + 1 > 64 (GET and RANGE take at most 64 runs) or a level
 * capacity past int64; all before any HIP call.
 * bloomhip_tree_put_batch: ops as for bloomhip_flush_batch; *nflushes_out
 * (optional) = the number of flushes the reference makes on them.  When the
 * reference would die with "No more space in tree" the call returns
 * BLOOMHIP_ERANGE; after that, or any other error, the tree is as it was.
 * BLOOMHIP_ERANGE also when buffer + ops reach 2^32 - 1 entries.
 * bloomhip_tree_get_batch, bloomhip_tree_range_batch: bloomhip_get_batch and
 * bloomhip_range_batch over the buffer and then the runs in LSMTree::get_run
 * order (level 0 newest to oldest, then level 1, ...; :141-151), with their
 * output contracts and their documented deviation (the reference's 4096-byte
 * page window).  found_run[i] is -1 for no run, 0 for the buffer and 1 + r
 * for run r in get_run order, empty runs counted.
 * bloomhip_tree_shape: runs per level (depth values) and the buffer's entries.
 * bloomhip_tree_run: run `index` (0 = newest) of `level`, or the buffer
 * (level -1, index 0, as a key-sorted run): its filter, its entries on the
 * device and their number, all owned by the tree and valid until its next
 * put_batch or destroy.  A run that ended with no entries (everything dropped
 * at the last level) still occupies its slot. */
typedef struct bloomhip_tree bloomhip_tree;
int bloomhip_tree_create(int device, uint64_t buffer_max_entries, int depth, int fanout,
                         float bits_per_entry, bloomhip_tree **out);
int bloomhip_tree_destroy(bloomhip_tree *t);
int bloomhip_tree_put_batch(bloomhip_tree *t, const void *ops, size_t n, int ops_on_device,
                            size_t *nflushes_out, void *stream);
int bloomhip_tree_get_batch(const bloomhip_tree *t, const void *keys, size_t n, size_t stride_bytes,
                            int keys_on_device, int32_t *vals, int32_t *found_run,
                            int out_on_device, void *stream);
int bloomhip_tree_range_batch(const bloomhip_tree *t, const int32_t *starts, const int32_t *ends,
                              size_t nq, int bounds_on_device, uint64_t *offsets, void *out_entries,
                              size_t out_capacity, size_t *total_out, int out_on_device, void *stream);
int bloomhip_tree_shape(const bloomhip_tree *t, uint32_t *runs_per_level, uint64_t *memtable_entries);
int bloomhip_tree_run(const bloomhip_tree *t, int level, int index, const bloomhip_filter **f_out,
                      const void **entries_dev_out, size_t *nentries_out);

/* Scalar compatibility entry points (one key; synchronous), for
 * BloomFilter::set (src/bloom_filter.cpp:49-53) and is_set (:55-59) called
 * once per key.  Low-latency path: the key travels as a kernel argument (no
 * host-to-device copy), one single-lane kernel on HIP's default stream, and
 * is_set's answer is written straight into a pinned, mapped host word of the
 * handle: one launch + one stream synchronisation per call (bench.py
 * `scalar_is_set` measures it).  Calls on one handle serialise on its lock;
 * batch callers should use bloomhip_set_batch / bloomhip_test_batch. */
int bloomhip_set(bloomhip_filter *f, int32_t key);
int bloomhip_is_set(const bloomhip_filter *f, int32_t key, int *hit_out);

/* Persistence: copy the bitmap out/in as ceil(m/64) uint64 blocks in the
 * reference's dynamic_bitset layout.  Host buffers; synchronous.  Upload
 * rejects blocks with bits set at positions >= m. */
int bloomhip_download(const bloomhip_filter *f, uint64_t *words, size_t nwords, void *stream);
int bloomhip_upload(bloomhip_filter *f, const uint64_t *words, size_t nwords, void *stream);

/* A copy of filter src (bitmap, run metadata, strategies) on `device`: a
 * peer copy over xGMI between GPUs, a device-to-device copy on one GPU.  The
 * probe side of per-run sharding: each GPU holds replicas of the
 * runs' filters and probes its own slice of the GET keys.  Synchronous. */
int bloomhip_clone(const bloomhip_filter *src, int device, bloomhip_filter **out);

/* Wait for all work queued on `stream` (NULL: the default stream). */
int bloomhip_sync(const bloomhip_filter *f, void *stream);

/* Build strategy override (BLOOMHIP_BUILD_*); AUTO by default. */
int bloomhip_set_strategy(bloomhip_filter *f, int strategy);
/* Probe strategy (BLOOMHIP_PROBE_*) for this filter; AUTO by default.  In a
 * test_batch the first filter's setting applies to filters left on AUTO. */
int bloomhip_set_probe_strategy(bloomhip_filter *f, int strategy);
/* Strategy AUTO resolved for a batch of n keys on this filter. */
int bloomhip_resolve_strategy(const bloomhip_filter *f, size_t n, int *strategy_out);

/* Per-kernel device timing.  While enabled, every kernel the handle launches
 * is bracketed by HIP events on its stream; bloomhip_profile_read returns,
 * for kernel slot `slot` (0..BLOOMHIP_PROF_SLOTS-1), its name, launch count
 * and summed device milliseconds (it synchronises the stream). */
#define BLOOMHIP_PROF_SLOTS 13
int bloomhip_profile_enable(bloomhip_filter *f, int enable);
int bloomhip_profile_read(bloomhip_filter *f, int slot, const char **name_out,
                          uint64_t *launches_out, double *ms_out);
int bloomhip_profile_reset(bloomhip_filter *f);

/* Free the scratch the partition build / partitioned probe cache per
 * (device, stream).  Waits for those streams; call when no build is queued. */
int bloomhip_trim(void);

/* Self-test hook (no GPU needed): the engine's own position arithmetic —
 * the same inline functions the kernels run — evaluated on the host.
 * out[3*i + j] = hash_{j+1}(keys[i]) % m. */
int bloomhip_host_positions(uint64_t m, const int32_t *keys, size_t n, uint64_t *out);

/* Self-test hook (no GPU needed): the plan bloomhip_tree_put_batch builds its
 * runs by.  Given the runs per level before a batch (depth values, each at
 * most fanout) and the number of flushes the batch makes, the flushes and
 * merge_downs (src/lsm_tree.cpp:44-139) are simulated on shapes only.  The
 * plan is flat int32 records, one per run of the final tree, level by level,
 * newest first:
 *     level, first_new_segment, n_new_segments, n_old,
 *     then n_old pairs (old_level, old_index), the newest old run first
 * (old_index counts from the newest run of its level before the batch).  The
 * run is the newest-wins merge of new segments [first, first + n_new) of the
 * op stream, all newer than its old runs; n_new_segments = 0 with one old run
 * of the same level means "kept as it is".  *plan_len_out = the int32 values
 * the plan takes.  BLOOMHIP_ERANGE when the reference would die with "No more
 * space in tree" (*plan_len_out = 0), and when plan_cap is too small
 * (*plan_len_out valid, nothing written). */
int bloomhip_tree_plan_host(const uint32_t *runs_per_level, int depth, int fanout,
                            uint64_t nflushes, int32_t *plan, size_t plan_cap,
                            size_t *plan_len_out);

#ifdef __cplusplus
}
#endif

#endif /* BLOOMHIP_H */
