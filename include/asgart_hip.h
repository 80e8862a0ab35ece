/*
 * asgart_hip.h -- C ABI of the MI355X-native segmental-duplication search core.
 *
 * Drop-in boundary for ONE path of delehef/asgart 2.5.1: the body of
 * `SearchDuplications::run` (reference src/bin/asgart.rs:137-258), i.e.
 *   suffix array  ->  Searcher (8-mer interval cache + k-mer equal range)
 *   ->  automaton::search_duplications over every chunk  ->  left fix-up.
 * Everything is plain pointers + sizes in the style of the reference's own FFI
 * to libdivsufsort (reference src/divsufsort.rs:8-33): extern "C", caller-owned
 * inputs, caller-allocated outputs (two-call count/copy), int32 status
 * (0 ok, <0 error), no callbacks, no torch types.
 *
 * All compute runs in hand-written HIP kernels for gfx950; there is NO CPU
 * fallback: every entry point that needs the GPU fails with ASGART_E_HIP when
 * no device is usable.
 *
 * The reference-side binding (Rust `extern "C"` block + build.rs line) is shown
 * in INTEGRATION.md.
 */
#ifndef ASGART_HIP_H
#define ASGART_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ASGART_OK 0
#define ASGART_E_ARG (-1)  /* bad argument / unsupported setting            */
#define ASGART_E_OOM (-2)  /* host or device allocation failed              */
#define ASGART_E_HIP (-3)  /* HIP runtime error, or no usable gfx950 device */
#define ASGART_E_CAP (-4)  /* an internal capacity was exceeded (see msg)   */

/* RunSettings as it reaches the path (reference src/structs.rs:36-58; Copy).
 * max_gap_size already includes +probe_size (reference src/bin/asgart.rs:681). */
typedef struct asgart_settings {
    uint64_t probe_size;              /* -k ; 8 <= k <= 128 in this build         */
    uint32_t max_gap_size;            /* -g + -k                                 */
    uint64_t min_duplication_length;  /* --min-length                            */
    uint64_t max_cardinality;         /* --max-cardinality.  The reference keeps the arms of a chunk in an unbounded
                                         Vec (src/automaton.rs:87).  Here the live arms of one automaton segment never
                                         exceed max_cardinality * (ceil(max_gap_size / (probe_size/2)) + 1) -- 6500 at
                                         the defaults -- and the last extension tier sizes its HBM slices for exactly
                                         that bound, whatever the settings (ASGART_E_CAP only if it reaches 2^24).   */
    uint8_t reverse;                  /* -R                                      */
    uint8_t complement;               /* -C                                      */
} asgart_settings;

/* ProtoSD (reference src/structs.rs:418-429).  `left` is already global (the
 * fix-up of src/bin/asgart.rs:229-237 is applied inside); identity is 0.0 and
 * reversed/complemented equal the settings of the call (:245-247). */
typedef struct asgart_proto_sd {
    uint64_t left, right, left_length, right_length;
} asgart_proto_sd;

/* Device-side timings (HIP events on the library's own stream) and work
 * counters of the LAST asgart_search_duplications / asgart_probe_hits call. */
typedef struct asgart_stats {
    double ms_total;        /* first kernel -> results on host                   */
    double ms_search;       /* probe-search + count kernels (dominant, HBM-bound) */
    double ms_scan;         /* prefix scans + segment detection                   */
    double ms_fill;         /* hit materialisation (CSR fill)                     */
    double ms_extend;       /* placement + all extension tiers + cascade            */
    uint64_t probes_total;
    uint64_t probes_n_skipped;
    uint64_t probes_searched;
    uint64_t probes_card_skipped;
    uint64_t probes_with_hits;
    uint64_t raw_hits;      /* sum of SA-interval sizes h_p (filled only when ASGART_STATS_RAW_HITS or
                               ASGART_STATS_YARDSTICK was requested: an untimed pass over the call's probes) */
    uint64_t filtered_hits; /* CSR size                                            */
    uint64_t segments;      /* independent automaton instances                     */
    uint64_t families;
    uint64_t proto_sds;
    uint64_t bisect_steps;  /* sum ceil(log2(b_p+1)), b_p = 8-mer bucket (yardstick;
                               filled only when ASGART_STATS_YARDSTICK was requested) */
    uint64_t search_launches; /* number of launches of the dominant kernel          */
    uint64_t overflow_segments; /* segments a tier gave up on (re-run by a larger tier)  */
    double ms_extend_tier2;   /* part of ms_extend spent re-running those (cascade)    */
    uint64_t heavy_segments;  /* segments placed in tiers 3..7 (workgroup kernels)      */
    double ms_probe_count;    /* probe_count_kernel alone (first kernel of ms_search) */
    /* filled only with ASGART_STATS_YARDSTICK, by an untimed accounting pass over the same probes: */
    uint64_t search_bytes;    /* bytes the probe-search kernels load and store BY DESIGN (window
                                 staging, position bits, prefix-table entries, keys read by the bisection,
                                 suffix-array entries read, outputs): the algorithmic bytes of this kernel */
    uint64_t probes_filter_rejected; /* probes answered by the position bits alone                  */
    uint64_t search_bytes_wide_loads; /* ... of search_bytes, those loaded as whole-wave 16-byte-per-lane reads (text windows,
                                         position bits): what FETCH_SIZE counts at half on gfx950 (accounting pass only) */
    double ms_longest_tier;   /* part of ms_extend: the longest chain of extension tiers on one stream, from the
                                 launch of the tiers to the end of the chain's last tier (early re-runs included) --
                                 the tiers run side by side, one stream per hardware queue the process may open
                                 (asgart_tier_plan), and tiers that share a stream run one after the other.  A tier
                                 the plan puts on the main stream runs behind the runs over ranges, and its chain
                                 counts them.  With a stream per tier this is the tier that ran longest: in practice
                                 the longest serial automaton segment of the call                               */
    uint64_t passes;          /* passes (orientations) the call ran as ONE job: 1 for a plain call; n for the passes call
                                 when it fuses them (the counters above are then sums over the passes, the timings those
                                 of the one job)                                                                 */
    double ms_longest_segment; /* part of ms_extend: the longest time ONE automaton segment took on its workgroup -- the
                                  serial floor of the call: src/automaton.rs:96-201 is serial per chunk, and neither more
                                  compute units nor more GPUs shorten a segment (ms_longest_tier is the tier that FINISHED
                                  last, which is throughput when the tier holds many segments)                    */
    uint64_t split_segments;   /* long segments that ran as ranges side by side (option split) ...                */
    uint64_t split_refused;    /* ... and those of them with a cut that did not hold (the rest behind it ran as one more
                                  run, or the whole segment again)                                                 */
} asgart_stats;

typedef struct asgart_index asgart_index;
typedef struct asgart_families asgart_families;

/* Replaces `divsufsort64` (reference src/divsufsort.rs:10, call site
 * src/bin/asgart.rs:473-479): signature-identical.  Builds the suffix array of
 * T[0..n) on the GPU (prefix doubling) into the caller-allocated SA. */
int32_t asgart_sa_build64(const uint8_t *T, int64_t *SA, int64_t n);

/* Replaces `Searcher::new(dna, sa, 0)` plus the Arc-sharing of text and SA
 * (reference src/bin/asgart.rs:142-155, src/searcher.rs:99-143): uploads text
 * and suffix array to HBM of `device` and builds the search structures.
 * T must consist of bytes in {A,C,G,T,N} with at most one '$', as its last
 * byte (what prepare_data produces, src/bin/asgart.rs:289-301,430).
 * SA may be NULL: the library then builds it on the GPU itself. */
int32_t asgart_index_create(const uint8_t *T, int64_t n, const int64_t *SA, int64_t sa_len,
                            int32_t device, asgart_index **out);
void asgart_index_destroy(asgart_index *idx);

/* Replicates an index on another device (text + suffix array copied device to device -- over xGMI
 * between two GPUs -- instead of sorting the suffixes once per GPU; the probe_size-specific tables are
 * rebuilt there on first use).  Replaces nothing in the reference (it has one address space); it is the
 * "SA + text replicated in each HBM" step of the multi-GPU design. */
int32_t asgart_index_clone(asgart_index *src, int32_t device, asgart_index **out);

/* The same for a host that is one process per GPU (the multi-GPU arrangement of BASELINE.json's north star): the
 * process that built the suffix array hands out the device addresses of text and suffix array
 * (asgart_index_export: valid while the index lives, read-only), broadcasts them with its collective library
 * (ncclBroadcast over xGMI; asgart_amd/multi.py: replicate_index) and every other process creates its replica from
 * the received DEVICE buffers, which are copied (asgart_index_create_device; d_text: n bytes; d_sa: n entries of
 * sa_entry_bytes = 4, or 8 when n >= 2^32 - 256, as asgart_index_export reports).  No suffix sort and no host copy
 * per GPU.  The text is validated on the device like asgart_index_create validates it. */
int32_t asgart_index_export(asgart_index *idx, const void **d_text, const void **d_sa, int32_t *sa_entry_bytes);
int32_t asgart_index_create_device(const void *d_text, int64_t n, const void *d_sa, int64_t sa_len,
                                   int32_t sa_entry_bytes, int32_t device, asgart_index **out);
/* (d_sa == NULL: the suffixes are sorted on the GPU, as asgart_index_create does for SA == NULL.) */

/* Replaces prepare_data behind the FASTA reader (reference src/bin/asgart.rs:273-430; the reader itself, bio's, stays
 * with the host): records[r] / record_lens[r] are the raw sequence bytes of record r as read (all files' records in
 * order, :375-395).  On the GPU: alphabet normalisation (:289-301: upper-cased unless skip_masked -- then lower-case
 * bases become N --, everything outside {A,T,G,C,N} becomes N), find_chunks_to_process per record (:317-366: cut at
 * runs of more than 5000 N; a record without any piece left gives one chunk over all of it), concatenation and the
 * final '$' (:430).
 *   text_out   nullable; sum(record_lens) + 1 bytes: the prepared strand (Strand.data) for hosts that want it
 *   chunks     (start, len) pairs in global coordinates, record order -- what asgart_search_duplications takes;
 *              *n_chunks receives their number; with chunks_cap too small: ASGART_E_CAP and *n_chunks = the room needed
 *              (chunks_cap = 0: count only)
 *   index_out  nullable; an index over the prepared text, its suffixes sorted on the GPU (what asgart_index_create
 *              would build from text_out, without the text travelling to the host and back)
 * The strand map (record names / offsets, src/structs.rs:60-65) is the host's: offsets are the prefix sums of
 * record_lens. */
int32_t asgart_prepare_data(const uint8_t *const *records, const uint64_t *record_lens, int64_t n_records,
                            int32_t skip_masked, int32_t device, uint8_t *text_out, uint64_t *chunks,
                            int64_t chunks_cap, int64_t *n_chunks, asgart_index **index_out);

/* Device memory the library keeps for reuse (released blocks of 256 MiB and more, so that an index build does not
 * pay the runtime's slow first allocation after large frees) goes back to the device: at the end of
 * asgart_index_prepare, when the last index of a device is destroyed, when one of the library's own allocations
 * fails -- and here, for a host about to allocate a lot by other means.  Returns the bytes released, < 0 on error. */
int64_t asgart_trim_cache(int32_t device);

/* Diagnostics for a host that suspects a stalled call (no reference counterpart: the reference has no device to wait
 * for): writes the NATIVE call stack of every thread of the process to stderr -- glibc backtrace from the handler of
 * a realtime signal of the library's own (SIGRTMIN + 6), installed at the first call and never removed, one thread
 * after the other, each acknowledging for itself -- so that a wait inside the HIP runtime, which a Python- or
 * Rust-level stack dump shows as one opaque frame -- names the runtime call it sits in.  Callable from any thread,
 * in particular from a watchdog thread while the main thread is blocked (tests/conftest.py does on a test time-out).
 * Returns the number of threads asked. */
int32_t asgart_debug_dump_stacks(void);

/* `--trim START END` (reference src/bin/asgart.rs:142-148, validation :432-463, README "trimming"):
 * the suffix array covers only data[start..end] + '$' -- its entries shifted by +start -- and the WHOLE
 * input is then searched against it (Searcher::new(&strand.data, &suffix_array, 0), :151-155).  SA: that
 * shifted array with sa_len == end - start + 1 entries (what the reference's r_divsufsort + shift
 * produces), or NULL to build it on the GPU.  Requires 0 <= start < end <= n - 1 (the trim the
 * reference's prepare_data lets through).  The array is sorted by the sub-strand's suffixes but
 * compared through the full text, so the suffixes ending within k bases of `end` are out of place; the
 * library replays the reference's two bisections (libdivsufsort sa_search for the 8-mer cache,
 * superslice equal_range_by per probe) wherever one of them is in range -- results equal the oracle's. */
int32_t asgart_index_create_trim(const uint8_t *T, int64_t n, const int64_t *SA, int64_t sa_len,
                                 int64_t trim_start, int64_t trim_end, int32_t device,
                                 asgart_index **out);

/* Tuning and test options of an index.  Production code never needs this call: the defaults
 * are the tuned ones.  Each option can also be preset through the environment variable
 * ASGART_<NAME> (upper case), which is read ONCE, inside asgart_index_create -- the search path
 * itself never reads the environment.  Values are range-checked; ASGART_E_ARG for an unknown
 * name or a value out of range.  Names: shard_lookback, shard_lookahead (halo sizes of a sharded
 * call, in probes); force_tier, arms_kernel, long3, cap1, cap3_pct, cap45_pct, cap6_pct, cap6w_pct, dense3, dense6,
 * tier_order, grid1..grid7, solo (placement of segments on the extension kernels); barren (segments that provably emit
 * nothing are not run: 0 none, 1 by their number of hit-probes, 2 also by the positions of their hits); split, split_len,
 * split_runs, split_warm, split_warm_max, split_min (long segments run as ranges side by side, each checked against its
 * predecessor at the cut; where a cut does not hold the ranges in front of it stand, the rest of the segment runs as one
 * more run, and the next call over the same input starts that segment's ranges as far in front of their cuts as the
 * failed one asked for; split = 2: with 64-bit positions as well);
 * fuse_passes, fuse_pole_pct (passes of one call as one job or pipelined); posbits, rank_lists, lazy_aux (the
 * position bits and the position-sorted lists, and when the lists come into being); cache_calls, prewarm
 * (memory); watchdog_s; debug; test_cap_limit, test_genbits, test_k8_delay, test_fail_alloc, test_stall_s,
 * test_wide_batch (parity and failure tests).  RESULTS NEVER DEPEND ON ANY OF THEM.  The full table with ranges is
 * kOptions in asgart_amd/csrc/index.hip, every field is described in struct Options
 * (asgart_amd/csrc/index.hpp).  ptab_depth and force_wide are fixed at creation (environment
 * only).  Blocks until no call is in flight. */
int32_t asgart_index_set_option(asgart_index *idx, const char *name, int64_t value);

/* The tail rule of the placement.  A call with fewer hardware queues than extension tiers runs some tiers behind each
 * other on one stream, and the second one's longest segment then starts when the first one's has ended.  The rule moves
 * the few segments that make up the tail of tier 2, 4 or 5 (those with at least the tier's threshold of hits; the thresholds
 * are part of the tier table, asgart_tier_profile) to the next arm-resident workgroup tier that holds more arms (4, 5 or 6,
 * never tier 3), whose launch a longer segment bounds anyway.  mode 0: off; 1 (the default): on in calls with fewer tier
 * streams than arm-resident tiers that can hold work; 2: always on.  hits > 0 replaces the table's thresholds (tests).
 * RESULTS NEVER DEPEND ON EITHER.  Blocks until no call is in flight.  ASGART_E_ARG: mode outside 0..2, hits outside
 * 0..2^31. */
int32_t asgart_index_set_tail_up(asgart_index *idx, int32_t mode, int64_t hits);

/* O(n) verifier of the suffix array held by the index, on the GPU: SA must be a permutation of
 * 0..n-1 whose adjacent suffixes are in strictly increasing bytewise order (the same rank trick as
 * the CPU oracle's checker).  Returns the number of violating slots (0 = valid), < 0 on error.
 * The reference never checks its suffix array (it even ignores divsufsort64's status,
 * src/bin/asgart.rs:475-477); this exists for the full-size parity tests, where the text is too
 * large for the CPU checker (n >= 2^32: 64-bit suffix numbers). */
int64_t asgart_index_check_sa(asgart_index *idx);

/* Optional: build the probe_size-specific search keys now (otherwise done
 * lazily by the first call that needs them; kept until another k is used). */
int32_t asgart_index_prepare(asgart_index *idx, uint64_t probe_size);

/* Replaces the body of SearchDuplications::run from the chunk fan-out to the
 * fold (reference src/bin/asgart.rs:201-253): for every chunk (start,len) runs
 * automaton::search_duplications (src/automaton.rs:57-204) on the prepared
 * needle and returns the families in (chunk, discovery) order.
 * chunks: n_chunks pairs (start, len).  progress: nullable, n_chunks entries; the reference stores
 * the needle offset of every probe as it goes (src/automaton.rs:98, Relaxed) for a progress bar that
 * polls every 500 ms (src/bin/asgart.rs:160-197).  Here all chunks advance together through a few
 * device-wide phases, so every entry jumps to its chunk's final offset at once: when every probe of the
 * call has been searched and its hits materialised (the HBM-bound, chip-wide part is over; the extension
 * automaton is under way) and again when the call returns.  A host that polls the array from another
 * thread can issue its next call at that moment: the new call's search phases then run beside this
 * call's extension, whose tail is a few serial segments on one compute unit each (bench.py pipelines the
 * -RC and the direct pass of a step that way: 338 instead of 441 ms per step on the GRCh38-sized input). */
int32_t asgart_search_duplications(asgart_index *idx, const uint64_t *chunks, int64_t n_chunks,
                                   const asgart_settings *settings, volatile uint64_t *progress,
                                   asgart_families **out);

/* Same, restricted to shard `shard` of `n_shards` (multi-GPU: one process per GPU, index replicated, no
 * exchange between shards): shard r owns the automaton segments that START in the r-th of n_shards equal slices of
 * the probe sequence; it searches its slice plus a look-back and a look-ahead halo (retrying with larger halos when a
 * decision is ambiguous).  The union of the shards' families, merged by asgart_families_keys -- or concatenated in shard
 * order -- is exactly the unsharded result (asgart_amd/multi.py merges by key). */
int32_t asgart_search_duplications_shard(asgart_index *idx, const uint64_t *chunks,
                                         int64_t n_chunks, const asgart_settings *settings,
                                         int32_t shard, int32_t n_shards,
                                         asgart_families **out);

/* Multi-GPU in ONE process: indices[r] is a replica of the same index on device r
 * (asgart_index_create on every device, or asgart_index_clone from the device that built it).  One host
 * thread per device runs shard r of n_devices; the per-shard families -- tens of MB -- come back over
 * each device's own host link and are concatenated in shard order: exactly the result of
 * asgart_search_duplications on one device.  No device-to-device exchange is needed inside one process
 * (the host is common); one-process-per-GPU hosts gather the shards' lists with RCCL instead, see
 * INTEGRATION.md section 4 and asgart_amd/multi.py.  The same index may appear more than once (each call
 * takes one of its internal contexts), which is how the sharding logic is tested on a single GPU. */
int32_t asgart_search_duplications_multi(asgart_index *const *indices, int32_t n_devices,
                                         const uint64_t *chunks, int64_t n_chunks,
                                         const asgart_settings *settings, volatile uint64_t *progress,
                                         asgart_families **out);

/* The general form of the two calls above: shard `shard` of `n_shards` (0 of 1: everything) with the
 * progress array of asgart_search_duplications (entries of ALL chunks are written). */
int32_t asgart_search_duplications_ex(asgart_index *idx, const uint64_t *chunks, int64_t n_chunks,
                                      const asgart_settings *settings, int32_t shard, int32_t n_shards,
                                      volatile uint64_t *progress, asgart_families **out);

/* Several passes over the same chunks in ONE call -- what the `asgart` binary does when it is run with
 * and without -R / -C over one strand (reference src/bin/asgart.rs:677-693 builds one RunSettings per
 * invocation; the direct and the -RC run of BASELINE.json's "direct+RC" are two of them): settings[j] are
 * the RunSettings of pass j, out[j] receives its families (exactly what asgart_search_duplications returns
 * for settings[j]).  Passes that differ in orientation only (same probe_size, max_gap_size,
 * min_duplication_length, max_cardinality; up to four) run as ONE job: the probe sequence is pass 0's
 * chunks followed by pass 1's ... (chunk order inside each pass as in src/bin/asgart.rs:201-253), searched, scanned
 * and placed in one sweep at full chip rate, and every extension tier is ONE launch over the merged, cost-sorted
 * segment list, so that every pass's longest serial segments start at once on compute units of their own
 * (asgart_stats.passes tells).  An unsharded call that finds ONE segment to be its whole extension (its longest single
 * segment above option fuse_pole_pct = 88 % of the extension: the other pass's front might hide beside that segment)
 * makes the index TIME the calls that follow both ways in turn -- one job, pipelined single-pass calls, two each -- and
 * keep the faster way for these settings; sharded calls always run as one job; option fuse_passes = 2 / 0 forces
 * either.  Otherwise (different
 * settings) the library pipelines the passes as single calls: pass j+1 is issued the moment the chip-wide,
 * HBM-bound phases of pass j are over (probe search, scans, hit materialisation -- the moment the `progress`
 * array of a single call jumps), so its search runs beside pass j's extension automaton, whose tail is a few
 * serial segments on one compute unit each; the passes are issued longest extension first (from the
 * durations the index remembers per orientation; reversed orientations first while nothing is known).
 * At most two passes are in flight (the index's two call contexts).  Results do not depend on the order.
 * On error every out[j] is NULL. */
int32_t asgart_search_duplications_passes(asgart_index *idx, const uint64_t *chunks, int64_t n_chunks,
                                          const asgart_settings *settings, int32_t n_passes,
                                          asgart_families **out);
/* ... restricted to shard `shard` of `n_shards`: the shard's slice of EVERY pass (see asgart_search_duplications_shard),
 * all of them as the same ONE job -- rank r of an n-GPU run executes the algorithm a single GPU does, on 1/n of the
 * probes of each pass.  Every pass's families carry keys counted from the start of their own pass. */
int32_t asgart_search_duplications_passes_shard(asgart_index *idx, const uint64_t *chunks, int64_t n_chunks,
                                                const asgart_settings *settings, int32_t n_passes,
                                                int32_t shard, int32_t n_shards, asgart_families **out);

void asgart_families_counts(const asgart_families *f, uint64_t *n_families, uint64_t *n_sds);
/* fam_offsets: n_families+1 entries; sds: n_sds entries */
void asgart_families_copy(const asgart_families *f, uint64_t *fam_offsets, asgart_proto_sd *sds);
/* keys: n_families entries, (first probe of the family's automaton segment << 32) | family ordinal inside it.
 * Ascending keys == the reference's order (chunk order, discovery order inside a chunk, src/bin/asgart.rs:241-253).
 * The shards of a sharded call own contiguous slices of every pass: a gatherer merges their families by key
 * (asgart_search_duplications_multi does; one-process-per-GPU hosts do it after the RCCL gather, asgart_amd/multi.py)
 * or concatenates them in shard order. */
void asgart_families_keys(const asgart_families *f, uint64_t *keys);
void asgart_families_free(asgart_families *f);

/* ---- ComputeScore (`--compute-score`) --------------------------------------
 * Replaces the ComputeScore step, reference src/bin/asgart.rs:98-112 with
 * ProtoSD::levenshtein, src/structs.rs:439-452: for each of the n_sd duplications
 * identity = 100 * (1 - levenshtein(left arm, right arm) / max(left_length, right_length)),
 * arms taken over the INCLUSIVE ranges [p ..= p + length] of the text, the right arm
 * reversed / complemented first when the flags say so; computed in f64, stored as f32
 * like `sd.identity`.  Exact unit-cost edit distance (anti-diagonal DP on the GPU).
 * Errors: a range that reaches past the text (the reference panics), two empty arms. */
int32_t asgart_compute_scores(asgart_index *idx, const asgart_proto_sd *sds, int64_t n_sd,
                              int32_t reversed, int32_t complemented, float *identity);

/* ComputeScore over several GPUs.  The reference scores every duplication of a run in one loop
 * (src/bin/asgart.rs:98-112); each identity depends on its own duplication alone, so the list splits by
 * duplication and the shards' values are copied, never reduced: every value is bit-equal to what
 * asgart_compute_scores gives for the same duplication.  The DP of one duplication is not split.
 *
 * asgart_score_owners: host code, needs no device.  owner[q] in [0, n_shards) for each of the n_sd
 * duplications: greedy, longest first (ties: lower q first) onto the least-loaded shard (ties: lower shard
 * first).  The load is the device time the Levenshtein kernels take for a duplication, in wave-steps, as
 * asgart_score_costs reports it: its (left_length + 1) x (right_length + 1) DP cells rounded up to the
 * shape of the kernel it is dispatched to (one wave per duplication, or a 16-wave band pipeline for left
 * arms of 8192 rows and more, with the pipeline's fill and drain).  Bound: the most loaded shard costs at
 * most total / n_shards + the largest single cost.  The result depends only on the lengths and n_shards.
 * Errors: n_shards < 1 (ASGART_E_ARG), arms of 2^32 bases (ASGART_E_CAP). */
int32_t asgart_score_owners(const asgart_proto_sd *sds, int64_t n_sd, int32_t n_shards, int32_t *owner);
/* The cost model asgart_score_owners balances: cost[q] for each duplication (host code, needs no device). */
int32_t asgart_score_costs(const asgart_proto_sd *sds, int64_t n_sd, uint64_t *cost);

/* asgart_tier_plan: host code, needs no device.  The streams the extension tiers of one search call run on, as the
 * call plans them: budget = the normal-priority hardware queues the process may open (GPU_MAX_HW_QUEUES, default 4;
 * at least 1, above 32 counts as 32), n_work[t - 1] != 0 for each tier t = 1..7 with work, tier_order as the option,
 * est_ms[t - 1] = tier t's estimated duration, main_ms = what the main stream carries ahead of the tiers (the runs
 * over ranges).  The tiers with work are packed longest first (ties: launch order) onto the least-loaded of
 * min(6, budget) tier streams (ties: lower stream first) and, with a budget of 2 or more, the main stream (after the
 * tier streams on ties), each behind what its stream already holds.  Writes stream_of[t - 1]: 0 = the main stream,
 * s = tier stream s (1-based), -1 = no work; launch[0..6] = the tiers with work in launch order, each once, 0 behind
 * them: the first tier of every stream, then the second ones, ..., each rank in tier_order's order (the tiers it names,
 * then the rest).  A budget of 1 gives one chain in tier_order's order.  Bound: the most
 * loaded stream carries at most main_ms + total / streams + the largest single estimate.  The result depends only on
 * the arguments.  Errors: budget < 1, a digit of tier_order outside 1..7, a negative or non-finite estimate
 * (ASGART_E_ARG). */
int32_t asgart_tier_plan(int32_t budget, const uint64_t *n_work, int64_t tier_order, const double *est_ms, double main_ms,
                         int32_t *stream_of, int32_t *launch);

/* Replaces the ComputeScore loop (src/bin/asgart.rs:98-112) for shard `shard` of `n_shards` -- one process
 * per GPU, index replicated: every rank passes the SAME full list; the call scores the duplications
 * asgart_score_owners gives to `shard` and writes identity[q] for those only (the other entries are not
 * touched).  The list goes to the device whole and the shard's duplications are gathered there, then
 * scheduled longest first like asgart_compute_scores.  The whole list is validated as asgart_compute_scores
 * validates it, so every rank fails alike.  Returns the number of duplications the shard owned, < 0 on
 * error.  A gatherer copies each shard's values back to their input positions (asgart_amd/multi.py:
 * compute_scores). */
int64_t asgart_compute_scores_shard(asgart_index *idx, const asgart_proto_sd *sds, int64_t n_sd,
                                    int32_t reversed, int32_t complemented, int32_t shard, int32_t n_shards,
                                    float *identity);

/* Replaces the same loop for ONE process over several GPUs, shaped like asgart_search_duplications_multi:
 * indices[r] is a replica of the same text on device r (asgart_index_clone); one host thread per replica
 * runs shard r of n_devices, and identity receives all n_sd values -- exactly asgart_compute_scores' array.
 * The same index may appear more than once.  If a shard fails the call fails, and the message names the
 * shard. */
int32_t asgart_compute_scores_multi(asgart_index *const *indices, int32_t n_devices, const asgart_proto_sd *sds,
                                    int64_t n_sd, int32_t reversed, int32_t complemented, float *identity);

/* The same three with ONE FLAG BYTE PER DUPLICATION instead of one pair of flags per call: ProtoSD::levenshtein
 * (reference src/structs.rs:439-452) reads `reversed` / `complemented` of the duplication it scores, so a list that
 * holds the duplications of several runs over one strand (the direct and the -RC one, as asgart-slice merges their
 * files, src/structs.rs:114-141) is scored in one call.  flags[q]: bit 0 reversed, bit 1 complemented, the encoding of
 * asgart_extract_sequences; NULL means all zero; any other bit set is ASGART_E_ARG (checked over the whole list, on
 * every shard).  identity[q] is bit-equal to what the call above gives for duplication q with q's two flags.  The
 * owners (asgart_score_owners) and the schedule do not look at the flags. */
int32_t asgart_compute_scores_flags(asgart_index *idx, const asgart_proto_sd *sds, const uint8_t *flags, int64_t n_sd,
                                    float *identity);
int64_t asgart_compute_scores_flags_shard(asgart_index *idx, const asgart_proto_sd *sds, const uint8_t *flags,
                                          int64_t n_sd, int32_t shard, int32_t n_shards, float *identity);
int32_t asgart_compute_scores_flags_multi(asgart_index *const *indices, int32_t n_devices, const asgart_proto_sd *sds,
                                          const uint8_t *flags, int64_t n_sd, float *identity);

/* ---- the alignment of the two arms of each duplication ------------------------------------------------------
 * ComputeScore above says how similar two arms are; this says where they differ: one optimal unit-cost path through the
 * edit matrix of every duplication, as run-length-encoded operations.  No counterpart in the reference.
 *   A = a_1..a_n  the left arm; B = b_1..b_m the right arm as the score walks it (reversed if flags[q] bit 0 is set,
 *                 complemented if bit 1 is set; ACGT and acgt swap, anything else is kept; bytes compare as bytes)
 *   inclusive     1: the arms are [p ..= p + length] (n = left_length + 1: the strings asgart_compute_scores compares);
 *                 0: [p, p + length) (what a PAF row describes)
 *   the path      D[i][0] = i, D[0][j] = j; traced from (n, m) while i > 0 or j > 0: if i > 0 and j > 0 and
 *                 D[i][j] == D[i-1][j-1] + (a_i != b_j): '=' on equal bases, 'X' otherwise, i--, j--; else if i > 0 and
 *                 D[i][j] == D[i-1][j] + 1: 'I' (a left-arm base without a partner), i--; else 'D', j--.  The operations
 *                 are then put in forward order and run-length encoded: the result is unique.
 *   budget_bytes  the device memory the checkpoints of one batch may take (asgart_align_bytes gives each duplication's
 *                 share); 0: half of what is free.  The duplications are packed largest first into batches that fit.  A
 *                 duplication that alone exceeds the budget is REFUSED: status[q] = 0, no runs, distance 0xFFFFFFFF,
 *                 identity NaN; the others are unaffected.  NO RESULT DEPENDS ON THE BUDGET OR ON THE BATCHING.
 *   out           asgart_alignment_counts / _copy / _free: run_offsets[n_sd + 1], the CSR rows of the runs; run_len and
 *                 run_op ('=', 'X', 'I', 'D') per run; distance[q] = the unit-cost edit distance; identity[q] =
 *                 100 (1 - distance / max(left_length, right_length)) as float, bit-equal to asgart_compute_scores_flags
 *                 when inclusive = 1; status[q] = 1 aligned, 0 refused.  Any array of _copy may be NULL.
 * Errors, those of the score: an arm past the text, two empty arms, a flag bit other than 0 and 1 (ASGART_E_ARG), arms of
 * 2^32 bases (ASGART_E_CAP).  One wave walks each pair, and this call walks the whole n x m matrix of it;
 * asgart_align_duplications_banded below walks a diagonal corridor of it, which is what a megabase pair needs.  Neither
 * has _shard / _multi variants. */
typedef struct asgart_alignment asgart_alignment;
int32_t asgart_align_duplications(asgart_index *idx, const asgart_proto_sd *sds, const uint8_t *flags, int64_t n_sd,
                                  int32_t inclusive, uint64_t budget_bytes, asgart_alignment **out);
void asgart_alignment_counts(const asgart_alignment *a, uint64_t *n_sd, uint64_t *n_runs, uint64_t *n_refused);
int32_t asgart_alignment_copy(const asgart_alignment *a, uint64_t *run_offsets, uint32_t *run_len, uint8_t *run_op,
                              uint32_t *distance, float *identity, uint8_t *status);
/* Milliseconds of the call behind a: [0] the upload, [1] the forward pass (distances and checkpoints), [2] the traceback and
 * the compaction, [3] the copy back; summed over the batches.  ASGART_E_ARG for a NULL argument. */
int32_t asgart_alignment_timings(const asgart_alignment *a, double *ms4);
void asgart_alignment_free(asgart_alignment *a);
/* Rows of one band, rows of one lane and columns of one tile (W) of the kernels behind asgart_align_duplications, for tests
 * that place their cases on the seams. */
void asgart_align_geometry(uint64_t *band_rows, uint64_t *lane_rows, uint64_t *tile_cols);
/* Host code, needs no device: bytes[q] = the checkpoint bytes of duplication q,
 * 4 (n_bands - 1)(m + 1) + 4 floor((m - 1) / W) n_bands band_rows, with n_bands = max(1, ceil(n / band_rows)) and no column
 * checkpoint for m = 0. */
int32_t asgart_align_bytes(const asgart_proto_sd *sds, int64_t n_sd, int32_t inclusive, uint64_t *bytes);

/* ---- the same alignment inside a diagonal corridor ---------------------------------------------------------
 * asgart_align_duplications spends n m cells and n m / 51 checkpoint bytes on a duplication; two arms at edit distance d
 * have every optimal path within about |m - n| + d diagonals.  This call spends cells and bytes in proportion to
 * n (band_rows + corridor width), and gives the same runs.
 * THE RULE.  For arms of n and m bases and a bound T = max_distance[q], let e = floor((T - |m - n|) / 2).
 *   T < |m - n|   more than T edits, without any work: a path needs |m - n| insertions or deletions.
 *   otherwise     every path of cost <= T stays on the diagonals k = j - i in [min(0, m - n) - e, max(0, m - n) + e].
 *                 (A path that reaches diagonal k > max(0, m - n) has k deletions to get there from diagonal 0 and k - (m - n)
 *                 insertions to get back to diagonal m - n: 2 k - (m - n) <= T gives k <= max(0, m - n) + e; below
 *                 min(0, m - n) likewise.)
 *   the region    for band b, the rows b band_rows + 1 .. min((b + 1) band_rows, n), the columns
 *                 lo_b = max(1, b band_rows + 1 + kmin) .. hi_b = min(m, min((b + 1) band_rows, n) + kmax): the smallest
 *                 rectangle that holds those diagonals of the band's rows, clipped to [1, m].  Row 0 is D[0][j] = j, column 0
 *                 is D[i][0] = i where lo_b = 1, and every other cell outside the rectangles counts as 2^30.  n + m and T stay
 *                 below 2^30 (see the errors), so a value that descends from such a cell is at least 2^30, more than any
 *                 bound, and at most 2^30 + n + m: `+ 1` never wraps.
 * Two facts follow; the tests rest on them.
 *   THE BOUND IS DECISIVE.  Every computed value is 2^30 or more, or the cost of a path from (0, 0) that stays inside the
 *                 region: the recurrence takes minima over such paths and over cells that count as 2^30.  So a computed
 *                 D[n][m] <= T is the cost of a real path, hence >= the distance; and a path of the distance's cost, which is
 *                 <= T then, stays on the diagonals above, inside the region, so the computed value is <= the distance: it IS
 *                 the distance.  If the distance is <= T the same path makes the computed value <= T; so a computed value
 *                 > T means a distance > T.
 *   THE PATH IS THE SAME PATH.  Let the computed D[n][m] be <= T.  A cell on an optimal path (one of the distance's cost) has
 *                 its true value: the path up to it is optimal for it and lies inside the region.  The trace stands on such
 *                 a cell and tests its predecessors in the rule's order: diagonal, up, left.  A predecessor that satisfies
 *                 its equality with true values lies on an optimal path too, so its computed value is its true value and the
 *                 equality holds with computed values; one that does not satisfy it has a computed value that is no smaller
 *                 than its true one (or counts as 2^30), so the equality fails with computed values as well.  Every test
 *                 comes out as in the full matrix, step after step: runs, distance and identity are bit-equal to
 *                 asgart_align_duplications'.
 *   max_distance  one bound per duplication, each < 2^30.  status[q] = 2: q has more edits than its bound; no runs, distance
 *                 0xFFFFFFFF, identity NaN, like a refusal.  status 0 (alone over the budget) and 1 as above; a status-1
 *                 entry equals asgart_align_duplications' entry bit for bit.
 *                 NULL: AUTOMATIC.  Every duplication starts at the bound |m - n| + max(64, max(n, m) / 64), at most n + m;
 *                 those that come out with status 2 are aligned again with 4 times the bound, at most n + m, round after
 *                 round; at n + m the corridor is the whole matrix, so no status 2 remains after the call.  The first bound
 *                 and the factor are design constants.  THEY WERE REASONED, NOT SWEPT (csrc/align_dev.hpp gives the
 *                 reasoning: a first corridor for young copies of 98.4 % identity and more; failed rounds that cost a third
 *                 of the one that succeeds).
 *   budget_bytes  as above, with asgart_align_bytes_banded's bytes: batching is by corridor bytes, and in automatic mode a
 *                 duplication is refused when the corridor of the round it has reached exceeds the budget alone.  NO
 *                 RESULT DEPENDS ON THE BUDGET OR ON THE BATCHING.
 *   out           as above.  asgart_alignment_timings sums over batches and rounds.  asgart_alignment_rounds: the passes over
 *                 the list (1 with given bounds, and for asgart_align_duplications) and the cells of the forward passes of
 *                 all rounds, the rectangles' (n m each for asgart_align_duplications); either may be NULL.
 * Errors: those above; a bound of 2^30 or more (ASGART_E_ARG); arms of 2^30 bases together, n + m (ASGART_E_CAP). */
int32_t asgart_align_duplications_banded(asgart_index *idx, const asgart_proto_sd *sds, const uint8_t *flags, int64_t n_sd,
                                         int32_t inclusive, const uint32_t *max_distance, uint64_t budget_bytes,
                                         asgart_alignment **out);
int32_t asgart_alignment_rounds(const asgart_alignment *a, uint32_t *rounds, uint64_t *cells);
/* Host code, needs no device: bytes[q] = the checkpoint bytes of duplication q within max_distance[q] (not NULL here).  With
 * span = |m - n| + 2 e, the corridor's diagonals less one, and wmax = min(m, band_rows + span), the widest rectangle:
 *   4 n_bands band_rows ceil((wmax - 1) / W) + 4 (n_bands - 1)(wmax + 1)
 * every band has column checkpoints at the multiples of W among its columns but the last and, but for the last band, a
 * bottom row, each laid out for wmax columns.  0 for T < |m - n| and for an empty arm.  Errors as above. */
int32_t asgart_align_bytes_banded(const asgart_proto_sd *sds, int64_t n_sd, int32_t inclusive, const uint32_t *max_distance,
                                  uint64_t *bytes);

/* ---- the steps behind the search step ------------------------------------------
 * Replaces FilterNs, ReOrder, ReduceOverlap and Sort of the reference's step chain (src/bin/asgart.rs:33-96 with
 * ProtoSD::n_content src/structs.rs:454-467, reduce_overlap :481-562; order :738-747) for the families of one run,
 * given as the arrays asgart_families_copy fills (fam_offsets: n_families + 1 entries).  ComputeScore, the optional
 * step between ReduceOverlap and Sort, is asgart_compute_scores (call it on the result: Sort does not look at it).
 * The N content of every arm is counted on the GPU over the resident text (inclusive ranges [p ..= p + length], the
 * f32 quotient and the 0.2 threshold as the reference computes them); the reduction runs on `threads` host threads
 * (0: all), one family at a time each.  out: the surviving families (asgart_families_counts / _copy / _free;
 * asgart_families_keys gives the input ordinal of every surviving family).
 * Errors: a duplication whose inclusive range reaches past the text (the reference panics there). */
int32_t asgart_post_process(asgart_index *idx, const uint64_t *fam_offsets, uint64_t n_families,
                            const asgart_proto_sd *sds, int32_t threads, asgart_families **out);

/* ---- the sequences of the duplicons (asgart-extract) -------------------------------------------------------
 * Replace the body of reference src/bin/asgart-extract.rs:110-200 behind its FASTA reader and JSON reader.
 * A source is the raw bytes of every record of every file, concatenated in order as the FASTA reader returns them
 * (:17-29, :110-117): NOT the normalised strand of the search (soft-masked lower case and IUPAC letters stay as they
 * are); its positions are the search's global positions (normalisation keeps lengths, src/bin/asgart.rs:289-310).
 * asgart_source_create takes the same record arrays as asgart_prepare_data and uploads them once to `device`
 * (through pinned staging pieces); it needs no suffix array and is independent of any index. */
typedef struct asgart_source asgart_source;
int32_t asgart_source_create(const uint8_t *const *records, const uint64_t *record_lens, int64_t n_records,
                             int32_t device, asgart_source **out);
void asgart_source_destroy(asgart_source *src);
/* The two arms of duplicons first, first + 1, ... of sds[n_sd] (global coordinates), left then right for each,
 * packed into the host buffer out[out_cap] for as many WHOLE duplicons as fit:
 *   left  = source[left .. left + left_length]                                                   (:123-125)
 *   right = source[right .. right + right_length], reversed if flags[j] & 1, then complemented if flags[j] & 2 with
 *           utils::complement_nucleotide (src/utils.rs:1-23: A<->T, G<->C keeping the case, N / n stay, any other
 *           byte becomes N)                                                                      (:126-134)
 * flags: one byte per duplicon of sds (NULL: all 0).  seq_ends[2 (j - first) + 0 / 1] receive the end offsets in
 * `out` of the left / right arm of duplicon j, *n_done the number of duplicons extracted (call again with
 * first + *n_done for the rest).  Errors: a duplicon whose first arm does not fit into out_cap (ASGART_E_CAP;
 * seq_ends[0..1] then hold its ends: seq_ends[1] is the room it needs), an arm past the source (ASGART_E_ARG: the
 * reference panics on the slice), a byte >= 0x80 in what is extracted (ASGART_E_ARG: the reference panics in
 * String::from_utf8, :136-137).  Calls from several host threads on one source are safe (they take turns). */
int32_t asgart_extract_sequences(asgart_source *src, const asgart_proto_sd *sds, const uint8_t *flags, int64_t n_sd,
                                 int64_t first, uint8_t *out, uint64_t out_cap, uint64_t *seq_ends, int64_t *n_done);

/* ---- the filters of asgart-slice on a result held as arrays ------------------------------------------------
 * Replaces the per-duplication work of reference src/bin/asgart-slice.rs:126-191 for a RunResult of any size: the arm
 * rewrite of RunResult::flatten (src/structs.rs:401-414), the retains of remove_direct .. remove_intra (:143-194), of
 * --min-length (asgart-slice.rs:150-155), max_family_members (:196-198), keep_ / restrict_ / exclude_fragments and their
 * _regexp forms (:232-348), every `families.retain(|f| !f.is_empty())`, and the global positions consolidate_families
 * (:216-227) and exclude_fragments (:311-318) recompute.  It needs no index and no source: only `device`.
 * Names never reach the device.  The host keeps a NAME TABLE (every fragment name of the map once, then every other name
 * an arm carries, such as "unknown") and answers each question that looks at a name per entry of that table -- the
 * reference asks them per arm, with string compares (`to_keep.iter().any(..)`, `to_flatten.iter().any(..)`):
 *   new_id, addend   flatten: the arm's name id and what is added to its chr_*_position (:405-412); both NULL: no collapse
 *   keep_mask        bit p set where the name passes pattern p of --keep-fragments (a literal list is ONE bit: the name
 *                    is in it); a duplication stays iff ((mask[left] | mask[right]) & keep_all) == keep_all -- the
 *                    patterns of -E are applied one after the other (asgart-slice.rs:159-169), so they intersect
 *   restrict_mask    the same for --restrict-fragments: ((mask[left] & mask[right]) & restrict_all) == restrict_all
 *   exclude          bit 0: the name is excluded by any pattern (or is in the literal list); bit 1: by the FIRST pattern
 *                    (the list); bit 2: the name is not in the map as keep / restrict left it.  A duplication that passes
 *                    keep, restrict and the first exclusion with bit 2 on an arm is where the reference panics
 *                    (`find_chr(..).unwrap()`, :313-316): ASGART_E_ARG, the message names the first such input ordinal
 *   final_pos        the position of the first fragment of that name in the final map, -1 when the map has none
 * table_len[0..5] are the entries of the six tables in this order; each table in use must have n_names of them.
 * options: flags_set / flags_clear are the flag bits (bit 0 reversed, bit 1 complemented) a survivor must / must not have
 * (--no-direct: set 1, --no-reversed: clear 1, --no-uncomplemented: set 2, --no-complemented: clear 2); inter_mode 1 is
 * --no-inter, 2 --no-inter-relaxed with collapsed_id the id of ASGART_COLLAPSED (-1: no such name); drop_empty is set when
 * any step runs that drops the families it emptied (every one but collapse and max_family_members); relocate when the
 * global positions are recomputed (keep, restrict or exclude ran): final_pos[id] + chr position, or 0 (`map_or(0, ..)`).
 * Order, as the reference's: collapse; the flag, inter / intra and length filters; max_family_members on the sizes they
 * leave (with drop_empty a family they emptied is gone before it is asked); keep, restrict, exclude.
 * in: fam_offsets[n_families + 1], sds[n_sd] (global coordinates), flags[n_sd], chr[2 n_sd] name ids (left, right),
 * chr_pos[2 n_sd].  out (asgart_slice_counts / _copy / _free): the surviving families and duplications IN INPUT ORDER
 * with the rewritten chr, chr_pos and global positions, and keys[q] = the input ordinal of surviving duplication q, by
 * which the caller gathers what the slice does not look at (identity, sequences).  Every copy target is nullable.
 * Checked on the host before anything is launched (ASGART_E_ARG): fam_offsets not starting at 0, decreasing or not ending
 * at n_sd; a name id outside the table; a table in use that is NULL or not n_names long. */
typedef struct asgart_slice asgart_slice;
typedef struct asgart_slice_options {
    uint8_t flags_set, flags_clear;
    uint8_t inter_mode;           /* 0 none, 1 --no-inter, 2 --no-inter-relaxed          */
    uint8_t no_intra;
    uint8_t drop_empty, relocate;
    uint8_t has_min_length, has_max_family;
    int32_t collapsed_id;
    uint32_t keep_all, restrict_all;  /* the bits of the patterns in use; 0: option off  */
    uint32_t exclude;                 /* 0 / 1                                           */
    uint64_t min_length, max_family_members;
} asgart_slice_options;
typedef struct asgart_slice_tables {
    int64_t n_names;
    const int32_t *new_id;
    const uint64_t *addend;
    const uint32_t *keep_mask, *restrict_mask;
    const uint8_t *exclude;
    const int64_t *final_pos;
    int64_t table_len[6];
} asgart_slice_tables;
int32_t asgart_slice_families(int32_t device, const uint64_t *fam_offsets, int64_t n_families, const asgart_proto_sd *sds,
                              const uint8_t *flags, const int32_t *chr, const uint64_t *chr_pos, int64_t n_sd,
                              const asgart_slice_tables *tables, const asgart_slice_options *options, asgart_slice **out);
void asgart_slice_counts(const asgart_slice *r, uint64_t *n_families, uint64_t *n_sds);
void asgart_slice_copy(const asgart_slice *r, uint64_t *fam_offsets, asgart_proto_sd *sds, int32_t *chr, uint64_t *chr_pos,
                       uint8_t *flags, int64_t *keys);
/* Milliseconds of the call behind r: [0] the whole call, [1] its kernels (HIP events), [2] of those the compaction. */
int32_t asgart_slice_timings(const asgart_slice *r, double *ms3);
void asgart_slice_free(asgart_slice *r);

/* ---- the filters of asgart-plot on a result held as arrays --------------------------------------------------
 * Replaces the per-duplication work of reference src/bin/asgart-plot.rs:463-481: the retains of --min-length (:463-465:
 * max(left_length, right_length) >= min_length; slice's asks the shorter arm) and of --min-identity / --max-identity
 * (:467-469: f32 compares, a NaN fails), then filter_families_in_features (:20-70), filter_duplicons_in_features (:72-119)
 * and filter_features_in_sds (:121-163), which the reference answers by testing every duplication against every position
 * of every feature of every track.  Here each is an interval join: two radix sorts and two bisections per arm for the
 * intervals in which nothing wraps mod 2^64, the literal `_overlap` (:25-30) on the wrapped values for the rest.
 * Names never reach the device.  The feature tracks come flattened in the order track, feature, position: per position
 * pos_start (GLOBAL: `chr.position + start` of a Relative position against the map as the fragment filters left it, by
 * the first fragment of that name), pos_length and pos_resolved (0: the map has no such fragment; start is ignored), and
 * feat_offsets[n_features + 1], the CSR offsets of the features over the positions.  A window is
 * (start - threshold, length + 2 * threshold), every operation wrapping as in the reference's release build.
 * With U the first unresolved position:
 *   filter_families   a family stays iff one of its duplications overlaps a window; with a U only positions before it are
 *                     windows, and a non-empty family whose FIRST duplication overlaps none is the reference's panic
 *   filter_duplicons  the same per duplication; families stay even when empty
 *   filter_features   feature_keep[f] = 1 iff one of its positions overlaps an arm of a surviving duplication; an unresolved
 *                     position with no overlapping position of its feature before it is the reference's panic
 * The panic is ASGART_E_ARG with *err_position = the flat ordinal of the position to name (otherwise -1).
 * Families emptied by the length and identity steps stay; filter_families drops the families it refuses.
 * out (asgart_plot_counts / _copy / _free): the surviving family offsets, keys[q] = the input ordinal of survivor q in input
 * order (the caller gathers everything else by it) and one keep byte per feature (all 1 without filter_features).
 * force_literal sends every pair of every join through the literal kernel (a debug path: the results are the same).
 * Checked on the host before anything is launched (ASGART_E_ARG): fam_offsets / feat_offsets not starting at 0, decreasing
 * or not ending at n_sd / n_positions. */
typedef struct asgart_plot asgart_plot;
typedef struct asgart_plot_options {
    uint8_t has_min_length, has_identity;
    uint8_t filter_families, filter_duplicons, filter_features;   /* which of the three joins run  */
    uint8_t force_literal;
    float min_identity, max_identity;
    uint64_t min_length;
    uint64_t families_threshold, duplicons_threshold, features_threshold;
} asgart_plot_options;
int32_t asgart_plot_filter(int32_t device, const uint64_t *fam_offsets, int64_t n_families, const asgart_proto_sd *sds,
                           const float *identity, int64_t n_sd, const uint64_t *feat_offsets, int64_t n_features,
                           const uint64_t *pos_start, const uint64_t *pos_length, const uint8_t *pos_resolved,
                           int64_t n_positions, const asgart_plot_options *options, int64_t *err_position,
                           asgart_plot **out);
void asgart_plot_counts(const asgart_plot *r, uint64_t *n_families, uint64_t *n_sds, uint64_t *n_features);
void asgart_plot_copy(const asgart_plot *r, uint64_t *fam_offsets, int64_t *keys, uint8_t *feature_keep);
/* Milliseconds of the call behind r: [0] the whole call, [1] from its first kernel to its last (HIP events; the small
 * read-backs between the stages included), [2] of those the interval joins. */
int32_t asgart_plot_timings(const asgart_plot *r, double *ms3);
void asgart_plot_free(asgart_plot *r);
/* Sizes the joins work in, for tests that place their counts on the seams: threads per workgroup, targets per LDS tile
 * of the literal kernel. */
void asgart_plot_geometry(uint64_t *block_threads, uint64_t *tile_windows);

/* ---- the duplicon clusters of the rosary plot ---------------------------------------------------------------
 * Replaces RosaryPlotter::duplicons_for_chr, reference src/plot/rosary_plot.rs:123-192, for every fragment name in one
 * call.  The reference, per fragment of the map, walks every duplication, compares names as strings, sorts the fragment's
 * arms by start (stable) and folds them one by one: an arm joins the last cluster when
 * `new.start <= last.start + last.length + margin` (:164) and then `last.length = new.start + new.length - last.start`
 * (:165), so that `last.start + last.length` is always the end of the arm just handled.  Here: one stable radix sort of the
 * arms by (name id, start), head[i] = i == 0 || name[i] != name[i-1] || start[i] > end[i-1] + margin (u64, every +
 * wrapping as in the reference's release build), one scan, one segmented reduction.
 * in: the arms in flatten order, arm 2q + side of duplication q (left 0, right 1): arm_name (ids into a table of n_names
 * names; names never reach the device), arm_start (the position within the fragment), arm_length; flags[q] bit 0 reversed,
 * bit 1 complemented (NULL: all 0).  Ties of (name, start) keep flatten order: the first arm of a cluster decides its colour.
 * out (asgart_rosary_counts / _copy / _free): name_offsets[n_names + 1], the CSR rows of the clusters per name id (a name
 * without arms has an empty row), and per cluster, in sorted order: start = its first member's, length = the end of its
 * LAST member - start (wrapping; not the largest end: a contained short arm shortens its cluster), klass = bit 0 reversed
 * and bit 1 complemented of the first member, bit 2 `both`: some member's two bits differ from the first's (:178), and
 * members = the number of arms.  Every copy target is nullable.
 * Checked on the host before anything is launched: NULL arrays with n_sds > 0, a negative count, or a name id outside
 * [0, n_names) (the message names the first such arm): ASGART_E_ARG; 2 * n_sds >= 2^32: ASGART_E_CAP; no usable device:
 * ASGART_E_HIP.  n_sds == 0 succeeds with n_names + 1 zero offsets.  No device memory is held once the call has returned. */
typedef struct asgart_rosary asgart_rosary;
int32_t asgart_rosary_clusters(int32_t device, const int32_t *arm_name, const uint64_t *arm_start,
                               const uint64_t *arm_length, const uint8_t *flags, int64_t n_sds, int64_t n_names,
                               uint64_t margin, asgart_rosary **out);
void asgart_rosary_counts(const asgart_rosary *r, uint64_t *n_names, uint64_t *n_clusters);
void asgart_rosary_copy(const asgart_rosary *r, uint64_t *name_offsets, uint64_t *start, uint64_t *length, uint8_t *klass,
                        uint32_t *members);
/* Milliseconds of the call behind r (rosary_plot.rs:123-192 on the device): [0] the upload, [1] the kernels from the first
 * to the last, [2] the copy back; HIP events for the first two.  ASGART_E_ARG for a NULL argument. */
int32_t asgart_rosary_timings(const asgart_rosary *r, double *ms3);
void asgart_rosary_free(asgart_rosary *r);
/* Threads per workgroup of the kernels behind asgart_rosary_clusters (rosary_plot.rs:123-192), for tests that place their
 * arm counts on the seams. */
void asgart_rosary_geometry(uint64_t *block_threads);

/* ---- paralogy groups: loci, copies ----------------------------------------------------------------------------
 * From pairs to the genome: the arms merged into disjoint LOCI, the loci linked by the duplications into GROUPS (the
 * connected components), copy numbers and non-redundant bases.  Nothing of the reference does this: its families are the
 * runs of the seed automaton, and the rosary clusters above end where their LAST member ends and never link two arms.
 * in: the arms in flatten order, arm 2q + side of duplication q (left 0, right 1): arm_name (ids into a table of n_names
 * names; names never reach the device), arm_start (the position within the fragment), arm_length; one parameter, margin.
 * Loci.  end = start + length.  Two arms of one name id are neighbours iff start_a < sat(end_b + margin) and
 * start_b < sat(end_a + margin), sat(x + margin) = min(x + margin, 2^64 - 1).  The loci are the connected components of
 * that relation, which is the fold over the arms sorted by (name id, start): an arm opens a locus iff it is the first of
 * its name or start >= sat(M + margin), M the LARGEST end of all earlier arms of that name -- the running maximum, not the
 * neighbour's end as in asgart_rosary_clusters.  Lengths are positive, so the partition does not depend on how ties of
 * (name, start) are ordered.  A locus has its name, start = the smallest start of its members, length = the largest end
 * - start, members = its number of arms.  Loci are numbered in (name id, start) order; name_offsets[n_names + 1] are their
 * CSR rows per name id (a name without arms has an empty row).
 * Groups.  Duplication q is an edge between the locus of arm 2q and the locus of arm 2q + 1; self-edges (both arms in one
 * locus) and parallel edges are legal.  The groups are the connected components of the loci under these edges, numbered
 * densely in the order of their SMALLEST locus index, so every output is a function of the input alone.  Per group: loci
 * (the copies), duplications, bases = the sum of its loci's lengths (mod 2^64; loci are disjoint: non-redundant).
 * Per locus also locus_group.  Per duplication: group[q] = the group of its left locus; order[n_sds] = the input ordinals
 * of the duplications, stable by group, with group_offsets[n_groups + 1]: the offsets and gather keys of a result whose
 * families are the groups.  Per arm: arm_locus[2 n_sds].
 * Checked on the host before anything is launched (ASGART_E_ARG, the message names the first offending arm): NULL arrays
 * with n_sds > 0, a negative count, a name id outside [0, n_names), an arm of length 0, start + length wrapping past
 * 2^64.  2 * n_sds >= 2^32: ASGART_E_CAP; no usable device: ASGART_E_HIP.  n_sds == 0 succeeds with n_names + 1 zero
 * offsets and no groups.  No device memory is held once the call has returned.  Every copy target is nullable. */
typedef struct asgart_groups asgart_groups;
int32_t asgart_duplication_groups(int32_t device, const int32_t *arm_name, const uint64_t *arm_start,
                                  const uint64_t *arm_length, int64_t n_sds, int64_t n_names, uint64_t margin,
                                  asgart_groups **out);
void asgart_groups_counts(const asgart_groups *r, uint64_t *n_names, uint64_t *n_loci, uint64_t *n_groups);
void asgart_groups_copy(const asgart_groups *r, uint64_t *name_offsets, int32_t *locus_name, uint64_t *locus_start,
                        uint64_t *locus_length, uint32_t *locus_members, uint32_t *locus_group, uint32_t *group_loci,
                        uint32_t *group_duplications, uint64_t *group_bases, uint32_t *group, uint32_t *order,
                        uint64_t *group_offsets, uint32_t *arm_locus);
/* Milliseconds of the call behind r: [0] the upload, [1] the kernels from the first to the last, [2] the copy back; HIP
 * events for the first two.  ASGART_E_ARG for a NULL argument. */
int32_t asgart_groups_timings(const asgart_groups *r, double *ms3);
void asgart_groups_free(asgart_groups *r);
/* Threads per workgroup of the kernels behind asgart_duplication_groups, for tests that place their counts on the seams. */
void asgart_groups_geometry(uint64_t *block_threads);

/* ---- chaining: collinear duplications joined into pairs -----------------------------------------------------------
 * The seed automaton closes an arm at the first stretch of max_gap_size bases without a hit, so one duplication with an
 * insertion, a diverged stretch or an interspersed repeat comes out as several that lie one behind the other on both
 * arms.  This call joins them.  Nothing of the reference does this; asgart_duplication_groups above joins arms into loci
 * and never makes a PAIR longer.
 * in: the anchors.  Duplication q has the name ids cl = chr[2q], cr = chr[2q + 1] (into a table of n_names names), the
 * positions within them pl = chr_pos[2q], pr = chr_pos[2q + 1], the lengths ll = length[2q], rl = length[2q + 1], each at
 * least 1, and a flag byte fl = flags[q] in 0 .. 3.  Both arms are stored on the forward strand, and bit 0 of the flag
 * (reversed) decides the geometry: the frame of asgart_alignment_variants.  el = pl + ll, er = pr + rl.
 * Two parameters: max_gap (u64, below 2^62; the tools default to 10 000, which is a choice, not a measurement) and
 * lookback H in 1 .. 1024 (the tools default to 64).
 * Groups and order.  Anchors of one (cl, cr, fl) form a group; inside it they are ordered by (pl, pr, q), and the rank is
 * the position in that order.
 * A link j -> i.  Both in one group, rank_i - H <= rank_j < rank_i.  It exists iff pl_i > pl_j and el_i > el_j (strict
 * progress on the left); on the right, for fl & 1 == 0, pr_i > pr_j and er_i > er_j with dr = pr_i - er_j, and for
 * fl & 1 == 1, pr_i < pr_j and er_i < er_j with dr = pr_j - er_i; and, with dl = pl_i - el_j (dl and dr signed, a
 * negative value is an overlap), gl = max(dl, 0) <= max_gap and gr = max(dr, 0) <= max_gap.  Its value is
 * t(j, i) = min(ll_i - max(-dl, 0), rl_i - max(-dr, 0)) - max(gl, gr): the new bases of i on its shorter side minus the
 * longer gap.
 * Scores (int64).  base(i) = min(ll_i, rl_i); f(i) = max(base(i), max_j f(j) + t(j, i)); pred(i) is the j of the maximum
 * if that is STRICTLY above base(i), ties among j to the LARGEST rank (the nearest anchor); otherwise -1.
 * Disjoint chains.  g(i) = max(f(i), max g(i') over pred(i') = i), the best score reachable through i; succ(j) is the
 * child with the largest g, ties to the SMALLEST rank; the link of i is kept iff succ(pred(i)) = i, then
 * link(i) = pred(i), otherwise -1.  The chains are the maximal paths of kept links, and a chain's score is base(head) plus
 * t(link(i), i) of every other member.  (g and not f: the best path of a tree stays whole.)
 * Numbering.  Chains are numbered densely in the order of their smallest member ordinal q.  order[n_sds] and
 * chain_offsets[n_chains + 1] are the members chain by chain, in rank order: by the progress rule the head holds the
 * smallest pl and the tail the largest el; on the right the head holds the smallest pr and the tail the largest er when
 * direct, the other way round when reversed.  f, pred, link and chain are indexed by q, and pred and link hold ordinals.
 * Example 1 (direct, max_gap 10 000, one group): A = (pl 100, pr 5 000, ll 400, rl 400), B = (800, 5 650, 300, 320),
 * C = (1 050, 5 900, 200, 200).  A -> B: dl = 800 - 500 = 300, dr = 5 650 - 5 400 = 250, t = min(300, 320) - 300 = 0, so
 * f(A) + t = 400 > base(B) = 300: f(B) = 400, pred(B) = A.  B -> C: dl = 1 050 - 1 100 = -50, dr = 5 900 - 5 970 = -70,
 * t = min(200 - 50, 200 - 70) - 0 = 130, f(B) + t = 530; A -> C: dl = 550, dr = 500, t = 200 - 550 = -350, which gives 50.  f(C) = 530,
 * pred(C) = B.  One chain A, B, C of score 400 + 0 + 130 = 530: left [100, 1 250), right [5 000, 6 100).
 * Example 2 (a branch, direct, max_gap 10 000): J = (0, 0, 100, 100), I = (100, 100, 10, 10), I' = (100, 130, 50, 50),
 * T = (200, 120, 1 000, 1 000), in rank order.  J -> I: dl = dr = 0, t = 10, f(I) = 110.  J -> I': dl = 0, dr = 30,
 * t = 50 - 30 = 20, f(I') = 120; I -> I' is no link (pl does not grow).  I -> T: dl = 90, dr = 10, t = 1 000 - 90 = 910,
 * f(T) = 1 020; J -> T gives 100 + 900, and I' -> T is no link (pr does not grow).  pred(I) = pred(I') = J, pred(T) = I.
 * g(T) = g(I) = 1 020, g(I') = 120: succ(J) = I although f(I') > f(I), so the chains are J, I, T of score
 * 100 + 10 + 910 = 1 020 = f(T), and I' alone, with link(I') = -1 and the score base(I') = 50.
 * The library cuts the ranks of a group into segments: rank i opens one iff it is the first of its group or
 * pl_i > sat(M + max_gap), M the largest el of the earlier ranks of its group (the running maximum of
 * asgart_duplication_groups, STRICTLY beyond it, as gl <= max_gap admits a gap of exactly max_gap).  No link crosses such
 * a boundary, so no output depends on the cut; n_segments counts the pieces.
 * Checked on the host before anything is launched, the message naming the first offending duplication (ASGART_E_ARG
 * unless said otherwise): NULL arrays with n_sds > 0, a negative count, lookback outside 1 .. 1024, max_gap >= 2^62,
 * n_sds >= 2^31 (ASGART_E_CAP); then per duplication, left arm before right: a name id outside [0, n_names), a length of
 * 0, position + length wrapping past 2^64, an arm of 2^32 bases or more (ASGART_E_CAP: f stays below 2^63), and a flag
 * byte above 3.  No usable device: ASGART_E_HIP.  n_sds == 0 succeeds with no chains.  No device memory is held once the
 * call has returned.  Every copy target is nullable. */
typedef struct asgart_chains asgart_chains;
int32_t asgart_chain_duplications(int32_t device, const int32_t *chr, const uint64_t *chr_pos, const uint64_t *length,
                                  const uint8_t *flags, int64_t n_sds, int64_t n_names, uint64_t max_gap, int32_t lookback,
                                  asgart_chains **out);
/* n_links: the kept links, n_sds - n_chains. */
void asgart_chains_counts(const asgart_chains *r, uint64_t *n_sds, uint64_t *n_chains, uint64_t *n_links,
                          uint64_t *n_segments);
void asgart_chains_copy(const asgart_chains *r, int64_t *f, int32_t *pred, int32_t *link, uint32_t *chain, uint32_t *order,
                        uint64_t *chain_offsets, int64_t *chain_score);
/* Milliseconds of the call behind r: [0] the upload, [1] the kernels from the first to the last, [2] the copy back; HIP
 * events for the first two.  ASGART_E_ARG for a NULL argument. */
int32_t asgart_chains_timings(const asgart_chains *r, double *ms3);
void asgart_chains_free(asgart_chains *r);
/* Threads per workgroup of the elementwise kernels behind asgart_chain_duplications, the lanes of one window round of its
 * segment walk (a lookback above them takes a second round, and the ring in place of the registers), and the largest
 * lookback, for tests that place their counts on the seams. */
void asgart_chain_geometry(uint64_t *block_threads, uint64_t *window_lanes, uint64_t *max_lookback);

/* ---- result files written on the GPU ------------------------------------------------------------------------
 * Replace the per-duplication work of the three exporters of reference src/exporters.rs for a result held as arrays: one
 * call gives the whole file, byte for byte what the exporter writes, in one device buffer.
 *   ASGART_EXPORT_JSON   JSONExporter::save (:12-25): serde_json::to_string_pretty of RunResult.families -- 2-space indent,
 *                        the SD fields in struct order (src/structs.rs:472-493), left_seq / right_seq `null`, identity as
 *                        serde_json prints an f32 (ryu: ASGART_F32_JSON below)
 *   ASGART_EXPORT_GFF2   GFF2Exporter::save (:27-67): two lines per duplication (:38-60), coordinates as stored, the score
 *                        `sd.identity * 100.0` (:44, one rounded f32 product, printed with `{}`: ASGART_F32_DISPLAY), an empty
 *                        line behind every family (:62)
 *   ASGART_EXPORT_GFF3   GFF3Exporter::save (:69-113): two lines per duplication (:86-106), 1 added to every start and end,
 *                        the score `sd.identity` with `{}`, an empty line behind every family (:108)
 * in: fam_offsets[n_families + 1], sds[n_sd], flags[n_sd] (bit 0 reversed, bit 1 complemented), identity[n_sd] or NULL
 * (every identity 0: `0.0` in JSON, `0` in GFF), chr[2 n_sd] (left, right) ids into the name table, chr_pos[2 n_sd].
 * The name table is the host's: name_bytes holds every name as the format prints it -- for JSON the quoted and escaped
 * string (serde_json's escaping), for GFF `str::replace(name.trim(), " ", "_")` (:41, :52, :89, :100) -- and name_offsets[n_names + 1]
 * where each starts.  prefix and suffix are opaque: for JSON everything up to and including `"families": ` and the closing
 * `\n}`, for GFF the track line (:30-35) or the `##gff-version` / `##sequence-region` lines (:72-82) and nothing.
 * Sums (start + length, + 1) wrap as u64.  A name of any length is legal.
 * out: asgart_export_size bytes on `device`; asgart_export_copy moves them into a caller buffer of at least that capacity.
 * The handle owns the device buffer until asgart_export_free; nothing else stays on the device.
 * Checked on the host before anything is launched (ASGART_E_ARG): an unknown format, fam_offsets or name_offsets not
 * starting at 0, decreasing or (fam_offsets) not ending at n_sd, a name id outside the table; n_sd + n_families >= 2^31 - 1:
 * ASGART_E_CAP; no usable device: ASGART_E_HIP. */
#define ASGART_EXPORT_JSON 0
#define ASGART_EXPORT_GFF2 1
#define ASGART_EXPORT_GFF3 2
typedef struct asgart_export asgart_export;
int32_t asgart_export_records(int32_t device, int32_t format, const uint64_t *fam_offsets, int64_t n_families,
                              const asgart_proto_sd *sds, const uint8_t *flags, const float *identity, const int32_t *chr,
                              const uint64_t *chr_pos, int64_t n_sd, const uint8_t *name_bytes, const uint64_t *name_offsets,
                              int64_t n_names, const uint8_t *prefix, uint64_t prefix_len, const uint8_t *suffix,
                              uint64_t suffix_len, asgart_export **out);
/* Bytes of the file behind e (exporters.rs: what `out.write_all` / `writeln!` have written when save returns). */
uint64_t asgart_export_size(const asgart_export *e);
/* The file into dst[capacity], capacity >= asgart_export_size(e): what exporters.rs:14, :29 and :71 hand to `out`; the
 * writer behind `out` stays the caller's. */
int32_t asgart_export_copy(asgart_export *e, uint8_t *dst, uint64_t capacity);
/* Milliseconds of the call behind e (exporters.rs:12-113 on the device): [0] the upload of the arrays, [1] the kernels
 * (lengths, scan, write; HIP events for both), [2] the last asgart_export_copy (host clock; 0 before one). */
int32_t asgart_export_timings(const asgart_export *e, double *ms3);
/* Gives the device buffer back (the file exporters.rs:12-113 wrote is the caller's copy from then on); NULL is allowed. */
void asgart_export_free(asgart_export *e);
/* Sizes the write stage of asgart_export_records works in (the loops of exporters.rs:36-63 and :84-109 cut into
 * workgroups), for tests that place their counts on the seams: threads per workgroup, units per workgroup (a unit is a
 * record or the framing between two families: n_sd + n_families + 1 in all), bytes of the LDS image of a workgroup's range;
 * a range larger than that is stored without the image. */
void asgart_export_geometry(uint64_t *block_threads, uint64_t *records_per_block, uint64_t *stage_bytes);

/* ---- PAF files written on the GPU -----------------------------------------------------------------------------
 * The alignments of asgart_align_duplications (inclusive = 0) as a PAF file: one call gives the whole file in one device
 * buffer, an asgart_export like the result files above (asgart_export_size, _copy, _timings and _free work on it).  No
 * counterpart in the reference.  For every duplication q with status[q] != 0, in order, one line of fifteen columns separated
 * by tabs and ended by `\n`; query = left arm, target = right arm:
 *    1  the name chr[2q]          2  name_length of it     3  chr_pos[2q]        4  column 3 + left_length
 *    5  `+` for flags[q] == 0, `-` for flags[q] == 3
 *    6  the name chr[2q + 1]      7  name_length of it     8  chr_pos[2q + 1]    9  column 8 + right_length
 *   10  the sum of the row's `=` run lengths    11  the sum of all its run lengths    12  `255`
 *   13  `NM:i:<distance[q]>`    14  `fm:i:<f>`, fam_offsets[f] <= q < fam_offsets[f + 1]    15  `cg:Z:<CIGAR>`
 * The CIGAR is `<run_len><run_op>` for the runs run_offsets[q] .. run_offsets[q + 1]; on a `-` row the runs are written in
 * reverse order, the operations unchanged (PAF's CIGAR runs along the target's forward strand).  A row without runs ends in
 * `cg:Z:`.  status[q] == 0 (a refused alignment): no row, whatever else is given for q.  The name table is the host's: the
 * bytes of every name as they are to be written (name_bytes, name_offsets[n_names + 1]) and the length of the fragment it
 * names (name_length[n_names]); a name of any length is legal.  The run count is run_offsets[n_sd]; columns 10 and 11 are
 * u64 sums.
 * Checked on the host before anything is launched or read further: NULL arrays with a positive count, fam_offsets /
 * run_offsets / name_offsets not starting at 0, decreasing or (fam_offsets) not ending at n_sd, a name id outside the table,
 * a flag other than 0 or 3 on a duplication with a row (the message names the first), a position + length that wraps past
 * 2^64 on one: ASGART_E_ARG; 2^31 duplications or 2^32 runs and more: ASGART_E_CAP; no usable device: ASGART_E_HIP.
 * n_sd == 0, or every status 0, succeeds with an empty file.  The handle owns the file until asgart_export_free; nothing
 * else stays on the device. */
int32_t asgart_paf_records(int32_t device, const uint64_t *fam_offsets, int64_t n_families, const asgart_proto_sd *sds,
                           const uint8_t *flags, const uint8_t *status, const uint32_t *distance, const int32_t *chr,
                           const uint64_t *chr_pos, int64_t n_sd, const uint64_t *run_offsets, const uint32_t *run_len,
                           const uint8_t *run_op, const uint8_t *name_bytes, const uint64_t *name_offsets,
                           const uint64_t *name_length, int64_t n_names, asgart_export **out);
/* Sizes the write stage of asgart_paf_records works in, for tests that place their counts on the seams: threads per
 * workgroup, the most runs one workgroup's range can hold (a run is two bytes at least), bytes of the file a workgroup owns
 * (its LDS image; workgroup i writes the bytes [i * stage_bytes, (i + 1) * stage_bytes) of the file). */
void asgart_paf_geometry(uint64_t *block_threads, uint64_t *runs_per_block, uint64_t *stage_bytes);
/* The same file with minimap2's difference string: a row of asgart_paf_records, byte for byte, with one more column before
 * the `\n`, `\tcs:Z:<CS>`: not only where the two arms differ, as the CIGAR says, but how.  The device and the text are the
 * index's; cs_mode 1 is the short form, 2 the long one.  Every other argument is asgart_paf_records', and so is the result.
 * CS is the concatenation of the texts of the row's runs, in the order of the CIGAR: as given for a `+` row, reversed for a
 * `-` row.  Run t of duplication q = (left, right, left_length ll, right_length rl), n = run_len[t] bases long, starts at the
 * arm offsets
 *    i_t = the sum of run_len over the row's runs BEFORE t (in the order given) with run_op `=`, `X` or `I`,
 *    j_t = the same sum for `=`, `X` or `D`,
 * and stands for the base positions v = 0 .. n-1 with
 *    row              query byte Q(v)                          target byte T(v)
 *    `+` (flag 0)     text[left + i_t + v]                     text[right + j_t + v]
 *    `-` (flag 3)     comp(text[left + i_t + n - 1 - v])       text[right + rl - j_t - n + v]
 * comp swaps ACGT and acgt and keeps every other byte (the complement of asgart_compute_scores); low maps `A`..`Z` to
 * `a`..`z` and keeps every other byte.  On a `-` row the string runs along the target's forward strand and the query is shown
 * reverse-complemented, as minimap2 does.  The text of a run:
 *    `=`   short: `:` and the decimal n.  Long: `=` and T(0 .. n-1) as stored
 *    `X`   for each v: `*`, low(T(v)), low(Q(v))
 *    `I`   `+` and low(Q(0 .. n-1))        (a left-arm base without a partner)
 *    `D`   `-` and low(T(0 .. n-1))
 * The writer prints what the runs say and compares no bases: an `X` over equal bytes prints two equal letters.  Example: the
 * text `ACGTTAGC` `GG` `ACCTAGCA`, the duplication (0, 10, 8, 8), flag 0, runs `2=1I1X4=1D`: `:2+g*ct:4-a`, long
 * `=AC+g*ct=TAGC-a`; with `TGCTAGGT` as the right arm and flag 3 the row's CIGAR is `1D4=1X1I2=` and its cs `-t:4*ga+c:2`,
 * long `-t=GCTA*ga+c=GT`.
 * Checked beyond the checks of asgart_paf_records, for the duplications with a row only (ASGART_E_ARG, the message names
 * the first such duplication): cs_mode other than 1 or 2 and idx NULL (before anything else); an arm that reaches past the
 * text; and, on the device, behind the layout and before a byte is written, a run_op outside `=XID`, a run_len of 0, runs
 * that do not consume exactly left_length and right_length bases.  A refused call leaves nothing on the device. */
int32_t asgart_paf_records_cs(asgart_index *idx, int32_t cs_mode, const uint64_t *fam_offsets, int64_t n_families,
                              const asgart_proto_sd *sds, const uint8_t *flags, const uint8_t *status,
                              const uint32_t *distance, const int32_t *chr, const uint64_t *chr_pos, int64_t n_sd,
                              const uint64_t *run_offsets, const uint32_t *run_len, const uint8_t *run_op,
                              const uint8_t *name_bytes, const uint64_t *name_offsets, const uint64_t *name_length,
                              int64_t n_names, asgart_export **out);
/* asgart_paf_geometry's three sizes, which hold for asgart_paf_records_cs too, and solo_bytes: the most bytes of one run's
 * cs text inside a workgroup's range that one thread composes alone; a run with more is composed by the whole workgroup. */
void asgart_paf_cs_geometry(uint64_t *block_threads, uint64_t *runs_per_block, uint64_t *stage_bytes, uint64_t *solo_bytes);

/* ---- the counts of an alignment ---------------------------------------------------------------------------------
 * What every catalogue of segmental duplications states per duplication (WGAC's genomicSuperDups, SEDEF, BISER), counted on
 * the GPU from the runs of asgart_align_duplications (inclusive = 0, as asgart_alignment_copy gives them) and the text of
 * the index.  No counterpart in the reference.  The frame is the alignment's, not the PAF row's: A is the left arm as
 * stored; B(j), j in [0, rl), is the right arm as asgart_align_duplications walks it, text[right + (flags[q] & 1 ?
 * rl - 1 - j : j)], complemented (ACGT and acgt swap, every other byte is kept) when bit 1 is set.  All four flag values
 * are legal.  Run t of duplication q starts at the arm offsets i_t and j_t of the cs:Z: section above (the sums of the
 * row's earlier `=XI` and `=XD` run lengths, in the order given); base v of it pairs a = text[left + i_t + v] with
 * b = B(j_t + v).  Per duplication with status[q] == 1:
 *    match, mismatch          the sums of the `=` and of the `X` run lengths
 *    ins_runs, ins_bases      the number and the sum of the `I` runs (left-arm bases without a partner)
 *    del_runs, del_bases      the same for `D`
 *    longest_match            the largest `=` run;   longest_gap   the largest `I` or `D` run
 *    transition, transversion over every base of every `X` run, A-Z folded to a-z: a transition where a != b and both are
 *                             in {a, g} or both in {c, t}; a transversion where one is in {a, g} and the other in {c, t};
 *                             neither otherwise (an N, any other byte, an `X` laid over equal bytes)
 * The first eight look at no base, and no `=` base is inspected: like the writers, the call believes the runs.  A
 * duplication with status[q] != 1 gets ten zeros; its runs, its arms and its flag are neither read nor checked.
 * Example: the text `ACGTTAGC` `GG` `ACCTAGCA`, the duplication (0, 10, 8, 8), flag 0, runs `2=1I1X4=1D`: the `X` pairs
 * a = text[3] = T with b = text[12] = C, a transition; the counts are 6, 1, 1, 0, 1, 1, 1, 1, 4, 1.
 * Checked, for the duplications with status 1 only and with the codes of asgart_paf_records_cs (ASGART_E_ARG, the message
 * names the first such duplication): idx NULL (before anything else); NULL arrays with a positive count, run_offsets not
 * from 0, decreasing; a flag byte above 3; an arm that reaches past the text; and, on the device, before a base is read,
 * a run_op outside `=XID`, a run_len of 0, runs that do not consume exactly left_length and right_length bases.  2^31
 * duplications, 2^32 runs, arms of 2^32 bases and more: ASGART_E_CAP.  counts[n_sd] is written only by a call that returns 0;
 * a refused call leaves nothing on the device.  ms3 (nullable): the milliseconds of upload, kernels and copy back. */
typedef struct asgart_align_counts {
    uint64_t match, mismatch;
    uint64_t transition, transversion;
    uint64_t ins_runs, ins_bases;
    uint64_t del_runs, del_bases;
    uint64_t longest_match, longest_gap;
} asgart_align_counts;
int32_t asgart_alignment_stats(asgart_index *idx, const asgart_proto_sd *sds, const uint8_t *flags, const uint8_t *status,
                               int64_t n_sd, const uint64_t *run_offsets, const uint32_t *run_len, const uint8_t *run_op,
                               asgart_align_counts *counts, double *ms3);
/* Sizes the kernels of asgart_alignment_stats work in, for tests that place their counts on the seams: threads per
 * workgroup, and the mismatch bases one workgroup of the bases kernel takes (a wave takes a quarter of them, 64 at a time). */
void asgart_alignment_stats_geometry(uint64_t *block_threads, uint64_t *bases_per_block);

/* ---- the duplication table written on the GPU ---------------------------------------------------------------------
 * The counts above as the table the field reads duplications by: one call gives the whole file in one device buffer, an
 * asgart_export (asgart_export_size, _copy, _timings and _free work on it).  The file is `prefix` (the caller's header
 * line: `#` and the 25 column names, tab-separated, `\n`) and, for every duplication q with status[q] != 0, in order, one
 * line of 25 columns separated by tabs and ended by `\n`.  The first ten are BEDPE, the rest carry the names of UCSC's
 * genomicSuperDups:
 *    1 chrom1   the name chr[2q]         2 start1   chr_pos[2q]        3 end1   column 2 + left_length
 *    4 chrom2   the name chr[2q + 1]     5 start2   chr_pos[2q + 1]    6 end2   column 5 + right_length
 *    7 name     `sd<q>`     8 score  `0`     9 strand1  `+`     10 strand2  `+` for flags[q] == 0, `-` for flags[q] == 3
 *   11 family   f, fam_offsets[f] <= q < fam_offsets[f + 1]
 *   12 alignL   alignB + indelS          13 alignB  match + mismatch   14 matchB   15 mismatchB
 *   16 transitionsB   17 transversionsB  18 indelN  ins_runs + del_runs    19 indelS  ins_bases + del_bases
 *   20 longestMatch   21 longestGap
 *   22 fracMatch      match / alignB                  23 fracMatchIndel   match / (alignB + indelN)
 *   24 jcK            -3/4 ln(1 - 4p/3), p = mismatch / alignB                               (Jukes-Cantor)
 *   25 k2K            -1/2 ln((1 - 2P - Q) sqrt(1 - 2Q)), P, Q = transition, transversion over alignB    (Kimura)
 * Columns 22 to 25 are NOT computed here: they are the caller's four f32 arrays, printed as ASGART_F32_DISPLAY prints an
 * f32 (`NaN` for NaN), so that the file does not depend on whose logarithm ran.  The convention of the Python host
 * (align.divergence): float64 arithmetic rounded once to f32; NaN where alignB is 0 or the argument of the logarithm is
 * not above 0, never an infinity; a zero is +0.  A mismatch that involves an N counts in p and in neither P nor Q.
 * A row worked by hand, the example of the counts above: the text `ACGTTAGC` `GG` `ACCTAGCA` as the fragment `chr1` from
 * 0, the duplication (0, 10, 8, 8), flag 0, family 0, runs `2=1I1X4=1D`, so the counts 6, 1, 1, 0, 1, 1, 1, 1, 4, 1:
 * alignB 7, indelN 2, indelS 2, alignL 9; fracMatch 6/7, fracMatchIndel 6/9; p = 1/7, jcK = -3/4 ln(17/21); P = 1/7,
 * Q = 0, k2K = -1/2 ln(5/7):
 *    chr1 0 8 chr1 10 18 sd0 0 + + 0 9 7 6 1 1 0 2 2 4 1 0.85714287 0.6666667 0.15848182 0.16823612
 * Checked on the host before anything is launched, as asgart_paf_records checks: NULL arrays with a positive count,
 * fam_offsets / name_offsets not starting at 0, decreasing or (fam_offsets) not ending at n_sd, a name id outside the table,
 * a flag other than 0 or 3 on a duplication with a row (the message names the first), a position + length that wraps past
 * 2^64 on one: ASGART_E_ARG; 2^31 duplications and more: ASGART_E_CAP; no usable device: ASGART_E_HIP.  n_sd == 0, or every
 * status 0, succeeds with the header alone.  The handle owns the file until asgart_export_free; nothing else stays on the
 * device. */
int32_t asgart_sdtable_records(int32_t device, const uint64_t *fam_offsets, int64_t n_families, const asgart_proto_sd *sds,
                               const uint8_t *flags, const uint8_t *status, const int32_t *chr, const uint64_t *chr_pos,
                               int64_t n_sd, const uint8_t *name_bytes, const uint64_t *name_offsets, int64_t n_names,
                               const asgart_align_counts *counts, const float *frac_match, const float *frac_match_indel,
                               const float *jc_k, const float *k2_k, const uint8_t *prefix, uint64_t prefix_len,
                               asgart_export **out);
/* Sizes the write stage of asgart_sdtable_records works in, as asgart_export_geometry gives them for its own: threads per
 * workgroup, rows per workgroup, bytes of the LDS image (a workgroup whose rows do not fit it stores them directly). */
void asgart_sdtable_geometry(uint64_t *block_threads, uint64_t *records_per_block, uint64_t *stage_bytes);
/* An array of f32 rendered on the device as the exporters print an identity: the shortest decimal digits that read back
 * as the same f32, in one of two forms.
 *   ASGART_F32_JSON      serde_json's (ryu's pretty printer; `identity` in exporters.rs:12-25): `97.3`, `100.0`, `0.0`,
 *                        `-0.0`, `1e-7`, `3.4028235e38` (an exponent for |v| < 1e-5 and |v| >= 1e13), `null` for NaN and
 *                        the infinities
 *   ASGART_F32_DISPLAY   Rust's `{}` (exporters.rs:44, :55, :92, :103): always positional, `97.3`, `100`, `0`, `-0`, `0.0000001`,
 *                        `NaN`, `inf`, `-inf`
 * out_bytes[n * ASGART_F32_TEXT_MAX]: value i at i * ASGART_F32_TEXT_MAX, out_lens[i] bytes of it. */
#define ASGART_F32_JSON 0
#define ASGART_F32_DISPLAY 1
#define ASGART_F32_TEXT_MAX 64
int32_t asgart_f32_shortest(int32_t device, const float *values, int64_t n, int32_t mode, uint8_t *out_bytes,
                            uint8_t *out_lens);
/* The table of powers of ten behind the digits (serde_json's ryu carries one of the same purpose): for k = *k_min ..
 * *k_max four words per entry -- hi, lo, x (a two's complement int64), exact -- with 10^-k = (hi * 2^64 + lo) * 2^x, exactly
 * where exact != 0 and rounded up otherwise; computed with integer arithmetic when first used.  Needs no device.
 * Returns the number of entries; every argument is nullable. */
int32_t asgart_f32_pow10_table(int32_t *k_min, int32_t *k_max, uint64_t *entries);

/* ---- result files read on the GPU ---------------------------------------------------------------------------
 * Replace, for a result wanted as arrays, RunResult::from_file of reference src/structs.rs:105-112 (serde_json::from_reader;
 * the 13 fields of SD, :471-495): the file's bytes are uploaded once, tokenised and parsed on the device.  The rule is
 * ACCEPT OR REFUSE, NEVER DIFFER: an accepted file gives exactly the arrays the host reader of the Python package gives; every
 * other file is refused with ASGART_E_REFUSED and asgart_last_error names the byte offset and the rule.  No error of the host
 * reader is ever reproduced here: the caller answers a refusal by running that reader.
 * Two calls on one handle, because the name table comes from the head of the file:
 *   asgart_result_scan    uploads bytes[size] (size below 2^32 - 2048) and classifies them: the quotes no odd run of
 *                         backslashes precedes, the in-string mask (their prefix XOR), the nesting depth (a scan over the
 *                         brackets outside strings), the tokens at depth 1 (more than 64: a refusal).  -> the byte span
 *                         [*families_begin, *families_end) of the value of "families".  The caller parses
 *                         bytes[:begin] + "[]" + bytes[end:] itself (strand and settings) and builds the name table.
 *   asgart_result_parse   name_bytes / name_offsets[n_names + 1]: names as UTF-8, SORTED as bytes and unique (the device
 *                         bisects them; ASGART_E_ARG otherwise).  Finds the families and records inside the span and parses
 *                         every record.  Once per scan.
 * The accepted grammar (everything else is a refusal):
 *   whitespace   space, \t, \n, \r between any two tokens: serde's pretty form, its compact form and everything between
 *   top level    one object; its keys hold no backslash and are exactly strand, settings, families, each once, in any
 *                order, each value an array or object; behind the closing brace only whitespace; no byte-order mark
 *   families     an array of arrays of objects; every byte of its span is whitespace, a structural character in its place,
 *                a string, or a number or literal in value position (no missing, doubled or trailing comma, no missing
 *                colon, no unbalanced bracket, no stray byte)
 *   records      keys hold no backslash and are among the 13 field names, each at most once, in any order; the 11 other
 *                than left_seq and right_seq are all present; left_seq and right_seq are absent or null (a string there is
 *                refused with a reason of its own: results with sequences are the host's); no nested array or object
 *   positions and lengths (6)   the literal 0|[1-9][0-9]* of at most 2^64 - 1
 *   reversed, complemented      the literal true or false
 *   identity     -?(0|[1-9][0-9]*)(\.[0-9]+)?([eE][+-]?[0-9]+)?; converted on the device where that is exact (a significand
 *                of at most 2^53 and a decimal exponent within +-22 once the fraction digits are folded in: one IEEE f64
 *                multiply or divide by an exact power of ten, then one cast to f32); every other literal is HARD: flags bit
 *                2 is set and identity_spans holds its bytes for the caller to convert
 *   chr_left, chr_right   a string without a raw byte below 0x20.  Without a backslash and equal to a table entry: that
 *                entry's index.  Any other string is a HARD name: chr is -1 and name_spans holds the bytes between its
 *                quotes for the caller to decode (and to refuse, if they do not decode)
 * out (asgart_result_copy, after a parse that succeeded; sizes from asgart_result_counts): fam_offsets[n_families + 1]
 * (empty families stay), sds[n_sd], flags[n_sd] (bit 0 reversed, bit 1 complemented, bit 2 hard identity), identity[n_sd],
 * chr[2 n_sd] and chr_pos[2 n_sd] (left, right), first_use[n_names] (the smallest 2 * record + side that uses the entry,
 * 0xFFFFFFFF: none -- with it the caller numbers names in order of first appearance), name_spans[2 n_sd][2] and
 * identity_spans[n_sd][2] (start, length; of every name and identity, hard or not).
 * The handle owns the device memory until asgart_result_free; a refused scan leaves no handle and no device memory.
 * No usable device: ASGART_E_HIP. */
#define ASGART_E_REFUSED (-5) /* result reader: the input is outside the accepted grammar (the host reader's to read) */
typedef struct asgart_result_read asgart_result_read;
int32_t asgart_result_scan(int32_t device, const uint8_t *bytes, uint64_t size, asgart_result_read **out,
                           uint64_t *families_begin, uint64_t *families_end);
int32_t asgart_result_parse(asgart_result_read *r, const uint8_t *name_bytes, const uint64_t *name_offsets, int64_t n_names);
/* Families and duplications of the parsed file (src/structs.rs:105-112: RunResult.families), and how many names and
 * identities were left to the caller; every argument is nullable. */
void asgart_result_counts(const asgart_result_read *r, uint64_t *n_families, uint64_t *n_sd, uint64_t *n_hard_names,
                          uint64_t *n_hard_identities);
int32_t asgart_result_copy(asgart_result_read *r, uint64_t *fam_offsets, asgart_proto_sd *sds, uint8_t *flags, float *identity,
                           int32_t *chr, uint64_t *chr_pos, uint32_t *first_use, uint32_t *name_spans,
                           uint32_t *identity_spans);
/* Milliseconds of the calls behind r (src/structs.rs:105-112 on the device): [0] the upload of the file, [1] the scan
 * kernels, [2] the parse kernels (HIP events for the three), [3] the last asgart_result_copy (host clock). */
int32_t asgart_result_timings(const asgart_result_read *r, double *ms4);
/* Gives the device memory back (what src/structs.rs:105-112 read is the caller's copy from then on); NULL is allowed. */
void asgart_result_free(asgart_result_read *r);
/* Sizes the reader behind asgart_result_scan works in (src/structs.rs:105-112 cut into workgroups), for tests that place
 * their bytes on the seams: bytes per tile of the scan, records per workgroup of the record stage, bytes of its LDS stage; a
 * range of records larger than that is walked in global memory. */
void asgart_result_geometry(uint64_t *tile_bytes, uint64_t *records_per_block, uint64_t *stage_bytes);

/* ---- FASTA files read on the GPU ---------------------------------------------------------------------------
 * Replace the FASTA reader in front of prepare_data and prepare_data itself (reference src/bin/asgart.rs:273-430: bio's
 * fasta::Reader and the per-record loop at :278-313, normalisation :289-301, find_chunks_to_process :317-366,
 * concatenation :375-395, '$' :430) and the reader of asgart-extract (src/bin/asgart-extract.rs:17-29, :110-117).
 * files[i] / file_lens[i] are the bytes of FASTA file i as they are on disk (for instance a read-only mapping); they are
 * copied to `device` through pinned pieces and parsed there:
 *   - lines end at '\n'; a '\r' is dropped iff only '\r's lie between it and the next '\n' or the end of the file (so
 *     "\r\n" ends a line, a '\r' with another byte behind it on its line is sequence and normalises to N);
 *   - a line whose first byte is '>' starts a record; '>' elsewhere is sequence; what precedes a file's first header
 *     line is ignored; blank lines add nothing; a last line without '\n' counts; a record may be empty;
 *   - the records of all files in the order given are one strand; N-runs are measured in the record, not in the lines.
 * The result holds, on the device, the raw strand (every record's bytes as they are: what asgart_source holds) and the
 * normalised strand with its '$' (Strand.data); on the host the record table and the chunks.  Names are the host's:
 * record r's header line is file_lens-checked bytes [header_offset, header_offset + header_len) of file `file`, '>'
 * included, line end excluded (a trailing '\r' may be part of it: the id is the first whitespace-separated token).
 * Errors: NULL / no files and no record in any file (ASGART_E_ARG, before the device is looked at), no usable device
 * (ASGART_E_HIP), more than 2^24 records (ASGART_E_CAP, as asgart_prepare_data).  No device memory stays behind. */
typedef struct asgart_fasta asgart_fasta;
typedef struct asgart_fasta_record {
    uint64_t file;           /* index into files[]                                   */
    uint64_t header_offset;  /* of the '>' in that file                              */
    uint64_t header_len;     /* bytes of the header line, without its '\n'           */
    uint64_t start;          /* Start.position: first base in the strand (:375-395)  */
    uint64_t len;            /* Start.length; may be 0                               */
} asgart_fasta_record;
int32_t asgart_fasta_read(const uint8_t *const *files, const uint64_t *file_lens, int64_t n_files, int32_t skip_masked,
                          int32_t device, asgart_fasta **out);
/* *n_text: bytes of the normalised strand, '$' included.  Any of the three may be NULL. */
int32_t asgart_fasta_counts(const asgart_fasta *f, int64_t *n_records, int64_t *n_chunks, uint64_t *n_text);
/* records[n_records], chunks[2 * n_chunks] ((start, len) pairs, record order: what asgart_search_duplications takes),
 * text[n_text]; each nullable.  asgart_fasta_read_text copies bytes [lo, hi) of the normalised strand only. */
int32_t asgart_fasta_copy(const asgart_fasta *f, asgart_fasta_record *records, uint64_t *chunks, uint8_t *text);
int32_t asgart_fasta_read_text(const asgart_fasta *f, uint64_t lo, uint64_t hi, uint8_t *out);
/* An index over the normalised strand (copied device to device), its suffixes sorted on the GPU: what
 * asgart_index_create builds from Strand.data (src/bin/asgart.rs:141-155), without the text visiting the host. */
int32_t asgart_fasta_index(asgart_fasta *f, asgart_index **out);
/* The raw strand as a source for asgart_extract_sequences, without another upload: the source takes the buffer over,
 * so this succeeds once per result (then ASGART_E_ARG); the source outlives asgart_fasta_free. */
int32_t asgart_fasta_source(asgart_fasta *f, asgart_source **out);
void asgart_fasta_free(asgart_fasta *f);
/* Milliseconds of the asgart_fasta_read call behind f: [0] the whole call, [1] host copies into the pinned pieces,
 * [2] host -> device copies and [3] kernels (sums over the pieces, HIP events; [2] and [3] overlap each other and [1]). */
int32_t asgart_fasta_timings(const asgart_fasta *f, double *ms4);
/* Sizes the reader works in, for tests that place line ends on its seams: file bytes per workgroup, file bytes per
 * staging piece, bytes per output store. */
void asgart_fasta_geometry(uint64_t *tile_bytes, uint64_t *piece_bytes, uint64_t *vector_bytes);

/* ---- masking: which bases the arms cover ----------------------------------------------------------------------
 * From a result back to the genome: the bases of the strand that at least min_depth arms hold.  Nothing of the reference
 * does this.  asgart_duplication_groups above folds the arms per NAME and counts no depth; here the arms lie on the strand.
 * in: the arms in flatten order (arm 2q + side of duplication q): arm_record (ids into the record table), arm_start (the
 * position WITHIN the record), arm_length; the record table record_start[n_records], record_len[n_records] in strand
 * coordinates (asgart_fasta_copy's start and len); margin; min_depth >= 1.
 * The rule.  With rs the start of its record, an arm covers the strand bases
 *     [rs + (start > margin ? start - margin : 0),  rs + min(record_len, sat(start + length + margin))),
 * sat saturating at 2^64 - 1: the margin never leaves the arm's own record.  depth(x) is the number of arms whose clipped
 * range holds base x.  The result is the MAXIMAL RUNS of strand bases with depth >= min_depth: (start, end) pairs, sorted,
 * disjoint and non-touching ([0,10) and [10,20) at depth 1 are one run, and nothing at depth 2).  A run may cross a record
 * start when both sides are covered; a caller that needs records splits the runs there.  Also: the number of intervals,
 * masked_bases = the sum of end - start, and max_depth = the largest depth anywhere.
 * Checked on the host before anything is launched (ASGART_E_ARG, the message names the first offender): NULL arrays with a
 * positive count, a negative count, min_depth == 0, records that are not ascending and non-overlapping (or wrap), a record
 * id outside the table, an arm of length 0, arm_start + arm_length > record_len (the arm leaves its record: the result does
 * not belong to these records).  n_arms >= 2^31: ASGART_E_CAP; no usable device: ASGART_E_HIP.  n_arms == 0 succeeds with
 * no intervals.  No device memory is held once the call has returned.  Every copy target is nullable. */
typedef struct asgart_mask asgart_mask;
int32_t asgart_mask_intervals(int32_t device, const int32_t *arm_record, const uint64_t *arm_start,
                              const uint64_t *arm_length, int64_t n_arms, const uint64_t *record_start,
                              const uint64_t *record_len, int64_t n_records, uint64_t margin, uint32_t min_depth,
                              asgart_mask **out);
void asgart_mask_counts(const asgart_mask *r, uint64_t *n_intervals, uint64_t *masked_bases, uint64_t *max_depth);
/* intervals[2 * n_intervals]: start, end of every run. */
void asgart_mask_copy(const asgart_mask *r, uint64_t *intervals);
/* Milliseconds of the call behind r: [0] the upload, [1] the kernels from the first to the last, [2] the copy back; HIP
 * events for the first two.  ASGART_E_ARG for a NULL argument. */
int32_t asgart_mask_timings(const asgart_mask *r, double *ms3);
void asgart_mask_free(asgart_mask *r);
/* Threads per workgroup of the kernels behind asgart_mask_intervals, for tests that place their counts on the seams. */
void asgart_mask_geometry(uint64_t *block_threads);

/* ---- FASTA files written on the GPU ---------------------------------------------------------------------------
 * The strand back as a file, with the bases inside the intervals masked.  src is read, not taken over: the raw strand on
 * its device (asgart_fasta_source or asgart_source_create).  record_start / record_len as for asgart_mask_intervals;
 * header_bytes and header_offsets[n_records + 1] are the header lines (header r is printed verbatim and followed by '\n':
 * the '>' is the caller's, a trailing '\r' should be left out); intervals[2 * n_intervals] are (start, end) pairs of strand
 * bases, ascending and disjoint (what asgart_mask_intervals gives, or any others); width = bases per line, 0 = the whole
 * record on one line; fill = 0 masks softly (a byte 'A'..'Z' inside an interval becomes byte | 0x20, every other byte
 * stays), any other value replaces every byte inside an interval.  Bytes outside the intervals are the source's, so
 * soft-masking that was there survives.
 * The file, record by record: the header, '\n', then the record's bytes in lines of `width` bases, each followed by '\n';
 * the last line may be shorter, an empty record has no sequence line, and there is no blank line when len is a multiple of
 * width.  The body of a record of len bases is len + ceil(len / width) bytes (width 0: len + 1, or 0 when len is 0); base b
 * sits at body offset b + b / width; body offset o is a '\n' iff o mod (width + 1) == width or o is the body's last byte,
 * and otherwise base o - o / (width + 1).  Sizes and offsets are 64-bit throughout.
 * out: an asgart_export; asgart_export_size, _copy, _timings ([0] upload, [1] the write kernel, [2] the last copy) and
 * _free work on it as on the other writers' handles.
 * Checked on the host before anything is launched (ASGART_E_ARG, naming the first offender): NULL or negative arguments, a
 * header that holds '\n', header_offsets not starting at 0 or decreasing, records not ascending, overlapping or past the
 * source's bytes, intervals that are empty, not ascending, overlapping or past the source's bytes, fill above 255 or equal
 * to '\n', '\r' or '>'.  More than 2^24 records or 2^32 intervals: ASGART_E_CAP; no usable device: ASGART_E_HIP. */
int32_t asgart_fasta_write(asgart_source *src, const uint64_t *record_start, const uint64_t *record_len, int64_t n_records,
                           const uint8_t *header_bytes, const uint64_t *header_offsets, const uint64_t *intervals,
                           int64_t n_intervals, uint32_t width, uint32_t fill, asgart_export **out);
/* Sizes the write stage of asgart_fasta_write works in, for tests that place their bytes on the seams: threads per
 * workgroup, bytes of the file per workgroup (a window, and the LDS image of it), bytes per store of the copy out. */
void asgart_fasta_write_geometry(uint64_t *block_threads, uint64_t *window_bytes, uint64_t *store_bytes);

/* ---- the variants between the copies: records, sites, and their two files -----------------------------------------
 * The differences an alignment found, as positions in the genome: the paralogous sequence variants (PSVs) that tell one
 * copy from another.  No counterpart in the reference.  asgart_alignment_variants takes the arguments of
 * asgart_alignment_stats and uses its frame: all four flag values are legal, only duplications with status[q] == 1 are read
 * or checked, run t of duplication q = (left, right, ll, rl) starts at the arm offsets i_t and j_t of the cs:Z: section, and
 * rev = flags[q] & 1.  The rule: one record per base of every `X` run and one per `I` run and per `D` run, in the order of
 * the duplications and, inside one, of the runs and bases.  All coordinates are global, on the forward strand, half-open:
 *    op              left interval            right interval
 *    `X`, base v     [left + i_t + v, +1)     [p, p + 1), p = right + (rev ? rl - 1 - (j_t + v) : j_t + v)
 *    `I`, n bases    [left + i_t, +n)         empty at right + (rev ? rl - j_t : j_t)
 *    `D`, n bases    empty at left + i_t      [right + (rev ? rl - j_t - n : j_t), +n)
 * left_base and right_base are the text's bytes AS STORED at the two positions of an `X` record (not complemented, case
 * kept) and 0 for an indel; flag is flags[q], sd is q.  Like the counts, the call believes the runs: an `X` laid over equal
 * bytes is a record with two equal bases.  var_offsets[n_sd + 1]: the records of duplication q are var_offsets[q] ..
 * var_offsets[q + 1].
 * Example 1: the text `ACGTTAGC` `GG` `ACCTAGCA`, the duplication (0, 10, 8, 8), flag 0, runs `2=1I1X4=1D`: three records,
 *    I  left [2, 3)  right empty at 12;     X  left [3, 4) `T`  right [12, 13) `C`;     D  left empty at 8  right [17, 18).
 * Example 2: `TGCTAGGT` as the right arm and flag 3: the `X` is left 3 (`T`) against right 15 (`G`); the `I` boundary is 16;
 * the `D` is [10, 11).
 * Checks and refusals are those of asgart_alignment_stats, under this call's name: idx NULL (before anything else); NULL
 * arrays with a positive count, run_offsets not from 0, decreasing; a flag byte above 3; an arm that reaches past the text;
 * and, on the device, through one atomic minimum before a base is read, a run_op outside `=XID`, a run_len of 0, runs that
 * do not consume exactly left_length and right_length bases (ASGART_E_ARG, the message names the first such duplication).
 * 2^31 duplications, 2^32 runs, arms of 2^32 bases, 2^31 variants and more: ASGART_E_CAP.  A refused call leaves nothing on
 * the device and no handle.  The handle keeps the records on the device of the index (asgart_variant_sites and
 * asgart_variants_records read them there) until asgart_variants_free. */
typedef struct asgart_variant {      /* 32 bytes */
    uint64_t left_pos, right_pos;
    uint32_t left_len, right_len;    /* 1/1, n/0, 0/n */
    uint32_t sd;                     /* q */
    uint8_t  op, left_base, right_base, flag;
} asgart_variant;
typedef struct asgart_variants asgart_variants;
int32_t asgart_alignment_variants(asgart_index *idx, const asgart_proto_sd *sds, const uint8_t *flags, const uint8_t *status,
                                  int64_t n_sd, const uint64_t *run_offsets, const uint32_t *run_len, const uint8_t *run_op,
                                  asgart_variants **out);
/* n_sd of the call, the number of records, the number of `X` records (SNVs).  Every target is nullable. */
void asgart_variants_counts(const asgart_variants *r, uint64_t *n_sd, uint64_t *n_variants, uint64_t *n_snv);
/* records[n_variants], var_offsets[n_sd + 1]; either may be NULL. */
int32_t asgart_variants_copy(const asgart_variants *r, asgart_variant *records, uint64_t *var_offsets);
/* Milliseconds of the call behind r: [0] the upload, [1] the kernels, [2] the copies back of the offsets and the counts. */
int32_t asgart_variants_timings(const asgart_variants *r, double *ms3);
void asgart_variants_free(asgart_variants *r);
/* Threads per workgroup and records per workgroup of the records kernel, for tests that place their runs on the seams. */
void asgart_variants_geometry(uint64_t *block_threads, uint64_t *records_per_block);

/* The sites of the `X` records of v: this call needs no index.  Every `X` record makes up to two ENTRIES,
 *    (left_pos,  ref = left_base,  alt = o(right_base))   and   (right_pos, ref = right_base, alt = o(left_base)),
 * where o complements (ACGT and acgt swap, every other byte is kept) when bit 1 of the record's flag is set.  The classes
 * are A, C, G, T with the case folded (0, 1, 2, 3) and N (4) for every other byte; an entry exists only where
 * class(ref) != class(alt).  A site is a distinct position; for each, in ascending position: pos; ref, the class of the
 * text's byte there; alt_mask, bit c set where an entry has the alt class c; pairs, the number of entries; (sd, side) of
 * its first entry in record order, left (0) before right (1).  A duplication whose arms overlap can hold one position in
 * both arms, and then counts twice in pairs.  Indels make no sites.
 * Example 1 above: sites 3 (ref T, alt C, pairs 1, sd 0, side 0) and 12 (ref C, alt T, pairs 1, sd 0, side 1); example 2:
 * 3 (T, alt C) and 15 (G, alt A).
 * The result stays on the device of the records until asgart_sites_free; all of it is integer, so it does not depend on
 * the order anything arrives in.  v NULL: ASGART_E_ARG; no usable device: ASGART_E_HIP. */
typedef struct asgart_sites asgart_sites;
int32_t asgart_variant_sites(const asgart_variants *v, asgart_sites **out);
void asgart_sites_counts(const asgart_sites *r, uint64_t *n_sites, uint64_t *n_entries);
/* pos, ref, alt_mask, pairs, sd, side: n_sites entries each; every target is nullable. */
int32_t asgart_sites_copy(const asgart_sites *r, uint64_t *pos, uint8_t *ref, uint8_t *alt_mask, uint32_t *pairs,
                          uint32_t *sd, uint8_t *side);
/* Milliseconds of the call behind r: [1] everything from the first kernel to the last (nothing is uploaded). */
int32_t asgart_sites_timings(const asgart_sites *r, double *ms3);
void asgart_sites_free(asgart_sites *r);
/* Threads per workgroup of the kernels behind asgart_variant_sites (a wave of 64 reduces its entries by site). */
void asgart_sites_geometry(uint64_t *block_threads);

/* The two files, each one call that gives the whole file in one device buffer, an asgart_export, on the device of the
 * handle.  The result arrays are those of asgart_sdtable_records and belong to the call the records were made from (the
 * same n_sd); a position becomes local as chr_pos[2q + s] + (global - start of arm s of duplication q).  `prefix` is the
 * caller's header.
 * asgart_variants_records: the pair table, one line per record, 12 columns separated by tabs and ended by `\n`:
 *    1 chrom1   the name chr[2q]        2 start1, 3 end1   the left interval
 *    4 chrom2   the name chr[2q + 1]    5 start2, 6 end2   the right interval
 *    7 `sd<q>`     8 op     9 strand2, `+` for flag 0 and `-` for flag 3     10 family
 *   11 base1, 12 base2   the two bytes as stored for `X`, `.` for an indel
 * asgart_sites_records: VCF 4.2 body rows, one per site: the name and the local position + 1 of the site's (sd, side),
 * `.`, REF (the class letter), ALT (the letters of alt_mask in the order A, C, G, T, N, joined by `,`), `.`, `.`,
 * `NP=<pairs>`.
 * Example 1 as the fragment `chr1` from 0, family 0:
 *    chr1 2 3 chr1 12 12 sd0 I + 0 . .      chr1 3 4 chr1 12 13 sd0 X + 0 T C      chr1 8 8 chr1 17 18 sd0 D + 0 . .
 *    chr1 4 . T C . . NP=1                  chr1 13 . C T . . NP=1
 * Checked on the host before anything is launched, as asgart_sdtable_records checks, for the duplications with a record:
 * NULL arrays with a positive count, n_sd other than the records' call had, fam_offsets / name_offsets not starting at 0,
 * decreasing or (fam_offsets) not ending at n_sd, a name id outside the table, a flag other than 0 or 3 (the message names
 * the first), a position + length that wraps past 2^64: ASGART_E_ARG; 2^31 families and more: ASGART_E_CAP.  No records or
 * no sites: the prefix alone. */
int32_t asgart_variants_records(const asgart_variants *v, const uint64_t *fam_offsets, int64_t n_families,
                                const asgart_proto_sd *sds, const uint8_t *flags, const int32_t *chr, const uint64_t *chr_pos,
                                int64_t n_sd, const uint8_t *name_bytes, const uint64_t *name_offsets, int64_t n_names,
                                const uint8_t *prefix, uint64_t prefix_len, asgart_export **out);
int32_t asgart_sites_records(const asgart_sites *r, const uint64_t *fam_offsets, int64_t n_families,
                             const asgart_proto_sd *sds, const uint8_t *flags, const int32_t *chr, const uint64_t *chr_pos,
                             int64_t n_sd, const uint8_t *name_bytes, const uint64_t *name_offsets, int64_t n_names,
                             const uint8_t *prefix, uint64_t prefix_len, asgart_export **out);
/* Sizes the write stages work in: threads per workgroup, rows per workgroup, bytes of the LDS image (a workgroup whose
 * rows do not fit it stores them directly: a name of any length is legal). */
void asgart_variants_records_geometry(uint64_t *block_threads, uint64_t *rows_per_block, uint64_t *stage_bytes);
void asgart_sites_records_geometry(uint64_t *block_threads, uint64_t *rows_per_block, uint64_t *stage_bytes);

/* ---- finer-grained entry points mirroring the reference's inner API;
 *      used by the parity tests ------------------------------------------ */

/* Searcher cache entries (reference src/searcher.rs:99-143): for each of the
 * n_pat 8-byte patterns the SA slot interval [lo,hi) of suffixes starting
 * with it.  Patterns must be over {A,T,G,C,N}. */
int32_t asgart_searcher_cache_get(asgart_index *idx, const uint8_t *patterns8, int64_t n_pat,
                                  uint64_t *lo, uint64_t *hi);
/* Searcher::search (reference src/searcher.rs:145-180) for n_pat patterns of
 * k bytes each: SA slot interval [lo,hi) whose entries are the hits, in SA
 * order.  Read the hit positions with asgart_sa_read. */
int32_t asgart_searcher_search(asgart_index *idx, const uint8_t *patterns, int64_t n_pat,
                               uint64_t k, uint64_t *lo, uint64_t *hi);
int32_t asgart_sa_read(asgart_index *idx, uint64_t lo, uint64_t hi, int64_t *out);
/* The bytes [lo, hi) of the index's normalised text into out[hi - lo] (an index built by the device FASTA reader is the only
 * copy of it: a host writer of cs:Z: tags reads the arms back with this).  lo > hi or hi past the text: ASGART_E_ARG. */
int32_t asgart_index_read_text(asgart_index *idx, uint64_t lo, uint64_t hi, uint8_t *out);

/* Per-probe filtered hit lists exactly as the automaton consumes them
 * (reference src/automaton.rs:96-117), for all chunks concatenated: probe j of
 * a chunk sits at needle offset (j+1)*(k/2).  status: 0 processed, 1 skipped
 * ('N' first base), 2 skipped (cardinality).  Two-call: with status==NULL
 * returns the probe count and *n_hits; then fills status[n_probes],
 * row_offsets[n_probes+1], hits[n_hits] (hit starts, SA order). <0 on error. */
int64_t asgart_probe_hits(asgart_index *idx, const uint64_t *chunks, int64_t n_chunks,
                          const asgart_settings *settings, uint8_t *status,
                          uint64_t *row_offsets, uint64_t *hits, uint64_t *n_hits);

#define ASGART_STATS_YARDSTICK 1u
#define ASGART_STATS_RAW_HITS 2u
/* asgart_search_duplications is re-entrant: up to two calls on one index may be in flight from
 * different host threads (e.g. the direct and the -RC pass), each in its own internal context.
 * ASGART_STATS_CTX(i), i = 0 or 1, selects the stats of context i instead of the last call's. */
#define ASGART_STATS_CTX(i) (((uint32_t)(i) + 1u) << 8)
/* Stats of the last search call on this index.  With ASGART_STATS_YARDSTICK in
 * `flags` extra (untimed) kernels also fill bisect_steps, the accounting fields and raw_hits; with
 * ASGART_STATS_RAW_HITS raw_hits alone (the probes the position filter answered are looked up for it). */
int32_t asgart_get_stats(asgart_index *idx, uint32_t flags, asgart_stats *out);

/* Segments per extension tier as the last search call on this index placed them: out[t - 1] for tier t = 1..7 (barren
 * segments, which are not run, are in none); out[7] = the segments the tail rule moved up (counted before the barren test
 * by position and option force_tier). */
int32_t asgart_tier_segments(asgart_index *idx, uint64_t *out);
/* The hit rows of the last search call on this index, by the kernel that filled them (summed up now, by an untimed pass
 * over what the call left in its workspace): out[0], out[1] = rows and suffix-array entries read of the rows with intervals
 * of up to 32 entries; out[2], out[3] = of the rows streamed from larger intervals; out[4], out[5] = rows filled from the
 * kept tail of their k-mer's position-sorted occurrence list, and the entries read for them (two per list position: the
 * position and the suffix-array slot it came from).
 * The ranked fill is governed by the environment variable ASGART_RANKED_FILL, read when an index is created: 0 = off (the
 * slots are not kept: 4 bytes per text position less), 1 or unset = rows of a whole k-mer interval of more than 256
 * entries that keep at most 512 hits, where that reads clearly less than the interval (R > 2 * kept + 64), 2 = all such
 * rows (tests).  Indexes with 64-bit positions always stream.  The rows are the same bytes either way. */
int32_t asgart_fill_counts(asgart_index *idx, uint64_t *out);
/* Diagnostic: the rows behind out[2..5] of asgart_fill_counts in four classes, for each the rows, the sum of their interval sizes and the sum of
 * their kept hits: out[0..2] streamed, interval of 33..256 entries; out[3..5] streamed, larger, kept count found by
 * streaming; out[6..8] streamed, kept count found by bisection; out[9..11] filled from the position-sorted list. */
int32_t asgart_fill_tally(asgart_index *idx, uint64_t *out);
/* Diagnostic (for tests of the rule): ASGART_RANKED_FILL = mode for a row that keeps `kept` hits of an interval of `interval` entries (host code,
 * needs no device): 1 = filled from the position-sorted list, 0 = streamed. */
int32_t asgart_ranked_fill_takes(uint64_t interval, uint64_t kept, int32_t mode);
/* Diagnostic (for tests of the rule): the hit filter of the probe at needle offset i of the chunk text[s, s + L), in a
 * reversed pass or a direct one, as the kernels state it (host code, needs no device): occurrence x is kept when
 * x >= out[0] && x != out[1]  (src/automaton.rs:105-114). */
void asgart_hit_rule(uint64_t i, uint64_t s, uint64_t L, int32_t reverse, uint64_t *out);
/* The run directory of the index as asgart_index_prepare built it last: a hash table of 64-byte buckets of four entries
 * that holds, for every k-mer with at least T occurrences, its suffix-array interval, so that the lookup of a repeated
 * k-mer reads one bucket instead of bisecting the keys.  An accelerator only: a k-mer that is not in it (it occurs less
 * often, or its bucket was full when it came) is looked up through the prefix table, and no result depends on it.
 * out[0] = bytes of the table (0: the index has none -- probe sizes above 21, a --trim index, ASGART_RUN_DIR=0, no memory),
 * out[1] = buckets, out[2] = T, out[3] = runs it holds, out[4] = runs that found their bucket full, out[5], out[6] =
 * lookups that found their k-mer in it and lookups that did not, as the accounting pass of the last asgart_get_stats call
 * with ASGART_STATS_YARDSTICK counted them (0 before), out[7] = ASGART_RUN_DIR as the index read it.
 * Environment, read when an index is created: ASGART_RUN_DIR (0 = off; 1 or unset = on), ASGART_RUN_DIR_T (the shortest run
 * that gets an entry, 2 when unset; doubled while the table would take more than an eighth of the bytes of the keys),
 * ASGART_RUN_DIR_BUCKETS (tests: the number of buckets, whatever the runs need). */
int32_t asgart_run_dir_info(asgart_index *idx, uint64_t *out);
/* Diagnostic: the loads of the probes that the accounting pass of the last asgart_get_stats call with
 * ASGART_STATS_YARDSTICK looked up, by array: out[0], out[1] = loads from the prefix table and their bytes; out[2], out[3] =
 * from the keys (bisections and walk); out[4], out[5] = from the suffix array; out[6], out[7] = run-directory buckets read
 * that held the k-mer / did not (64 bytes each); out[8..12] = lookups whose interval has 1, 2-8, 9-32, 33-256, more slots;
 * out[13] = lookups that found nothing; out[14], out[15] = 0. */
int32_t asgart_lookup_account(asgart_index *idx, uint64_t *out);
/* Diagnostic (for tests of the rule; host code, needs no device): an entry of the run directory and the bucket function.
 * out[0] = the entry's second word for a run of `len` slots that starts at slot `lo` (lo in the low 40 bits, the length in
 * the high 24, saturated at 2^24 - 1: "bisect the end from lo"), out[1], out[2] = lo and length read back from it, out[3] =
 * the bucket of `key` in a table of n_buckets buckets, out[4] = the key word that marks an empty entry. */
void asgart_run_dir_rule(uint64_t key, uint64_t lo, uint64_t len, uint64_t n_buckets, uint64_t *out);
/* asgart_join_cuts: host code, needs no device (for tests of the rule).  What a search call decides for ONE long segment
 * that ran as n_ranges ranges side by side (option split): cut_held[j] bit 0 = cut j, between ranges j and j + 1, held
 * (n_ranges - 1 verdicts); flushes[j] = the families range j flushed; last_gave_up != 0: the run over the last range gave
 * up.  Every cut held: the family ordinals of range j count on from the flushes of ranges 0 .. j - 1 (fix[j] = their sum)
 * and the segment is joined.  Otherwise f is the first cut that did not hold: ranges 0 .. f stand (fix = 0xFFFFFFFE: held
 * until the tail run has come back), the records of the ranges behind it are dropped (fix = 0xFFFFFFFF), and ONE more run
 * covers the rest, from where range f started, its family ordinals counting on from the flushes of ranges 0 .. f.  f = 0,
 * or every cut held but the last run gave up (f = 0 then): every range is dropped and the whole segment runs again.
 * Writes fix[n_ranges]; settled[n_ranges + 1]: fix when the tail run has come back -- ranges 0 .. f get their bases,
 * settled[n_ranges] is the tail run's base (0xFFFFFFFF: no tail run) -- and with tail_gave_up != 0 every entry is dropped
 * and the whole segment runs again; out[0] = f (n_ranges - 1: every cut held), out[1] = the action (0 = joined, 1 = one more
 * run from range f, 2 = the whole segment again), out[2] = the tail run's base, out[3] = the action when the tail run has
 * come back.  Errors: n_ranges outside 1..4096, a null pointer (ASGART_E_ARG). */
int32_t asgart_join_cuts(int32_t n_ranges, const uint32_t *cut_held, const uint32_t *flushes, int32_t last_gave_up,
                         int32_t tail_gave_up, uint32_t *fix, uint32_t *settled, uint32_t *out);
/* asgart_split_warm_next: host code, needs no device (for tests of the rule).  The warm-up, in probes, the index remembers
 * for a segment a cut of which did not hold: warm_used = the warm-up its ranges had (0: the warm-up is not the matter),
 * need = how far in front of the failed cut the oldest arm of the range before it was born, range_len = probes per range,
 * split_warm_max as the option.  limit = min(split_warm_max, 2 * range_len).  need > warm_used: need + 64 rounded up to a
 * multiple of 256; else the limit itself while warm_used is below it.  0 when warm_used = 0 or the result would exceed the
 * limit: the segment keeps the call's own warm-up and only the cuts that held are planned again. */
uint32_t asgart_split_warm_next(uint32_t warm_used, uint32_t need, uint32_t range_len, uint64_t split_warm_max);
/* The tier table's figures a call starts from (host code, needs no device): profile_ms[0] = the runs over ranges,
 * profile_ms[t] = tier t's estimated duration on the GRCh38-shaped profile (what asgart_tier_plan is fed before a call
 * has measurements of its own), for a thresholded tier what is left of it where the tail rule is in force; tail_hits[t] =
 * tier t's threshold of the tail rule, 0 = none (8 entries each). */
int32_t asgart_tier_profile(double *profile_ms, uint64_t *tail_hits);

/* Thread-local message of the last error returned on this thread. */
const char *asgart_last_error(void);
/* "asgart-hip <version> gfx950" */
const char *asgart_version(void);

#ifdef __cplusplus
}
#endif
#endif
