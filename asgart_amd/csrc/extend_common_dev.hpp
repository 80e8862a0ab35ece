// extend_common_dev.hpp -- what the four extension kernels share (extend_wave_dev.hpp, extend_heavy_dev.hpp,
// extend_fast_dev.hpp, extend_k8_dev.hpp): the launch parameters, the record list, the statistics of the persistent
// workgroups, the arm predicate, and the walk over the probes of a segment -- where a segment ends, the batch of up to
// 64 probes under the cursor, the next hit-probe of a batch, the record of a retired arm.  The representation of the
// automaton is described in extend_wave_dev.hpp; plan_ranges_kernel and validate_cuts_kernel (ranges_dev.hpp) read
// what the runs over ranges leave behind (RangeRun, SplitSeg, kDumpWords).
#pragma once

#include "device_base.hpp"

namespace asgart {

// create_seq of the record that voids a family: arms were still alive where the chunk ended (src/automaton.rs:201-203)
constexpr uint32_t kTombstone = 0xFFFFFFFFu;

// Diagnostic build only (-DASGART_PROFILE_EXTEND): per-phase cycle sums of the extension kernel
// are added to ctr[16..]; never enabled in the shipped library.
#ifdef ASGART_PROFILE_EXTEND
#define PROF_DECL unsigned long long pf_t0 = 0, pf_acc[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}
#define PROF_START() pf_t0 = __builtin_amdgcn_s_memtime()
#define PROF_STOP(slot) pf_acc[slot] += __builtin_amdgcn_s_memtime() - pf_t0
#define PROF_COUNT(slot, v) pf_acc[slot] += (v)  // (slots 10, 11: sums of live arms and hits over the hit-probes)
#define PROF_MAX(slot, v) pf_acc[slot] = pf_acc[slot] > (unsigned long long)(v) ? pf_acc[slot] : (unsigned long long)(v)
#define PROF_SEG_BEGIN() const unsigned long long pf_seg0 = __builtin_amdgcn_s_memtime()
#define PROF_FLUSH()                                                             \
    do {                                                                         \
        const unsigned long long pf_dt = __builtin_amdgcn_s_memtime() - pf_seg0; \
        if (lane == 0 && atomicMax(&P.ctr[28], pf_dt) < pf_dt) {                 \
            P.ctr[29] = g0;                                                      \
            P.ctr[30] = ((unsigned long long)pf_acc[5] << 32) | pf_acc[3];       \
            P.ctr[31] = ((unsigned long long)pf_acc[10] << 32) | pf_acc[11];     \
            P.ctr[32] = pf_acc[0];                                               \
            P.ctr[33] = pf_acc[6];                                               \
            P.ctr[25] = pf_acc[9];                                               \
            for (int pf_i = 0; pf_i < 12; ++pf_i) P.ctr[56 + pf_i] = pf_acc[pf_i]; \
        }                                                                        \
        if (lane == 0)                                                           \
            for (int pf_i = 0; pf_i < 12; ++pf_i)                                \
                if (pf_acc[pf_i]) atomicAdd(&P.ctr[16 + pf_i], pf_acc[pf_i]);     \
        if (lane == 0) {                                                         \
            int pf_b = 0;                                                        \
            while (pf_b < 15 && (2ull << pf_b) <= pf_acc[9]) ++pf_b;             \
            atomicAdd(&P.ctr[CT_HIST_PEAK + pf_b], 1ull);                        \
            pf_b = 0;                                                            \
            while (pf_b < 15 && (2ull << pf_b) <= pf_acc[5] + pf_acc[3]) ++pf_b; \
            atomicAdd(&P.ctr[CT_HIST_PROBES + pf_b], pf_acc[5] + pf_acc[3]);     \
        }                                                                        \
        for (int pf_i = 0; pf_i < 12; ++pf_i) pf_acc[pf_i] = 0;                  \
    } while (0)
#define DBG_ADD(slot, v) atomicAdd(&P.ctr[40 + (slot)], (unsigned long long)(v))
#else
#define DBG_ADD(slot, v)
#define PROF_DECL
#define PROF_START()
#define PROF_STOP(slot)
#define PROF_COUNT(slot, v)
#define PROF_MAX(slot, v)
#define PROF_SEG_BEGIN()
#define PROF_FLUSH()
#endif
constexpr int kHitBatch = 1024;  // LDS staging for the hit rows of one probe batch
constexpr uint32_t kNoSeq = 0xFFFFFFFFu;  // s_seq value of an empty slot

// A RUN over part of a long segment (extend_k8_kernel<..., RANGE = true>; plan_ranges_kernel makes them): the walk starts at
// probe g_begin with no arm and stops in front of g_stop; records are written from probe emit_from on (the cut: a hit-probe;
// what lies in front of it is the run's warm-up and belongs to the range before).
struct RangeRun {
    uint32_t g_begin, g_stop;  // [g_begin, g_stop) (g_stop = ~0u: to the segment's end)
    uint32_t g_seg0;           // first probe of the segment (record key, chunk)
    uint32_t emit_from;        // the cut this run reports from (g_seg0: from the start)
    uint32_t flags;            // kRunNoEmit | kRunLast
    uint32_t split;            // which split segment (struct SplitSeg)
    uint32_t pad0, pad1;
};
constexpr uint32_t kRunNoEmit = 1u;    // a warm-up on its own: only its final state is wanted (what the run behind the cut starts from)
constexpr uint32_t kRunLast = 2u;      // the run that reaches the segment's end
constexpr uint32_t kRunDumpCap = 5120; // arms a run can leave alive (the long shape's slots)
// per run two states, 8 words each (run_meta): [0] what it holds when it STOPS, [1] what it holds when it reaches its cut:
// 0 arms written to run_dump  1 flushes since the cut  2 family open  3 probes a flush is still held back for  4 ([0] only) gave up
// (more arms than slots, a probe with more hits than the staging area)
// per run two dumps of kRunDumpCap arms (run_dump), kDumpWords per arm, the creation number first (32-bit positions: creation
// number, left start, left end, right start | right end, threshold, gap, 0; 64-bit: creation number, threshold, gap, 0 | left
// start, left end | right start, right end)
template <class PosT> constexpr uint32_t kDumpWords = sizeof(PosT) == 4 ? 8u : 12u;
struct SplitSeg {
    uint32_t g_seg0, run_base, n_ranges, cut_base;  // runs run_base .. + n_ranges - 1: the ranges; cuts cut_base .. + n_ranges - 2
    uint32_t span, hits, tier, warm;                // (what the placement knew of the segment; the warm-up its ranges got)
};

template <class PosT>
struct ExtParams {
    const RangeRun *runs;                 // (RANGE launches) the work list
    uint32_t *run_meta, *run_dump;        // ... and what the runs leave behind (see RangeRun)
    RunParams rp;
    const uint32_t *p_filt;
    const unsigned long long *row_off;
    const PosT *hits;
    const uint32_t *seg_list;
    const unsigned long long *n_seg_ptr;  // device count of seg_list entries
    unsigned long long *cursor;           // work-fetch cursor
    SdRec *recs;
    unsigned long long rec_cap;
    uint32_t *ovf_list;                   // segments this launch gives up on go here (may be null)
    unsigned long long *ovf_count;        // ... appended at *ovf_count (device counter)
    char *scratch;                        // heavy global tier: per-workgroup arm storage
    uint32_t gen_bits;                    // arm-resident kernels: bits of the table generation counter (tests shrink it)
    uint32_t escalate_cost;               // one-wave tiers: give up after this much LDS-path work
    uint32_t cap_limit;                   // effective live-arm capacity (<= CAP; tests lower it)
    uint32_t heavy_cap;                   // K4b MODE 2 (tier 7): arm slots per workgroup in its HBM slice
    uint32_t solo_hits;                   // K6: probes with up to this many hits may run on wave 0 alone (0: never)
    uint32_t k8_delay;                    // K8 (tests): cycles the ranking wave waits before it reads the free counts
    uint32_t tier;                        // the tier this launch runs as (statistics)
    unsigned long long *seg_slots;        // 4096 words of this launch's tier: start time of the segment a workgroup is on (seg_clock)
    unsigned long long *ctr;
    unsigned long long *hb;               // heartbeat slots of this launch's tier (pinned host memory; null: none)
};

// a workgroup's sign of life (see SearchCtx::heartbeat): which segment it is on and how far
template <class PosT>
__device__ inline void heartbeat(const ExtParams<PosT> &P, uint32_t g0, uint32_t at) {
    if (P.hb) {
        unsigned long long *slot = P.hb + 2u * (blockIdx.x % 256u);
        __builtin_nontemporal_store((unsigned long long)g0 | 1ull << 63, slot);
        __builtin_nontemporal_store((unsigned long long)at, slot + 1);
    }
}

// The whole predicate of try_extend_arms (src/automaton.rs:68-70) for an active arm with right
// segment [rs, re], threshold thr, and a hit m = [x, x+k]:
//     d_ss(a.right, m) < thr  &&  m.end > a.right.end
// Because len(right) >= k always (an arm starts as [x0, x0+k] and re only grows), this is
// exactly   re - k < x < re + thr   (thr >= 1), i.e. (x - lo) < w in unsigned arithmetic with
// lo = re - k + 1, w = thr + k - 1:
//   x <= re : x > re-k >= rs so m.start lies in [rs, re]            -> d_ss = 0 < thr
//   x >  re : no containment, d_ss = min(x+k-rs, x-re) = x - re     -> accept iff x - re < thr
// (thr == 0 accepts nothing.)  tests/test_oracle_golden.py checks the equivalence exhaustively
// against the oracle's literal d_ss.
template <class PosT>
__device__ inline bool arm_accepts(PosT x, PosT re, uint32_t thr, uint32_t k) {
    const PosT lo = (PosT)(re - k + 1u);
    const uint64_t w = thr ? (uint64_t)thr + k - 1u : 0u;
    return (uint64_t)(PosT)(x - lo) < w;
}

// max(e, (0.1 * len as f64) as i64)   (src/automaton.rs:69).  The double product truncates to
// len / 10 for every len < 9e15 (0.1 rounds UP to 0.1000000000000000055, so the product can only
// cross an integer boundary once len / 10 * 1.1e-16 reaches 0.1; checked for 3M values up to 2^40 in
// tests/test_oracle_golden.py::test_tenth_threshold_is_integer_division), so the kernels divide.
__device__ inline uint32_t arm_threshold(uint64_t left_len, uint32_t G) {
    const uint64_t tenth = left_len <= 0xFFFFFFFFull ? (uint64_t)((uint32_t)left_len / 10u) : left_len / 10u;
    const uint64_t thr = tenth > (uint64_t)G ? tenth : (uint64_t)G;
    return thr > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)thr;
}

// Output records are appended to one device-wide list.  A global atomic WITH its return value costs
// a full memory round trip (a microsecond on the critical path of a serial segment), so every wave
// reserves kRecChunk slots at a time and hands them out from registers; what is left of a chunk
// when the wave takes the next one (or exits) is marked void (g_start = kVoidStart: sorts last, the
// host stops there).
constexpr uint32_t kRecChunk = 32;
constexpr uint32_t kVoidStart = 0xFFFFFFFFu;
struct RecAlloc {
    unsigned long long next = 0;  // wave-uniform
    uint32_t left = 0;
};
// Statistics of the persistent workgroups, kept in DEVICE memory (not in registers: the 1024-thread shapes sit at their
// 128-VGPR cap and every value that lives across the segment loop is a spill into it):
//   wg_begin / wg_busy   the workgroup's lifetime goes into its tier's tally (- start, + end: two atomics per workgroup)
//   seg_clock            called by ONE thread where the workgroup takes its next segment: the time since the previous
//                        call is one segment's duration; the longest per tier is the serial floor of the extension
template <class PosT>
__device__ inline void wg_begin(const ExtParams<PosT> &P) {
    if (threadIdx.x == 0 && P.tier >= 1u && P.tier <= (uint32_t)kRunsStat) {
        atomicAdd(&P.ctr[CT_BUSY1 + P.tier - 1u], 0ull - wall_clock64());
    }
}
// (the slots are zero when a launch starts -- the host clears them, and a workgroup leaves its slot zero -- : the thread
// that fetches the segments and the thread that closes the last one need not be the same)
#ifdef ASGART_SEG_TOP
constexpr unsigned long long kSegTopMin = 200000;  // (diagnostic build: 2 ms; the log holds 511 segments per tier)
constexpr uint32_t kSegTopWords = 512;
#endif
template <class PosT>
__device__ inline void seg_clock(const ExtParams<PosT> &P, bool last = false) {
    if (!P.seg_slots || P.tier < 2u || P.tier > (uint32_t)kRunsStat) return;  // (tier 1: a million tiny segments)
    const unsigned long long now = wall_clock64();
    const unsigned long long prev = atomicExch(&P.seg_slots[blockIdx.x & 4095u], last ? 0ull : now);
    if (prev && now > prev) atomicMax(&P.ctr[CT_SEGMAX1 + P.tier - 1u], now - prev);
#ifdef ASGART_SEG_TOP
    // diagnostic build (make segtop; never shipped): every segment of kSegTopMin ticks and more is also logged, per tier, in
    // block 1 of the segment slots (tier 1 keeps no segment clock): 512 words per statistics slot, [count | durations]
    if (prev && now > prev && now - prev >= kSegTopMin) {
        unsigned long long *log = P.seg_slots - (size_t)4096 * (P.tier & 7u) + 4096 + (size_t)kSegTopWords * (P.tier & 7u);
        const unsigned long long at = atomicAdd(log, 1ull);
        if (at + 1u < kSegTopWords) log[1u + at] = now - prev;
    }
#endif
}
template <class PosT>
__device__ inline void wg_busy(const ExtParams<PosT> &P) {
    if (threadIdx.x == 0 && P.tier >= 1u && P.tier <= (uint32_t)kRunsStat) {
        seg_clock(P, true);  // (closes the last segment)
        atomicAdd(&P.ctr[CT_BUSY1 + P.tier - 1u], wall_clock64());
        atomicAdd(&P.ctr[CT_WGS1 + P.tier - 1u], 1ull);
    }
}
template <class PosT>
__device__ inline void rec_flush(RecAlloc &ra, const ExtParams<PosT> &P, int lane) {
    if ((uint32_t)lane < ra.left && ra.next + (unsigned)lane < P.rec_cap) P.recs[ra.next + (unsigned)lane].g_start = kVoidStart;
    ra.left = 0;
}
// all 64 lanes call; em = ballot of the emitting lanes (non-zero); returns this lane's slot
template <class PosT>
__device__ inline unsigned long long rec_slot(RecAlloc &ra, const ExtParams<PosT> &P, unsigned long long em, int lane) {
    const uint32_t n = (uint32_t)__popcll(em);
    if (n > ra.left) {
        rec_flush(ra, P, lane);
        const uint32_t take = n > kRecChunk ? n : kRecChunk;
        unsigned long long b = 0;
        if (lane == 0) b = atomicAdd(&P.ctr[CT_SD], (unsigned long long)take);
        ra.next = lane_of(b, 0u);
        ra.left = take;
    }
    const unsigned long long at = ra.next + (unsigned)__popcll(em & ((1ull << lane) - 1ull));
    ra.next += n;
    ra.left -= n;
    return at;
}

// ---------------------------------------------------------------- the walk over a segment ---------
// Where the segment that starts at probe g0 lives and where its walk ends (wave-uniform).
struct SegHeader {
    uint64_t cs, cl;     // text start and length of its chunk
    bool rev;            // the orientation of the chunk's pass
    uint32_t pb;         // the chunk's first probe ...
    uint32_t chunk_end;  // ... and the one behind its last
    uint32_t g_end;      // where the walk stops: there, or (sharded calls) where the window ends if that comes first
};
__device__ inline SegHeader load_segment(const RunParams &rp, uint32_t g0) {
    const int c = chunk_of_uniform(rp.ch, g0);
    SegHeader s;
    s.cs = rp.ch.start[c];
    s.cl = rp.ch.len[c];
    s.rev = (rp.mode_of(c) & 2u) != 0u;
    s.pb = rp.ch.pbase[c];
    s.chunk_end = rp.ch.pbase[c + 1];
    s.g_end = min(s.chunk_end, rp.win_end(g0));
    return s;
}

// The probes g .. g + 63 (short of g_end), one per lane: their hit rows are contiguous in the CSR, and as many of them as
// fit a staging area of HB hits form a batch.  Describes the batch; staging its rows is the caller's business.
struct ProbeBatch {
    uint32_t f_l, rel_l;         // this lane's probe: its hits (or kSkipN / kPending), its row's offset behind base
    unsigned long long base;     // the first probe's row
    uint32_t n;                  // probes in the batch (0: the first probe alone has more than HB hits; tot, hm, qm are empty)
    uint32_t tot;                // hits of the batch
    unsigned long long hm, qm;   // its hit-probes and its quiet probes, a bit per lane
};
template <int HB>
__device__ inline ProbeBatch load_batch(const uint32_t *p_filt, const unsigned long long *row_off, uint32_t g, uint32_t g_end,
                                        int lane) {
    ProbeBatch b;
    const uint32_t nb = min(64u, g_end - g);
    b.f_l = (uint32_t)lane < nb ? p_filt[g + lane] : kSkipN;
    const unsigned long long r_l = (uint32_t)lane < nb ? row_off[g + lane] : 0ull;
    const unsigned long long r_hi = uni(row_off[g + nb]);
    b.base = lane_of(r_l, 0u);
    unsigned long long r_next = __shfl_down(r_l, 1);
    if ((uint32_t)lane + 1 >= nb) r_next = r_hi;
    const bool fits = (uint32_t)lane < nb && r_next - b.base <= (unsigned long long)HB;
    const unsigned long long fm = __ballot(fits);
    b.n = (~fm == 0ull) ? 64u : (uint32_t)(__ffsll((long long)~fm) - 1);
    if (b.n > nb) b.n = nb;
    b.rel_l = (uint32_t)(r_l - b.base);
    b.tot = (uint32_t)((b.n == nb ? r_hi : lane_of(r_l, b.n)) - b.base);
    const unsigned long long in_batch = b.n >= 64 ? ~0ull : ((1ull << b.n) - 1ull);
    b.hm = __ballot(b.f_l >= 1u && b.f_l < kPending) & in_batch;
    b.qm = __ballot(b.f_l == 0u) & in_batch;
    return b;
}
// The next hit-probe of the batch at or behind position pos (64: none is left) and the quiet probes between pos and it.
__device__ inline uint32_t next_hit(const ProbeBatch &b, uint32_t pos, uint32_t &quiet_before) {
    const unsigned long long hmr = pos >= 64 ? 0ull : (b.hm >> pos) << pos;
    const uint32_t at = hmr ? (uint32_t)(__ffsll((long long)hmr) - 1) : 64u;
    const unsigned long long upto = at >= 64 ? ~0ull : ((1ull << at) - 1ull);
    const unsigned long long from = pos >= 64 ? 0ull : ~((1ull << pos) - 1ull);
    quiet_before = (uint32_t)__popcll(b.qm & upto & from);
    return at;
}

// The record of one arm of the segment at g0 (slot `at` from rec_slot; past the list's capacity nothing is written):
// positions relative to the chunk (start cs, length cl, pass orientation rev) become text positions.
template <class PosT>
__device__ inline void write_record(const ExtParams<PosT> &P, unsigned long long at, uint32_t g0, uint32_t fam_seq, uint32_t seq,
                                    uint32_t pad, uint64_t cs, uint64_t cl, bool rev, PosT ls, PosT le, PosT rs, PosT re) {
    if (at >= P.rec_cap) return;
    const uint64_t ll = (uint64_t)le - (uint64_t)ls;
    SdRec r;
    r.g_start = g0;
    r.fam_seq = fam_seq;
    r.create_seq = seq;
    r.pad = pad;
    r.sd.left = rev ? cs + cl - (uint64_t)ls - ll : (uint64_t)ls + cs;  // left fix-up, src/bin/asgart.rs:229-237
    r.sd.right = rs;
    r.sd.left_length = ll;
    r.sd.right_length = (uint64_t)re - (uint64_t)rs;
    P.recs[at] = r;
}

// bucket(re) = re >> bsh with 2^bsh >= G + k: the window of an arm at its floor threshold G meets at most two buckets
__device__ inline uint32_t bucket_shift(uint32_t G, uint32_t k) {
    uint32_t bsh = 3;
    while ((1ull << bsh) < (unsigned long long)G + k) ++bsh;
    return bsh;
}

// Hit-table entries of the arm-resident kernels (K6, K8): generation and hit index above, the position below.
//   32-bit positions  [gen:22 | hit:10 | x:32]      64-bit positions  [gen:12 | hit:10 | x:42]
template <class PosT>
struct ArmTable {
    static constexpr bool kWidePos = sizeof(PosT) == 8;
    static constexpr uint32_t kTagShift = kWidePos ? 42u : 32u;
    static constexpr uint32_t kGenMax = kWidePos ? 12u : 22u;  // bits of the generation counter
    static constexpr unsigned long long kPosMask = (1ull << kTagShift) - 1ull;
    using WinT = typename std::conditional<kWidePos, uint64_t, uint32_t>::type;  // width of an arm's window
    static __device__ inline unsigned long long entry(uint32_t tag, PosT x) {
        return ((unsigned long long)tag << kTagShift) | ((unsigned long long)x & kPosMask);
    }
    static __device__ inline uint32_t tag_of(unsigned long long e) { return (uint32_t)(e >> kTagShift); }
    static __device__ inline PosT pos_of(unsigned long long e) { return (PosT)(e & kPosMask); }
};
constexpr uint32_t kNone = 0xFFFFFFFFu;   // best[]: no arm accepts this hit
constexpr uint32_t kNever = 0xFFFFFFFEu;  // what a candidate read of an idle lane returns: no creation number
// candidate register of an arm: up to three hit indices, 10 bits each, count in bits 30..31;
// kCoop: more than three, a window too wide for the table walk, or a probe whose stash overflowed
constexpr uint32_t kCoop = 0xFFFFFFFFu;
constexpr uint32_t kStash = 64;           // hits of a probe that found their table row full

}  // namespace asgart
