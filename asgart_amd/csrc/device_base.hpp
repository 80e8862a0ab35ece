// device_base.hpp -- what every device header of the pipeline starts from: the tier count, the device counters, the chunk
// lookup, a probe's place (ProbeAt) and the hit filter (HitRule), the LDS barriers, and the wave-level primitives (uniform
// values, lane reads, DPP scans).
#pragma once

#include "search_dev.hpp"

#include <type_traits>

namespace asgart {

constexpr int kTiers = 7;  // extension tiers (see the placement in call_place.hpp)
constexpr int kRunsStat = kTiers + 1;  // statistics slot (ExtParams::tier) of the runs over ranges: after the tiers'

// device counters (u64 each)
enum Counter {
    CT_BIG = 0,       // entries in big_list
    CT_SEG,           // entries in seg_list
    CT_SCAN_TICKET,   // scan_segments_kernel: the next tile
    CT_FAM,           // families emitted
    CT_SD,            // ProtoSDs emitted
    CT_OVF,           // segments that overflowed the arm capacity
    CT_TOTAL_HITS,    // CSR size
    CT_N_SKIPPED,
    CT_CARD_SKIPPED,
    CT_WITH_HITS,
    CT_RAW_HITS,
    CT_SEARCHED,
    CT_BISECT,        // yardstick
    CT_OVF_CURSOR,
    CT_AMBIG,         // sharding: start decisions that need a longer look-back
    CT_RANOUT,        // sharding: segments that ran past the look-ahead window
    // 16..33 and 56..67: per-phase cycle sums of the diagnostic build (-DASGART_PROFILE_EXTEND)
    CT_EARLY_N = 34,    // early cascade launches (of tiers 3 and 6): list lengths ...
    CT_EARLY_CUR = 36,  // ... and work cursors
    CT_RANK = 38,       // entries in rank_list (large intervals counted by bisection of the position-sorted lists)
    CT_BIG0 = 39,       // entries of big_list that big_count_kernel counted (later ones were appended for the fill)
    CT_RANKED = 40,     // entries in ranked_list (rows rank_count_kernel gives to fill_ranked_kernel instead of big_list)
    CT_ALG_BYTES = 68,  // accounting pass: bytes the probe-search kernels move by design
    CT_FLT_REJECTED,    // accounting pass: probes answered by the position bits alone
    CT_LONGSEG,         // placement: segments the lane-per-segment walk handed to the wave-per-segment kernel
    CT_ALG_BYTES16,     // accounting pass: the part of CT_ALG_BYTES that is wide coalesced loads (16 bytes per lane)
    CT_HIST_PEAK = 72,   // diagnostic build: log2 histograms per launch (16 bins each)
    CT_HIST_PROBES = 88,
    CT_N1 = 104,       // list lengths of the extension tiers 1..kTiers (kTiers entries)
    CT_NF = 111,       // ... of a cascade launch
    CT_CUR1 = 112,     // work cursors of the tiers (kTiers entries)
    CT_CURF = 119,
    CT_OVF1 = 120,     // segments tier t gave up on (kTiers entries; the last one has nowhere to go)
    CT_BUSY1 = 128,    // per tier: sum over its workgroups of their lifetime, in 10-ns ticks (how much of the chip a tier holds:
                       // persistent workgroups own their share of a compute unit from launch to exit) ...
    CT_WGS1 = 136,     // ... and the number of workgroups summed
    CT_TPROBES1 = 144, // placement statistics (option debug only): hit-probes per tier ...
    CT_THITS1 = 152,   // ... and hits per tier
    CT_SEGMAX1 = 160,  // per tier: the longest time one workgroup spent on ONE segment, in 10-ns ticks -- the serial floor of
                       // the extension (what neither more compute units nor more GPUs shorten)
    CT_CLUSTER_BARREN = 168,  // segments cluster_barren_kernel proved barren
    CT_CLUSTER_CUR = 169,     // its work cursors (two launches)
    CT_TAIL_UP = 171,         // placement: segments the tail rule moved to the next tier that holds more (place_tier)
    CT_FILL_ACCT = 176,       // fill_account_kernel (asgart_fill_counts, asgart_fill_tally): its 18 sums
    CT_LOOKUP_ACCT = 196,     // accounting pass: the looked-up probes' loads by array (LookupAcct, search_dev.hpp: 16 sums)
    CT_COUNT = 212
};

__device__ inline int chunk_of(const ChunkTable &ch, uint32_t g) {
    // last c with pbase[c] <= g  (pbase non-decreasing; empty chunks repeat values)
    int lo = 0, hi = ch.n_chunks;  // answer in [lo, hi)
    while (hi - lo > 1) {
        int mid = (lo + hi) >> 1;
        if (ch.pbase[mid] <= g) lo = mid; else hi = mid;
    }
    return lo;
}

// same for a wave-uniform probe number: keeps the bisection in scalar registers / scalar loads
__device__ inline int chunk_of_uniform(const ChunkTable &ch, uint32_t g) {
    g = __builtin_amdgcn_readfirstlane(g);
    int lo = 0, hi = ch.n_chunks;
    while (hi - lo > 1) {
        const int mid = __builtin_amdgcn_readfirstlane((lo + hi) >> 1);
        if (ch.pbase[mid] <= g) lo = mid; else hi = mid;
    }
    return __builtin_amdgcn_readfirstlane(lo);
}

// Where a probe lies: probe g of chunk c is the needle offset i = (g - pbase[c] + 1) * step into the chunk text[s, s + L),
// the needle prepared the way of the chunk's pass (md: bit 1 = reversed, bit 0 = complemented).  The + 1, the stride and
// the pass's mode are part of the parity argument of DESIGN.md 5.4: every kernel that needs a probe's place takes it from
// here.  (load_segment, extend_common_dev.hpp, reads the same table for a segment.)
struct ProbeAt {
    uint64_t i, s, L;
    uint32_t md;
};
__device__ inline ProbeAt probe_at(const RunParams &rp, int c, uint32_t g) {  // c = chunk_of(rp.ch, g), known to the caller
    ProbeAt pa;
    pa.i = (uint64_t)(g - rp.ch.pbase[c] + 1) * (uint64_t)rp.step;
    pa.s = rp.ch.start[c];
    pa.L = rp.ch.len[c];
    pa.md = rp.mode_of(c);
    return pa;
}
__device__ inline ProbeAt probe_at(const RunParams &rp, uint32_t g) { return probe_at(rp, chunk_of(rp.ch, g), g); }

// The text position whose position bit (RunParams::pbits) belongs to the probe: the first base its k-mer covers in the
// text.  Signed: the idle lanes of a staged tile may ask in front of the text.
__device__ inline long long probe_bit_pos(const ProbeAt &pa, int k) {
    return (pa.md & 2u) ? (long long)(pa.s + pa.L - pa.i) - k : (long long)(pa.s + pa.i);
}

// The hit filter of src/automaton.rs:105-114 -- which occurrences x of a probe's k-mer are kept -- as two numbers:
//     x is kept  <=>  x >= thr && x != self
// THIS is the definition every kernel filters by: two numbers travel from a row's owner lane to its wave in four lane
// reads, and a position-sorted list is bisected at thr.  A direct pass keeps x > i + s, which implies x != i: self = 0
// lies below every thr there (thr >= 1) and is never met.  A reversed pass keeps x >= s + L - i less the needle offset
// itself (`m.start != i`: a chunk offset compared with a text position, as the reference does).
struct HitRule {
    unsigned long long thr, self;
    __host__ __device__ inline bool keeps(unsigned long long x) const { return x >= thr && x != self; }
};
__host__ __device__ inline HitRule hit_rule(uint64_t i, uint64_t s, uint64_t L, bool reverse) {
    HitRule h;
    h.thr = reverse ? s + L - i : i + s + 1u;
    h.self = reverse ? i : 0ull;
    return h;
}
__device__ inline HitRule hit_rule(const ProbeAt &pa) { return hit_rule(pa.i, pa.s, pa.L, (pa.md & 2u) != 0u); }

// Workgroup barrier for data exchanged through LDS only.  __syncthreads() also waits for the
// wave's outstanding GLOBAL stores (vmcnt(0)): one record written to HBM would stall every wave
// of the workgroup for a memory round trip at the next barrier.  The extension kernels never
// read back what they store to global memory, so their per-probe barriers only drain LDS traffic.
__device__ inline void lds_barrier() { __asm__ volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// Wave-uniform values the compiler cannot prove uniform (read from LDS, or a lane of a vector):
// forcing them into scalar registers keeps the per-probe bookkeeping and branches on the scalar
// unit instead of exec-masked vector code and LDS permutes.
__device__ inline uint32_t uni(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
__device__ inline unsigned long long uni(unsigned long long v) {
    return ((unsigned long long)uni((uint32_t)(v >> 32)) << 32) | uni((uint32_t)v);
}
__device__ inline uint32_t lane_of(uint32_t v, uint32_t l) {
    return (uint32_t)__builtin_amdgcn_readlane((int)v, (int)l);
}
__device__ inline unsigned long long lane_of(unsigned long long v, uint32_t l) {
    return ((unsigned long long)lane_of((uint32_t)(v >> 32), l) << 32) | lane_of((uint32_t)v, l);
}
__device__ inline uint32_t lane_get(uint32_t v, uint32_t l) {  // lane l's v, l per lane (every lane takes part)
    return (uint32_t)__builtin_amdgcn_ds_bpermute((int)(l << 2), (int)v);
}
__device__ inline unsigned long long lane_get(unsigned long long v, uint32_t l) {
    return ((unsigned long long)lane_get((uint32_t)(v >> 32), l) << 32) | lane_get((uint32_t)v, l);
}
// a row's hit filter, from its owner lane to the wave
__device__ inline HitRule lane_of(const HitRule &h, uint32_t l) { return HitRule{lane_of(h.thr, l), lane_of(h.self, l)}; }
__device__ inline HitRule lane_get(const HitRule &h, uint32_t l) { return HitRule{lane_get(h.thr, l), lane_get(h.self, l)}; }
__device__ inline void wave_lds_sync() {  // LDS traffic of ONE wave: what its lanes wrote is there for its other lanes
    __builtin_amdgcn_wave_barrier();
    __asm__ volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
}

// inclusive prefix sum across the 64 lanes of a wave (gfx9 DPP: row shifts + row broadcasts)
__device__ inline uint32_t wave_incl_scan(uint32_t x) {
#define ASGART_DPP_ADD(ctrl, rows) \
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, ctrl, rows, 0xf, false)
    ASGART_DPP_ADD(0x111, 0xf);  // row_shr:1
    ASGART_DPP_ADD(0x112, 0xf);  // row_shr:2
    ASGART_DPP_ADD(0x114, 0xf);  // row_shr:4
    ASGART_DPP_ADD(0x118, 0xf);  // row_shr:8
    ASGART_DPP_ADD(0x142, 0xa);  // row_bcast:15 -> rows 1, 3
    ASGART_DPP_ADD(0x143, 0xc);  // row_bcast:31 -> rows 2, 3
#undef ASGART_DPP_ADD
    return x;
}

// inclusive running maximum across the 64 lanes of a wave (values >= 0: lanes without a source contribute 0)
__device__ inline uint32_t wave_incl_max_scan(uint32_t x) {
#define ASGART_DPP_MAX(ctrl, rows) \
    x = max(x, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, ctrl, rows, 0xf, false))
    ASGART_DPP_MAX(0x111, 0xf);  // row_shr:1
    ASGART_DPP_MAX(0x112, 0xf);  // row_shr:2
    ASGART_DPP_MAX(0x114, 0xf);  // row_shr:4
    ASGART_DPP_MAX(0x118, 0xf);  // row_shr:8
    ASGART_DPP_MAX(0x142, 0xa);  // row_bcast:15 -> rows 1, 3
    ASGART_DPP_MAX(0x143, 0xc);  // row_bcast:31 -> rows 2, 3
#undef ASGART_DPP_MAX
    return x;
}

}  // namespace asgart
