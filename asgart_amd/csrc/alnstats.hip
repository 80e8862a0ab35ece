// alnstats.hip -- the counts every duplication catalogue is read by, taken on the GPU from the runs of an alignment and
// the text of the index: asgart_alignment_stats, the counterpart of align.stats_host for a caller of the C ABI.
//
// What is counted is stated once, in include/asgart_hip.h; the pieces are in alnstats_dev.hpp.  The work is over runs and
// over bases, never over the runs or the bases of a row:
//   runs      one thread per run: its duplication by bisection of the run offsets; for a duplication with status 1 the two
//             checks of a run (paf_dev.hpp's codes, ONE atomic minimum names the lowest offending duplication), its bases
//             on either arm and its `X` bases.  The run's share of the eight counts that look at no base is reduced over
//             the lanes of the wave that hold runs of the same duplication (alnstats_dev.hpp: row_sum, row_max), and the
//             lane that opens the duplication's part of the wave adds it: one atomic per count that is not 0, per
//             duplication and wave;
//   scans     three 64-bit exclusive scans over the runs (rocPRIM): I and J, paf_dev.hpp's arm offsets, and X, the number
//             of mismatch bases in front of a run;
//   rows      one thread per duplication, a constant of work: the runs of a duplication with status 1 must consume exactly
//             its two arms (differences of I and J).  The host reads the atomic minimum back; a refused call ends here,
//             before a byte of the text is read, so the bases kernel forms no address outside an arm;
//   bases     mismatch base k of all X[n_runs] finds its run by bisection of X and its duplication by bisection of the run
//             offsets, both inside the few runs and duplications its workgroup's kBases bases span (found once per
//             workgroup).  Neighbouring lanes take neighbouring k: neighbouring bases of a run, neighbouring bytes of the
//             text (descending ones of a reversed right arm).  A wave owns kBases / 4 consecutive k, 64 at a time; the
//             lanes' kinds are two ballots, and the lane that opens a duplication's part of the wave adds the two
//             popcounts of its part.  A wave whose bases all belong to one duplication -- every wave of a long run --
//             keeps the two sums in scalars and adds them once: one atomic per count, duplication and wave; a wave that
//             crosses a duplication's end adds per 64 bases.
// Everything is integer: the counts do not depend on the order the atomics arrive in.
// kBases = 1024: four bases a lane, so that the workgroup's two bisections of the whole arrays are paid once per 1024
// bases and a wave's atomics once per 256.  A design constant, reasoned and not measured: no sweep was run.
#include "index.hpp"
#include "tool_base.hpp"
#include "alnstats_dev.hpp"

namespace asgart {
namespace {

constexpr uint32_t kThreads = 256;   // per workgroup of both kernels
constexpr uint32_t kBases = 1024;    // mismatch bases per workgroup of the bases kernel
constexpr uint32_t kWaveBases = kBases / (kThreads / 64);
static_assert(kWaveBases % 64 == 0, "a wave takes its bases 64 at a time");

__device__ __forceinline__ void add_u64(uint64_t *p, uint64_t v) {
    if (v) atomicAdd((unsigned long long *)p, (unsigned long long)v);
}
__device__ __forceinline__ void max_u64(uint64_t *p, uint64_t v) {
    if (v) atomicMax((unsigned long long *)p, (unsigned long long)v);
}

__global__ __launch_bounds__(kThreads) void alnstats_runs_kernel(AlnStatsIn in) {
    const uint64_t t = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    const uint32_t lane = __lane_id();
    const bool is_run = t < in.n_runs;
    // (the lanes behind the last run keep a row no run has, so that the rows still never decrease along the wave)
    const uint32_t q = is_run ? row_of_run(in.run_off, 0, (uint64_t)in.n_sd + 1, t) : 0xFFFFFFFFu;
    const bool counted = is_run && in.status[q] == 1;
    uint32_t len = 0;
    uint8_t op = 0;
    if (counted) {
        len = in.run_len[t];
        op = in.run_op[t];
        if (!run_op_known(op) || len == 0) {
            atomicMin((unsigned long long *)in.bad,
                      (unsigned long long)((uint64_t)q << 2 | (run_op_known(op) ? kPafBadLen : kPafBadOp)));
            len = 0;
            op = 0;
        }
    }
    if (t <= in.n_runs) {   // (t == n_runs: the closing entry, the scans end in the totals)
        in.I[t] = op ? run_on_left(op, len) : 0;
        in.J[t] = op ? run_on_right(op, len) : 0;
        in.X[t] = op == 'X' ? len : 0;
    }
    const uint32_t below = __shfl_up(q, 1);
    const bool opens = lane == 0 || below != q;
    const uint32_t end = row_end_lane(__ballot(opens), lane);
    if (__ballot(counted) == 0) return;   // (the same in every lane)
    const bool gap = op == 'I' || op == 'D';
    const uint64_t match = row_sum(op == '=' ? len : 0, lane, end), mismatch = row_sum(op == 'X' ? len : 0, lane, end);
    const uint64_t ins = row_sum(op == 'I' ? len : 0, lane, end), del = row_sum(op == 'D' ? len : 0, lane, end);
    const uint32_t longest_match = row_max(op == '=' ? len : 0, lane, end), longest_gap = row_max(gap ? len : 0, lane, end);
    const unsigned long long ins_mask = __ballot(op == 'I'), del_mask = __ballot(op == 'D');
    if (opens && counted) {
        const unsigned long long mine = lanes_from_to(lane, end);
        uint64_t *c = in.counts + (size_t)q * kAlnCounts;
        add_u64(c + kAlnMatch, match);
        add_u64(c + kAlnMismatch, mismatch);
        add_u64(c + kAlnInsRuns, (uint64_t)__popcll(ins_mask & mine));
        add_u64(c + kAlnInsBases, ins);
        add_u64(c + kAlnDelRuns, (uint64_t)__popcll(del_mask & mine));
        add_u64(c + kAlnDelBases, del);
        max_u64(c + kAlnLongestMatch, longest_match);
        max_u64(c + kAlnLongestGap, longest_gap);
    }
}

__global__ __launch_bounds__(kThreads) void alnstats_rows_kernel(AlnStatsIn in) {
    const uint32_t q = blockIdx.x * kThreads + threadIdx.x;
    if (q >= in.n_sd || in.status[q] != 1) return;
    const uint64_t b = in.run_off[q], e = in.run_off[q + 1];
    if (in.I[e] - in.I[b] != in.sds[4 * (size_t)q + 2] || in.J[e] - in.J[b] != in.sds[4 * (size_t)q + 3])
        atomicMin((unsigned long long *)in.bad, (unsigned long long)((uint64_t)q << 2 | kPafBadSums));
}

__global__ __launch_bounds__(kThreads) void alnstats_bases_kernel(AlnStatsIn in, uint64_t n_bases) {
    const uint32_t lane = __lane_id(), wave = threadIdx.x >> 6;
    // the runs and the duplications of the workgroup's first and last base: every bisection below stays between them
    const uint64_t g0 = (uint64_t)blockIdx.x * kBases, g1 = min(g0 + kBases, n_bases);
    const uint64_t t_lo = first_above(in.X, 0, in.n_runs + 1, g0) - 1, t_hi = first_above(in.X, t_lo, in.n_runs + 1, g1 - 1);
    const uint64_t q_lo = row_of_run(in.run_off, 0, (uint64_t)in.n_sd + 1, t_lo);
    const uint64_t q_hi = first_above(in.run_off, q_lo, (uint64_t)in.n_sd + 1, t_hi - 1);
    const uint64_t w0 = g0 + (uint64_t)wave * kWaveBases, w1 = min(w0 + kWaveBases, g1);
    if (w0 >= w1) return;   // (the same in every lane of the wave)
    const uint32_t q_first = row_of_run(in.run_off, q_lo, q_hi, first_above(in.X, t_lo, t_hi, w0) - 1);
    const uint32_t q_last = row_of_run(in.run_off, q_lo, q_hi, first_above(in.X, t_lo, t_hi, w1 - 1) - 1);
    const bool one_row = __builtin_amdgcn_readfirstlane((int)(q_first == q_last)) != 0;
    uint32_t n_ts = 0, n_tv = 0;   // (one_row: the wave's sums, the same in every lane)
    for (uint64_t k0 = w0; k0 < w1; k0 += 64) {
        const uint64_t k = k0 + lane;
        const bool is_base = k < w1;
        uint32_t q = 0xFFFFFFFFu, kind = 0;
        if (is_base) {
            const uint64_t t = first_above(in.X, t_lo, t_hi, k) - 1;
            q = one_row ? q_first : row_of_run(in.run_off, q_lo, q_hi, t);
            kind = kind_of_base(in, q, t, k - in.X[t]);
        }
        const unsigned long long ts = __ballot(kind == 1), tv = __ballot(kind == 2);
        if (one_row) {
            n_ts += (uint32_t)__popcll(ts);
            n_tv += (uint32_t)__popcll(tv);
            continue;
        }
        const uint32_t below = __shfl_up(q, 1);
        const bool opens = lane == 0 || below != q;
        const uint32_t end = row_end_lane(__ballot(opens), lane);
        if (opens && is_base) {
            const unsigned long long mine = lanes_from_to(lane, end);
            add_u64(in.counts + (size_t)q * kAlnCounts + kAlnTransition, (uint64_t)__popcll(ts & mine));
            add_u64(in.counts + (size_t)q * kAlnCounts + kAlnTransversion, (uint64_t)__popcll(tv & mine));
        }
    }
    if (one_row && lane == 0) {
        add_u64(in.counts + (size_t)q_first * kAlnCounts + kAlnTransition, n_ts);
        add_u64(in.counts + (size_t)q_first * kAlnCounts + kAlnTransversion, n_tv);
    }
}

struct StatsWork : ToolWork {
    DevBuf &sds = buf(), &flags = buf(), &status = buf(), &run_off = buf(), &run_len = buf(), &run_op = buf(), &I = buf(),
           &J = buf(), &X = buf(), &SI = buf(), &SJ = buf(), &SX = buf(), &tail = buf(), &counts = buf();
};

const char kWho[] = "asgart_alignment_stats";

int32_t run_stats(StatsWork &w, const uint8_t *text, const asgart_proto_sd *sds, const uint8_t *flags, const uint8_t *status,
                  uint32_t n, const uint64_t *run_offsets, const uint32_t *run_len, const uint8_t *run_op,
                  asgart_align_counts *counts, double *ms3) {
    const uint64_t n_runs = run_offsets[n];
    RC_TRY(w.open(4));
    hipStream_t s = w.s;
    HIP_TRY(hipEventRecord(w.ev[0], s));
    RC_TRY(w.upload(w.sds, sds, (size_t)n * sizeof(asgart_proto_sd)));
    RC_TRY(w.upload(w.flags, flags, n));
    RC_TRY(w.upload(w.status, status, n));
    RC_TRY(w.upload(w.run_off, run_offsets, ((size_t)n + 1) * 8));
    RC_TRY(w.upload(w.run_len, run_len, (size_t)n_runs * 4));
    RC_TRY(w.upload(w.run_op, run_op, (size_t)n_runs));
    HIP_TRY(hipEventRecord(w.ev[1], s));
    for (DevBuf *b : {&w.I, &w.J, &w.X, &w.SI, &w.SJ, &w.SX}) RC_TRY(b->reserve(((size_t)n_runs + 1) * 8));
    RC_TRY(w.tail.reserve(16));
    RC_TRY(w.counts.reserve((size_t)n * sizeof(asgart_align_counts)));
    HIP_TRY(hipMemsetAsync(w.tail.p, 0xff, 8, s));
    HIP_TRY(hipMemsetAsync(w.counts.p, 0, (size_t)n * sizeof(asgart_align_counts), s));
    AlnStatsIn in{};
    in.sds = w.sds.as<uint64_t>();
    in.flags = w.flags.as<uint8_t>();
    in.status = w.status.as<uint8_t>();
    in.run_off = w.run_off.as<uint64_t>();
    in.run_len = w.run_len.as<uint32_t>();
    in.run_op = w.run_op.as<uint8_t>();
    in.text = text;
    in.I = w.I.as<uint64_t>();
    in.J = w.J.as<uint64_t>();
    in.X = w.X.as<uint64_t>();
    in.bad = w.tail.as<uint64_t>();
    in.counts = w.counts.as<uint64_t>();
    in.n_sd = n;
    in.n_runs = n_runs;
    alnstats_runs_kernel<<<blocks_for(n_runs + 1, kThreads), kThreads, 0, s>>>(in);
    HIP_TRY(hipGetLastError());
    RC_TRY(w.exclusive_scan(w.I.as<uint64_t>(), w.SI.as<uint64_t>(), (size_t)n_runs + 1));
    RC_TRY(w.exclusive_scan(w.J.as<uint64_t>(), w.SJ.as<uint64_t>(), (size_t)n_runs + 1));
    RC_TRY(w.exclusive_scan(w.X.as<uint64_t>(), w.SX.as<uint64_t>(), (size_t)n_runs + 1));
    in.I = w.SI.as<uint64_t>();
    in.J = w.SJ.as<uint64_t>();
    in.X = w.SX.as<uint64_t>();
    alnstats_rows_kernel<<<blocks_for(n, kThreads), kThreads, 0, s>>>(in);
    HIP_TRY(hipGetLastError());
    // the lowest refused duplication and, behind it, the number of mismatch bases, in one copy
    HIP_TRY(hipMemcpyAsync(in.bad + 1, in.X + n_runs, 8, hipMemcpyDeviceToDevice, s));
    uint64_t tail[2] = {0, 0};
    HIP_TRY(read_back(tail, in.bad, 16, s));
    if (tail[0] != ~(uint64_t)0) return refuse_runs(kWho, tail[0], sds, run_offsets, run_len, run_op);
    HIP_TRY(hipEventRecord(w.ev[2], s));
    if (tail[1]) {
        alnstats_bases_kernel<<<blocks_for(tail[1], kBases), kThreads, 0, s>>>(in, tail[1]);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipEventRecord(w.ev[3], s));
    HIP_TRY(stream_sync(s));
    const auto t0 = std::chrono::steady_clock::now();
    HIP_TRY(read_back(counts, w.counts.p, (size_t)n * sizeof(asgart_align_counts), s));
    if (ms3) {
        float up = 0, a = 0, b = 0;
        HIP_TRY(hipEventElapsedTime(&up, w.ev[0], w.ev[1]));
        HIP_TRY(hipEventElapsedTime(&a, w.ev[1], w.ev[2]));
        HIP_TRY(hipEventElapsedTime(&b, w.ev[2], w.ev[3]));
        ms3[0] = up;
        ms3[1] = (double)a + (double)b;
        ms3[2] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
    return 0;
}

}  // namespace
}  // namespace asgart

using namespace asgart;

static_assert(sizeof(asgart_align_counts) == kAlnCounts * 8, "ten u64 counts, in alnstats_dev.hpp's order");

extern "C" int32_t asgart_alignment_stats(asgart_index *idx, const asgart_proto_sd *sds, const uint8_t *flags,
                                          const uint8_t *status, int64_t n_sd, const uint64_t *run_offsets,
                                          const uint32_t *run_len, const uint8_t *run_op, asgart_align_counts *counts,
                                          double *ms3) {
    RC_TRY(check_alignment_arguments(kWho, idx, sds, flags, status, n_sd, run_offsets, run_len, run_op, counts));
    REFUSE_POISONED(idx);
    RC_TRY(use_device(kWho, idx->device));
    if (ms3) ms3[0] = ms3[1] = ms3[2] = 0;
    if (n_sd == 0) return 0;
    StatsWork w;
    return run_stats(w, idx->d_text, sds, flags, status, (uint32_t)n_sd, run_offsets, run_len, run_op, counts, ms3);
}

extern "C" void asgart_alignment_stats_geometry(uint64_t *block_threads, uint64_t *bases_per_block) {
    if (block_threads) *block_threads = kThreads;
    if (bases_per_block) *bases_per_block = kBases;
}
