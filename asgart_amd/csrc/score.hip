// score.hip -- ComputeScore on the GPU: exact Levenshtein identity of the two arms of each
// duplication (reference `--compute-score`: src/bin/asgart.rs:98-112, ProtoSD::levenshtein
// src/structs.rs:439-452, bio::alignment::distance::levenshtein = unit-cost global edit distance).
//
// One WAVEFRONT per duplication, systolic dynamic programming: lane l owns R consecutive rows of the
// DP matrix (the left arm) in registers and walks the columns (the right arm) one step behind lane
// l-1, so a step computes 64 x R cells with two cross-lane moves (the value above the lane's first
// row and the column's base travel down the lanes) and no barrier or LDS traffic.  Arms longer than
// 64 x R rows are processed in bands; the bottom row of a band is the top boundary of the next and
// goes through an HBM scratch row, read and written 64 columns at a time.  Long duplications get a
// workgroup of 16 waves that walk 16 consecutive bands as a pipeline (see levenshtein_long_kernel).  Integer work, bit-exact by
// construction; the identity is formed in f64 like the reference and narrowed to f32.
// The right arm, its orientation, the identity and the host's checks of a list are in lev_dev.hpp, shared with align.hip.
// That header also states the step below once, for align.hip's two kernels.  The two score kernels keep their own text of
// it: built on the header's helpers the score call measured 1.0 - 1.5 % slower, outside the parent's spread, although
// band_steps' loop came out instruction for instruction as before (levenshtein_kernel's, at 95 VGPRs for 93, was not
// compared; DESIGN_HISTORY.md).
// The orientation of the right arm is per duplication (asgart_compute_scores_flags*: one flag byte each) or per call
// (asgart_compute_scores*: the same kernels without a flag array).
#include "index.hpp"
#include "lev_dev.hpp"

#include <algorithm>
#include <functional>
#include <new>
#include <queue>
#include <string>
#include <thread>
#include <utility>
#include <vector>

namespace asgart {
namespace {

constexpr int kScoreThreads = 256;  // four duplications per workgroup
constexpr int kScoreRows = 16;      // rows per lane
constexpr uint32_t kBand = 64u * kScoreRows;  // rows of one band (a wave's 64 lanes)
// (lev_dev.hpp states the same geometry for align.hip)
static_assert(kScoreRows == kLevRows && kBand == kLevBand, "score.hip and lev_dev.hpp disagree on the band");
constexpr int kLongWaves = 16;                // waves of levenshtein_long_kernel's workgroup ...
constexpr int kLongRows = kLongWaves + 2;     // ... and the boundary rows it has in flight
// A duplication whose left arm has at least half a workgroup's bands goes to levenshtein_long_kernel, the rest to
// levenshtein_kernel.  The dispatch (score_plan) and the cost model of the shards (score_cost) both read these.
constexpr uint64_t kLongMinRows = (uint64_t)kBand * kLongWaves / 2u;

__host__ __device__ inline bool score_is_long(uint64_t left_length) { return left_length + 1u >= kLongMinRows; }

// steps per chunk of levenshtein_long_kernel for a right arm of n_steps - 63 bases: at most 2 kLongWaves chunks per band,
// and >= 128 steps (a band's bottom row is stored 64 columns at a time, 62 steps late)
__host__ __device__ inline uint32_t long_chunk_steps(uint64_t n_steps) {
    uint32_t C = (uint32_t)((n_steps + 2u * kLongWaves - 1u) / (2u * kLongWaves));
    C = (C + 63u) & ~63u;
    return C > 128u ? C : 128u;
}

// one lane's share of a band of 64 x R rows
struct BandState {
    uint32_t a[kScoreRows], col[kScoreRows];
    uint32_t diag_in;    // D[i0][j-1] for the lane's next column
    uint32_t last_out;   // D[i0+R][j] of the column just done
    uint32_t b_pipe;     // base of the lane's current column (travels down the lanes)
    uint32_t top_chunk, b_chunk, out_chunk;
};

__device__ inline void band_init(BandState &st, uint32_t band, int lane, uint32_t la, const uint8_t *A) {
    constexpr int R = kScoreRows;
    const uint32_t i0 = band + (uint32_t)lane * R;  // rows i0+1 .. i0+R (1-based) are this lane's
#pragma unroll
    for (int r = 0; r < R; ++r) {
        st.a[r] = i0 + r < la ? (uint32_t)A[i0 + r] : 0x100u;  // padding rows match nothing
        st.col[r] = i0 + r + 1u;                               // D[i][0] = i
    }
    st.diag_in = i0;
    st.last_out = st.b_pipe = st.top_chunk = st.b_chunk = st.out_chunk = 0;
}

// steps [s_lo, s_hi) of a band (s_lo a multiple of 64); lane l works on column s - l + 1
__device__ inline void band_steps(BandState &st, uint32_t s_lo, uint32_t s_hi, uint32_t band, int lane, uint32_t la,
                                  const RightArm &rb, const uint32_t *top_row, uint32_t *bottom_row,
                                  uint32_t &result) {
    constexpr int R = kScoreRows;
    const uint32_t lb = rb.lb;
    const uint32_t i0 = band + (uint32_t)lane * R;
    const bool more_bands = band + 64u * R < la;
    for (uint32_t s = s_lo; s < s_hi; ++s) {
        if ((s & 63u) == 0u) {  // 64 columns of the top boundary and of the right arm at a time
            const uint32_t j1 = s + 1u + (uint32_t)lane;  // column of lane 0 at step s + lane
            // (the boundary row was written by this or another wave of the workgroup: read past the L1)
            st.top_chunk = band == 0 ? j1 : (j1 <= lb ? __atomic_load_n(&top_row[j1], __ATOMIC_RELAXED) : 0u);
            st.b_chunk = s + (uint32_t)lane < lb ? rb.at(s + (uint32_t)lane) : 0u;
        }
        // the value above the lane's first row, D[i0][j]: lane l-1 finished column j one step ago
        uint32_t up_in = __shfl_up(st.last_out, 1);
        const uint32_t top0 = __shfl(st.top_chunk, (int)(s & 63u));
        uint32_t b_in = __shfl_up(st.b_pipe, 1);
        const uint32_t b0 = __shfl(st.b_chunk, (int)(s & 63u));
        if (lane == 0) {
            up_in = top0;
            b_in = b0;
        }
        st.b_pipe = b_in;
        const int64_t j = (int64_t)s - lane + 1;
        if (j >= 1 && j <= (int64_t)lb) {
            uint32_t up = up_in, diag = st.diag_in;
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const uint32_t left = st.col[r];
                const uint32_t v = min(diag + (st.a[r] != b_in ? 1u : 0u), min(up, left) + 1u);
                diag = left;
                up = v;
                st.col[r] = v;
            }
            st.diag_in = up_in;
            st.last_out = st.col[R - 1];
            if ((uint32_t)j == lb && la > i0 && la <= i0 + R) {
                uint32_t v = 0;
#pragma unroll
                for (int r = 0; r < R; ++r)
                    if (i0 + r + 1u == la) v = st.col[r];
                result = v;
            }
        }
        if (more_bands) {
            // lane 63 finishes column jo = s - 62; collect 64 of them, store them together
            const uint32_t v63 = __shfl(st.last_out, 63);
            const int64_t jo = (int64_t)s - 62;
            if (jo >= 1 && jo <= (int64_t)lb) {
                if ((uint32_t)lane == ((uint32_t)jo & 63u)) st.out_chunk = v63;
                if (((uint32_t)jo & 63u) == 63u || (uint32_t)jo == lb) {
                    const uint32_t jw = ((uint32_t)jo & ~63u) + (uint32_t)lane;
                    if (jw >= 1u && jw <= (uint32_t)jo) bottom_row[jw] = st.out_chunk;
                }
            }
        }
    }
}

// ---- one wave per duplication: the bulk (the band loop written out: the shared band_steps form of
// this kernel hung on gfx950 with ROCm 7.2 although the multi-wave kernel below runs the same code) ---
__global__ __launch_bounds__(kScoreThreads) void levenshtein_kernel(const uint8_t *__restrict__ text,
                                                                    const asgart_proto_sd *__restrict__ sds,
                                                                    const uint32_t *__restrict__ list, uint64_t n_list,
                                                                    const uint8_t *__restrict__ flags, int reversed0,
                                                                    int complemented0,
                                                                    uint32_t *__restrict__ scratch, uint64_t scratch_stride,
                                                                    unsigned long long *__restrict__ cursor,
                                                                    float *__restrict__ identity) {
    constexpr int R = kScoreRows;
    const int lane = threadIdx.x & 63;
    const uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    uint32_t *row_a = scratch + wave * 2u * scratch_stride, *row_b = row_a + scratch_stride;
    for (;;) {
        unsigned long long pos = 0;
        if (lane == 0) pos = atomicAdd(cursor, 1ull);
        pos = __shfl(pos, 0);
        if (pos >= n_list) break;
        const uint32_t item = list[pos];
        const asgart_proto_sd sd = sds[item];
        // inclusive ranges [p ..= p + len] (src/structs.rs:441-442): len + 1 bases each
        const uint32_t la = (uint32_t)sd.left_length + 1u, lb = (uint32_t)sd.right_length + 1u;
        const uint8_t *A = text + sd.left;
        const uint8_t *B = text + sd.right;
        const uint32_t orient = orientation_of(flags, item, reversed0, complemented0);
        const bool reversed = orient & 1u, complemented = orient & 2u;
        auto b_at = [&](uint32_t j) -> uint32_t {  // j-th base of the right arm after reverse/complement
            const uint32_t c = B[reversed ? lb - 1u - j : j];
            return complemented ? complement_base(c) : c;
        };
        uint32_t result = 0;
        uint32_t *top_row = row_a, *bottom_row = row_b;
        for (uint32_t band = 0; band < la; band += 64u * R) {
            const uint32_t i0 = band + (uint32_t)lane * R;  // rows i0+1 .. i0+R (1-based) are this lane's
            const bool more_bands = band + 64u * R < la;
            uint32_t a[R], col[R];
#pragma unroll
            for (int r = 0; r < R; ++r) {
                a[r] = i0 + r < la ? (uint32_t)A[i0 + r] : 0x100u;  // padding rows match nothing
                col[r] = i0 + r + 1u;                               // D[i][0] = i
            }
            uint32_t diag_in = i0;       // D[i0][j-1] for the lane's next column
            uint32_t last_out = 0;       // D[i0+R][j] of the column just done
            uint32_t b_pipe = 0;         // base of the lane's current column (travels down the lanes)
            uint32_t top_chunk = 0, b_chunk = 0, out_chunk = 0;
            const uint32_t n_steps = lb + 63u;
            for (uint32_t s = 0; s < n_steps; ++s) {
                if ((s & 63u) == 0u) {  // 64 columns of the top boundary and of the right arm at a time
                    const uint32_t j1 = s + 1u + (uint32_t)lane;  // column of lane 0 at step s + lane
                    // (written by this wave one band ago: read past the vector L1)
                    top_chunk = band == 0 ? j1 : (j1 <= lb ? __atomic_load_n(&top_row[j1], __ATOMIC_RELAXED) : 0u);
                    b_chunk = s + (uint32_t)lane < lb ? b_at(s + (uint32_t)lane) : 0u;
                }
                // the value above the lane's first row, D[i0][j]: lane l-1 finished column j one step ago
                uint32_t up_in = __shfl_up(last_out, 1);
                const uint32_t top0 = __shfl(top_chunk, (int)(s & 63u));
                uint32_t b_in = __shfl_up(b_pipe, 1);
                const uint32_t b0 = __shfl(b_chunk, (int)(s & 63u));
                if (lane == 0) {
                    up_in = top0;
                    b_in = b0;
                }
                b_pipe = b_in;
                const int64_t j = (int64_t)s - lane + 1;
                if (j >= 1 && j <= (int64_t)lb) {
                    uint32_t up = up_in, diag = diag_in;
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        const uint32_t left = col[r];
                        const uint32_t v = min(diag + (a[r] != b_in ? 1u : 0u), min(up, left) + 1u);
                        diag = left;
                        up = v;
                        col[r] = v;
                    }
                    diag_in = up_in;
                    last_out = col[R - 1];
                    if ((uint32_t)j == lb && la > i0 && la <= i0 + R) {
                        uint32_t v = 0;
#pragma unroll
                        for (int r = 0; r < R; ++r)
                            if (i0 + r + 1u == la) v = col[r];
                        result = v;
                    }
                }
                if (more_bands) {
                    // lane 63 finishes column jo = s - 62; collect 64 of them, store them together
                    const uint32_t v63 = __shfl(last_out, 63);
                    const int64_t jo = (int64_t)s - 62;
                    if (jo >= 1 && jo <= (int64_t)lb) {
                        if ((uint32_t)lane == ((uint32_t)jo & 63u)) out_chunk = v63;
                        if (((uint32_t)jo & 63u) == 63u || (uint32_t)jo == lb) {
                            const uint32_t jbase = (uint32_t)jo & ~63u;
                            const uint32_t jw = jbase + (uint32_t)lane;
                            if (jw >= 1u && jw <= (uint32_t)jo) bottom_row[jw] = out_chunk;
                        }
                    }
                }
            }
            // the next band reads what this one wrote (same wave: program order; make it visible)
            __threadfence_block();
            uint32_t *t = top_row; top_row = bottom_row; bottom_row = t;
        }
        // the lane that holds row la has the distance
        const uint32_t owner = ((la - 1u) % (64u * R)) / R;  // lane of row la in the last band
        const uint32_t dist = __shfl(result, (int)owner);
        if (lane == 0) {
            const uint64_t longest = sd.left_length > sd.right_length ? sd.left_length : sd.right_length;
            identity[item] = (float)(100.0 * (1.0 - (double)dist / (double)longest));
        }
    }
}


// ---- one workgroup of kLongWaves waves per LONG duplication -----------------------------------------
// Band b is walked by wave b mod kLongWaves in chunks of C steps; a workgroup barrier separates the
// chunks and band b+1 runs two chunks behind band b (its top boundary is band b's bottom row, whose
// columns up to (c+1) C are complete after chunk c+1).  With at most 2 kLongWaves chunks per band a
// wave finishes band b exactly when band b + kLongWaves may start, so every wave stays busy.
__global__ __launch_bounds__(64 * kLongWaves) void levenshtein_long_kernel(
    const uint8_t *__restrict__ text, const asgart_proto_sd *__restrict__ sds, const uint32_t *__restrict__ list,
    uint64_t n_list, const uint8_t *__restrict__ flags, int reversed0, int complemented0, uint32_t *__restrict__ scratch,
    uint64_t scratch_stride, float *__restrict__ identity) {
    constexpr int R = kScoreRows;
    constexpr uint32_t BAND = kBand;
    __shared__ uint32_t s_dist;
    const int lane = threadIdx.x & 63;
    const uint32_t w = threadIdx.x >> 6;
    uint32_t *rows = scratch + (size_t)blockIdx.x * kLongRows * scratch_stride;
    for (uint64_t pos = blockIdx.x; pos < n_list; pos += gridDim.x) {
        const uint32_t item = list[pos];
        const asgart_proto_sd sd = sds[item];
        const uint32_t la = (uint32_t)sd.left_length + 1u, lb = (uint32_t)sd.right_length + 1u;
        const uint32_t orient = orientation_of(flags, item, reversed0, complemented0);
        const RightArm rb{text + sd.right, lb, (int)(orient & 1u), (int)(orient >> 1)};
        const uint32_t n_bands = (la + BAND - 1u) / BAND;
        const uint32_t n_steps = lb + 63u;
        const uint32_t C = long_chunk_steps(n_steps);
        const uint32_t n_chunks = (n_steps + C - 1u) / C;  // <= 2 kLongWaves
        const uint32_t n_super = 2u * (n_bands - 1u) + n_chunks;
        uint32_t result = 0;
        BandState st;
        for (uint32_t t = 0; t < n_super; ++t) {
            if (t >= 2u * w) {
                const uint32_t rel = t - 2u * w;
                const uint32_t m = rel / (2u * kLongWaves), c = rel % (2u * kLongWaves);
                const uint32_t b = w + m * kLongWaves;
                if (b < n_bands && c < n_chunks) {
                    const uint32_t band = b * BAND;
                    if (c == 0) band_init(st, band, lane, la, text + sd.left);
                    const uint32_t *top_row = rows + (size_t)((b + kLongRows - 1u) % kLongRows) * scratch_stride;
                    uint32_t *bottom_row = rows + (size_t)(b % kLongRows) * scratch_stride;
                    band_steps(st, c * C, min((c + 1u) * C, n_steps), band, lane, la, rb, top_row, bottom_row, result);
                }
            }
            __syncthreads();
        }
        // the wave and lane that hold row la have the distance
        const uint32_t last_band = n_bands - 1u;
        const uint32_t owner = ((la - 1u) % BAND) / R;
        if (w == last_band % kLongWaves && (uint32_t)lane == owner) s_dist = result;
        __syncthreads();
        if (threadIdx.x == 0) identity[item] = identity_of(sd, s_dist);
        __syncthreads();
    }
}

// ---- a shard of a ComputeScore call: its duplications gathered out of the full list, on the device --------------
// sub[k] = sds[owned[k]], with its flag byte when the call has flags (sub_flags[k] = flags[owned[k]]); the Levenshtein
// kernels then walk sub through list[k] = k and write identity[k].
__global__ __launch_bounds__(256) void gather_owned_kernel(const asgart_proto_sd *__restrict__ sds,
                                                           const uint8_t *__restrict__ flags,
                                                           const uint32_t *__restrict__ owned, uint64_t n_owned,
                                                           asgart_proto_sd *__restrict__ sub,
                                                           uint8_t *__restrict__ sub_flags, uint32_t *__restrict__ list) {
    for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n_owned; k += (uint64_t)gridDim.x * blockDim.x) {
        sub[k] = sds[owned[k]];
        if (flags) sub_flags[k] = flags[owned[k]];
        list[k] = (uint32_t)k;
    }
}

// What one duplication costs the device, in wave-steps (a step: one column of a band, 64 lanes x kScoreRows cells), the
// way the kernels dispatch it.  Short: one wave walks ceil(la / kBand) bands of lb + 63 steps.  Long: kLongWaves waves
// are held for the 2 (n_bands - 1) + n_chunks chunks of C steps of the band pipeline, its fill and drain included.
// Inclusive ranges: la = left_length + 1, lb = right_length + 1 (la x lb DP cells).
uint64_t score_cost(const asgart_proto_sd &sd) {
    const uint64_t la = sd.left_length + 1u, lb = sd.right_length + 1u;
    const uint64_t n_bands = (la + kBand - 1u) / kBand, n_steps = lb + 63u;
    if (!score_is_long(sd.left_length)) return n_bands * n_steps;
    const uint64_t C = long_chunk_steps(n_steps);
    const uint64_t n_chunks = (n_steps + C - 1u) / C;
    return (uint64_t)kLongWaves * (2u * (n_bands - 1u) + n_chunks) * C;
}

// Greedy longest first onto the least-loaded shard (ties: lower ordinal first, lower shard first).  Only the first
// min(n_shards, n_sd) shards can receive anything: the heap holds those.
void score_owners(const asgart_proto_sd *sds, int64_t n_sd, int32_t n_shards, int32_t *owner) {
    std::vector<uint64_t> cost((size_t)n_sd);
    std::vector<uint32_t> order((size_t)n_sd);
    for (int64_t q = 0; q < n_sd; ++q) {
        cost[(size_t)q] = score_cost(sds[q]);
        order[(size_t)q] = (uint32_t)q;
    }
    std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return cost[x] > cost[y]; });
    using Load = std::pair<unsigned __int128, int32_t>;
    std::priority_queue<Load, std::vector<Load>, std::greater<Load>> heap;
    const int64_t used = std::min<int64_t>(n_shards, n_sd);
    for (int32_t r = 0; r < (int32_t)used; ++r) heap.push(Load{0, r});
    for (uint32_t q : order) {
        Load l = heap.top();
        heap.pop();
        owner[q] = l.second;
        l.first += cost[q];
        heap.push(l);
    }
}

// The orientations of one call: a flag byte per duplication (bit 0 reversed, bit 1 complemented), or one pair for all.
struct Orientations {
    const uint8_t *flags;  // host, one per duplication of the call's list; NULL: the two constants below
    int32_t reversed, complemented;
};

// what every entry point checks of a non-empty list, the flag bytes first (the score's ranges are inclusive)
int32_t check_scores_input(const char *fn, const asgart_index *idx, const asgart_proto_sd *sds, int64_t n_sd,
                           const Orientations &o) {
    RC_TRY(check_flags(fn, o.flags, n_sd));
    return check_arms(fn, (uint64_t)idx->n, sds, n_sd, 1);
}

// Long duplications (many bands) get a whole workgroup each, the rest one wave each; both lists are served largest first.
struct ScorePlan {
    std::vector<uint32_t> long_list, wave_list;  // ordinals into the caller's sds
    uint64_t max_lb_long = 0, max_lb_wave = 0;   // longest right arm of each list (of the multi-band ones for wave_list)
    unsigned grid_w = 0, grid_l = 0;
    uint64_t stride_w = 0, stride_l = 0;
    size_t scratch_w = 0, scratch_l = 0;         // u32 entries
};

ScorePlan score_plan(const asgart_proto_sd *sds, std::vector<uint32_t> order) {
    ScorePlan p;
    auto cells = [&](uint32_t q) { return (double)(sds[q].left_length + 1u) * (double)(sds[q].right_length + 1u); };
    std::sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return cells(x) > cells(y); });
    for (uint32_t q : order) {
        const asgart_proto_sd &sd = sds[q];
        if (score_is_long(sd.left_length)) {
            p.long_list.push_back(q);
            p.max_lb_long = std::max<uint64_t>(p.max_lb_long, sd.right_length + 1u);
        } else {
            p.wave_list.push_back(q);
            if (sd.left_length + 1u > kBand) p.max_lb_wave = std::max<uint64_t>(p.max_lb_wave, sd.right_length + 1u);
        }
    }
    const unsigned waves_per_wg = kScoreThreads / 64;
    p.grid_w = (unsigned)std::min<size_t>((p.wave_list.size() + waves_per_wg - 1) / waves_per_wg, 512);
    p.grid_l = (unsigned)std::min<size_t>(p.long_list.size(), 256);
    p.stride_w = p.max_lb_wave ? p.max_lb_wave + 64u : 0u;
    p.stride_l = p.max_lb_long + 64u;
    p.scratch_w = (size_t)p.stride_w * 2u * p.grid_w * waves_per_wg;
    p.scratch_l = (size_t)p.stride_l * kLongRows * p.grid_l;
    return p;
}

int32_t score_reserve(Workspace &w, const ScorePlan &p) {
    RC_TRY(w.scratch.reserve((p.scratch_w + p.scratch_l) * 4u + 64));
    return w.counters.reserve(1024);  // the search pipeline keeps its device counters here too
}

// d_list: the plan's long list, then its wave list, as indices into d_sds (and into d_flags, the device copy of
// o.flags; NULL without); identities go to d_identity[d_list[..]]
int32_t score_launch(const asgart_index *idx, Workspace &w, hipStream_t s, const ScorePlan &p,
                     const asgart_proto_sd *d_sds, const uint32_t *d_list, const uint8_t *d_flags, const Orientations &o,
                     float *d_identity) {
    unsigned long long *cursor = w.counters.as<unsigned long long>();
    HIP_TRY(hipMemsetAsync(cursor, 0, 8, s));
    if (p.grid_l)
        levenshtein_long_kernel<<<p.grid_l, 64 * kLongWaves, 0, s>>>(
            idx->d_text, d_sds, d_list, (uint64_t)p.long_list.size(), d_flags, o.reversed != 0, o.complemented != 0,
            w.scratch.as<uint32_t>() + p.scratch_w, p.stride_l, d_identity);
    if (p.grid_w)
        levenshtein_kernel<<<p.grid_w, kScoreThreads, 0, s>>>(
            idx->d_text, d_sds, d_list + p.long_list.size(), (uint64_t)p.wave_list.size(), d_flags, o.reversed != 0,
            o.complemented != 0, w.scratch.as<uint32_t>(), p.stride_w, cursor, d_identity);
    HIP_TRY(hipGetLastError());
    return 0;
}

// the ordinals q with owner[q] == shard, ascending
std::vector<uint32_t> owned_by(const int32_t *owner, int64_t n_sd, int32_t shard) {
    std::vector<uint32_t> mine;
    for (int64_t q = 0; q < n_sd; ++q)
        if (owner[q] == shard) mine.push_back((uint32_t)q);
    return mine;
}

// Scores the duplications `mine` (distinct ordinals into sds) on one of idx's call contexts; writes identity[q] for those
// only.  Returns how many, < 0 on error.  The full list goes to the device once.  A part of it is gathered there; the whole
// list needs no gather: the kernels walk it where it lies and the identities are read back straight into the caller's array.
int64_t score_shard(asgart_index *idx, const asgart_proto_sd *sds, int64_t n_sd, std::vector<uint32_t> mine,
                    const Orientations &o, float *identity) {
    if (mine.empty()) return 0;
    REFUSE_POISONED(idx);
    HIP_TRY(hipSetDevice(idx->device));
    int which = 0;
    SearchCtx &cx = idx->acquire_one(&which);
    struct Unlock {
        asgart_index *i;
        int w;
        ~Unlock() { i->release_one(w); }
    } unlock{idx, which};
    Workspace &w = cx.ws;
    hipStream_t s = cx.stream;
    const ScorePlan p = score_plan(sds, std::move(mine));
    std::vector<uint32_t> owned(p.long_list);  // the schedule, as ordinals into the full list
    owned.insert(owned.end(), p.wave_list.begin(), p.wave_list.end());
    const size_t m = owned.size();
    const bool whole = m == (size_t)n_sd;
    // out_a = full list, then the gathered one; seg_vals = the kernels' list, then the ordinals to gather, then the flag
    // bytes of the full list and of the gathered one
    RC_TRY(w.out_a.reserve(((size_t)n_sd + (whole ? 0 : m)) * sizeof(asgart_proto_sd)));
    RC_TRY(w.seg_vals.reserve(m * 8 + (size_t)n_sd + m + 64));
    RC_TRY(w.out_b.reserve(m * sizeof(float) + 64));
    RC_TRY(score_reserve(w, p));
    const asgart_proto_sd *d_sds = w.out_a.as<asgart_proto_sd>();
    asgart_proto_sd *d_sub = w.out_a.as<asgart_proto_sd>() + n_sd;
    uint32_t *d_list = w.seg_vals.as<uint32_t>(), *d_owned = d_list + m;
    uint8_t *d_flags = o.flags ? (uint8_t *)(d_owned + m) : nullptr, *d_sub_flags = o.flags ? d_flags + n_sd : nullptr;
    HIP_TRY(hipMemcpyAsync(w.out_a.p, sds, (size_t)n_sd * sizeof(asgart_proto_sd), hipMemcpyHostToDevice, s));
    if (o.flags) HIP_TRY(hipMemcpyAsync(d_flags, o.flags, (size_t)n_sd, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(whole ? d_list : d_owned, owned.data(), m * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(stream_sync(s));  // (pageable host sources, `owned` among them: no copy is in flight at a return below)
    if (whole) {  // the schedule is the kernels' list, and identity[q] is entry q of what they write
        RC_TRY(score_launch(idx, w, s, p, d_sds, d_list, d_flags, o, w.out_b.as<float>()));
        HIP_TRY(read_back(identity, w.out_b.p, m * sizeof(float), s));
        return (int64_t)m;
    }
    const unsigned grid_g = (unsigned)std::min<size_t>((m + 255) / 256, 1024);
    gather_owned_kernel<<<grid_g, 256, 0, s>>>(d_sds, d_flags, d_owned, (uint64_t)m, d_sub, d_sub_flags, d_list);
    HIP_TRY(hipGetLastError());
    RC_TRY(score_launch(idx, w, s, p, d_sub, d_list, d_sub_flags, o, w.out_b.as<float>()));
    std::vector<float> got(m);
    HIP_TRY(read_back(got.data(), w.out_b.p, m * sizeof(float), s));
    for (size_t k = 0; k < m; ++k) identity[owned[k]] = got[k];
    return (int64_t)m;
}

int32_t check_shard_args(const char *fn, const asgart_proto_sd *sds, int64_t n_sd, int32_t n_shards, const void *out) {
    RC_TRY(check_list_pointers(fn, sds, n_sd, out));
    if (n_shards < 1) {
        set_error("%s: %d shards (at least 1)", fn, n_shards);
        return ASGART_E_ARG;
    }
    RC_TRY(check_list_count(fn, n_sd));
    for (int64_t q = 0; q < n_sd; ++q)  // (before the bounds of any duplication: the cost model needs no text)
        if (arms_too_long(sds[q])) {
            set_error("%s: arms of 2^32 bases are not supported", fn);
            return ASGART_E_CAP;
        }
    return 0;
}

// asgart_compute_scores[_flags]: the whole list on one call context
int32_t score_all(const char *fn, asgart_index *idx, const asgart_proto_sd *sds, int64_t n_sd, const Orientations &o,
                  float *identity) {
    if (!idx) {
        set_error("%s: bad argument", fn);
        return ASGART_E_ARG;
    }
    RC_TRY(check_list_pointers(fn, sds, n_sd, identity));
    if (n_sd == 0) return 0;
    RC_TRY(check_scores_input(fn, idx, sds, n_sd, o));
    try {
        std::vector<uint32_t> all((size_t)n_sd);
        for (int64_t q = 0; q < n_sd; ++q) all[(size_t)q] = (uint32_t)q;
        const int64_t rc = score_shard(idx, sds, n_sd, std::move(all), o, identity);
        return rc < 0 ? (int32_t)rc : 0;
    } catch (const std::bad_alloc &) {
        set_error("%s: out of host memory", fn);
        return ASGART_E_OOM;
    }
}

}  // namespace
}  // namespace asgart

extern "C" int32_t asgart_compute_scores(asgart_index *idx, const asgart_proto_sd *sds, int64_t n_sd,
                                         int32_t reversed, int32_t complemented, float *identity) {
    return asgart::score_all("asgart_compute_scores", idx, sds, n_sd, {nullptr, reversed, complemented}, identity);
}

extern "C" int32_t asgart_compute_scores_flags(asgart_index *idx, const asgart_proto_sd *sds, const uint8_t *flags,
                                               int64_t n_sd, float *identity) {
    return asgart::score_all("asgart_compute_scores_flags", idx, sds, n_sd, {flags, 0, 0}, identity);
}

extern "C" int32_t asgart_score_costs(const asgart_proto_sd *sds, int64_t n_sd, uint64_t *cost) {
    using namespace asgart;
    RC_TRY(check_shard_args("asgart_score_costs", sds, n_sd, 1, cost));
    for (int64_t q = 0; q < n_sd; ++q) cost[q] = score_cost(sds[q]);
    return 0;
}

extern "C" int32_t asgart_score_owners(const asgart_proto_sd *sds, int64_t n_sd, int32_t n_shards, int32_t *owner) {
    using namespace asgart;
    RC_TRY(check_shard_args("asgart_score_owners", sds, n_sd, n_shards, owner));
    try {
        score_owners(sds, n_sd, n_shards, owner);
    } catch (const std::bad_alloc &) {
        set_error("asgart_score_owners: out of host memory");
        return ASGART_E_OOM;
    }
    return 0;
}

// asgart_compute_scores[_flags]_shard
static int64_t score_one_shard(const char *fn, asgart_index *idx, const asgart_proto_sd *sds, int64_t n_sd,
                               const asgart::Orientations &o, int32_t shard, int32_t n_shards, float *identity) {
    using namespace asgart;
    if (!idx) {
        set_error("%s: bad argument", fn);
        return ASGART_E_ARG;
    }
    RC_TRY(check_shard_args(fn, sds, n_sd, n_shards, identity));
    if (shard < 0 || shard >= n_shards) {
        set_error("%s: bad shard %d of %d", fn, shard, n_shards);
        return ASGART_E_ARG;
    }
    if (n_sd == 0) return 0;
    RC_TRY(check_scores_input(fn, idx, sds, n_sd, o));  // the whole list: every rank fails alike
    try {
        std::vector<int32_t> owner((size_t)n_sd);
        score_owners(sds, n_sd, n_shards, owner.data());
        return score_shard(idx, sds, n_sd, owned_by(owner.data(), n_sd, shard), o, identity);
    } catch (const std::bad_alloc &) {
        set_error("%s: out of host memory", fn);
        return ASGART_E_OOM;
    }
}

extern "C" int64_t asgart_compute_scores_shard(asgart_index *idx, const asgart_proto_sd *sds, int64_t n_sd,
                                               int32_t reversed, int32_t complemented, int32_t shard, int32_t n_shards,
                                               float *identity) {
    return score_one_shard("asgart_compute_scores_shard", idx, sds, n_sd, {nullptr, reversed, complemented}, shard,
                           n_shards, identity);
}

extern "C" int64_t asgart_compute_scores_flags_shard(asgart_index *idx, const asgart_proto_sd *sds, const uint8_t *flags,
                                                     int64_t n_sd, int32_t shard, int32_t n_shards, float *identity) {
    return score_one_shard("asgart_compute_scores_flags_shard", idx, sds, n_sd, {flags, 0, 0}, shard, n_shards, identity);
}

// asgart_compute_scores[_flags]_multi
static int32_t score_devices(const char *fn, asgart_index *const *indices, int32_t n_devices, const asgart_proto_sd *sds,
                             int64_t n_sd, const asgart::Orientations &o, float *identity) {
    using namespace asgart;
    if (!indices || n_devices < 1 || n_devices > 64) {
        set_error("%s: bad argument: %d devices", fn, n_devices);
        return ASGART_E_ARG;
    }
    for (int32_t r = 0; r < n_devices; ++r)
        if (!indices[r] || indices[r]->n != indices[0]->n) {
            set_error("%s: index %d is NULL or not a replica of index 0", fn, r);
            return ASGART_E_ARG;
        }
    RC_TRY(check_shard_args(fn, sds, n_sd, n_devices, identity));
    if (n_sd == 0) return 0;
    RC_TRY(check_scores_input(fn, indices[0], sds, n_sd, o));
    try {
        std::vector<int32_t> owner((size_t)n_sd);
        score_owners(sds, n_sd, n_devices, owner.data());
        // one host thread per device, shard r of n_devices; the shards write disjoint entries of identity
        std::vector<int64_t> rcs((size_t)n_devices, 0);
        std::vector<std::string> errs((size_t)n_devices);
        std::vector<std::thread> workers;
        for (int32_t r = 0; r < n_devices; ++r)
            workers.emplace_back([&, r]() {
                try {
                    rcs[r] = score_shard(indices[r], sds, n_sd, owned_by(owner.data(), n_sd, r), o, identity);
                    if (rcs[r] < 0) errs[r] = asgart_last_error();  // the message is thread-local
                } catch (const std::bad_alloc &) {
                    rcs[r] = ASGART_E_OOM;
                    errs[r] = "out of host memory";
                }
            });
        for (auto &t : workers) t.join();
        for (int32_t r = 0; r < n_devices; ++r)
            if (rcs[r] < 0) {
                set_error("%s: shard %d of %d: %s", fn, r, n_devices, errs[r].c_str());
                return (int32_t)rcs[r];
            }
    } catch (const std::bad_alloc &) {
        set_error("%s: out of host memory", fn);
        return ASGART_E_OOM;
    }
    return 0;
}

extern "C" int32_t asgart_compute_scores_multi(asgart_index *const *indices, int32_t n_devices,
                                               const asgart_proto_sd *sds, int64_t n_sd, int32_t reversed,
                                               int32_t complemented, float *identity) {
    return score_devices("asgart_compute_scores_multi", indices, n_devices, sds, n_sd, {nullptr, reversed, complemented},
                         identity);
}

extern "C" int32_t asgart_compute_scores_flags_multi(asgart_index *const *indices, int32_t n_devices,
                                                     const asgart_proto_sd *sds, const uint8_t *flags, int64_t n_sd,
                                                     float *identity) {
    return score_devices("asgart_compute_scores_flags_multi", indices, n_devices, sds, n_sd, {flags, 0, 0}, identity);
}
