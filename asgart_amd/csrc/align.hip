// align.hip -- the alignment of the two arms of each duplication on the GPU: asgart_align_duplications.
//
// `--compute-score` (score.hip) walks the whole unit-cost edit matrix of two arms and keeps its last cell.  This file keeps
// enough of that walk to recover ONE optimal path, the canonical one: traced from (n, m), a diagonal step wherever
// D[i][j] == D[i-1][j-1] + (a_i != b_j), else an up step (`I`, a left-arm base without a partner) wherever
// D[i][j] == D[i-1][j] + 1, else a left step (`D`).  The rule makes the path unique, so the runs can be compared byte for
// byte with a host statement of the same rule (asgart_amd/align.py: align_host).
//
// Directions for every cell would take n m / 4 bytes (2.5 GB for two 100 kb arms).  Instead:
//   forward   levenshtein_kernel's systolic scheme, one wave per duplication, 64 lanes x 16 rows, bands of 1024 rows.  The
//             bottom row of every band but the last is KEPT (a row of its own per band) and every lane stores its 16 values
//             of each column j with j % W == 0: the checkpoints (align_dev.hpp: AlignShape), about n m / 51 bytes.
//   traceback one wave per duplication.  A tile is one band x W columns; it is rebuilt from the row checkpoint above it and
//             the column checkpoint left of it with the same systolic step, which now also writes two direction bits per cell
//             into LDS.  The path is walked through the tile until it leaves by the top edge, the left edge or the corner;
//             at most n_bands + ceil(m / W) tiles are rebuilt.  Runs are emitted backwards into the duplication's slot of
//             2 distance + 1 entries (a run that is not `=` holds an edit, and `=` runs lie between them).
//   compact   reverses the slots into CSR order.
// The host packs the duplications, largest first, into batches whose checkpoints fit the caller's budget; a duplication that
// alone exceeds it is refused, the others are unaffected, and no result depends on the budget or on the batching.
//
// asgart_align_duplications_banded is the same three stages inside a diagonal corridor: for a bound on the distance every
// band walks the column rectangle around the diagonals a path within the bound can reach, and keeps checkpoints of that
// width (align_dev.hpp: BandedShape; include/asgart_hip.h has the rule and the proofs that the runs are the same runs).
// The forward and the traceback kernel are templates of one flag: <false> is the code above, on the path and in the
// registers it had before the corridor (profiles/align_banded_resources.txt), <true> moves the walk's columns to the rectangle.  A duplication beyond its bound leaves
// between the two kernels (the host reads the distances), so slot counts and compaction see aligned ones only.  Without
// bounds from the caller the host runs rounds: the library's first bound, then four times as much for those beyond it.
// Integer work throughout; plain vector loads and stores and LDS.
// The systolic step of both kernels, with and without the direction bits, is lev_dev.hpp's (lev_inputs, lev_column,
// lev_store_bottom); the right arm, the identity and the checks of the list are there too, shared with score.hip.
#include "index.hpp"
#include "tool_base.hpp"
#include "align_dev.hpp"

#include <algorithm>
#include <cmath>
#include <limits>
#include <new>

namespace asgart {
namespace {

constexpr int kFwdThreads = 256;  // four duplications per workgroup of the forward pass
constexpr uint32_t kBlock = 256;

// what a kernel needs of one batch: its members (ordinals into the call's list, ascending), the order they are served in
// (positions into members, largest first) and the base of each member's checkpoints (u32 words into ck)
struct Batch {
    const asgart_proto_sd *sds;
    const uint8_t *flags;     // NULL: all zero
    const uint32_t *members;
    const uint32_t *order;
    const uint64_t *ck_off;
    uint64_t n;
    int inclusive;
    const uint32_t *bound;    // max_distance of every duplication of the list (the corridor kernels only)
};

// D[band][j] for a band of the corridor: the bottom row of the band above where that band has column j (its columns
// plo .. phi), kAlignBig elsewhere.  kFresh: written by this wave one band ago, read past the vector L1.
template <bool kFresh>
__device__ __forceinline__ uint32_t corridor_top(const uint32_t *top_row, uint32_t plo, uint32_t phi, uint32_t j) {
    if (j < plo || j > phi) return kAlignBig;
    if constexpr (kFresh) return __atomic_load_n(&top_row[j - plo + 1u], __ATOMIC_RELAXED);
    return top_row[j - plo + 1u];
}

// the column left of a corridor band's rectangle
__device__ __forceinline__ void corridor_first_column(uint32_t (&col)[kLevRows]) {
#pragma unroll
    for (int r = 0; r < kLevRows; ++r) col[r] = kAlignBig;
}

// ---- forward: distances and checkpoints (the band loop written out, as in levenshtein_kernel) -----------------------
// kBanded: every band walks the columns lo .. hi of its corridor rectangle (align_dev.hpp: BandedShape) instead of 1 .. m;
// a step's column is then counted from lo, and what lies outside the rectangles is kAlignBig.  A distance beyond the bound
// is stored as 0xFFFFFFFF.
template <bool kBanded>
__global__ __launch_bounds__(kFwdThreads) void align_forward_kernel(const uint8_t *__restrict__ text, Batch bt,
                                                                    uint32_t *__restrict__ ck,
                                                                    unsigned long long *__restrict__ cursor,
                                                                    uint32_t *__restrict__ distance,
                                                                    float *__restrict__ identity) {
    constexpr int R = kLevRows;
    constexpr uint32_t W = kAlignTile;
    const int lane = threadIdx.x & 63;
    for (;;) {
        unsigned long long pos = 0;
        if (lane == 0) pos = atomicAdd(cursor, 1ull);
        pos = __shfl(pos, 0);
        if (pos >= bt.n) break;
        const uint32_t k = bt.order[pos];
        const uint32_t item = bt.members[k];
        const asgart_proto_sd sd = bt.sds[item];
        const AlignShape g = align_shape(sd, bt.inclusive);
        const uint32_t la = (uint32_t)g.n, lb = (uint32_t)g.m;
        const uint8_t *A = text + sd.left;
        const RightArm rb = right_arm(text + sd.right, lb, orientation_of(bt.flags, item, 0, 0));
        uint32_t *colck = ck + bt.ck_off[k];
        BandedShape c{};
        uint32_t bound = 0;
        if constexpr (kBanded) {
            bound = bt.bound[item];
            c = banded_shape(sd, bt.inclusive, bound);
        }
        uint32_t *rowck = colck + (kBanded ? c.col_words() : g.col_words());
        const uint64_t row_stride = kBanded ? c.row_stride : g.m + 1u;
        uint32_t result = 0;
        uint32_t bi = 0;
        for (uint32_t band = 0; band < la && lb > 0; band += kLevBand, ++bi) {
            const uint32_t i0 = band + (uint32_t)lane * R;  // rows i0+1 .. i0+R (1-based) are this lane's
            const bool more_bands = band + kLevBand < la;
            const uint32_t *top_row = bi ? rowck + (uint64_t)(bi - 1u) * row_stride : rowck;  // (read for bi > 0 only)
            uint32_t *bottom_row = rowck + (uint64_t)bi * row_stride;                         // (written if more_bands)
            uint32_t a[R], col[R];
            lev_rows(a, i0, la, A);
            uint32_t diag_in = i0;       // D[i0][j-1] for the lane's next column
            uint32_t lo = 1, hi = lb, plo = 1, phi = 0, ck0 = 0;  // the band's columns, those of the band above, the first checkpoint
            if constexpr (kBanded) {
                lo = c.lo(bi), hi = c.hi(bi), ck0 = c.first_ck(bi);
                if (bi) plo = c.lo(bi - 1u), phi = c.hi(bi - 1u);
                if (lo == 1u) {
                    lev_first_column(col, i0);
                } else {  // D[..][lo - 1] is outside, but for D[band][lo - 1], which the band above may have
                    corridor_first_column(col);
                    diag_in = lane ? kAlignBig : (band == 0 ? lo - 1u : corridor_top<true>(top_row, plo, phi, lo - 1u));
                }
            } else {
                lev_first_column(col, i0);
            }
            const uint32_t wb = hi - lo + 1u;  // (lb without a corridor)
            uint32_t last_out = 0;       // D[i0+R][j] of the column just done
            uint32_t b_pipe = 0;         // base of the lane's current column (travels down the lanes)
            uint32_t top_chunk = 0, b_chunk = 0, out_chunk = 0;
            const uint32_t n_steps = (kBanded ? wb : lb) + 63u;
            for (uint32_t s = 0; s < n_steps; ++s) {
                if ((s & 63u) == 0u) {  // 64 columns of the top boundary and of the right arm at a time
                    if constexpr (kBanded) {
                        const uint32_t j1 = lo + s + (uint32_t)lane;  // the chunks start at the rectangle's first column
                        top_chunk = band == 0 ? j1 : corridor_top<true>(top_row, plo, phi, j1);
                        b_chunk = j1 <= lb ? rb.at(j1 - 1u) : 0u;
                    } else {
                        const uint32_t j1 = s + 1u + (uint32_t)lane;  // column of lane 0 at step s + lane
                        // (written by this wave one band ago: read past the vector L1)
                        top_chunk = band == 0 ? j1 : (j1 <= lb ? __atomic_load_n(&top_row[j1], __ATOMIC_RELAXED) : 0u);
                        b_chunk = s + (uint32_t)lane < lb ? rb.at(s + (uint32_t)lane) : 0u;
                    }
                }
                const LevIn in = lev_inputs(last_out, top_chunk, b_pipe, b_chunk, s, lane);
                const int64_t j = (int64_t)s - lane + 1;  // (kBanded: counted from lo)
                if (j >= 1 && j <= (int64_t)(kBanded ? wb : lb)) {
                    lev_column<false>(a, col, diag_in, in);
                    last_out = col[R - 1];
                    const uint32_t ja = kBanded ? lo - 1u + (uint32_t)j : (uint32_t)j;
                    if (ja == lb && la > i0 && la <= i0 + R) result = lev_row_value(col, i0, la);
                    // a column checkpoint: the lane's 16 values of column j, 64 contiguous bytes
                    if ((ja & (W - 1u)) == 0u && ja < (kBanded ? hi : lb)) {
                        uint4 *dst = reinterpret_cast<uint4 *>(
                            kBanded ? colck + ((uint64_t)bi * c.ck_per_band + (ja / W - ck0)) * kLevBand + (uint32_t)lane * R
                                    : colck + (uint64_t)(ja / W - 1u) * g.rows_padded + i0);
#pragma unroll
                        for (int v4 = 0; v4 < R / 4; ++v4)
                            dst[v4] = make_uint4(col[4 * v4], col[4 * v4 + 1], col[4 * v4 + 2], col[4 * v4 + 3]);
                    }
                }
                if (more_bands) lev_store_bottom(last_out, s, lane, kBanded ? wb : lb, out_chunk, bottom_row);
            }
            // the next band reads what this one wrote (same wave: program order; make it visible)
            __threadfence_block();
        }
        uint32_t dist;
        if (la == 0 || lb == 0) {
            dist = la + lb;  // one arm is empty: the other one, base by base
        } else {
            const uint32_t owner = ((la - 1u) % kLevBand) / R;  // lane of row la in the last band
            dist = __shfl(result, (int)owner);
        }
        if constexpr (kBanded)
            if (dist > bound) dist = 0xFFFFFFFFu;  // more than the bound, and nothing else is known
        if (lane == 0) {
            distance[item] = dist;
            identity[item] = identity_of(sd, dist);
        }
    }
}

// cnt[k] = the entries of member k's slot, 2 distance + 1; the closing entry is zero (the scan over n + 1 ends in the total)
__global__ __launch_bounds__(kBlock) void align_slot_counts_kernel(const uint32_t *__restrict__ members, uint64_t n,
                                                                   const uint32_t *__restrict__ distance,
                                                                   uint64_t *__restrict__ cnt) {
    const uint64_t k = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (k < n) cnt[k] = 2ull * distance[members[k]] + 1ull;
    if (k == n) cnt[k] = 0;
}

// ---- traceback: one wave per duplication, a tile at a time --------------------------------------------------------
// kBanded: over the forward pass's corridor checkpoints.  A tile is rebuilt where its band's rectangle is: the columns
// jt0 + 1 .. jt0 + wt, seeded like the forward pass.  (Only duplications within their bound are handed over.)
template <bool kBanded>
__global__ __launch_bounds__(64) void align_traceback_kernel(const uint8_t *__restrict__ text, Batch bt,
                                                             const uint32_t *__restrict__ ck,
                                                             const uint32_t *__restrict__ distance,
                                                             const uint64_t *__restrict__ slot_off,
                                                             uint32_t *__restrict__ slot_len, uint8_t *__restrict__ slot_op,
                                                             uint64_t *__restrict__ n_runs,
                                                             unsigned long long *__restrict__ cursor,
                                                             uint32_t *__restrict__ overflow) {
    constexpr int R = kLevRows;
    constexpr uint32_t W = kAlignTile;
    __shared__ uint32_t dirs[kAlignDirWords];  // dirs[c * 64 + lane]: the directions of the lane's 16 rows in column c of the tile
    const int lane = threadIdx.x;
    for (;;) {
        unsigned long long pos = 0;
        if (lane == 0) pos = atomicAdd(cursor, 1ull);
        pos = __shfl(pos, 0);
        if (pos >= bt.n) break;
        const uint32_t k = bt.order[pos];
        const uint32_t item = bt.members[k];
        const asgart_proto_sd sd = bt.sds[item];
        const AlignShape g = align_shape(sd, bt.inclusive);
        const uint32_t la = (uint32_t)g.n, lb = (uint32_t)g.m;
        const uint8_t *A = text + sd.left;
        const RightArm rb = right_arm(text + sd.right, lb, orientation_of(bt.flags, item, 0, 0));
        const uint32_t *colck = ck + bt.ck_off[k];
        BandedShape c{};
        if constexpr (kBanded) c = banded_shape(sd, bt.inclusive, bt.bound[item]);
        const uint32_t *rowck = colck + (kBanded ? c.col_words() : g.col_words());
        const uint64_t row_stride = kBanded ? c.row_stride : g.m + 1u;
        const uint64_t slot = slot_off[k];
        const uint64_t slot_cap = 2ull * distance[item] + 1ull;
        // the run being collected (every lane keeps the same copy; lane 0 writes) and how many were written
        uint32_t run_op = kOpNone, run_len = 0;
        uint64_t n_out = 0;
        auto flush = [&]() {
            if (run_op == kOpNone) return;
            if (lane == 0 && n_out < slot_cap) {
                slot_len[slot + n_out] = run_len;
                slot_op[slot + n_out] = (uint8_t)run_op;
            }
            ++n_out;
        };
        auto emit = [&](uint32_t op, uint32_t count) {
            if (op == run_op) {
                run_len += count;
            } else {
                flush();
                run_op = op;
                run_len = count;
            }
        };
        uint32_t i = la, j = lb;  // the cell the path stands on
        while (i > 0 && j > 0) {
            const uint32_t b = (i - 1u) / kLevBand, cb = (j - 1u) / W;
            const uint32_t band = b * kLevBand, j0 = cb * W;
            const uint32_t *top_row = b ? rowck + (uint64_t)(b - 1u) * row_stride : rowck;  // D[band][..] (read for b > 0 only)
            uint32_t jt0 = j0, wt = min(W, lb - j0);  // columns jt0+1 .. jt0+wt
            uint32_t lo = 1, plo = 1, phi = 0;
            if constexpr (kBanded) {
                lo = c.lo(b);
                if (b) plo = c.lo(b - 1u), phi = c.hi(b - 1u);
                if (j < lo || j > c.hi(b)) {  // (no optimal path leaves the corridor: never, and never a tile without columns)
                    if (lane == 0) atomicOr(overflow, 1u);
                    i = j = 0;
                    run_op = kOpNone;
                    break;
                }
                jt0 = max(j0, lo - 1u);
                wt = min(j0 + W, c.hi(b)) - jt0;
            }
            {
                // rebuild the tile: the forward step, seeded with the column left of the tile and the cell above it
                const uint32_t i0 = band + (uint32_t)lane * R;
                uint32_t a[R], col[R];
                if (jt0 == 0) {
                    lev_first_column(col, i0);
                } else if (kBanded && j0 < lo) {  // the tile starts at the rectangle's first column
                    corridor_first_column(col);
                } else {
                    const uint4 *src = reinterpret_cast<const uint4 *>(
                        kBanded ? colck + ((uint64_t)b * c.ck_per_band + (cb - c.first_ck(b))) * kLevBand + (uint32_t)lane * R
                                : colck + (uint64_t)(cb - 1u) * g.rows_padded + i0);
#pragma unroll
                    for (int v4 = 0; v4 < R / 4; ++v4) {
                        const uint4 v = src[v4];
                        col[4 * v4] = v.x;
                        col[4 * v4 + 1] = v.y;
                        col[4 * v4 + 2] = v.z;
                        col[4 * v4 + 3] = v.w;
                    }
                }
                lev_rows(a, i0, la, A);
                // D[i0][j0]: the last seed value of the lane above; for lane 0 the boundary itself
                uint32_t diag_in = __shfl_up(col[R - 1], 1);
                if constexpr (kBanded) {
                    if (lane == 0) diag_in = b == 0 ? jt0 : (jt0 == 0 ? band : corridor_top<false>(top_row, plo, phi, jt0));
                } else {
                    if (lane == 0) diag_in = b == 0 ? j0 : (j0 == 0 ? band : top_row[j0]);
                }
                uint32_t last_out = 0, b_pipe = 0, top_chunk = 0, b_chunk = 0;
                const uint32_t n_steps = wt + 63u;
                for (uint32_t s = 0; s < n_steps; ++s) {
                    if ((s & 63u) == 0u) {
                        const uint32_t j1 = jt0 + s + 1u + (uint32_t)lane;
                        if constexpr (kBanded) top_chunk = b == 0 ? j1 : corridor_top<false>(top_row, plo, phi, j1);
                        else top_chunk = b == 0 ? j1 : (j1 <= lb ? top_row[j1] : 0u);
                        b_chunk = j1 <= lb ? rb.at(j1 - 1u) : 0u;
                    }
                    const LevIn in = lev_inputs(last_out, top_chunk, b_pipe, b_chunk, s, lane);
                    const int32_t c = (int32_t)s - lane;  // column of the tile, 0-based
                    if (c >= 0 && c < (int32_t)wt) {
                        dirs[(uint32_t)c * 64u + (uint32_t)lane] = lev_column<true>(a, col, diag_in, in);
                        last_out = col[R - 1];
                    }
                }
            }
            __syncthreads();
            // walk the path through the tile (the same walk in every lane: uniform LDS reads)
            while (i > band && j > jt0) {
                const uint32_t row = i - 1u - band;
                const uint32_t d = (dirs[(j - 1u - jt0) * 64u + row / R] >> (2u * (row % R))) & 3u;
                emit(d, 1u);
                if (d != kOpDelete) --i;
                if (d != kOpInsert) --j;
            }
            __syncthreads();  // the next tile overwrites what was just read
        }
        if (i > 0) emit(kOpInsert, i);  // column 0: D[i][0] = D[i-1][0] + 1
        if (j > 0) emit(kOpDelete, j);  // row 0
        flush();
        if (lane == 0) {
            n_runs[k] = n_out;
            if (n_out > slot_cap) atomicOr(overflow, 1u);
        }
    }
}

// ---- compact: run t of the batch, in CSR order, is its member's slot read from the back -----------------------------
__global__ __launch_bounds__(kBlock) void align_compact_kernel(const uint64_t *__restrict__ out_off, uint32_t n_members,
                                                               uint32_t n_total, const uint64_t *__restrict__ slot_off,
                                                               const uint64_t *__restrict__ n_runs,
                                                               const uint32_t *__restrict__ slot_len,
                                                               const uint8_t *__restrict__ slot_op,
                                                               uint32_t *__restrict__ out_len, uint8_t *__restrict__ out_op) {
    const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
    if (t >= n_total) return;
    const uint32_t k = segment_of(out_off, n_members, t);
    const uint64_t src = slot_off[k] + (n_runs[k] - 1u - ((uint64_t)t - out_off[k]));
    const uint32_t op = slot_op[src];
    out_len[t] = slot_len[src];
    out_op[t] = op == kOpMatch ? '=' : op == kOpMismatch ? 'X' : op == kOpInsert ? 'I' : 'D';
}

}  // namespace
}  // namespace asgart

using namespace asgart;

struct asgart_alignment {
    std::vector<uint64_t> run_offsets;
    std::vector<uint32_t> run_len, distance;
    std::vector<uint8_t> run_op, status;
    std::vector<float> identity;
    uint64_t n_refused = 0;
    double ms[4] = {0, 0, 0, 0};
    uint32_t rounds = 0;  // passes over the list (one, unless the bounds are the library's)
    uint64_t cells = 0;   // cells of the forward passes of all rounds
};

namespace {

struct AlignWork : ToolWork {
    DevBuf &sds = buf(), &flags = buf(), &distance = buf(), &identity = buf(), &counters = buf(), &bound = buf();
    DevBuf &members = buf(), &order = buf(), &ck_off = buf(), &ck = buf();
    DevBuf &cnt = buf(), &slot_off = buf(), &slot_len = buf(), &slot_op = buf(), &n_runs = buf(), &out_off = buf();
    DevBuf &out_len = buf(), &out_op = buf();
};

// the runs of one batch on the host, in the order of its members
struct BatchRuns {
    std::vector<uint32_t> members;
    std::vector<uint64_t> off;
    std::vector<uint32_t> len;
    std::vector<uint8_t> op;
};

// the checkpoint bytes and the forward pass's cells of one duplication: of the whole matrix, or of the corridor of its bound
uint64_t checkpoint_bytes(const asgart_proto_sd &sd, int inclusive, const uint32_t *bound, size_t q) {
    return bound ? banded_shape(sd, inclusive, bound[q]).bytes() : align_shape(sd, inclusive).bytes();
}

uint64_t forward_cells(const asgart_proto_sd &sd, int inclusive, const uint32_t *bound, size_t q) {
    if (bound) return banded_shape(sd, inclusive, bound[q]).cells();
    const AlignShape g = align_shape(sd, inclusive);
    return g.n * g.m;
}

// One batch.  bound: NULL, or max_distance of every duplication of the list (it is in w.bound then): the corridor kernels
// run, the members found beyond their bound go to `beyond` and leave br.members, and the traceback sees the others only.
int32_t run_batch(AlignWork &w, asgart_alignment *res, const asgart_index *idx, const asgart_proto_sd *sds, bool has_flags,
                  int64_t n_sd, int inclusive, BatchRuns &br, const uint32_t *bound, std::vector<uint32_t> &beyond) {
    hipStream_t s = w.s;
    uint64_t nk = br.members.size();
    // served largest first; the checkpoints of member k start at ck_off[k] (slots of whole 16-byte vectors)
    std::vector<uint32_t> order((size_t)nk);
    std::vector<uint64_t> ck_off((size_t)nk), cells((size_t)nk);
    uint64_t words = 0;
    for (uint64_t k = 0; k < nk; ++k) {
        const uint32_t q = br.members[(size_t)k];
        order[(size_t)k] = (uint32_t)k;
        ck_off[(size_t)k] = words;
        words += (checkpoint_bytes(sds[q], inclusive, bound, q) / 4u + 3u) & ~(uint64_t)3;
        cells[(size_t)k] = forward_cells(sds[q], inclusive, bound, q);
        res->cells += cells[(size_t)k];
    }
    std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return cells[x] > cells[y]; });

    HIP_TRY(hipEventRecord(w.ev[0], s));
    RC_TRY(w.upload(w.members, br.members.data(), (size_t)nk * 4));
    RC_TRY(w.upload(w.order, order.data(), (size_t)nk * 4));
    RC_TRY(w.upload(w.ck_off, ck_off.data(), (size_t)nk * 8));
    RC_TRY(w.ck.reserve((size_t)words * 4 + 64));
    for (DevBuf *b : {&w.cnt, &w.slot_off, &w.n_runs, &w.out_off}) RC_TRY(b->reserve(((size_t)nk + 1) * 8));
    unsigned long long *cursors = w.counters.as<unsigned long long>();  // [0] forward, [1] traceback, then the overflow mark
    uint32_t *overflow = reinterpret_cast<uint32_t *>(cursors + 2);
    HIP_TRY(hipMemsetAsync(cursors, 0, 32, s));
    HIP_TRY(stream_sync(s));  // (pageable host sources)
    HIP_TRY(hipEventRecord(w.ev[1], s));

    Batch bt{w.sds.as<asgart_proto_sd>(), has_flags ? w.flags.as<uint8_t>() : nullptr, w.members.as<uint32_t>(),
             w.order.as<uint32_t>(), w.ck_off.as<uint64_t>(), nk, inclusive, bound ? w.bound.as<uint32_t>() : nullptr};
    uint32_t *d_dist = w.distance.as<uint32_t>();
    const unsigned waves_per_wg = kFwdThreads / 64;
    const unsigned grid_f = (unsigned)std::min<uint64_t>((nk + waves_per_wg - 1) / waves_per_wg, 1024);
    if (bound)
        align_forward_kernel<true><<<grid_f, kFwdThreads, 0, s>>>(idx->d_text, bt, w.ck.as<uint32_t>(), cursors, d_dist,
                                                                   w.identity.as<float>());
    else
        align_forward_kernel<false><<<grid_f, kFwdThreads, 0, s>>>(idx->d_text, bt, w.ck.as<uint32_t>(), cursors, d_dist,
                                                                    w.identity.as<float>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(w.ev[2], s));

    if (bound) {  // who is within the bound?  The others have no path to trace.
        std::vector<uint32_t> dist((size_t)n_sd);
        HIP_TRY(read_back(dist.data(), d_dist, (size_t)n_sd * 4, s));
        std::vector<uint32_t> kept;
        std::vector<uint64_t> kept_off, kept_cells;
        for (uint64_t k = 0; k < nk; ++k) {
            const uint32_t q = br.members[(size_t)k];
            if (dist[q] == 0xFFFFFFFFu) {
                beyond.push_back(q);
            } else {
                kept.push_back(q);
                kept_off.push_back(ck_off[(size_t)k]);
                kept_cells.push_back(cells[(size_t)k]);
            }
        }
        if (kept.size() != nk) {
            br.members.swap(kept);
            ck_off.swap(kept_off);
            cells.swap(kept_cells);
            nk = br.members.size();
            order.resize((size_t)nk);
            for (uint64_t k = 0; k < nk; ++k) order[(size_t)k] = (uint32_t)k;
            std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return cells[x] > cells[y]; });
            RC_TRY(w.upload(w.members, br.members.data(), (size_t)nk * 4));
            RC_TRY(w.upload(w.order, order.data(), (size_t)nk * 4));
            RC_TRY(w.upload(w.ck_off, ck_off.data(), (size_t)nk * 8));
            HIP_TRY(stream_sync(s));  // (pageable host sources)
            bt.n = nk;
        }
    }
    if (nk == 0) {  // nobody is left: no runs
        HIP_TRY(hipEventRecord(w.ev[3], s));
        HIP_TRY(stream_sync(s));
        br.off.assign(1, 0);
        for (int k = 0; k < 3; ++k) {
            float ms = 0;
            HIP_TRY(hipEventElapsedTime(&ms, w.ev[k], w.ev[k + 1]));
            res->ms[k] += (double)ms;
        }
        return 0;
    }

    uint64_t *cnt = w.cnt.as<uint64_t>(), *slot_off = w.slot_off.as<uint64_t>();
    uint64_t *n_runs = w.n_runs.as<uint64_t>(), *out_off = w.out_off.as<uint64_t>();
    align_slot_counts_kernel<<<blocks_for(nk + 1, kBlock), kBlock, 0, s>>>(bt.members, nk, d_dist, cnt);
    HIP_TRY(hipGetLastError());
    RC_TRY(w.exclusive_scan(cnt, slot_off, (size_t)nk + 1));
    uint64_t n_slots = 0;
    HIP_TRY(read_back(&n_slots, slot_off + nk, 8, s));
    RC_TRY(w.slot_len.reserve((size_t)n_slots * 4 + 16));
    RC_TRY(w.slot_op.reserve((size_t)n_slots + 16));
    HIP_TRY(hipMemsetAsync(n_runs + nk, 0, 8, s));
    const unsigned grid_t = (unsigned)std::min<uint64_t>(nk, 2048);
    if (bound)
        align_traceback_kernel<true><<<grid_t, 64, 0, s>>>(idx->d_text, bt, w.ck.as<uint32_t>(), d_dist, slot_off,
                                                           w.slot_len.as<uint32_t>(), w.slot_op.as<uint8_t>(), n_runs,
                                                           cursors + 1, overflow);
    else
        align_traceback_kernel<false><<<grid_t, 64, 0, s>>>(idx->d_text, bt, w.ck.as<uint32_t>(), d_dist, slot_off,
                                                            w.slot_len.as<uint32_t>(), w.slot_op.as<uint8_t>(), n_runs,
                                                            cursors + 1, overflow);
    HIP_TRY(hipGetLastError());
    RC_TRY(w.exclusive_scan(n_runs, out_off, (size_t)nk + 1));
    uint64_t n_total = 0;
    uint32_t h_overflow = 0;
    HIP_TRY(read_back(&n_total, out_off + nk, 8, s));
    HIP_TRY(read_back(&h_overflow, overflow, 4, s));
    if (h_overflow || n_total > n_slots) {
        set_error("asgart_align_duplications: a path has more runs than 2 distance + 1");
        return ASGART_E_HIP;
    }
    if (n_total >= 0xFFFFFFFFull) {
        set_error("asgart_align_duplications: 2^32 runs in one batch are not supported");
        return ASGART_E_CAP;
    }
    RC_TRY(w.out_len.reserve((size_t)n_total * 4 + 16));
    RC_TRY(w.out_op.reserve((size_t)n_total + 16));
    if (n_total)
        align_compact_kernel<<<blocks_for(n_total, kBlock), kBlock, 0, s>>>(out_off, (uint32_t)nk, (uint32_t)n_total, slot_off,
                                                                            n_runs, w.slot_len.as<uint32_t>(),
                                                                            w.slot_op.as<uint8_t>(), w.out_len.as<uint32_t>(),
                                                                            w.out_op.as<uint8_t>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(w.ev[3], s));
    HIP_TRY(stream_sync(s));

    const auto t0 = std::chrono::steady_clock::now();
    br.off.resize((size_t)nk + 1);
    br.len.resize((size_t)n_total);
    br.op.resize((size_t)n_total);
    HIP_TRY(hipMemcpyAsync(br.off.data(), out_off, ((size_t)nk + 1) * 8, hipMemcpyDeviceToHost, s));
    if (n_total) {
        HIP_TRY(hipMemcpyAsync(br.len.data(), w.out_len.p, (size_t)n_total * 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(br.op.data(), w.out_op.p, (size_t)n_total, hipMemcpyDeviceToHost, s));
    }
    HIP_TRY(stream_sync(s));
    res->ms[3] += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    for (int k = 0; k < 3; ++k) {
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, w.ev[k], w.ev[k + 1]));
        res->ms[k] += (double)ms;
    }
    return 0;
}

// what the corridor kernels count in 32 bits: kAlignBig + n + m, and a bound below kAlignBig (max_distance NULL: the library's)
int32_t check_banded(const char *fn, const asgart_proto_sd *sds, int64_t n_sd, int inclusive, const uint32_t *max_distance) {
    for (int64_t q = 0; q < n_sd; ++q) {
        const AlignShape g = align_shape(sds[q], inclusive);
        if (g.n + g.m >= kAlignBandedCap) {
            set_error("%s: duplication %lld has arms of 2^30 bases together; a corridor is not supported for them", fn,
                      (long long)q);
            return ASGART_E_CAP;
        }
        if (max_distance && max_distance[q] >= kAlignBandedCap) {
            set_error("%s: max_distance[%lld] = %u; it must be below 2^30", fn, (long long)q, (unsigned)max_distance[q]);
            return ASGART_E_ARG;
        }
    }
    return 0;
}

// One pass over the duplications `items` (ascending), each within bound[q] where there is a bound: batches by checkpoint
// bytes, largest first, a new one whenever the next duplication no longer fits.  Sets status[q] to 0 (alone over the
// budget) or 2 (beyond its bound) and says where the runs of the others are.
int32_t run_round(AlignWork &w, asgart_alignment *res, const asgart_index *idx, const asgart_proto_sd *sds, bool has_flags,
                  int64_t n_sd, int inclusive, uint64_t budget, const std::vector<uint32_t> &items, const uint32_t *bound,
                  std::vector<BatchRuns> &batches, std::vector<uint32_t> &batch_of, std::vector<uint32_t> &slot_of) {
    ++res->rounds;
    if (bound) {
        RC_TRY(w.upload(w.bound, bound, (size_t)n_sd * 4));
        HIP_TRY(stream_sync(w.s));  // (a pageable host source)
    }
    std::vector<uint64_t> bytes((size_t)n_sd, 0);
    std::vector<uint32_t> by_size;
    for (uint32_t q : items) {
        if (bound && banded_shape(sds[q], inclusive, bound[q]).beyond) {  // T < |m - n|: no work
            res->status[q] = 2;
            continue;
        }
        bytes[q] = checkpoint_bytes(sds[q], inclusive, bound, q);
        if (bytes[q] > budget)
            res->status[q] = 0;
        else
            by_size.push_back(q);
    }
    std::stable_sort(by_size.begin(), by_size.end(), [&](uint32_t x, uint32_t y) { return bytes[x] > bytes[y]; });
    const size_t first = batches.size();
    uint64_t held = 0;
    for (uint32_t q : by_size) {
        if (batches.size() == first || held + bytes[q] > budget) {
            batches.emplace_back();
            held = 0;
        }
        batches.back().members.push_back(q);
        held += bytes[q];
    }
    std::vector<uint32_t> beyond;
    for (size_t b = first; b < batches.size(); ++b) {
        BatchRuns &br = batches[b];
        std::sort(br.members.begin(), br.members.end());
        RC_TRY(run_batch(w, res, idx, sds, has_flags, n_sd, inclusive, br, bound, beyond));
        for (size_t k = 0; k < br.members.size(); ++k) {
            batch_of[br.members[k]] = (uint32_t)b;
            slot_of[br.members[k]] = (uint32_t)k;
        }
    }
    for (uint32_t q : beyond) res->status[q] = 2;
    return 0;
}

// max_distance: the caller's bounds; automatic: the library's (align_dev.hpp: align_auto_first, align_auto_next), round
// after round for those that were beyond theirs; neither: the whole matrix of every duplication.
int32_t run_align(AlignWork &w, asgart_alignment *res, const asgart_index *idx, const asgart_proto_sd *sds,
                  const uint8_t *flags, int64_t n_sd, int inclusive, uint64_t budget, const uint32_t *max_distance,
                  bool automatic) {
    RC_TRY(w.open(4));
    hipStream_t s = w.s;
    if (budget == 0) {  // half of what is free
        size_t free_b = 0, total_b = 0;
        HIP_TRY(hipMemGetInfo(&free_b, &total_b));
        budget = (uint64_t)free_b / 2u;
    }
    const auto t_up = std::chrono::steady_clock::now();
    RC_TRY(w.upload(w.sds, sds, (size_t)n_sd * sizeof(asgart_proto_sd)));
    if (flags) RC_TRY(w.upload(w.flags, flags, (size_t)n_sd));
    RC_TRY(w.distance.reserve((size_t)n_sd * 4 + 16));
    RC_TRY(w.identity.reserve((size_t)n_sd * 4 + 16));
    RC_TRY(w.counters.reserve(64));
    HIP_TRY(hipMemsetAsync(w.distance.p, 0xFF, (size_t)n_sd * 4, s));  // refused: 0xFFFFFFFF and a NaN
    HIP_TRY(hipMemsetAsync(w.identity.p, 0xFF, (size_t)n_sd * 4, s));
    HIP_TRY(stream_sync(s));
    res->ms[0] += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_up).count();

    res->status.assign((size_t)n_sd, 1);
    std::vector<BatchRuns> batches;
    std::vector<uint32_t> batch_of((size_t)n_sd, 0), slot_of((size_t)n_sd, 0), items((size_t)n_sd), auto_bound;
    for (int64_t q = 0; q < n_sd; ++q) items[(size_t)q] = (uint32_t)q;
    if (automatic) {
        auto_bound.resize((size_t)n_sd);
        for (int64_t q = 0; q < n_sd; ++q) {
            const AlignShape g = align_shape(sds[q], inclusive);
            auto_bound[(size_t)q] = align_auto_first(g.n, g.m);
        }
        max_distance = auto_bound.data();
    }
    for (;;) {
        RC_TRY(run_round(w, res, idx, sds, flags != nullptr, n_sd, inclusive, budget, items, max_distance, batches, batch_of,
                         slot_of));
        if (!automatic) break;
        // again, with a larger bound, for those beyond theirs; at n + m the corridor is the matrix and nobody is beyond it
        std::vector<uint32_t> again;
        for (uint32_t q : items) {
            const AlignShape g = align_shape(sds[q], inclusive);
            if (res->status[q] != 2 || auto_bound[q] >= g.n + g.m) continue;
            auto_bound[q] = align_auto_next(auto_bound[q], g.n, g.m);
            res->status[q] = 1;
            again.push_back(q);
        }
        if (again.empty()) break;
        items.swap(again);
    }
    for (int64_t q = 0; q < n_sd; ++q) res->n_refused += res->status[(size_t)q] == 0;

    const auto t0 = std::chrono::steady_clock::now();
    res->distance.resize((size_t)n_sd);
    res->identity.resize((size_t)n_sd);
    HIP_TRY(read_back(res->distance.data(), w.distance.p, (size_t)n_sd * 4, s));
    HIP_TRY(read_back(res->identity.data(), w.identity.p, (size_t)n_sd * 4, s));
    res->run_offsets.assign((size_t)n_sd + 1, 0);
    for (int64_t q = 0; q < n_sd; ++q) {
        uint64_t runs = 0;
        if (res->status[(size_t)q] == 1) {
            const BatchRuns &br = batches[batch_of[(size_t)q]];
            runs = br.off[slot_of[(size_t)q] + 1u] - br.off[slot_of[(size_t)q]];
        } else {
            res->identity[(size_t)q] = std::numeric_limits<float>::quiet_NaN();
        }
        res->run_offsets[(size_t)q + 1] = res->run_offsets[(size_t)q] + runs;
    }
    const uint64_t n_runs = res->run_offsets[(size_t)n_sd];
    res->run_len.resize((size_t)n_runs);
    res->run_op.resize((size_t)n_runs);
    for (int64_t q = 0; q < n_sd; ++q) {
        if (res->status[(size_t)q] != 1) continue;
        const BatchRuns &br = batches[batch_of[(size_t)q]];
        const uint64_t from = br.off[slot_of[(size_t)q]], runs = br.off[slot_of[(size_t)q] + 1u] - from;
        if (!runs) continue;
        memcpy(res->run_len.data() + res->run_offsets[(size_t)q], br.len.data() + from, (size_t)runs * 4);
        memcpy(res->run_op.data() + res->run_offsets[(size_t)q], br.op.data() + from, (size_t)runs);
    }
    res->ms[3] += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return 0;
}

}  // namespace

namespace {

// the two entry points: the whole matrix (banded = false), or corridors for the caller's bounds or, without any, the library's
int32_t align_entry(const char *fn, asgart_index *idx, const asgart_proto_sd *sds, const uint8_t *flags, int64_t n_sd,
                    int32_t inclusive, bool banded, const uint32_t *max_distance, uint64_t budget_bytes,
                    asgart_alignment **out) {
    if (out) *out = nullptr;
    if (!idx || !out) {  // (the result is made for an empty list too)
        set_error("%s: bad argument", fn);
        return ASGART_E_ARG;
    }
    RC_TRY(check_list_args(fn, sds, n_sd, out));
    RC_TRY(check_flags(fn, flags, n_sd));
    RC_TRY(check_arms(fn, (uint64_t)idx->n, sds, n_sd, inclusive != 0));
    if (banded) RC_TRY(check_banded(fn, sds, n_sd, inclusive != 0, max_distance));
    REFUSE_POISONED(idx);
    HIP_TRY(hipSetDevice(idx->device));
    try {
        if (n_sd == 0) {  // nothing is launched
            *out = new asgart_alignment;
            (*out)->run_offsets.assign(1, 0);
            return 0;
        }
        return run_tool<AlignWork>(out, [&](AlignWork &w, asgart_alignment *res) {
            return run_align(w, res, idx, sds, flags, n_sd, inclusive != 0, budget_bytes, max_distance,
                             banded && !max_distance);
        });
    } catch (const std::bad_alloc &) {
        set_error("%s: out of host memory", fn);
        return ASGART_E_OOM;
    }
}

}  // namespace

extern "C" int32_t asgart_align_duplications(asgart_index *idx, const asgart_proto_sd *sds, const uint8_t *flags,
                                             int64_t n_sd, int32_t inclusive, uint64_t budget_bytes,
                                             asgart_alignment **out) {
    return align_entry("asgart_align_duplications", idx, sds, flags, n_sd, inclusive, false, nullptr, budget_bytes, out);
}

extern "C" int32_t asgart_align_duplications_banded(asgart_index *idx, const asgart_proto_sd *sds, const uint8_t *flags,
                                                    int64_t n_sd, int32_t inclusive, const uint32_t *max_distance,
                                                    uint64_t budget_bytes, asgart_alignment **out) {
    return align_entry("asgart_align_duplications_banded", idx, sds, flags, n_sd, inclusive, true, max_distance,
                       budget_bytes, out);
}

extern "C" int32_t asgart_alignment_rounds(const asgart_alignment *a, uint32_t *rounds, uint64_t *cells) {
    if (!a) {
        set_error("asgart_alignment_rounds: bad argument");
        return ASGART_E_ARG;
    }
    if (rounds) *rounds = a->rounds;
    if (cells) *cells = a->cells;
    return 0;
}

extern "C" void asgart_alignment_counts(const asgart_alignment *a, uint64_t *n_sd, uint64_t *n_runs, uint64_t *n_refused) {
    if (n_sd) *n_sd = a ? a->run_offsets.size() - 1 : 0;
    if (n_runs) *n_runs = a ? a->run_len.size() : 0;
    if (n_refused) *n_refused = a ? a->n_refused : 0;
}

extern "C" int32_t asgart_alignment_copy(const asgart_alignment *a, uint64_t *run_offsets, uint32_t *run_len, uint8_t *run_op,
                                         uint32_t *distance, float *identity, uint8_t *status) {
    if (!a) {
        set_error("asgart_alignment_copy: bad argument");
        return ASGART_E_ARG;
    }
    const size_t n = a->run_offsets.size() - 1, nr = a->run_len.size();
    if (run_offsets) memcpy(run_offsets, a->run_offsets.data(), (n + 1) * 8);
    if (run_len && nr) memcpy(run_len, a->run_len.data(), nr * 4);
    if (run_op && nr) memcpy(run_op, a->run_op.data(), nr);
    if (distance && n) memcpy(distance, a->distance.data(), n * 4);
    if (identity && n) memcpy(identity, a->identity.data(), n * 4);
    if (status && n) memcpy(status, a->status.data(), n);
    return 0;
}

extern "C" int32_t asgart_alignment_timings(const asgart_alignment *a, double *ms4) {
    if (!a || !ms4) {
        set_error("asgart_alignment_timings: bad argument");
        return ASGART_E_ARG;
    }
    for (int k = 0; k < 4; ++k) ms4[k] = a->ms[k];
    return 0;
}

extern "C" void asgart_alignment_free(asgart_alignment *a) { delete a; }

extern "C" void asgart_align_geometry(uint64_t *band_rows, uint64_t *lane_rows, uint64_t *tile_cols) {
    if (band_rows) *band_rows = kLevBand;
    if (lane_rows) *lane_rows = kLevRows;
    if (tile_cols) *tile_cols = kAlignTile;
}

extern "C" int32_t asgart_align_bytes_banded(const asgart_proto_sd *sds, int64_t n_sd, int32_t inclusive,
                                             const uint32_t *max_distance, uint64_t *bytes) {
    const char *fn = "asgart_align_bytes_banded";
    if (!bytes || !max_distance) {
        set_error("%s: bad argument", fn);
        return ASGART_E_ARG;
    }
    RC_TRY(check_list_args(fn, sds, n_sd, bytes));
    RC_TRY(check_banded(fn, sds, n_sd, inclusive != 0, max_distance));
    for (int64_t q = 0; q < n_sd; ++q) bytes[q] = banded_shape(sds[q], inclusive != 0, max_distance[q]).bytes();
    return 0;
}

extern "C" int32_t asgart_align_bytes(const asgart_proto_sd *sds, int64_t n_sd, int32_t inclusive, uint64_t *bytes) {
    if (!bytes) {
        set_error("asgart_align_bytes: bad argument");
        return ASGART_E_ARG;
    }
    RC_TRY(check_list_args("asgart_align_bytes", sds, n_sd, bytes));
    for (int64_t q = 0; q < n_sd; ++q) bytes[q] = align_shape(sds[q], inclusive != 0).bytes();
    return 0;
}
