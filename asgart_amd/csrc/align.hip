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
};

// ---- forward: distances and checkpoints (the band loop written out, as in levenshtein_kernel) -----------------------
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
        uint32_t *rowck = colck + g.col_words();
        const uint64_t row_stride = g.m + 1u;
        uint32_t result = 0;
        uint32_t bi = 0;
        for (uint32_t band = 0; band < la && lb > 0; band += kLevBand, ++bi) {
            const uint32_t i0 = band + (uint32_t)lane * R;  // rows i0+1 .. i0+R (1-based) are this lane's
            const bool more_bands = band + kLevBand < la;
            const uint32_t *top_row = bi ? rowck + (uint64_t)(bi - 1u) * row_stride : rowck;  // (read for bi > 0 only)
            uint32_t *bottom_row = rowck + (uint64_t)bi * row_stride;                         // (written if more_bands)
            uint32_t a[R], col[R];
            lev_rows(a, i0, la, A);
            lev_first_column(col, i0);
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
                    b_chunk = s + (uint32_t)lane < lb ? rb.at(s + (uint32_t)lane) : 0u;
                }
                const LevIn in = lev_inputs(last_out, top_chunk, b_pipe, b_chunk, s, lane);
                const int64_t j = (int64_t)s - lane + 1;
                if (j >= 1 && j <= (int64_t)lb) {
                    lev_column<false>(a, col, diag_in, in);
                    last_out = col[R - 1];
                    if ((uint32_t)j == lb && la > i0 && la <= i0 + R) result = lev_row_value(col, i0, la);
                    // a column checkpoint: the lane's 16 values of column j, 64 contiguous bytes
                    if (((uint32_t)j & (W - 1u)) == 0u && (uint32_t)j < lb) {
                        uint4 *dst = reinterpret_cast<uint4 *>(colck + (uint64_t)((uint32_t)j / W - 1u) * g.rows_padded + i0);
#pragma unroll
                        for (int v4 = 0; v4 < R / 4; ++v4)
                            dst[v4] = make_uint4(col[4 * v4], col[4 * v4 + 1], col[4 * v4 + 2], col[4 * v4 + 3]);
                    }
                }
                if (more_bands) lev_store_bottom(last_out, s, lane, lb, out_chunk, bottom_row);
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
        const uint32_t *rowck = colck + g.col_words();
        const uint64_t row_stride = g.m + 1u;
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
            const uint32_t wt = min(W, lb - j0);  // columns j0+1 .. j0+wt
            const uint32_t *top_row = b ? rowck + (uint64_t)(b - 1u) * row_stride : rowck;  // D[band][..] (read for b > 0 only)
            {
                // rebuild the tile: the forward step, seeded with the column left of the tile and the cell above it
                const uint32_t i0 = band + (uint32_t)lane * R;
                uint32_t a[R], col[R];
                if (cb == 0) {
                    lev_first_column(col, i0);
                } else {
                    const uint4 *src = reinterpret_cast<const uint4 *>(colck + (uint64_t)(cb - 1u) * g.rows_padded + i0);
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
                if (lane == 0) diag_in = b == 0 ? j0 : (j0 == 0 ? band : top_row[j0]);
                uint32_t last_out = 0, b_pipe = 0, top_chunk = 0, b_chunk = 0;
                const uint32_t n_steps = wt + 63u;
                for (uint32_t s = 0; s < n_steps; ++s) {
                    if ((s & 63u) == 0u) {
                        const uint32_t j1 = j0 + s + 1u + (uint32_t)lane;
                        top_chunk = b == 0 ? j1 : (j1 <= lb ? top_row[j1] : 0u);
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
            while (i > band && j > j0) {
                const uint32_t row = i - 1u - band;
                const uint32_t d = (dirs[(j - 1u - j0) * 64u + row / R] >> (2u * (row % R))) & 3u;
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
};

namespace {

struct AlignWork : ToolWork {
    DevBuf &sds = buf(), &flags = buf(), &distance = buf(), &identity = buf(), &counters = buf();
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

int32_t run_batch(AlignWork &w, asgart_alignment *res, const asgart_index *idx, const asgart_proto_sd *sds, bool has_flags,
                  int inclusive, BatchRuns &br) {
    hipStream_t s = w.s;
    const uint64_t nk = br.members.size();
    // served largest first; the checkpoints of member k start at ck_off[k] (slots of whole 16-byte vectors)
    std::vector<uint32_t> order((size_t)nk);
    std::vector<uint64_t> ck_off((size_t)nk);
    uint64_t words = 0;
    for (uint64_t k = 0; k < nk; ++k) {
        order[(size_t)k] = (uint32_t)k;
        ck_off[(size_t)k] = words;
        words += (align_shape(sds[br.members[(size_t)k]], inclusive).bytes() / 4u + 3u) & ~(uint64_t)3;
    }
    auto cells = [&](uint32_t k) {
        const AlignShape g = align_shape(sds[br.members[k]], inclusive);
        return (double)g.n * (double)g.m;
    };
    std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return cells(x) > cells(y); });

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

    const Batch bt{w.sds.as<asgart_proto_sd>(), has_flags ? w.flags.as<uint8_t>() : nullptr, w.members.as<uint32_t>(),
                   w.order.as<uint32_t>(), w.ck_off.as<uint64_t>(), nk, inclusive};
    uint32_t *d_dist = w.distance.as<uint32_t>();
    const unsigned waves_per_wg = kFwdThreads / 64;
    const unsigned grid_f = (unsigned)std::min<uint64_t>((nk + waves_per_wg - 1) / waves_per_wg, 1024);
    align_forward_kernel<<<grid_f, kFwdThreads, 0, s>>>(idx->d_text, bt, w.ck.as<uint32_t>(), cursors, d_dist,
                                                         w.identity.as<float>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(w.ev[2], s));

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
    align_traceback_kernel<<<grid_t, 64, 0, s>>>(idx->d_text, bt, w.ck.as<uint32_t>(), d_dist, slot_off,
                                                 w.slot_len.as<uint32_t>(), w.slot_op.as<uint8_t>(), n_runs, cursors + 1,
                                                 overflow);
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

int32_t run_align(AlignWork &w, asgart_alignment *res, const asgart_index *idx, const asgart_proto_sd *sds,
                  const uint8_t *flags, int64_t n_sd, int inclusive, uint64_t budget) {
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

    // batches: largest first, a new one whenever the next duplication no longer fits
    res->status.assign((size_t)n_sd, 1);
    std::vector<uint64_t> bytes((size_t)n_sd);
    std::vector<uint32_t> by_size;
    for (int64_t q = 0; q < n_sd; ++q) {
        bytes[(size_t)q] = align_shape(sds[q], inclusive).bytes();
        if (bytes[(size_t)q] > budget) {
            res->status[(size_t)q] = 0;
            ++res->n_refused;
        } else {
            by_size.push_back((uint32_t)q);
        }
    }
    std::stable_sort(by_size.begin(), by_size.end(), [&](uint32_t x, uint32_t y) { return bytes[x] > bytes[y]; });
    std::vector<BatchRuns> batches;
    uint64_t held = 0;
    for (uint32_t q : by_size) {
        if (batches.empty() || held + bytes[q] > budget) {
            batches.emplace_back();
            held = 0;
        }
        batches.back().members.push_back(q);
        held += bytes[q];
    }
    std::vector<uint32_t> batch_of((size_t)n_sd, 0), slot_of((size_t)n_sd, 0);
    for (size_t b = 0; b < batches.size(); ++b) {
        BatchRuns &br = batches[b];
        std::sort(br.members.begin(), br.members.end());
        for (size_t k = 0; k < br.members.size(); ++k) {
            batch_of[br.members[k]] = (uint32_t)b;
            slot_of[br.members[k]] = (uint32_t)k;
        }
        RC_TRY(run_batch(w, res, idx, sds, flags != nullptr, inclusive, br));
    }

    const auto t0 = std::chrono::steady_clock::now();
    res->distance.resize((size_t)n_sd);
    res->identity.resize((size_t)n_sd);
    HIP_TRY(read_back(res->distance.data(), w.distance.p, (size_t)n_sd * 4, s));
    HIP_TRY(read_back(res->identity.data(), w.identity.p, (size_t)n_sd * 4, s));
    res->run_offsets.assign((size_t)n_sd + 1, 0);
    for (int64_t q = 0; q < n_sd; ++q) {
        uint64_t runs = 0;
        if (res->status[(size_t)q]) {
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
        if (!res->status[(size_t)q]) continue;
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

extern "C" int32_t asgart_align_duplications(asgart_index *idx, const asgart_proto_sd *sds, const uint8_t *flags,
                                             int64_t n_sd, int32_t inclusive, uint64_t budget_bytes,
                                             asgart_alignment **out) {
    const char *fn = "asgart_align_duplications";
    if (out) *out = nullptr;
    if (!idx || !out) {  // (the result is made for an empty list too)
        set_error("%s: bad argument", fn);
        return ASGART_E_ARG;
    }
    RC_TRY(check_list_args(fn, sds, n_sd, out));
    RC_TRY(check_flags(fn, flags, n_sd));
    RC_TRY(check_arms(fn, (uint64_t)idx->n, sds, n_sd, inclusive != 0));
    REFUSE_POISONED(idx);
    HIP_TRY(hipSetDevice(idx->device));
    try {
        if (n_sd == 0) {  // nothing is launched
            *out = new asgart_alignment;
            (*out)->run_offsets.assign(1, 0);
            return 0;
        }
        return run_tool<AlignWork>(out, [&](AlignWork &w, asgart_alignment *res) {
            return run_align(w, res, idx, sds, flags, n_sd, inclusive != 0, budget_bytes);
        });
    } catch (const std::bad_alloc &) {
        set_error("%s: out of host memory", fn);
        return ASGART_E_OOM;
    }
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

extern "C" int32_t asgart_align_bytes(const asgart_proto_sd *sds, int64_t n_sd, int32_t inclusive, uint64_t *bytes) {
    if (!bytes) {
        set_error("asgart_align_bytes: bad argument");
        return ASGART_E_ARG;
    }
    RC_TRY(check_list_args("asgart_align_bytes", sds, n_sd, bytes));
    for (int64_t q = 0; q < n_sd; ++q) bytes[q] = align_shape(sds[q], inclusive != 0).bytes();
    return 0;
}
