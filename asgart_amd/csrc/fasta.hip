// fasta.hip -- FASTA files read on the GPU: asgart_fasta_*.
//
// Replaces the FASTA reader in front of prepare_data, reference src/bin/asgart.rs:278-313 (bio::io::fasta::Reader and the
// per-record loop behind it) and the same reader of asgart-extract (src/bin/asgart-extract.rs:17-29): the bytes of the
// files go in, the record table, the raw strand (what asgart_source holds), the normalised strand with its '$', the
// chunks and an index come out.  The rules are those of prep.read_records (asgart_amd/prep.py), the project's stand-in
// for bio's reader:
//   * lines end at '\n'; a '\r' is dropped iff nothing but '\r's lie between it and the next '\n' or the end of the file;
//   * a line whose first byte is '>' starts a record, whatever precedes a file's first such line is ignored;
//   * every other byte of a record is sequence (a '\r' in mid-line and a '>' in mid-line included).
// Per staging piece (kPiece file bytes, copied through pinned memory while the kernels of the piece before run) three
// launches:
//   fasta_classify_kernel  one workgroup per tile of kTile bytes: what the tile does to the state that crosses tiles
//                          (TileSum: does a line start in it and of which kind is the last; is it all '\r' and, if not,
//                          is its first other byte a '\n'; its header lines; its kept bytes under each of the four
//                          combinations of the two things it cannot know -- the kind of the line it starts in and
//                          whether a '\r' run at its end is dropped);
//   fasta_scan_kernel      one workgroup: resolves both unknowns for every tile (the line kind travels forwards, the
//                          fate of a trailing '\r' run backwards: over any number of tiles, to the end of the piece,
//                          where the host says what follows) and scans kept bytes and headers exclusively, 64-bit, on
//                          top of the carry the piece before left on the device;
//   fasta_write_kernel     one workgroup per tile: classifies again (the piece is 16 MiB: the second read is served by
//                          the cache), stages the kept bytes in LDS in output order and writes the raw and the
//                          normalised strand as aligned 16-byte vectors -- the vectors its span only shares with a
//                          neighbouring tile byte by byte -- and the record table entries of its header lines.
// No workgroup waits for another one: the order between tiles is the order of the launches.
#include "index.hpp"
#include "prep.hpp"
#include "tool_base.hpp"

#include <algorithm>

namespace asgart {
namespace {

constexpr uint32_t kBlock = 256;                // lanes per workgroup; each owns 16 consecutive file bytes
constexpr uint32_t kTile = kBlock * 16u;        // file bytes per workgroup
constexpr uint64_t kPiece = 16ull << 20;        // file bytes per staging piece (a multiple of kTile)
constexpr uint32_t kHead = 16;                  // bytes in front of a piece in its buffers; the last is the file byte before it
constexpr uint32_t kScanBlock = 1024;
constexpr uint64_t kNoEnd = ~0ull;              // header end of a record whose header line the file ends in
static_assert(kPiece % kTile == 0, "a piece is a whole number of tiles");

struct TileSum {
    uint32_t kept[4];  // [2 * (starts in a header line) + (a trailing '\r' run is dropped)]
    uint32_t n_hdr;
    uint32_t flags;    // 1: a line starts here, 2: the last such line is a header, 4: not all '\r', 8: first other byte is '\n'
};
struct TilePre {
    uint64_t out;      // kept bytes in front of the tile (strand position of its first kept byte)
    uint64_t rec;      // header lines in front of the tile
    uint32_t flags;    // 1: the tile starts inside a header line, 2: a '\r' run at its end is dropped
    uint32_t pad;
};
struct Carry {         // what a piece leaves for the next one (device memory)
    uint64_t out, rec, kind, pad;
};

struct LaneBits {
    uint32_t valid, nl, cr, gt, ls;  // one bit per byte of the lane: inside the piece, '\n', '\r', '>', first byte of a line
    uint32_t hm0, prefix;            // header-line bytes if the lane starts in a sequence line; bytes in front of its first line start
    uint32_t drop0, tail;            // dropped '\r's if what follows the lane is sequence; the '\r' run at its end
    __device__ inline uint32_t hdr_bytes(bool kind) const { return hm0 | (kind ? prefix : 0u); }
    __device__ inline uint32_t keep(bool kind, bool after) const {
        return valid & ~hdr_bytes(kind) & ~nl & ~(drop0 | (after ? tail : 0u));
    }
};

__device__ inline LaneBits lane_bits(const uint4 v, uint32_t prev, uint32_t n_valid) {
    LaneBits b;
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    b.valid = n_valid >= 16u ? 0xFFFFu : ((1u << n_valid) - 1u);
    b.nl = b.cr = b.gt = 0;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const uint32_t c = (w[j >> 2] >> (8 * (j & 3))) & 0xFFu;
        b.nl |= (c == '\n' ? 1u : 0u) << j;
        b.cr |= (c == '\r' ? 1u : 0u) << j;
        b.gt |= (c == '>' ? 1u : 0u) << j;
    }
    b.nl &= b.valid;
    b.cr &= b.valid;
    b.gt &= b.valid;
    b.ls = ((b.nl << 1) | (prev == '\n' ? 1u : 0u)) & b.valid;
    b.prefix = b.ls ? ((b.ls & (0u - b.ls)) - 1u) : 0xFFFFu;
    uint32_t kind = 0;
    b.hm0 = 0;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        if ((b.ls >> j) & 1u) kind = (b.gt >> j) & 1u;
        b.hm0 |= kind << j;
    }
    const uint32_t other = b.valid & ~b.cr;
    b.tail = other ? (b.valid & ~((2u << (31 - __clz((int)other))) - 1u)) : b.valid;
    uint32_t d = 0;
    b.drop0 = 0;
#pragma unroll
    for (int j = 15; j >= 0; --j) {
        const uint32_t is_nl = (b.nl >> j) & 1u, is_cr = (b.cr >> j) & 1u, in = (b.valid >> j) & 1u;
        b.drop0 |= (is_cr & d) << j;
        d = in ? (is_nl ? 1u : (is_cr ? d : 0u)) : d;
    }
    return b;
}

struct LaneCtx {
    bool kind_known, kind, after_known, after;
};

// What a lane can learn from the other lanes of its tile: the kind of the line it starts in (from the last line start
// in front of it) and what follows the '\r' run at its end (from the first byte other than '\r' behind it).
// s_wave[4]: per wave the same four flags as TileSum::flags.  Returns the tile's flags through *tile_flags.
__device__ inline LaneCtx tile_context(const LaneBits &b, uint32_t *s_wave, uint32_t *tile_flags) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const bool has_ls = b.ls != 0;
    const bool last_kind = has_ls && ((b.gt >> (31 - __clz((int)b.ls))) & 1u);
    const uint32_t other = b.valid & ~b.cr;
    const bool has_other = other != 0;
    const bool first_nl = has_other && ((b.nl >> (__ffs((int)other) - 1)) & 1u);
    const unsigned long long m_ls = __ballot(has_ls), m_lk = __ballot(last_kind), m_ot = __ballot(has_other),
                             m_fn = __ballot(first_nl);
    if (lane == 0) {
        uint32_t f = 0;
        if (m_ls) f |= 1u | (((m_lk >> (63 - __clzll((long long)m_ls))) & 1ull) ? 2u : 0u);
        if (m_ot) f |= 4u | (((m_fn >> (__ffsll((long long)m_ot) - 1)) & 1ull) ? 8u : 0u);
        s_wave[wave] = f;
    }
    __syncthreads();
    LaneCtx c = {false, false, false, false};
    const unsigned long long below = m_ls & ((1ull << lane) - 1ull);
    if (below) {
        c.kind_known = true;
        c.kind = (m_lk >> (63 - __clzll((long long)below))) & 1ull;
    } else {
        for (int w = (int)wave - 1; w >= 0 && !c.kind_known; --w)
            if (s_wave[w] & 1u) {
                c.kind_known = true;
                c.kind = (s_wave[w] & 2u) != 0;
            }
    }
    const unsigned long long above = lane == 63u ? 0ull : (m_ot & (~0ull << (lane + 1u)));
    if (above) {
        c.after_known = true;
        c.after = (m_fn >> (__ffsll((long long)above) - 1)) & 1ull;
    } else {
        for (uint32_t w = wave + 1; w < kBlock / 64u && !c.after_known; ++w)
            if (s_wave[w] & 4u) {
                c.after_known = true;
                c.after = (s_wave[w] & 8u) != 0;
            }
    }
    uint32_t f = 0;
    for (uint32_t w = 0; w < kBlock / 64u; ++w) {
        if (s_wave[w] & 1u) f = (f & ~3u) | (s_wave[w] & 3u);
        if (!(f & 4u) && (s_wave[w] & 4u)) f |= s_wave[w] & 12u;
    }
    *tile_flags = f;
    return c;
}

__device__ inline uint32_t wave_sum(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor((int)v, o);
    return v;
}

// the 16 bytes of this lane and the byte in front of them; in[-1] is the file byte before the piece
__device__ inline LaneBits load_lane(const uint8_t *__restrict__ in, uint64_t len, uint32_t tile, uint4 *bytes) {
    const uint64_t pos = (uint64_t)tile * kTile + (uint64_t)threadIdx.x * 16u;
    const uint32_t n_valid = pos >= len ? 0u : (uint32_t)std::min<uint64_t>(16u, len - pos);
    uint4 v = make_uint4(0, 0, 0, 0);
    uint32_t prev = 0;
    if (n_valid) {  // (the buffer holds kPiece bytes and a pad: the whole vector may be read)
        v = *reinterpret_cast<const uint4 *>(in + pos);
        prev = in[(int64_t)pos - 1];
    }
    *bytes = v;
    return lane_bits(v, prev, n_valid);
}

__global__ __launch_bounds__(kBlock) void fasta_classify_kernel(const uint8_t *__restrict__ in, uint64_t len,
                                                                TileSum *__restrict__ sums) {
    __shared__ uint32_t s_wave[kBlock / 64u];
    __shared__ uint32_t s_cnt[kBlock / 64u][5];
    uint4 v;
    const LaneBits b = load_lane(in, len, blockIdx.x, &v);
    uint32_t flags;
    const LaneCtx c = tile_context(b, s_wave, &flags);
    uint32_t cnt[5];
#pragma unroll
    for (int h = 0; h < 4; ++h)
        cnt[h] = __popc(b.keep(c.kind_known ? c.kind : (h & 2) != 0, c.after_known ? c.after : (h & 1) != 0));
    cnt[4] = __popc(b.ls & b.gt);
#pragma unroll
    for (int h = 0; h < 5; ++h) cnt[h] = wave_sum(cnt[h]);
    if ((threadIdx.x & 63u) == 0)
        for (int h = 0; h < 5; ++h) s_cnt[threadIdx.x >> 6][h] = cnt[h];
    __syncthreads();
    if (threadIdx.x == 0) {
        TileSum t;
        uint32_t tot[5] = {0, 0, 0, 0, 0};
        for (uint32_t w = 0; w < kBlock / 64u; ++w)
            for (int h = 0; h < 5; ++h) tot[h] += s_cnt[w][h];
        for (int h = 0; h < 4; ++h) t.kept[h] = tot[h];
        t.n_hdr = tot[4];
        t.flags = flags;
        sums[blockIdx.x] = t;
    }
}

// One workgroup over the tiles of a piece (thread t: tiles [t * per, (t + 1) * per)).  first_of_file: the piece starts
// a file (at a header line: what the file before ended in does not matter); after_piece: what follows the piece makes
// a '\r' run at its end one that is dropped (only '\r's up to the next '\n' or the end of the file: the host looked).
__global__ __launch_bounds__(kScanBlock) void fasta_scan_kernel(const TileSum *__restrict__ sums, uint32_t n_tiles,
                                                                TilePre *__restrict__ pre, Carry *__restrict__ carry,
                                                                int first_of_file, int after_piece) {
    __shared__ uint32_t s_flags[kScanBlock];
    __shared__ uint64_t s_out[kScanBlock], s_rec[kScanBlock];
    const uint32_t t = threadIdx.x;
    const uint32_t per = (n_tiles + kScanBlock - 1) / kScanBlock;
    const uint32_t lo = std::min(t * per, n_tiles), hi = std::min(lo + per, n_tiles);
    const uint64_t out0 = carry->out, rec0 = carry->rec;
    const uint32_t kind0 = first_of_file ? 0u : (uint32_t)carry->kind;
    uint32_t f = 0;  // the thread's tiles as one: the same four flags
    for (uint32_t i = lo; i < hi; ++i) {
        const uint32_t g = sums[i].flags;
        if (g & 1u) f = (f & ~3u) | (g & 3u);
        if (!(f & 4u) && (g & 4u)) f |= g & 12u;
    }
    s_flags[t] = f;
    __syncthreads();
    uint32_t kind = kind0, after = after_piece ? 1u : 0u;
    for (int j = (int)t - 1; j >= 0; --j)
        if (s_flags[j] & 1u) {
            kind = (s_flags[j] >> 1) & 1u;
            break;
        }
    for (uint32_t j = t + 1; j < kScanBlock; ++j)
        if (s_flags[j] & 4u) {
            after = (s_flags[j] >> 3) & 1u;
            break;
        }
    // backwards: what follows every tile; forwards: the kind it starts in, and with both its kept bytes
    for (uint32_t i = hi; i > lo; --i) {
        pre[i - 1].flags = after << 1;
        const uint32_t g = sums[i - 1].flags;
        if (g & 4u) after = (g >> 3) & 1u;
    }
    uint64_t n_out = 0, n_rec = 0;
    for (uint32_t i = lo; i < hi; ++i) {
        const uint32_t a = (pre[i].flags >> 1) & 1u;
        pre[i].flags = (a << 1) | kind;
        n_out += sums[i].kept[2u * kind + a];
        n_rec += sums[i].n_hdr;
        const uint32_t g = sums[i].flags;
        if (g & 1u) kind = (g >> 1) & 1u;
    }
    s_out[t] = n_out;
    s_rec[t] = n_rec;
    __syncthreads();
    for (uint32_t o = 1; o < kScanBlock; o <<= 1) {  // inclusive scan of the threads' totals
        const uint64_t a = t >= o ? s_out[t - o] : 0ull, b = t >= o ? s_rec[t - o] : 0ull;
        __syncthreads();
        s_out[t] += a;
        s_rec[t] += b;
        __syncthreads();
    }
    uint64_t at_out = out0 + s_out[t] - n_out, at_rec = rec0 + s_rec[t] - n_rec;
    for (uint32_t i = lo; i < hi; ++i) {
        pre[i].out = at_out;
        pre[i].rec = at_rec;
        at_out += sums[i].kept[2u * (pre[i].flags & 1u) + ((pre[i].flags >> 1) & 1u)];
        at_rec += sums[i].n_hdr;
    }
    if (t == kScanBlock - 1) {  // (its tiles, if it has any, are the last ones: kind is the piece's last)
        carry->out = at_out;
        carry->rec = at_rec;
        carry->kind = kind;
    }
}

struct RecTable {
    uint64_t *start;   // [cap + 1] strand position of the record's first base
    uint64_t *hoff;    // [cap] file offset of its '>'
    uint64_t *hend;    // [cap] file offset of the '\n' that ends its header line (kNoEnd: the file ends in the line)
    uint32_t *file;    // [cap]
    uint64_t cap;
};

__global__ __launch_bounds__(kBlock) void fasta_write_kernel(const uint8_t *__restrict__ in, uint64_t len,
                                                             const TilePre *__restrict__ pre, uint64_t file_off,
                                                             uint32_t file, int skip_masked, uint8_t *__restrict__ raw,
                                                             uint8_t *__restrict__ text, uint64_t out_cap, RecTable rt) {
    __shared__ uint32_t s_wave[kBlock / 64u];
    __shared__ uint32_t s_pk[kBlock / 64u], s_ph[kBlock / 64u];
    __shared__ __attribute__((aligned(16))) uint8_t s_stage[kTile + 32u];
    uint4 v;
    const LaneBits b = load_lane(in, len, blockIdx.x, &v);
    uint32_t tile_flags;
    const LaneCtx c = tile_context(b, s_wave, &tile_flags);
    const TilePre p = pre[blockIdx.x];
    const bool kind = c.kind_known ? c.kind : (p.flags & 1u) != 0;
    const bool after = c.after_known ? c.after : (p.flags & 2u) != 0;
    const uint32_t keep = b.keep(kind, after), hdr = b.ls & b.gt;
    // exclusive prefixes of the kept bytes and of the header lines inside the tile
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t ik = __popc(keep), ih = __popc(hdr);
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t a = (uint32_t)__shfl_up((int)ik, o), h = (uint32_t)__shfl_up((int)ih, o);
        if (lane >= (uint32_t)o) {
            ik += a;
            ih += h;
        }
    }
    if (lane == 63u) {
        s_pk[wave] = ik;
        s_ph[wave] = ih;
    }
    __syncthreads();
    uint32_t k0 = ik - __popc(keep), h0 = ih - __popc(hdr), n_kept = 0;
    for (uint32_t w = 0; w < kBlock / 64u; ++w) {
        if (w < wave) {
            k0 += s_pk[w];
            h0 += s_ph[w];
        }
        n_kept += s_pk[w];
    }
    const uint64_t pos = file_off + (uint64_t)blockIdx.x * kTile + (uint64_t)threadIdx.x * 16u;
    // record table: a header line starts a record; the '\n' of a header line ends that record's header
    for (uint32_t m = hdr; m; m &= m - 1u) {
        const uint32_t j = (uint32_t)__ffs((int)m) - 1u, lowj = (1u << j) - 1u;
        const uint64_t r = p.rec + h0 + __popc(hdr & lowj);
        if (r < rt.cap) {
            rt.start[r] = p.out + k0 + __popc(keep & lowj);
            rt.hoff[r] = pos + j;
            rt.file[r] = file;
        }
    }
    for (uint32_t m = b.nl & b.hdr_bytes(kind); m; m &= m - 1u) {  // a '\n' of a header line: of the last header up to it
        const uint32_t j = (uint32_t)__ffs((int)m) - 1u;
        const uint64_t seen = p.rec + h0 + __popc(hdr & ((2u << j) - 1u));
        if (seen > 0 && seen - 1 < rt.cap) rt.hend[seen - 1] = pos + j;
    }
    // the kept bytes into LDS in output order, shifted so that LDS offset 0 is a 16-byte boundary of the output
    const uint32_t sh = (uint32_t)(p.out & 15u);
    {
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
        uint32_t q = sh + k0;
#pragma unroll
        for (int j = 0; j < 16; ++j)
            if ((keep >> j) & 1u) s_stage[q++] = (uint8_t)((w[j >> 2] >> (8 * (j & 3))) & 0xFFu);
    }
    __syncthreads();
    const uint32_t end = sh + n_kept;             // the tile's span of the stage: [sh, end)
    const uint64_t g0 = p.out - sh;               // output position of stage offset 0
    for (uint32_t v = threadIdx.x; v * 16u < end; v += kBlock) {
        const uint32_t lo = v * 16u, hi = lo + 16u;
        if (g0 + hi > out_cap) continue;          // (cannot happen: the buffers hold every file byte and a pad)
        if (lo >= sh && hi <= end) {
            const uint4 x = *reinterpret_cast<const uint4 *>(s_stage + lo);
            *reinterpret_cast<uint4 *>(raw + g0 + lo) = x;
            uint32_t w[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                uint32_t o = 0;
#pragma unroll
                for (int k = 0; k < 4; ++k) o |= norm_byte((w[a] >> (8 * k)) & 0xFFu, skip_masked != 0) << (8 * k);
                w[a] = o;
            }
            *reinterpret_cast<uint4 *>(text + g0 + lo) = make_uint4(w[0], w[1], w[2], w[3]);
        } else {  // shared with the tile in front or behind: only the bytes of this one
            for (uint32_t x = std::max(lo, sh); x < std::min(hi, end); ++x) {
                const uint32_t ch = s_stage[x];
                raw[g0 + x] = (uint8_t)ch;
                text[g0 + x] = (uint8_t)norm_byte(ch, skip_masked != 0);
            }
        }
    }
}

// first header line of a file: offset of its '>' (len: none)
uint64_t first_header(const uint8_t *f, uint64_t len) {
    if (!len) return len;
    if (f[0] == '>') return 0;
    const void *hit = memmem(f, (size_t)len, "\n>", 2);
    return hit ? (uint64_t)(static_cast<const uint8_t *>(hit) - f) + 1u : len;
}

// does a '\r' run that ends at f[at - 1] continue to a '\n' or to the end of the file?
bool run_is_dropped(const uint8_t *f, uint64_t len, uint64_t at) {
    while (at < len && f[at] == '\r') ++at;
    return at == len || f[at] == '\n';
}

}  // namespace
}  // namespace asgart

using namespace asgart;

struct asgart_fasta {
    int32_t device = 0;
    uint64_t n_bases = 0;                      // the strand without its '$'
    DevBuf raw, text;                          // raw: n_bases bytes (+ pad); text: n_bases + 1 bytes (+ pad)
    bool raw_taken = false;
    std::vector<asgart_fasta_record> records;
    std::vector<uint64_t> chunks;              // (start, len) pairs
    double ms[4] = {0, 0, 0, 0};               // whole call, host staging copies, host -> device copies, kernels
};

namespace {

struct Reader {  // everything asgart_fasta_read holds only while it runs
    hipStream_t s_copy = nullptr, s_k = nullptr;
    hipEvent_t ev_c0[2] = {}, ev_c1[2] = {}, ev_k0[2] = {}, ev_k1[2] = {};
    uint8_t *h_stage[2] = {nullptr, nullptr};
    DevBuf d_in[2], d_sums, d_pre, d_carry, d_start, d_hoff, d_hend, d_file;
    bool used[2] = {false, false};
    double ms_h2d = 0, ms_kernels = 0;
    int32_t collect(int slot) {  // waits for the piece in `slot` and adds its times
        if (!used[slot]) return 0;
        HIP_TRY(hipEventSynchronize(ev_k1[slot]));
        float a = 0, b = 0;
        HIP_TRY(hipEventElapsedTime(&a, ev_c0[slot], ev_c1[slot]));
        HIP_TRY(hipEventElapsedTime(&b, ev_k0[slot], ev_k1[slot]));
        ms_h2d += a;
        ms_kernels += b;
        used[slot] = false;
        return 0;
    }
    void release() {
        if (s_copy) (void)hipStreamSynchronize(s_copy);
        if (s_k) (void)hipStreamSynchronize(s_k);
        for (int k = 0; k < 2; ++k) {
            for (hipEvent_t e : {ev_c0[k], ev_c1[k], ev_k0[k], ev_k1[k]})
                if (e) (void)hipEventDestroy(e);
            if (h_stage[k]) (void)hipHostFree(h_stage[k]);
            d_in[k].release();
        }
        for (DevBuf *b : {&d_sums, &d_pre, &d_carry, &d_start, &d_hoff, &d_hend, &d_file}) b->release();
        if (s_copy) (void)hipStreamDestroy(s_copy);
        if (s_k) (void)hipStreamDestroy(s_k);
    }
};

int32_t read_files(asgart_fasta *f, Reader &R, const uint8_t *const *files, const uint64_t *file_lens, int64_t n_files,
                   const std::vector<uint64_t> &first, uint64_t bound, int32_t skip_masked) {
    const auto t0 = std::chrono::steady_clock::now();
    double ms_stage = 0;
    const uint64_t rec_cap = std::min<uint64_t>((uint64_t)kMaxRecords + 1, bound / 2 + 1);
    const uint64_t out_cap = bound + 96;  // '$', the 64 bytes behind it, and a whole last vector
    HIP_TRY(hipStreamCreateWithFlags(&R.s_copy, hipStreamNonBlocking));
    HIP_TRY(hipStreamCreateWithFlags(&R.s_k, hipStreamNonBlocking));
    const uint64_t piece_max = std::min<uint64_t>(kPiece, (bound + kTile - 1) / kTile * kTile);
    const uint32_t tiles_max = (uint32_t)(piece_max / kTile);
    for (int k = 0; k < 2; ++k) {
        for (hipEvent_t *e : {&R.ev_c0[k], &R.ev_c1[k], &R.ev_k0[k], &R.ev_k1[k]}) HIP_TRY(hipEventCreate(e));
        HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&R.h_stage[k]), (size_t)(kHead + piece_max), hipHostMallocDefault));
        RC_TRY(R.d_in[k].reserve((size_t)(kHead + piece_max + 64)));
    }
    RC_TRY(R.d_sums.reserve((size_t)tiles_max * sizeof(TileSum)));
    RC_TRY(R.d_pre.reserve((size_t)tiles_max * sizeof(TilePre)));
    RC_TRY(R.d_carry.reserve(sizeof(Carry)));
    RC_TRY(R.d_start.reserve((size_t)(rec_cap + 1) * 8));
    RC_TRY(R.d_hoff.reserve((size_t)rec_cap * 8));
    RC_TRY(R.d_hend.reserve((size_t)rec_cap * 8));
    RC_TRY(R.d_file.reserve((size_t)rec_cap * 4));
    RC_TRY(f->raw.reserve((size_t)out_cap));
    RC_TRY(f->text.reserve((size_t)out_cap));
    HIP_TRY(hipMemsetAsync(R.d_carry.p, 0, sizeof(Carry), R.s_k));
    HIP_TRY(hipMemsetAsync(R.d_hend.p, 0xFF, (size_t)rec_cap * 8, R.s_k));
    const RecTable rt = {R.d_start.as<uint64_t>(), R.d_hoff.as<uint64_t>(), R.d_hend.as<uint64_t>(),
                         R.d_file.as<uint32_t>(), rec_cap};
    uint64_t n_piece = 0;
    for (int64_t fi = 0; fi < n_files; ++fi) {
        const uint8_t *src = files[fi];
        const uint64_t len = file_lens[fi];
        for (uint64_t at = first[(size_t)fi]; at < len; at += kPiece, ++n_piece) {
            const int slot = (int)(n_piece & 1u);
            const uint64_t take = std::min(kPiece, len - at);
            RC_TRY(R.collect(slot));  // the piece before last: its copy has left the pinned buffer, its kernels d_in
            const auto c0 = std::chrono::steady_clock::now();
            R.h_stage[slot][kHead - 1] = at == first[(size_t)fi] ? (uint8_t)'\n' : src[at - 1];
            memcpy(R.h_stage[slot] + kHead, src + at, (size_t)take);
            ms_stage += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - c0).count();
            const bool after = src[at + take - 1] == '\r' && run_is_dropped(src, len, at + take);
            uint8_t *d_in = R.d_in[slot].as<uint8_t>();
            HIP_TRY(hipEventRecord(R.ev_c0[slot], R.s_copy));
            HIP_TRY(hipMemcpyAsync(d_in + kHead - 1, R.h_stage[slot] + kHead - 1, (size_t)take + 1, hipMemcpyHostToDevice,
                                   R.s_copy));
            HIP_TRY(hipEventRecord(R.ev_c1[slot], R.s_copy));
            HIP_TRY(hipStreamWaitEvent(R.s_k, R.ev_c1[slot], 0));
            const uint32_t n_tiles = (uint32_t)((take + kTile - 1) / kTile);
            HIP_TRY(hipEventRecord(R.ev_k0[slot], R.s_k));
            fasta_classify_kernel<<<n_tiles, kBlock, 0, R.s_k>>>(d_in + kHead, take, R.d_sums.as<TileSum>());
            fasta_scan_kernel<<<1, kScanBlock, 0, R.s_k>>>(R.d_sums.as<TileSum>(), n_tiles, R.d_pre.as<TilePre>(),
                                                           R.d_carry.as<Carry>(), at == first[(size_t)fi] ? 1 : 0,
                                                           after ? 1 : 0);
            fasta_write_kernel<<<n_tiles, kBlock, 0, R.s_k>>>(d_in + kHead, take, R.d_pre.as<TilePre>(), at, (uint32_t)fi,
                                                              skip_masked, f->raw.as<uint8_t>(), f->text.as<uint8_t>(),
                                                              out_cap, rt);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipEventRecord(R.ev_k1[slot], R.s_k));
            R.used[slot] = true;
        }
    }
    RC_TRY(R.collect(0));
    RC_TRY(R.collect(1));
    Carry h_carry = {0, 0, 0, 0};
    HIP_TRY(read_back(&h_carry, R.d_carry.p, sizeof(Carry), R.s_k));
    if (h_carry.rec > (uint64_t)kMaxRecords) {
        set_error("asgart_fasta_read: %llu records, more than %lld", (unsigned long long)h_carry.rec, (long long)kMaxRecords);
        return ASGART_E_CAP;
    }
    if (h_carry.rec == 0 || h_carry.out > bound) {
        set_error("asgart_fasta_read: internal: %llu records, %llu bases out of %llu bytes", (unsigned long long)h_carry.rec,
                  (unsigned long long)h_carry.out, (unsigned long long)bound);
        return ASGART_E_HIP;
    }
    const uint64_t n_rec = h_carry.rec, n_bases = h_carry.out;
    f->n_bases = n_bases;
    HIP_TRY(hipMemcpyAsync(rt.start + n_rec, &n_bases, 8, hipMemcpyHostToDevice, R.s_k));
    HIP_TRY(stream_sync(R.s_k));
    RC_TRY(finish_text(f->text.as<uint8_t>(), n_bases, R.s_k));
    std::vector<uint64_t> runs, start((size_t)n_rec + 1), hoff((size_t)n_rec), hend((size_t)n_rec);
    std::vector<uint32_t> file((size_t)n_rec);
    RC_TRY(find_long_n_runs("asgart_fasta_read", f->text.as<uint8_t>(), n_bases, rt.start, (int64_t)n_rec, R.s_k, runs));
    HIP_TRY(read_back(start.data(), rt.start, ((size_t)n_rec + 1) * 8, R.s_k));
    HIP_TRY(read_back(hoff.data(), rt.hoff, (size_t)n_rec * 8, R.s_k));
    HIP_TRY(read_back(hend.data(), rt.hend, (size_t)n_rec * 8, R.s_k));
    HIP_TRY(read_back(file.data(), rt.file, (size_t)n_rec * 4, R.s_k));
    chunks_from_runs(start.data(), (int64_t)n_rec, runs, f->chunks);
    f->records.resize((size_t)n_rec);
    for (size_t r = 0; r < (size_t)n_rec; ++r) {
        asgart_fasta_record &o = f->records[r];
        o.file = file[r];
        o.header_offset = hoff[r];
        o.header_len = (hend[r] == kNoEnd ? file_lens[file[r]] : hend[r]) - hoff[r];
        o.start = start[r];
        o.len = start[r + 1] - start[r];
    }
    f->ms[0] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    f->ms[1] = ms_stage;
    f->ms[2] = R.ms_h2d;
    f->ms[3] = R.ms_kernels;
    return 0;
}

}  // namespace

extern "C" void asgart_fasta_geometry(uint64_t *tile_bytes, uint64_t *piece_bytes, uint64_t *vector_bytes) {
    if (tile_bytes) *tile_bytes = kTile;
    if (piece_bytes) *piece_bytes = kPiece;
    if (vector_bytes) *vector_bytes = 16;
}

extern "C" int32_t asgart_fasta_read(const uint8_t *const *files, const uint64_t *file_lens, int64_t n_files,
                                     int32_t skip_masked, int32_t device, asgart_fasta **out) {
    if (out) *out = nullptr;
    if (!out || !files || !file_lens || n_files <= 0) {
        set_error("asgart_fasta_read: bad argument");
        return ASGART_E_ARG;
    }
    std::vector<uint64_t> first((size_t)n_files);
    uint64_t bound = 0;  // file bytes from each file's first header line on: no strand is longer
    for (int64_t i = 0; i < n_files; ++i) {
        if (file_lens[i] && !files[i]) {
            set_error("asgart_fasta_read: file %lld is NULL", (long long)i);
            return ASGART_E_ARG;
        }
        first[(size_t)i] = first_header(files[i], file_lens[i]);
        bound += file_lens[i] - first[(size_t)i];
    }
    if (bound == 0) {
        set_error("asgart_fasta_read: no record in %lld file(s) (no line starts with '>')", (long long)n_files);
        return ASGART_E_ARG;
    }
    RC_TRY(use_device("asgart_fasta_read", device));
    asgart_fasta *f = new asgart_fasta;
    f->device = device;
    Reader R;
    const int32_t rc = read_files(f, R, files, file_lens, n_files, first, bound, skip_masked);
    R.release();
    if (rc != 0) {
        asgart_fasta_free(f);
        return rc;
    }
    *out = f;
    return 0;
}

extern "C" int32_t asgart_fasta_counts(const asgart_fasta *f, int64_t *n_records, int64_t *n_chunks, uint64_t *n_text) {
    if (!f) {
        set_error("asgart_fasta_counts: bad argument");
        return ASGART_E_ARG;
    }
    if (n_records) *n_records = (int64_t)f->records.size();
    if (n_chunks) *n_chunks = (int64_t)(f->chunks.size() / 2);
    if (n_text) *n_text = f->n_bases + 1;
    return 0;
}

extern "C" int32_t asgart_fasta_read_text(const asgart_fasta *f, uint64_t lo, uint64_t hi, uint8_t *out) {
    if (!f || lo > hi || hi > f->n_bases + 1 || (hi > lo && !out)) {
        set_error("asgart_fasta_read_text: bad argument");
        return ASGART_E_ARG;
    }
    if (hi == lo) return 0;
    HIP_TRY(hipSetDevice(f->device));
    HIP_TRY(hipMemcpy(out, f->text.as<uint8_t>() + lo, (size_t)(hi - lo), hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int32_t asgart_fasta_copy(const asgart_fasta *f, asgart_fasta_record *records, uint64_t *chunks, uint8_t *text) {
    if (!f) {
        set_error("asgart_fasta_copy: bad argument");
        return ASGART_E_ARG;
    }
    if (records) memcpy(records, f->records.data(), f->records.size() * sizeof(asgart_fasta_record));
    if (chunks) memcpy(chunks, f->chunks.data(), f->chunks.size() * 8);
    if (text) return asgart_fasta_read_text(f, 0, f->n_bases + 1, text);
    return 0;
}

extern "C" int32_t asgart_fasta_timings(const asgart_fasta *f, double *ms4) {
    if (!f || !ms4) {
        set_error("asgart_fasta_timings: bad argument");
        return ASGART_E_ARG;
    }
    for (int k = 0; k < 4; ++k) ms4[k] = f->ms[k];
    return 0;
}

extern "C" int32_t asgart_fasta_index(asgart_fasta *f, asgart_index **out) {
    if (out) *out = nullptr;
    if (!f || !out) {
        set_error("asgart_fasta_index: bad argument");
        return ASGART_E_ARG;
    }
    HIP_TRY(hipSetDevice(f->device));
    return index_over_text(f->text.as<uint8_t>(), f->n_bases + 1, f->device, out);
}

extern "C" int32_t asgart_fasta_source(asgart_fasta *f, asgart_source **out) {
    if (out) *out = nullptr;
    if (!f || !out || f->raw_taken) {
        set_error(f && f->raw_taken ? "asgart_fasta_source: the raw strand of this result has been handed out already"
                                    : "asgart_fasta_source: bad argument");
        return ASGART_E_ARG;
    }
    RC_TRY(source_adopt(f->raw, f->n_bases, f->device, out));
    f->raw_taken = true;
    return 0;
}

extern "C" void asgart_fasta_free(asgart_fasta *f) {
    if (!f) return;
    (void)hipSetDevice(f->device);
    f->raw.release();
    f->text.release();
    delete f;
}
