// result_read.hip -- result files read on the GPU: asgart_result_scan, asgart_result_parse and their handle.
//
// Replaces, for a result wanted as arrays, RunResult::from_file of reference src/structs.rs:105-112 (serde_json::from_reader
// into RunResult, the 13 fields of SD :471-495).  The rule is ACCEPT OR REFUSE, NEVER DIFFER: the grammar below (stated in
// include/asgart_hip.h) is a subset of what the host reader (asgart_amd.extract.parse_result) reads, and everything outside
// it is a refusal (ASGART_E_REFUSED, the byte offset and the rule in asgart_last_error) that the caller answers with the host
// reader.  What a record consists of is stated once, in result_read_dev.hpp.  Here:
//   scan    the file is cut into tiles of kTile bytes, one wave each, a lane 16 bytes.  Four passes, each carried across tiles
//           by a scan of one word per tile (rocPRIM): (1) backslash runs -- a tile's summary is (all backslashes, parity of its
//           trailing run), combined so that a run may span any number of tiles; (2) the quotes no odd run precedes, their
//           parity per tile; (3) the in-string mask as a prefix XOR of those quotes, and with it the tile's sum of brackets
//           outside strings; (4) a class byte per byte of the file (in string, quote, nesting depth) and the positions of the
//           tokens at depth 1.  The host reads those few tokens: the three top-level keys and the span of "families".
//   parse   inside that span the structural tokens of depths 2 to 4 (families' brackets, family brackets, record braces,
//           the commas between them) are counted, placed (count, scan, scatter) and checked pair by pair; the family
//           offsets are two scans over them.  A workgroup then owns kRecs consecutive records, so one contiguous byte range,
//           staged in LDS when it fits kStage (one thread walks one record); a range that does not fit (a name of thousands
//           of bytes is legal) is walked in global memory: slower, never refused.
// This file is compiled WITHOUT fast-math (the Makefile passes none): the identity of a record is one IEEE f64 multiply or
// divide by an exact power of ten and one cast, and both have to round as the host's float() and np.float32() do.
#include "tool_base.hpp"
#include "result_read_dev.hpp"

namespace asgart {
namespace {

constexpr uint32_t kTile = 1024;      // bytes per tile: one wave, 16 bytes a lane
constexpr uint32_t kLanes = 64;
constexpr uint32_t kRecs = 64;        // records per workgroup of the record stage, one thread each
constexpr uint32_t kStage = 40960;    // bytes of the LDS stage: 640 per record (a pretty record with short names has about 450)
constexpr uint32_t kTopMax = 64;      // depth-1 tokens of a conforming file: 19; more than this is a refusal
constexpr uint32_t kTopCap = 96;      // (room of the list: what is counted beyond it is not stored)

struct Ctrl {
    unsigned long long err;           // (byte offset << 8 | rule) of the first violation; ~0: none
    uint32_t n_top, end_in_string;
    int32_t end_depth;
    uint32_t n_hard_names, n_hard_ident, pad;
    uint32_t top[kTopCap];
};

template <class T, class Op>
__device__ __forceinline__ T wave_inclusive(T v, Op op) {
    const uint32_t lane = threadIdx.x & 63;
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const T o = __shfl_up(v, d);
        if (lane >= d) v = op(o, v);
    }
    return v;
}
struct PlusI32 {
    __device__ int32_t operator()(int32_t a, int32_t b) const { return a + b; }
};
struct PlusU32 {
    __device__ uint32_t operator()(uint32_t a, uint32_t b) const { return a + b; }
};

__device__ __forceinline__ uint32_t byte_of(const uint4 &w, uint32_t k) {
    const uint32_t word = k < 4 ? w.x : k < 8 ? w.y : k < 12 ? w.z : w.w;
    return (word >> (8 * (k & 3))) & 0xFFu;
}

// (1) the backslash summary of a tile
__global__ __launch_bounds__(kLanes) void rr_backslash_kernel(const uint4 *__restrict__ bytes, uint32_t *__restrict__ tile_bs) {
    const uint32_t lane = threadIdx.x, t = blockIdx.x;
    const uint4 w = bytes[(size_t)t * kLanes + lane];
    uint32_t all = 1, par = 0, open = 1;   // open: the trailing run still reaches back
#pragma unroll
    for (int k = 15; k >= 0; --k) {
        const bool bs = byte_of(w, (uint32_t)k) == '\\';
        if (!bs) all = 0, open = 0;
        par ^= (open && bs) ? 1u : 0u;
    }
    const uint32_t s = wave_inclusive(all << 1 | par, BsOp());
    if (lane == kLanes - 1) tile_bs[t] = s;
}

// (2) the quotes that are not escaped: 16 bits per lane, and the parity of their number in the tile
__global__ __launch_bounds__(kLanes) void rr_quotes_kernel(const uint4 *__restrict__ bytes, const uint32_t *__restrict__ bs_incl,
                                                           uint16_t *__restrict__ qmask, uint32_t *__restrict__ tile_q) {
    const uint32_t lane = threadIdx.x, t = blockIdx.x;
    const uint4 w = bytes[(size_t)t * kLanes + lane];
    uint32_t all = 1, par = 0, open = 1;
#pragma unroll
    for (int k = 15; k >= 0; --k) {
        const bool bs = byte_of(w, (uint32_t)k) == '\\';
        if (!bs) all = 0, open = 0;
        par ^= (open && bs) ? 1u : 0u;
    }
    const uint32_t seed = 2u | (t ? (bs_incl[t - 1] & 1u) : 0u);   // the run that reaches this tile, as an all-backslash element
    const uint32_t incl = wave_inclusive(all << 1 | par, BsOp());
    uint32_t before = __shfl_up(incl, 1);
    before = lane ? BsOp()(seed, before) : seed;
    uint32_t run = before & 1u, q = 0;
#pragma unroll
    for (uint32_t k = 0; k < 16; ++k) {
        const uint32_t c = byte_of(w, k);
        if (c == '\\') {
            run ^= 1u;
        } else {
            if (c == '"' && !run) q |= 1u << k;
            run = 0;
        }
    }
    qmask[(size_t)t * kLanes + lane] = (uint16_t)q;
    const unsigned long long odd = __ballot(__popc(q) & 1);
    if (lane == 0) tile_q[t] = (uint32_t)(__popcll(odd) & 1);
}

// the in-string state in front of this lane's bytes
__device__ __forceinline__ uint32_t string_state(uint32_t q, uint32_t tile_carry, uint32_t lane) {
    const unsigned long long odd = __ballot(__popc(q) & 1);
    return (tile_carry ^ (uint32_t)__popcll(odd & ((1ull << lane) - 1ull))) & 1u;
}

// (3) the sum of the brackets outside strings in a tile
__global__ __launch_bounds__(kLanes) void rr_depth_kernel(const uint4 *__restrict__ bytes, const uint16_t *__restrict__ qmask,
                                                          const uint32_t *__restrict__ carry_q, int32_t *__restrict__ tile_d) {
    const uint32_t lane = threadIdx.x, t = blockIdx.x;
    const uint4 w = bytes[(size_t)t * kLanes + lane];
    const uint32_t q = qmask[(size_t)t * kLanes + lane];
    uint32_t s = string_state(q, carry_q[t], lane);
    int32_t delta = 0;
#pragma unroll
    for (uint32_t k = 0; k < 16; ++k) {
        const uint32_t c = byte_of(w, k);
        if (q >> k & 1u) s ^= 1u;
        else if (!s) delta += (c == '{' || c == '[') ? 1 : (c == '}' || c == ']') ? -1 : 0;
    }
    const int32_t sum = wave_inclusive(delta, PlusI32());
    if (lane == kLanes - 1) tile_d[t] = sum;
}

// (4) the class byte of every byte, the depth-1 tokens, the state at the end of the file
__global__ __launch_bounds__(kLanes) void rr_classify_kernel(const uint4 *__restrict__ bytes, const uint16_t *__restrict__ qmask,
                                                             const uint32_t *__restrict__ carry_q,
                                                             const int32_t *__restrict__ carry_d, uint32_t size,
                                                             uint32_t n_tiles, uint4 *__restrict__ cls, Ctrl *__restrict__ ctrl) {
    const uint32_t lane = threadIdx.x, t = blockIdx.x;
    const uint4 w = bytes[(size_t)t * kLanes + lane];
    const uint32_t q = qmask[(size_t)t * kLanes + lane];
    const uint32_t s0 = string_state(q, carry_q[t], lane);
    uint32_t s = s0;
    int32_t delta = 0;
#pragma unroll
    for (uint32_t k = 0; k < 16; ++k) {
        const uint32_t c = byte_of(w, k);
        if (q >> k & 1u) s ^= 1u;
        else if (!s) delta += (c == '{' || c == '[') ? 1 : (c == '}' || c == ']') ? -1 : 0;
    }
    const int32_t incl = wave_inclusive(delta, PlusI32());
    int32_t depth = carry_d[t] + incl - delta;
    s = s0;
    uint32_t out[4] = {0, 0, 0, 0};
    const uint32_t at = t * kTile + lane * 16;
#pragma unroll
    for (uint32_t k = 0; k < 16; ++k) {
        const uint32_t c = byte_of(w, k);
        const bool quote = q >> k & 1u;
        uint32_t cl;
        int32_t d = depth;
        bool bracket = false;
        if (quote) {
            s ^= 1u;
            cl = kClsString | kClsQuote;
        } else if (s) {
            cl = kClsString;
        } else {
            cl = 0;
            if (c == '{' || c == '[') d = ++depth, bracket = true;        // an opener carries the depth it opens
            else if (c == '}' || c == ']') --depth, bracket = true;       // a closer the depth it closes
        }
        cl |= (uint32_t)min(max(d, 0), 15);
        out[k >> 2] |= cl << (8 * (k & 3));
        const bool top = bracket ? d <= 2 : quote ? d <= 1 : (!s && !is_ws(c) && d <= 1);
        if (top && at + k < size) {
            const uint32_t slot = atomicAdd(&ctrl->n_top, 1u);
            if (slot < kTopCap) ctrl->top[slot] = at + k;
        }
    }
    cls[(size_t)t * kLanes + lane] = make_uint4(out[0], out[1], out[2], out[3]);
    if (t == n_tiles - 1 && lane == kLanes - 1) {   // (the padding behind the file is spaces: the state of the last byte)
        ctrl->end_in_string = s;
        ctrl->end_depth = depth;
    }
}

__device__ __forceinline__ void refuse(Ctrl *ctrl, uint32_t pos, uint32_t rule) {
    atomicMin(&ctrl->err, (unsigned long long)pos << 8 | rule);
}

// The structural tokens of the families span [a, b): kScatter false counts them per tile, true places them.  Every byte of
// the span at depth 3 and less that is neither whitespace nor such a token is a refusal here; what lies inside a record
// (depth 4 and more) is the record walk's.
template <bool kScatter>
__global__ __launch_bounds__(kLanes) void rr_struct_kernel(const uint4 *__restrict__ bytes, const uint4 *__restrict__ cls,
                                                           uint32_t a, uint32_t b, uint32_t t0, uint32_t *__restrict__ tile_n,
                                                           uint32_t *__restrict__ tok_pos, Ctrl *__restrict__ ctrl) {
    const uint32_t lane = threadIdx.x, t = t0 + blockIdx.x;
    const uint4 w = bytes[(size_t)t * kLanes + lane], cw = cls[(size_t)t * kLanes + lane];
    const uint32_t at = t * kTile + lane * 16;
    uint32_t tok = 0;
#pragma unroll
    for (uint32_t k = 0; k < 16; ++k) {
        const uint32_t p = at + k;
        if (p < a || p >= b) continue;
        const uint32_t c = byte_of(w, k), cl = byte_of(cw, k), d = cl & kClsDepth;
        const int ty = struct_type(c, cl);
        if (ty >= 0) tok |= 1u << k;
        else if (ty == kStructBad && !kScatter) refuse(ctrl, p, d >= 4 ? kRuleNest : kRuleStray);
    }
    const uint32_t n = (uint32_t)__popc(tok);
    const uint32_t incl = wave_inclusive(n, PlusU32());
    if (!kScatter) {
        if (lane == kLanes - 1) tile_n[blockIdx.x] = incl;
        return;
    }
    uint32_t at_tok = tile_n[blockIdx.x] + incl - n;
#pragma unroll
    for (uint32_t k = 0; k < 16; ++k)
        if (tok >> k & 1u) tok_pos[at_tok++] = at + k;
}

__device__ __forceinline__ int token_type(const uint8_t *bytes, const uint8_t *cls, uint32_t pos) {
    return struct_type(bytes[pos], cls[pos]);
}

// the tokens pair by pair; is_fam / is_rec of every token and a closing zero
__global__ __launch_bounds__(256) void rr_pairs_kernel(const uint8_t *__restrict__ bytes, const uint8_t *__restrict__ cls,
                                                       const uint32_t *__restrict__ tok_pos, uint32_t n_tok,
                                                       uint32_t *__restrict__ is_fam, uint32_t *__restrict__ is_rec,
                                                       Ctrl *__restrict__ ctrl) {
    const uint32_t j = blockIdx.x * 256 + threadIdx.x;
    if (j > n_tok) return;
    if (j == n_tok) {
        is_fam[j] = is_rec[j] = 0;
        return;
    }
    const uint32_t pos = tok_pos[j];
    const int ty = token_type(bytes, cls, pos);
    is_fam[j] = ty == kTokFamOpen;
    is_rec[j] = ty == kTokRecOpen;
    bool ok;
    if (j + 1 == n_tok) {
        ok = ty == kTokAllClose;
    } else {
        const int nx = token_type(bytes, cls, tok_pos[j + 1]);
        ok = pair_allowed(ty, nx);
    }
    if (j == 0 && ty != kTokAllOpen) ok = false;
    if (!ok) refuse(ctrl, pos, kRuleStruct);
}

// the family offsets and the place of every record from the two scans; rec_pos[n] = b closes the last range
__global__ __launch_bounds__(256) void rr_place_kernel(const uint32_t *__restrict__ tok_pos, uint32_t n_tok,
                                                       const uint32_t *__restrict__ is_fam, const uint32_t *__restrict__ is_rec,
                                                       const uint32_t *__restrict__ rank_fam,
                                                       const uint32_t *__restrict__ rank_rec, uint32_t b,
                                                       uint64_t *__restrict__ offs, uint32_t *__restrict__ rec_pos) {
    const uint32_t j = blockIdx.x * 256 + threadIdx.x;
    if (j > n_tok) return;
    if (j == n_tok) {
        offs[rank_fam[j]] = rank_rec[j];
        rec_pos[rank_rec[j]] = b;
    } else if (is_fam[j]) {
        offs[rank_fam[j]] = rank_rec[j];
    } else if (is_rec[j]) {
        rec_pos[rank_rec[j]] = tok_pos[j];
    }
}

__global__ __launch_bounds__(kRecs) void rr_records_kernel(const uint8_t *__restrict__ bytes, const uint32_t *__restrict__ rec_pos,
                                                           uint32_t n, uint32_t b, NameTable table, RecordOut out,
                                                           Ctrl *__restrict__ ctrl) {
    __shared__ __align__(16) uint8_t stage[kStage];
    const uint32_t first = blockIdx.x * kRecs, last = min(first + kRecs, n);
    const uint32_t g0 = rec_pos[first], g1 = rec_pos[last];   // the workgroup's bytes (rec_pos[n] = b)
    const uint32_t a0 = g0 & ~15u;
    const bool staged = g1 - a0 <= kStage;                    // (the same in every thread of the workgroup)
    if (staged) {
        const uint32_t lines = (g1 - a0 + 15) / 16;          // (the file's buffer is padded to whole tiles)
        for (uint32_t l = threadIdx.x; l < lines; l += kRecs)
            *reinterpret_cast<uint4 *>(stage + l * 16) = *reinterpret_cast<const uint4 *>(bytes + a0 + l * 16);
        __syncthreads();
    }
    const uint32_t r = first + threadIdx.x;
    if (r >= last) return;
    const Src src{bytes, stage, staged ? a0 : 0u, staged ? g1 : 0u, b};
    RecordErr e{0, 0};
    uint32_t hard_names = 0, hard_ident = 0;
    if (!walk_record(src, rec_pos[r], r, table, out, e, hard_names, hard_ident)) refuse(ctrl, e.pos, e.rule);
    if (hard_names) atomicAdd(&ctrl->n_hard_names, hard_names);
    if (hard_ident) atomicAdd(&ctrl->n_hard_ident, hard_ident);
}

const char *rule_text(uint32_t rule) {
    switch (rule) {
    case kRuleStray: return "a byte between the families and records that is no whitespace, bracket, brace or comma in its place";
    case kRuleStruct: return "a missing, doubled or trailing comma, or unbalanced brackets, between records or families";
    case kRuleKey: return "a record key that is no string, holds a backslash or is none of the 13 field names";
    case kRuleDup: return "a record key that appears twice";
    case kRuleMissing: return "a record without one of its 11 required keys";
    case kRuleColon: return "no colon behind a record key";
    case kRuleUint: return "a position or length that is not the literal 0|[1-9][0-9]* of at most 2^64-1";
    case kRuleBool: return "reversed or complemented that is not the literal true or false";
    case kRuleSeq: return "left_seq or right_seq holds a sequence: results with sequences are read on the host";
    case kRuleSeqNull: return "left_seq or right_seq that is neither null nor a string";
    case kRuleIdent: return "identity that is no JSON number literal";
    case kRuleName: return "chr_left or chr_right that is no string, or holds a raw byte below 0x20";
    case kRuleNest: return "a nested array or object as a value";
    case kRuleComma: return "no comma or closing brace behind a value";
    case kRuleEnd: return "the families end inside a record";
    default: return "an unknown rule";
    }
}

int32_t refusal(uint64_t pos, const char *why) {
    set_error("asgart_result_read: refused at byte %llu: %s", (unsigned long long)pos, why);
    return ASGART_E_REFUSED;
}

struct ReadWork : ToolWork {
    DevBuf &bytes = buf(), &cls = buf(), &ctrl = buf(), &tile_bs = buf(), &bs_incl = buf(), &qmask = buf(), &tile_q = buf(),
           &carry_q = buf(), &tile_d = buf(), &carry_d = buf(), &tile_n = buf(), &tile_at = buf(), &tok_pos = buf(),
           &is_fam = buf(), &is_rec = buf(), &rank_fam = buf(), &rank_rec = buf(), &rec_pos = buf(), &names = buf(),
           &name_off = buf(), &offs = buf(), &sds = buf(), &chr_pos = buf(), &flags = buf(), &identity = buf(), &chr = buf(),
           &name_span = buf(), &ident_span = buf(), &first_use = buf();
};

// The depth-1 tokens (sorted positions) against `{ "key" : value , ... }` with the three keys, each once, every value an
// array or object, nothing in front and nothing but whitespace behind; -> the span of the value of "families".
int32_t find_families(const uint8_t *bytes, const std::vector<uint32_t> &top, uint64_t *a, uint64_t *b) {
    static const char *const kKeys[3] = {"strand", "settings", "families"};
    const char *shape = "the top level is not one object with the keys strand, settings and families, each once";
    auto tok = [&](size_t k) -> uint8_t { return k < top.size() ? bytes[top[k]] : 0; };
    auto at = [&](size_t k) -> uint64_t { return k < top.size() ? top[k] : (top.empty() ? 0 : top.back()); };
    if (tok(0) != '{') return refusal(at(0), shape);
    size_t k = 1;
    unsigned seen = 0;
    for (;;) {
        if (tok(k) != '"' || tok(k + 1) != '"') return refusal(at(k), shape);
        const uint8_t *key = bytes + top[k] + 1;
        const size_t len = top[k + 1] - top[k] - 1;
        int which = -1;
        for (int i = 0; i < 3; ++i)
            if (len == strlen(kKeys[i]) && memcmp(key, kKeys[i], len) == 0) which = i;
        if (which < 0 || (seen >> which & 1u)) return refusal(at(k), shape);
        seen |= 1u << which;
        k += 2;
        if (tok(k) != ':') return refusal(at(k), shape);
        ++k;
        const uint8_t open = tok(k), close = tok(k + 1);
        if (!((open == '{' && close == '}') || (open == '[' && close == ']'))) return refusal(at(k), shape);
        if (which == 2) {
            if (open != '[') return refusal(at(k), "families is not an array");
            *a = top[k];
            *b = (uint64_t)top[k + 1] + 1;
        }
        k += 2;
        if (tok(k) == ',') {
            ++k;
            continue;
        }
        if (tok(k) == '}') {
            ++k;
            break;
        }
        return refusal(at(k), shape);
    }
    if (k != top.size()) return refusal(at(k), "bytes behind the closing brace of the top level");
    if (seen != 7u) return refusal(at(k - 1), shape);
    return 0;
}

}  // namespace
}  // namespace asgart

using namespace asgart;

struct asgart_result_read {
    int32_t device = 0;
    std::unique_ptr<ReadWork> w;      // the file, its class bytes and later the arrays, on the device, until the copy or the free
    uint64_t size = 0, a = 0, b = 0;
    uint32_t n_tiles = 0;
    bool parsed = false;
    uint64_t n_fam = 0, n_sd = 0, n_names = 0, n_hard_names = 0, n_hard_ident = 0;
    double ms[4] = {0, 0, 0, 0};
    ~asgart_result_read() {
        if (w && hipSetDevice(device) == hipSuccess) w.reset();
    }
};

namespace {

int32_t run_scan(asgart_result_read *res, const uint8_t *bytes, uint64_t size) {
    ReadWork &w = *res->w;
    RC_TRY(w.open(5));
    hipStream_t s = w.s;
    const uint32_t n_tiles = (uint32_t)((size + kTile - 1) / kTile);
    const size_t padded = (size_t)n_tiles * kTile;
    res->n_tiles = n_tiles;
    HIP_TRY(hipEventRecord(w.ev[0], s));
    RC_TRY(w.bytes.reserve(padded));
    HIP_TRY(hipMemcpyAsync(w.bytes.p, bytes, size, hipMemcpyHostToDevice, s));
    if (padded > size) HIP_TRY(hipMemsetAsync(w.bytes.as<uint8_t>() + size, ' ', padded - size, s));
    HIP_TRY(hipEventRecord(w.ev[1], s));
    RC_TRY(w.cls.reserve(padded));
    RC_TRY(w.ctrl.reserve(sizeof(Ctrl)));
    RC_TRY(w.qmask.reserve((size_t)n_tiles * kLanes * 2));
    for (DevBuf *b : {&w.tile_bs, &w.bs_incl, &w.tile_q, &w.carry_q, &w.tile_d, &w.carry_d}) RC_TRY(b->reserve((size_t)n_tiles * 4));
    Ctrl init{};
    init.err = ~0ull;
    HIP_TRY(hipMemcpyAsync(w.ctrl.p, &init, sizeof(Ctrl), hipMemcpyHostToDevice, s));
    const uint4 *d_bytes = w.bytes.as<uint4>();
    rr_backslash_kernel<<<n_tiles, kLanes, 0, s>>>(d_bytes, w.tile_bs.as<uint32_t>());
    HIP_TRY(hipGetLastError());
    {
        size_t tmp = 0;
        HIP_TRY(rocprim::inclusive_scan(nullptr, tmp, w.tile_bs.as<uint32_t>(), w.bs_incl.as<uint32_t>(), n_tiles, BsOp(), s));
        RC_TRY(w.scan_tmp.reserve(tmp + 16));
        HIP_TRY(rocprim::inclusive_scan(w.scan_tmp.p, tmp, w.tile_bs.as<uint32_t>(), w.bs_incl.as<uint32_t>(), n_tiles, BsOp(), s));
    }
    rr_quotes_kernel<<<n_tiles, kLanes, 0, s>>>(d_bytes, w.bs_incl.as<uint32_t>(), w.qmask.as<uint16_t>(), w.tile_q.as<uint32_t>());
    HIP_TRY(hipGetLastError());
    RC_TRY(w.exclusive_scan(w.tile_q.as<uint32_t>(), w.carry_q.as<uint32_t>(), n_tiles));
    rr_depth_kernel<<<n_tiles, kLanes, 0, s>>>(d_bytes, w.qmask.as<uint16_t>(), w.carry_q.as<uint32_t>(), w.tile_d.as<int32_t>());
    HIP_TRY(hipGetLastError());
    RC_TRY(w.exclusive_scan(w.tile_d.as<int32_t>(), w.carry_d.as<int32_t>(), n_tiles));
    rr_classify_kernel<<<n_tiles, kLanes, 0, s>>>(d_bytes, w.qmask.as<uint16_t>(), w.carry_q.as<uint32_t>(), w.carry_d.as<int32_t>(),
                                                 (uint32_t)size, n_tiles, w.cls.as<uint4>(), w.ctrl.as<Ctrl>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(w.ev[2], s));
    Ctrl c;
    HIP_TRY(read_back(&c, w.ctrl.p, sizeof(Ctrl), s));
    float up = 0, scan = 0;
    HIP_TRY(hipEventElapsedTime(&up, w.ev[0], w.ev[1]));
    HIP_TRY(hipEventElapsedTime(&scan, w.ev[1], w.ev[2]));
    res->ms[0] = up;
    res->ms[1] = scan;
    if (c.n_top > kTopMax) return refusal(0, "more than 64 tokens at the top level");
    if (c.end_in_string) return refusal(size, "the file ends inside a string");
    std::vector<uint32_t> top(c.top, c.top + c.n_top);
    std::sort(top.begin(), top.end());
    RC_TRY(find_families(bytes, top, &res->a, &res->b));
    if (c.end_depth != 0) return refusal(size, "unbalanced brackets");
    return 0;
}

int32_t run_parse(asgart_result_read *res, const uint8_t *name_bytes, const uint64_t *name_offsets, uint32_t n_names) {
    ReadWork &w = *res->w;
    hipStream_t s = w.s;
    const uint32_t a = (uint32_t)res->a, b = (uint32_t)res->b;
    const uint32_t t0 = a / kTile, t1 = (b - 1) / kTile, nt = t1 - t0 + 1;
    Ctrl *ctrl = w.ctrl.as<Ctrl>();
    const uint4 *d_bytes = w.bytes.as<uint4>(), *d_cls = w.cls.as<uint4>();
    HIP_TRY(hipEventRecord(w.ev[3], s));
    RC_TRY(w.upload(w.names, name_bytes, (size_t)name_offsets[n_names]));
    RC_TRY(w.upload(w.name_off, name_offsets, ((size_t)n_names + 1) * 8));
    RC_TRY(w.first_use.reserve(std::max<size_t>((size_t)n_names * 4, 16)));
    HIP_TRY(hipMemsetAsync(w.first_use.p, 0xFF, std::max<size_t>((size_t)n_names * 4, 16), s));
    RC_TRY(w.tile_n.reserve(((size_t)nt + 1) * 4));
    RC_TRY(w.tile_at.reserve(((size_t)nt + 1) * 4));
    HIP_TRY(hipMemsetAsync(w.tile_n.p, 0, ((size_t)nt + 1) * 4, s));
    rr_struct_kernel<false><<<nt, kLanes, 0, s>>>(d_bytes, d_cls, a, b, t0, w.tile_n.as<uint32_t>(), nullptr, ctrl);
    HIP_TRY(hipGetLastError());
    RC_TRY(w.exclusive_scan(w.tile_n.as<uint32_t>(), w.tile_at.as<uint32_t>(), (size_t)nt + 1));
    uint32_t n_tok = 0;
    HIP_TRY(read_back(&n_tok, w.tile_at.as<uint32_t>() + nt, 4, s));
    Ctrl c;
    HIP_TRY(read_back(&c, w.ctrl.p, sizeof(Ctrl), s));
    if (c.err != ~0ull) return refusal(c.err >> 8, rule_text((uint32_t)(c.err & 0xFF)));
    RC_TRY(w.tok_pos.reserve(((size_t)n_tok + 1) * 4));
    for (DevBuf *d : {&w.is_fam, &w.is_rec, &w.rank_fam, &w.rank_rec}) RC_TRY(d->reserve(((size_t)n_tok + 1) * 4));
    rr_struct_kernel<true><<<nt, kLanes, 0, s>>>(d_bytes, d_cls, a, b, t0, w.tile_at.as<uint32_t>(), w.tok_pos.as<uint32_t>(), ctrl);
    HIP_TRY(hipGetLastError());
    rr_pairs_kernel<<<blocks_for((uint64_t)n_tok + 1), 256, 0, s>>>(w.bytes.as<uint8_t>(), w.cls.as<uint8_t>(), w.tok_pos.as<uint32_t>(),
                                                                     n_tok, w.is_fam.as<uint32_t>(), w.is_rec.as<uint32_t>(), ctrl);
    HIP_TRY(hipGetLastError());
    RC_TRY(w.exclusive_scan(w.is_fam.as<uint32_t>(), w.rank_fam.as<uint32_t>(), (size_t)n_tok + 1));
    RC_TRY(w.exclusive_scan(w.is_rec.as<uint32_t>(), w.rank_rec.as<uint32_t>(), (size_t)n_tok + 1));
    uint32_t nf = 0, n = 0;
    HIP_TRY(read_back(&nf, w.rank_fam.as<uint32_t>() + n_tok, 4, s));
    HIP_TRY(read_back(&n, w.rank_rec.as<uint32_t>() + n_tok, 4, s));
    HIP_TRY(read_back(&c, w.ctrl.p, sizeof(Ctrl), s));
    if (c.err != ~0ull) return refusal(c.err >> 8, rule_text((uint32_t)(c.err & 0xFF)));
    RC_TRY(w.offs.reserve(((size_t)nf + 1) * 8));
    RC_TRY(w.rec_pos.reserve(((size_t)n + 1) * 4));
    RC_TRY(w.sds.reserve(std::max<size_t>((size_t)n * 32, 16)));
    RC_TRY(w.chr_pos.reserve(std::max<size_t>((size_t)n * 16, 16)));
    RC_TRY(w.flags.reserve(std::max<size_t>(n, 16)));
    RC_TRY(w.identity.reserve(std::max<size_t>((size_t)n * 4, 16)));
    RC_TRY(w.chr.reserve(std::max<size_t>((size_t)n * 8, 16)));
    RC_TRY(w.name_span.reserve(std::max<size_t>((size_t)n * 16, 16)));
    RC_TRY(w.ident_span.reserve(std::max<size_t>((size_t)n * 8, 16)));
    rr_place_kernel<<<blocks_for((uint64_t)n_tok + 1), 256, 0, s>>>(w.tok_pos.as<uint32_t>(), n_tok, w.is_fam.as<uint32_t>(),
                                                                     w.is_rec.as<uint32_t>(), w.rank_fam.as<uint32_t>(),
                                                                     w.rank_rec.as<uint32_t>(), b, w.offs.as<uint64_t>(),
                                                                     w.rec_pos.as<uint32_t>());
    HIP_TRY(hipGetLastError());
    if (n) {
        NameTable table{w.names.as<uint8_t>(), w.name_off.as<uint64_t>(), n_names, w.first_use.as<uint32_t>()};
        RecordOut out{w.sds.as<uint64_t>(), w.chr_pos.as<uint64_t>(), w.flags.as<uint8_t>(), w.identity.as<float>(),
                      w.chr.as<int32_t>(), w.name_span.as<uint32_t>(), w.ident_span.as<uint32_t>()};
        rr_records_kernel<<<(n + kRecs - 1) / kRecs, kRecs, 0, s>>>(w.bytes.as<uint8_t>(), w.rec_pos.as<uint32_t>(), n, b, table, out,
                                                                    ctrl);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipEventRecord(w.ev[4], s));
    HIP_TRY(read_back(&c, w.ctrl.p, sizeof(Ctrl), s));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, w.ev[3], w.ev[4]));
    res->ms[2] = ms;
    if (c.err != ~0ull) return refusal(c.err >> 8, rule_text((uint32_t)(c.err & 0xFF)));
    res->n_fam = nf;
    res->n_sd = n;
    res->n_names = n_names;
    res->n_hard_names = c.n_hard_names;
    res->n_hard_ident = c.n_hard_ident;
    res->parsed = true;
    return 0;
}

}  // namespace

extern "C" int32_t asgart_result_scan(int32_t device, const uint8_t *bytes, uint64_t size, asgart_result_read **out,
                                      uint64_t *families_begin, uint64_t *families_end) {
    if (out) *out = nullptr;
    if (!out || !families_begin || !families_end || (size && !bytes)) {
        set_error("asgart_result_scan: bad argument");
        return ASGART_E_ARG;
    }
    if (size == 0) return refusal(0, "an empty file");
    // (32-bit byte offsets in the kernels, and two tiles of room so that no offset a walk steps to wraps)
    if (size >= ((uint64_t)1 << 32) - 2 * kTile) return refusal(0, "a file of 2^32 - 2048 bytes and more");
    RC_TRY(use_device("asgart_result_scan", device));
    std::unique_ptr<asgart_result_read> res(new asgart_result_read);
    res->device = device;
    res->size = size;
    res->w.reset(new ReadWork);
    RC_TRY(run_scan(res.get(), bytes, size));   // (a refusal: the handle goes, and with it the device memory)
    *families_begin = res->a;
    *families_end = res->b;
    *out = res.release();
    return 0;
}

extern "C" int32_t asgart_result_parse(asgart_result_read *r, const uint8_t *name_bytes, const uint64_t *name_offsets,
                                       int64_t n_names) {
    if (!r || !r->w || r->parsed || n_names < 0 || n_names >= ((int64_t)1 << 31) || !name_offsets ||
        (name_offsets[n_names] && !name_bytes)) {
        set_error("asgart_result_parse: bad argument (one parse per scan)");
        return ASGART_E_ARG;
    }
    if (name_offsets[0] != 0 || name_offsets[n_names] >= ((uint64_t)1 << 32)) {
        set_error("asgart_result_parse: name_offsets must start at 0 and end below 2^32 bytes of names");
        return ASGART_E_ARG;
    }
    for (int64_t k = 0; k < n_names; ++k)
        if (name_offsets[k] > name_offsets[k + 1]) {
            set_error("asgart_result_parse: name_offsets decrease at name %lld", (long long)k);
            return ASGART_E_ARG;
        }
    for (int64_t k = 1; k < n_names; ++k) {   // sorted and unique, as bytes: the device bisects it
        const uint64_t la = name_offsets[k] - name_offsets[k - 1], lb = name_offsets[k + 1] - name_offsets[k];
        const int c = memcmp(name_bytes + name_offsets[k - 1], name_bytes + name_offsets[k], (size_t)std::min(la, lb));
        if (c > 0 || (c == 0 && la >= lb)) {
            set_error("asgart_result_parse: the name table is not sorted and unique at name %lld", (long long)k);
            return ASGART_E_ARG;
        }
    }
    HIP_TRY(hipSetDevice(r->device));
    return run_parse(r, name_bytes, name_offsets, (uint32_t)n_names);
}

extern "C" void asgart_result_counts(const asgart_result_read *r, uint64_t *n_families, uint64_t *n_sd, uint64_t *n_hard_names,
                                     uint64_t *n_hard_identities) {
    if (n_families) *n_families = r ? r->n_fam : 0;
    if (n_sd) *n_sd = r ? r->n_sd : 0;
    if (n_hard_names) *n_hard_names = r ? r->n_hard_names : 0;
    if (n_hard_identities) *n_hard_identities = r ? r->n_hard_ident : 0;
}

extern "C" int32_t asgart_result_copy(asgart_result_read *r, uint64_t *fam_offsets, asgart_proto_sd *sds, uint8_t *flags,
                                      float *identity, int32_t *chr, uint64_t *chr_pos, uint32_t *first_use,
                                      uint32_t *name_spans, uint32_t *identity_spans) {
    if (!r || !r->w || !r->parsed || !fam_offsets || (r->n_names && !first_use) ||
        (r->n_sd && (!sds || !flags || !identity || !chr || !chr_pos || !name_spans || !identity_spans))) {
        set_error("asgart_result_copy: bad argument (after a parse that succeeded)");
        return ASGART_E_ARG;
    }
    const auto t0 = std::chrono::steady_clock::now();
    HIP_TRY(hipSetDevice(r->device));
    ReadWork &w = *r->w;
    const size_t n = (size_t)r->n_sd;
    HIP_TRY(hipMemcpy(fam_offsets, w.offs.p, ((size_t)r->n_fam + 1) * 8, hipMemcpyDeviceToHost));
    if (r->n_names) HIP_TRY(hipMemcpy(first_use, w.first_use.p, (size_t)r->n_names * 4, hipMemcpyDeviceToHost));
    if (n) {
        HIP_TRY(hipMemcpy(sds, w.sds.p, n * 32, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(flags, w.flags.p, n, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(identity, w.identity.p, n * 4, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(chr, w.chr.p, n * 8, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(chr_pos, w.chr_pos.p, n * 16, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(name_spans, w.name_span.p, n * 16, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(identity_spans, w.ident_span.p, n * 8, hipMemcpyDeviceToHost));
    }
    r->ms[3] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return 0;
}

extern "C" int32_t asgart_result_timings(const asgart_result_read *r, double *ms4) {
    if (!r || !ms4) {
        set_error("asgart_result_timings: bad argument");
        return ASGART_E_ARG;
    }
    for (int k = 0; k < 4; ++k) ms4[k] = r->ms[k];
    return 0;
}

extern "C" void asgart_result_free(asgart_result_read *r) { delete r; }

extern "C" void asgart_result_geometry(uint64_t *tile_bytes, uint64_t *records_per_block, uint64_t *stage_bytes) {
    if (tile_bytes) *tile_bytes = kTile;
    if (records_per_block) *records_per_block = kRecs;
    if (stage_bytes) *stage_bytes = kStage;
}
