// extract.hip -- the sequences of the duplicons on the GPU: asgart_source_* and asgart_extract_sequences.
//
// Replaces the body of reference src/bin/asgart-extract.rs:110-200: the raw bytes of every record of every file are
// concatenated as the FASTA reader returns them (:17-29, :110-117; NOT the normalised strand of the search: soft-masked
// lower case and IUPAC letters stay as they are), the left arm of a duplicon is source[left .. left + left_length], the
// right arm source[right .. right + right_length], reversed when the duplicon is, then complemented when it is
// (:120-134) with utils::complement_nucleotide (src/utils.rs:1-23: A<->T, G<->C in either case, N and n stay, any other
// byte becomes N).  On the host this is a loop over the duplicons; here it is one bandwidth-bound gather: the arms' output
// offsets come from a scan on the device, every lane writes one aligned 16-byte vector of the output (long arms are
// spread over as many workgroups as their length asks for), and the copy of one piece to the host runs beside the
// gather of the next.
#include "tool_base.hpp"
#include "prep.hpp"

#include <algorithm>

#include <rocprim/rocprim.hpp>

namespace asgart {
namespace {

constexpr uint64_t kStage = 32ull << 20;    // bytes per staging buffer (device and pinned host, two of each)
constexpr int64_t kMaxPieceSds = 1 << 20;   // duplicons per call at most (bounds the device metadata of one call)
constexpr uint32_t kBlock = 256;            // lanes per workgroup; each writes 16 output bytes
constexpr uint32_t kPad = 64;               // zero bytes behind the source: the aligned 32-byte windows stay inside

// 0xFF in every byte of v that equals the byte replicated in c4, 0x00 elsewhere (exact: no false positives)
__device__ inline uint32_t eq_bytes(uint32_t v, uint32_t c4) {
    const uint32_t x = v ^ c4;
    const uint32_t nonzero = ((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x;  // bit 7 of a byte set iff that byte of x != 0
    return ((~nonzero & 0x80808080u) >> 7) * 0xFFu;
}

// utils::complement_nucleotide (reference src/utils.rs:1-19) on four bytes at once, without a branch per byte:
// A^T = 0x15 and C^G = 0x04 in both cases, `| 0x20` folds the case (only 'X' and 'x' become 'x').
__device__ inline uint32_t complement_word(uint32_t w) {
    const uint32_t f = w | 0x20202020u;
    const uint32_t at = eq_bytes(f, 0x61616161u) | eq_bytes(f, 0x74747474u);  // a, t
    const uint32_t cg = eq_bytes(f, 0x63636363u) | eq_bytes(f, 0x67676767u);  // c, g
    const uint32_t nn = eq_bytes(f, 0x6E6E6E6Eu);                             // n
    return (at & (w ^ 0x15151515u)) | (cg & (w ^ 0x04040404u)) | (nn & w) | (~(at | cg | nn) & 0x4E4E4E4Eu);
}

// first arm a in [lo, hi] whose end lies behind x (ends: inclusive scan of the arm lengths; ends[hi] > x)
__device__ inline uint32_t arm_of(const uint64_t *__restrict__ ends, uint32_t lo, uint32_t hi, uint64_t x) {
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (ends[mid] > x) hi = mid; else lo = mid + 1;
    }
    return lo;
}

struct Arm {
    uint64_t src, len, out;  // source start, length, first output byte (piece coordinates)
    uint32_t flags;          // bit 0 reversed, bit 1 complemented (right arms only)
};

__device__ inline Arm arm_info(const asgart_proto_sd *__restrict__ sds, const uint8_t *__restrict__ flags,
                               const uint64_t *__restrict__ ends, uint32_t a) {
    const asgart_proto_sd &d = sds[a >> 1];
    Arm r;
    const bool right = (a & 1u) != 0;
    r.src = right ? d.right : d.left;
    r.len = right ? d.right_length : d.left_length;
    r.out = ends[a] - r.len;
    r.flags = right ? flags[a >> 1] : 0u;
    return r;
}

__global__ __launch_bounds__(kBlock) void arm_lengths_kernel(const asgart_proto_sd *__restrict__ sds, uint32_t n_sd,
                                                             uint64_t *__restrict__ lens) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_sd) {
        lens[2 * i] = sds[i].left_length;
        lens[2 * i + 1] = sds[i].right_length;
    }
}

// Output bytes [b0, b1) of the piece into stage[0 .. b1 - b0).  Lane t of workgroup g owns the 16 bytes at
// b0 + 16 (g * kBlock + t); stage holds a whole number of such vectors (kStage), so the last one may run past b1.
// Where the 16 bytes lie inside one arm (every vector of an arm but its misaligned head and tail), the source window is
// read as two aligned 16-byte vectors and shifted into place (v_alignbyte); a reversed arm reads the mirrored window and
// reverses it (dword order, then the bytes of each dword).  The vectors that straddle an arm boundary, or the end of the
// piece, are assembled byte by byte.  Any output byte >= 0x80 sets *bad (the reference's String::from_utf8 panics).
__global__ __launch_bounds__(kBlock) void extract_gather_kernel(const uint8_t *__restrict__ text,
                                                                const asgart_proto_sd *__restrict__ sds,
                                                                const uint8_t *__restrict__ flags,
                                                                const uint64_t *__restrict__ ends, uint32_t n_arms,
                                                                uint64_t b0, uint64_t b1, uint8_t *__restrict__ stage,
                                                                uint32_t *__restrict__ bad) {
    __shared__ uint32_t range[2];
    const uint64_t blk0 = b0 + (uint64_t)blockIdx.x * kBlock * 16u;
    if (threadIdx.x < 2) {
        const uint64_t at = threadIdx.x == 0 ? blk0 : std::min<uint64_t>(blk0 + kBlock * 16u, b1) - 1;
        range[threadIdx.x] = arm_of(ends, 0, n_arms - 1, at);
    }
    __syncthreads();
    const uint64_t x = blk0 + (uint64_t)threadIdx.x * 16u;
    if (x >= b1) return;
    uint32_t a = arm_of(ends, range[0], range[1], x);
    Arm arm = arm_info(sds, flags, ends, a);
    uint32_t w[4];
    if (x + 16u <= arm.out + arm.len) {
        const uint64_t i = x - arm.out;
        const bool rev = (arm.flags & 1u) != 0;
        const uint64_t p = arm.src + (rev ? arm.len - i - 16u : i);
        const uint4 *q = reinterpret_cast<const uint4 *>(text + (p & ~(uint64_t)15));
        const uint4 lo = q[0], hi = q[1];
        const uint32_t v[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
        const uint32_t o = (uint32_t)(p & 15u), d = o >> 2, r = o & 3u;
        uint32_t s[5];
#pragma unroll
        for (int k = 0; k < 5; ++k) s[k] = d == 0 ? v[k] : d == 1 ? v[k + 1] : d == 2 ? v[k + 2] : v[k + 3];
#pragma unroll
        for (int k = 0; k < 4; ++k) w[k] = __builtin_amdgcn_alignbyte(s[k + 1], s[k], r);
        if (rev) {
            const uint32_t t0 = w[0], t1 = w[1];
            w[0] = __builtin_bswap32(w[3]);
            w[1] = __builtin_bswap32(w[2]);
            w[2] = __builtin_bswap32(t1);
            w[3] = __builtin_bswap32(t0);
        }
        if (arm.flags & 2u) {
#pragma unroll
            for (int k = 0; k < 4; ++k) w[k] = complement_word(w[k]);
        }
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) w[k] = 0;
#pragma unroll
        for (int b = 0; b < 16; ++b) {
            const uint64_t xb = x + (uint64_t)b;
            if (xb >= b1) break;
            while (xb >= arm.out + arm.len) arm = arm_info(sds, flags, ends, ++a);  // (empty arms are stepped over)
            const uint64_t i = xb - arm.out;
            uint32_t c = text[arm.src + ((arm.flags & 1u) ? arm.len - 1u - i : i)];
            if (arm.flags & 2u) c = complement_word(c) & 0xFFu;
            w[b >> 2] |= c << (8 * (b & 3));
        }
    }
    if ((w[0] | w[1] | w[2] | w[3]) & 0x80808080u) atomicOr(bad, 1u);
    *reinterpret_cast<uint4 *>(stage + (x - b0)) = make_uint4(w[0], w[1], w[2], w[3]);
}

}  // namespace
}  // namespace asgart

using namespace asgart;

struct asgart_source {
    int32_t device = 0;
    uint64_t n = 0;
    DevBuf text;
    std::mutex mu;  // one extraction at a time per source: the staging buffers and streams below are shared
    hipStream_t s_gather = nullptr, s_copy = nullptr;
    hipEvent_t ev_gather[2] = {nullptr, nullptr}, ev_copy[2] = {nullptr, nullptr};
    DevBuf d_stage[2], d_sds, d_flags, d_lens, d_ends, d_scan_tmp, d_bad;
    uint8_t *h_stage[2] = {nullptr, nullptr};

    void release() {
        (void)hipSetDevice(device);
        if (s_gather) (void)hipStreamSynchronize(s_gather);
        if (s_copy) (void)hipStreamSynchronize(s_copy);
        for (int k = 0; k < 2; ++k) {
            d_stage[k].release();
            if (h_stage[k]) (void)hipHostFree(h_stage[k]);
            if (ev_gather[k]) (void)hipEventDestroy(ev_gather[k]);
            if (ev_copy[k]) (void)hipEventDestroy(ev_copy[k]);
            h_stage[k] = nullptr;
            ev_gather[k] = ev_copy[k] = nullptr;
        }
        for (DevBuf *b : {&text, &d_sds, &d_flags, &d_lens, &d_ends, &d_scan_tmp, &d_bad}) b->release();
        if (s_gather) (void)hipStreamDestroy(s_gather);
        if (s_copy) (void)hipStreamDestroy(s_copy);
        s_gather = s_copy = nullptr;
    }
};

namespace asgart {

// A source of n bytes on the current device with its streams, events and staging buffers, its text still empty.
static int32_t source_new(uint64_t n, int32_t device, asgart_source **out) {
    asgart_source *src = new asgart_source;
    src->device = device;
    src->n = n;
    const int32_t rc = [&]() -> int32_t {
        HIP_TRY(hipStreamCreateWithFlags(&src->s_gather, hipStreamNonBlocking));
        HIP_TRY(hipStreamCreateWithFlags(&src->s_copy, hipStreamNonBlocking));
        for (int k = 0; k < 2; ++k) {
            HIP_TRY(hipEventCreateWithFlags(&src->ev_gather[k], hipEventDisableTiming));
            HIP_TRY(hipEventCreateWithFlags(&src->ev_copy[k], hipEventDisableTiming));
            HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&src->h_stage[k]), (size_t)kStage, hipHostMallocDefault));
        }
        RC_TRY(src->d_bad.reserve(64));
        return 0;
    }();
    if (rc != 0) {
        src->release();
        delete src;
        return rc;
    }
    *out = src;
    return 0;
}

// A source over bytes that are on the device already (fasta.hip: the raw strand the FASTA reader wrote): `text` holds
// n bytes and room for the pad behind them; the source takes the buffer over (text is left empty) -- on success only.
int32_t source_adopt(DevBuf &text, uint64_t n, int32_t device, asgart_source **out) {
    if (text.cap < (size_t)n + kPad) {
        set_error("source_adopt: the buffer lacks the %u bytes of pad", kPad);
        return ASGART_E_ARG;
    }
    HIP_TRY(hipSetDevice(device));
    asgart_source *src = nullptr;
    RC_TRY(source_new(n, device, &src));
    const int32_t rc = [&]() -> int32_t {
        HIP_TRY(hipMemsetAsync(static_cast<uint8_t *>(text.p) + n, 0, kPad, src->s_copy));
        HIP_TRY(stream_sync(src->s_copy));
        return 0;
    }();
    if (rc != 0) {
        src->release();
        delete src;
        return rc;
    }
    src->text = text;
    text = DevBuf();
    *out = src;
    return 0;
}

// What a reader of the raw strand needs of a source (fasta_write.hip): its device, its bytes and where they are.
void source_view(const asgart_source *src, int32_t *device, uint64_t *n, const uint8_t **text) {
    *device = src->device;
    *n = src->n;
    *text = src->text.as<uint8_t>();
}

}  // namespace asgart

namespace {

// The raw records into src->text through the two pinned staging buffers: the copy of one staging buffer runs while
// the host fills the other.
int32_t upload_records(asgart_source *src, const uint8_t *const *records, const uint64_t *record_lens, int64_t n_records) {
    uint8_t *dst = src->text.as<uint8_t>();
    uint64_t at = 0, fill = 0;
    int slot = 0;
    bool pending[2] = {false, false};
    auto flush = [&]() -> int32_t {
        if (!fill) return 0;
        HIP_TRY(hipMemcpyAsync(dst + at - fill, src->h_stage[slot], (size_t)fill, hipMemcpyHostToDevice, src->s_copy));
        HIP_TRY(hipEventRecord(src->ev_copy[slot], src->s_copy));
        pending[slot] = true;
        slot ^= 1;
        fill = 0;
        if (pending[slot]) HIP_TRY(hipEventSynchronize(src->ev_copy[slot]));
        pending[slot] = false;
        return 0;
    };
    for (int64_t r = 0; r < n_records; ++r) {
        for (uint64_t done = 0; done < record_lens[r];) {
            const uint64_t take = std::min(record_lens[r] - done, kStage - fill);
            memcpy(src->h_stage[slot] + fill, records[r] + done, (size_t)take);
            fill += take;
            done += take;
            at += take;
            if (fill == kStage) RC_TRY(flush());
        }
    }
    RC_TRY(flush());
    HIP_TRY(hipMemsetAsync(dst + src->n, 0, kPad, src->s_copy));
    HIP_TRY(stream_sync(src->s_copy));
    return 0;
}

}  // namespace

extern "C" int32_t asgart_source_create(const uint8_t *const *records, const uint64_t *record_lens, int64_t n_records,
                                        int32_t device, asgart_source **out) {
    if (out) *out = nullptr;
    if (!out || n_records < 0 || (n_records && (!records || !record_lens))) {
        set_error("asgart_source_create: bad argument");
        return ASGART_E_ARG;
    }
    uint64_t n = 0;
    for (int64_t r = 0; r < n_records; ++r) {
        if (record_lens[r] && !records[r]) {
            set_error("asgart_source_create: record %lld is NULL", (long long)r);
            return ASGART_E_ARG;
        }
        n += record_lens[r];
    }
    RC_TRY(use_device("asgart_source_create", device));
    asgart_source *src = nullptr;
    RC_TRY(source_new(n, device, &src));
    int32_t rc = src->text.reserve((size_t)n + kPad);
    if (rc == 0) rc = upload_records(src, records, record_lens, n_records);
    if (rc != 0) {
        src->release();
        delete src;
        return rc;
    }
    *out = src;
    return 0;
}

extern "C" void asgart_source_destroy(asgart_source *src) {
    if (!src) return;
    src->release();
    delete src;
}

extern "C" int32_t asgart_extract_sequences(asgart_source *src, const asgart_proto_sd *sds, const uint8_t *flags,
                                            int64_t n_sd, int64_t first, uint8_t *out, uint64_t out_cap,
                                            uint64_t *seq_ends, int64_t *n_done) {
    if (n_done) *n_done = 0;
    if (!src || !n_done || n_sd < 0 || first < 0 || first > n_sd ||
        (first < n_sd && (!sds || !seq_ends || (out_cap && !out)))) {
        set_error("asgart_extract_sequences: bad argument");
        return ASGART_E_ARG;
    }
    if (first == n_sd) return 0;
    // what fits: whole duplicons, both arms inside the source (the reference's slice panics, :119-124)
    uint64_t total = 0;
    int64_t m = 0;
    for (int64_t j = first; j < n_sd && m < kMaxPieceSds; ++j, ++m) {
        const asgart_proto_sd &d = sds[j];
        if (d.left_length > src->n || d.left > src->n - d.left_length || d.right_length > src->n ||
            d.right > src->n - d.right_length) {
            set_error("asgart_extract_sequences: duplicon %lld (left %llu+%llu, right %llu+%llu) runs past the source "
                      "(%llu bytes)", (long long)j, (unsigned long long)d.left, (unsigned long long)d.left_length,
                      (unsigned long long)d.right, (unsigned long long)d.right_length, (unsigned long long)src->n);
            return ASGART_E_ARG;
        }
        const uint64_t need = d.left_length + d.right_length;
        if (need > out_cap - total) {
            if (m == 0) {
                seq_ends[0] = d.left_length;
                seq_ends[1] = need;
                set_error("asgart_extract_sequences: duplicon %lld needs %llu bytes, room for %llu (seq_ends[1])",
                          (long long)j, (unsigned long long)need, (unsigned long long)out_cap);
                return ASGART_E_CAP;
            }
            break;
        }
        total += need;
    }
    std::lock_guard<std::mutex> lk(src->mu);
    HIP_TRY(hipSetDevice(src->device));
    hipStream_t sg = src->s_gather, sc = src->s_copy;
    const uint32_t n_arms = (uint32_t)(2 * m);
    RC_TRY(src->d_sds.reserve((size_t)m * sizeof(asgart_proto_sd)));
    RC_TRY(src->d_flags.reserve((size_t)m));
    RC_TRY(src->d_lens.reserve((size_t)n_arms * 8));
    RC_TRY(src->d_ends.reserve((size_t)n_arms * 8));
    for (int k = 0; k < 2; ++k)
        if (total) RC_TRY(src->d_stage[k].reserve((size_t)kStage));
    HIP_TRY(hipMemcpyAsync(src->d_sds.p, sds + first, (size_t)m * sizeof(asgart_proto_sd), hipMemcpyHostToDevice, sg));
    if (flags)
        HIP_TRY(hipMemcpyAsync(src->d_flags.p, flags + first, (size_t)m, hipMemcpyHostToDevice, sg));
    else
        HIP_TRY(hipMemsetAsync(src->d_flags.p, 0, (size_t)m, sg));
    HIP_TRY(hipMemsetAsync(src->d_bad.p, 0, 4, sg));
    const asgart_proto_sd *d_sds = src->d_sds.as<asgart_proto_sd>();
    uint64_t *lens = src->d_lens.as<uint64_t>(), *ends = src->d_ends.as<uint64_t>();
    arm_lengths_kernel<<<(unsigned)((m + kBlock - 1) / kBlock), kBlock, 0, sg>>>(d_sds, (uint32_t)m, lens);
    HIP_TRY(hipGetLastError());
    size_t tmp_bytes = 0;
    HIP_TRY(rocprim::inclusive_scan(nullptr, tmp_bytes, lens, ends, (size_t)n_arms, rocprim::plus<uint64_t>(), sg));
    RC_TRY(src->d_scan_tmp.reserve(tmp_bytes + 16));
    HIP_TRY(rocprim::inclusive_scan(src->d_scan_tmp.p, tmp_bytes, lens, ends, (size_t)n_arms,
                                    rocprim::plus<uint64_t>(), sg));
    // pieces of kStage output bytes: gather k on s_gather beside the copy of k - 1 on s_copy; the host takes piece
    // k - 2 out of its pinned buffer before that buffer (and its device twin) is used again
    const uint64_t n_sub = (total + kStage - 1) / kStage;
    auto take = [&](uint64_t k) -> int32_t {
        HIP_TRY(hipEventSynchronize(src->ev_copy[k & 1]));
        memcpy(out + k * kStage, src->h_stage[k & 1], (size_t)(std::min(total, (k + 1) * kStage) - k * kStage));
        return 0;
    };
    for (uint64_t k = 0; k < n_sub; ++k) {
        if (k >= 2) RC_TRY(take(k - 2));
        const uint64_t b0 = k * kStage, b1 = std::min(total, b0 + kStage);
        const uint64_t vecs = (b1 - b0 + 15) / 16;
        extract_gather_kernel<<<(unsigned)((vecs + kBlock - 1) / kBlock), kBlock, 0, sg>>>(
            src->text.as<uint8_t>(), d_sds, src->d_flags.as<uint8_t>(), ends, n_arms, b0, b1,
            src->d_stage[k & 1].as<uint8_t>(), src->d_bad.as<uint32_t>());
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(src->ev_gather[k & 1], sg));
        HIP_TRY(hipStreamWaitEvent(sc, src->ev_gather[k & 1], 0));
        HIP_TRY(hipMemcpyAsync(src->h_stage[k & 1], src->d_stage[k & 1].p, (size_t)(b1 - b0), hipMemcpyDeviceToHost, sc));
        HIP_TRY(hipEventRecord(src->ev_copy[k & 1], sc));
    }
    for (uint64_t k = n_sub >= 2 ? n_sub - 2 : 0; k < n_sub; ++k) RC_TRY(take(k));
    uint32_t h_bad = 0;
    HIP_TRY(read_back(&h_bad, src->d_bad.p, 4, sg));
    HIP_TRY(read_back(seq_ends, ends, (size_t)n_arms * 8, sg));
    if (h_bad) {
        set_error("asgart_extract_sequences: a byte >= 0x80 in the sequences of duplicons %lld..%lld (the reference "
                  "refuses them: String::from_utf8)", (long long)first, (long long)(first + m - 1));
        return ASGART_E_ARG;
    }
    *n_done = m;
    return 0;
}
