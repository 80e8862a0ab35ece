// paf.hip -- PAF files written on the GPU: asgart_paf_records, the counterpart of align.paf_text for a caller of the C ABI.
//
// What a row consists of is stated once, in paf_dev.hpp.  A row's CIGAR is as long as its two arms have edits, so nothing
// here works row by row except the head:
//   runs      one thread per run: the bytes of its text (the digits of its length and the operation), its `=` bases, its bases;
//   scans     three 64-bit exclusive scans over the runs (rocPRIM): P, M and B.  A row's CIGAR bytes, its column 10 and its
//             column 11 are differences of them at the row's first run and behind its last;
//   rows      one thread per row (a duplication with status != 0; the host numbers them while it checks the flags): its
//             family by bisection, the length of its head by running the head through a sink that counts, its length;
//   scan      a 64-bit exclusive scan of the row lengths: every row's place in the file, and the file's size;
//   write     a workgroup owns kStage consecutive BYTES of the file -- not rows, not runs -- so that its range starts on a
//             16-byte line whatever the rows hold.  It finds the rows of its first and last byte by bisection of the row
//             starts and the runs of those two rows that reach into its range by bisection of P; the heads in the range are
//             dealt out a row per thread, the runs a run per thread, each storing the bytes that fall inside the range into
//             an LDS image of it.  Then all threads move the image out with one aligned 16-byte store per lane.  A head
//             longer than the image (a 20 000-byte name) is composed by the workgroups it spans, each its own part; there is
//             no second path.
//
// asgart_paf_records_cs adds the cs:Z: column (paf_dev.hpp states the rule): the same stages from the same text -- the rows
// kernel and the write kernel are templates of whether the rows have the column, so the path of asgart_paf_records holds no
// branch on it -- and on top of them
//   runs      a second kernel, one thread per run: the bytes of its cs text, its bases of the left and of the right arm; a
//             run with an operation that is none or of no base reports its row;
//   scans     three more 64-bit exclusive scans: C, I and J;
//   rows      a row's runs must consume exactly its two arms (differences of I and J): a row that does not reports itself.
//             All three checks go through ONE atomic minimum of (row, check), read back with the file's size: the lowest
//             offending row is named and nothing is written;
//   write     the cs text of a run is as long as the edit (a 40 kb insertion is 40 001 bytes, an `X` run 3 n), so a run per
//             thread is not enough: a thread composes at most kSolo bytes of one run alone; a run with more than that inside
//             the window goes on a list in LDS, and behind a barrier the bytes of every listed run are dealt out by position
//             across all 256 threads, neighbouring lanes reading neighbouring bytes of the text (paf_cs_collect, paf_cs_deal).
// kSolo = kStage / kThreads = 64: a thread's even share of its window.  A run at or below it costs its thread no more than
// the share every thread has anyway; a longer one would leave lanes idle behind it.  It also bounds the list: the listed
// texts are disjoint and longer than kSolo, so kStage / (kSolo + 1) = 252 entries of 32 bytes (8 KiB of LDS beside the
// 16 KiB image: six workgroups a CU) hold them.  A design constant, reasoned and not measured: no sweep was run.
#include "index.hpp"
#include "file_writer.hpp"
#include "paf_dev.hpp"

namespace asgart {
namespace {

constexpr uint32_t kThreads = 256;          // per workgroup of the write stage
constexpr uint32_t kStage = 16384;          // bytes of the file per workgroup, and of its LDS image: nine fit a CU's 160 KiB
constexpr uint32_t kRunsMax = kStage / 2;   // a run is two bytes at least: the runs one image can hold
constexpr uint32_t kLine = 16;              // bytes per store of the copy out
constexpr uint32_t kSolo = kStage / kThreads;        // bytes of one run's cs text a thread composes alone (see above)
constexpr uint32_t kLongMax = kStage / (kSolo + 1);  // the runs with more than that inside one window
static_assert(sizeof(CsRun) == 32, "the list of long runs is sized by this");
static_assert(kSolo >= 11, "a short `=` (a sign and ten digits) is never listed");

__global__ __launch_bounds__(256) void paf_runs_kernel(const uint32_t *__restrict__ run_len,
                                                       const uint8_t *__restrict__ run_op, uint64_t n_runs,
                                                       uint64_t *__restrict__ text, uint64_t *__restrict__ match,
                                                       uint64_t *__restrict__ bases) {
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (t > n_runs) return;
    if (t == n_runs) {   // the closing entry: the scans end in the totals
        text[t] = match[t] = bases[t] = 0;
        return;
    }
    const uint32_t len = run_len[t];
    text[t] = decimal_digits(len) + 1;
    match[t] = run_op[t] == '=' ? len : 0;
    bases[t] = len;
}

// The cs writer's view of a run: the bytes of its cs text and its bases on either arm.  A run that is none (an operation
// outside `=XID`, no base) counts nothing and reports the row it belongs to, if that duplication has a row.
__global__ __launch_bounds__(256) void paf_cs_runs_kernel(PafIn in, uint64_t n_runs, uint32_t n_sd, uint64_t *__restrict__ cs,
                                                          uint64_t *__restrict__ on_left, uint64_t *__restrict__ on_right) {
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (t > n_runs) return;
    if (t == n_runs) {
        cs[t] = on_left[t] = on_right[t] = 0;
        return;
    }
    const uint32_t len = in.run_len[t];
    const uint8_t op = in.run_op[t];
    const bool known = run_op_known(op);
    if (known && len != 0) {
        cs[t] = cs_text_bytes(op, len, in.cs_mode);
        on_left[t] = run_on_left(op, len);
        on_right[t] = run_on_right(op, len);
        return;
    }
    cs[t] = on_left[t] = on_right[t] = 0;
    const uint32_t q = (uint32_t)(first_above(in.run_off, 0, (uint64_t)n_sd + 1, t) - 1);
    uint32_t lo = 0, hi = in.n_rows;
    while (lo < hi) {
        const uint32_t m = (lo + hi) >> 1;
        if (in.kept[m] >= q) hi = m; else lo = m + 1;
    }
    if (lo < in.n_rows && in.kept[lo] == q)
        atomicMin((unsigned long long *)in.bad, (unsigned long long)((uint64_t)lo << 2 | (known ? kPafBadLen : kPafBadOp)));
}

template <bool kCs>
__global__ __launch_bounds__(256) void paf_rows_kernel(PafIn in, uint32_t *__restrict__ head_len, uint32_t *__restrict__ fam,
                                                       uint64_t *__restrict__ lens) {
    const uint32_t k = blockIdx.x * 256 + threadIdx.x;
    if (k > in.n_rows) return;
    if (k == in.n_rows) {
        lens[k] = 0;
        return;
    }
    const uint32_t q = in.kept[k];
    const uint32_t f = segment_of(in.offs, in.n_fam, q);
    CountSink c;
    emit_paf_head(c, in, q, f);
    head_len[k] = (uint32_t)c.n;
    fam[k] = f;
    const uint64_t b = in.run_off[q], e = in.run_off[q + 1];
    uint64_t len = c.n + (in.P[e] - in.P[b]) + 1;
    if constexpr (kCs) {
        len += kCsTagBytes + (in.C[e] - in.C[b]);
        if (in.I[e] - in.I[b] != in.sds[4 * (size_t)q + 2] || in.J[e] - in.J[b] != in.sds[4 * (size_t)q + 3])
            atomicMin((unsigned long long *)in.bad, (unsigned long long)((uint64_t)k << 2 | kPafBadSums));
    }
    lens[k] = len;
}

template <bool kCs>
__global__ __launch_bounds__(kThreads) void paf_write_kernel(PafIn in, uint64_t size, uint8_t *__restrict__ out) {
    __shared__ __align__(16) uint8_t stage[kStage];
    const uint64_t g0 = (uint64_t)blockIdx.x * kStage;
    if (g0 >= size) return;
    const uint64_t g1 = min(g0 + kStage, size);
    paf_compose<kCs>(in, g0, g1, threadIdx.x, kThreads, stage);
    if constexpr (kCs) {
        __shared__ CsRun long_runs[kLongMax];
        __shared__ uint32_t n_long;
        if (threadIdx.x == 0) n_long = 0;
        __syncthreads();
        paf_cs_collect<kSolo, kLongMax>(in, g0, g1, threadIdx.x, kThreads, stage, long_runs, &n_long);
        __syncthreads();
        paf_cs_deal<kLongMax>(in, g0, g1, threadIdx.x, kThreads, stage, long_runs, &n_long);
    }
    __syncthreads();
    // file_writer.hpp's copy_out_image where the image starts with the range (a0 == g0), kept as its own loop: through
    // the general one the cs kernel spills two more scalar registers (profiles/writers_resources.txt)
    const uint32_t bytes = (uint32_t)(g1 - g0), lines = (bytes + kLine - 1) / kLine;
    for (uint32_t l = threadIdx.x; l < lines; l += kThreads) {
        if ((l + 1) * kLine <= bytes) {
            *reinterpret_cast<uint4 *>(out + g0 + (uint64_t)l * kLine) = *reinterpret_cast<const uint4 *>(stage + l * kLine);
        } else {   // the last line of the file
            for (uint32_t b = l * kLine; b < bytes; ++b) out[g0 + b] = stage[b];
        }
    }
}

struct PafWork : FileWork {
    DevBuf &distance = buf(), &run_off = buf(), &run_len = buf(), &run_op = buf(), &name_len = buf(), &kept = buf(),
           &text = buf(), &match = buf(), &bases = buf(), &P = buf(), &M = buf(), &B = buf(), &head_len = buf(), &fam = buf(),
           &lens = buf(), &row_start = buf(), &cs = buf(), &on_left = buf(), &on_right = buf(), &C = buf(), &I = buf(),
           &J = buf();
};

// what the cs writer takes from the index; nullptr: the rows have no cs:Z: column
struct CsText {
    const uint8_t *text;
    uint32_t mode;
};

const char kWho[] = "asgart_paf_records", kWhoCs[] = "asgart_paf_records_cs";

// Every argument check of the call, before the device is looked at; kept: the duplications with a row.
int32_t check_arguments(const char *who, const ResultArg &a, const uint8_t *status, const uint32_t *distance,
                        const uint64_t *run_offsets, const uint32_t *run_len, const uint8_t *run_op, const uint64_t *name_length,
                        asgart_export **out, std::vector<uint32_t> &kept) {
    const int64_t n_sd = a.n_sd;
    if (!out || a.missing() || (a.n_names && !name_length) || (n_sd && (!status || !distance || !run_offsets))) {
        set_error("%s: bad argument", who);
        return ASGART_E_ARG;
    }
    if (n_sd >= (int64_t)1 << 31 || a.n_families >= (int64_t)1 << 31) {
        set_error("%s: 2^31 rows (or families) and more are not supported", who);
        return ASGART_E_CAP;
    }
    RC_TRY(check_result_arg(who, a));
    const uint64_t n_runs = n_sd ? run_offsets[n_sd] : 0;
    if (n_runs >= (uint64_t)1 << 32) {
        set_error("%s: run_offsets end at %llu; 2^32 runs and more are not supported", who, (unsigned long long)n_runs);
        return ASGART_E_CAP;
    }
    if (n_sd) RC_TRY(check_csr(who, "run_offsets", run_offsets, n_sd, (int64_t)n_runs, "the run count", "duplication"));
    if (n_runs && (!run_len || !run_op)) {
        set_error("%s: bad argument (%llu runs and no run_len or run_op)", who, (unsigned long long)n_runs);
        return ASGART_E_ARG;
    }
    return check_strand_rows(who, a.sds, a.flags, status, a.chr_pos, n_sd, kept);
}

template <bool kCs>
int32_t run_paf(PafWork &w, asgart_export *res, CsText cs, const ResultArg &a, const uint32_t *distance,
                const uint64_t *run_offsets, const uint32_t *run_len, const uint8_t *run_op, const uint64_t *name_length,
                const std::vector<uint32_t> &kept) {
    const uint32_t n = (uint32_t)a.n_sd, n_rows = (uint32_t)kept.size();
    if (n_rows == 0) return 0;   // an empty file: nothing to launch
    const uint64_t n_runs = run_offsets[n];
    RC_TRY(w.open_call());
    hipStream_t s = w.s;
    RC_TRY(w.upload(a));
    RC_TRY(w.upload(w.distance, distance, (size_t)n * 4));
    RC_TRY(w.upload(w.run_off, run_offsets, ((size_t)n + 1) * 8));
    RC_TRY(w.upload(w.run_len, run_len, (size_t)n_runs * 4));
    RC_TRY(w.upload(w.run_op, run_op, (size_t)n_runs));
    RC_TRY(w.upload(w.name_len, name_length, (size_t)a.n_names * 8));
    RC_TRY(w.upload(w.kept, kept.data(), (size_t)n_rows * 4));
    RC_TRY(w.stamp(w.kUploaded));
    for (DevBuf *b : {&w.text, &w.match, &w.bases, &w.P, &w.M, &w.B}) RC_TRY(b->reserve(((size_t)n_runs + 1) * 8));
    RC_TRY(w.head_len.reserve((size_t)n_rows * 4));
    RC_TRY(w.fam.reserve((size_t)n_rows * 4));
    RC_TRY(w.lens.reserve(((size_t)n_rows + 1) * 8));
    RC_TRY(w.row_start.reserve(((size_t)n_rows + 2) * 8));   // (behind the file's size: the cs writer's lowest refused row)
    paf_runs_kernel<<<blocks_for(n_runs + 1), 256, 0, s>>>(w.run_len.as<uint32_t>(), w.run_op.as<uint8_t>(), n_runs,
                                                          w.text.as<uint64_t>(), w.match.as<uint64_t>(),
                                                          w.bases.as<uint64_t>());
    HIP_TRY(hipGetLastError());
    RC_TRY(w.exclusive_scan(w.text.as<uint64_t>(), w.P.as<uint64_t>(), (size_t)n_runs + 1));
    RC_TRY(w.exclusive_scan(w.match.as<uint64_t>(), w.M.as<uint64_t>(), (size_t)n_runs + 1));
    RC_TRY(w.exclusive_scan(w.bases.as<uint64_t>(), w.B.as<uint64_t>(), (size_t)n_runs + 1));
    PafIn in{};
    static_cast<ResultView &>(in) = w.view();
    in.distance = w.distance.as<uint32_t>();
    in.run_off = w.run_off.as<uint64_t>();
    in.run_len = w.run_len.as<uint32_t>();
    in.run_op = w.run_op.as<uint8_t>();
    in.name_len = w.name_len.as<uint64_t>();
    in.kept = w.kept.as<uint32_t>();
    in.P = w.P.as<uint64_t>();
    in.M = w.M.as<uint64_t>();
    in.B = w.B.as<uint64_t>();
    in.head_len = w.head_len.as<uint32_t>();
    in.fam = w.fam.as<uint32_t>();
    in.row_start = w.row_start.as<uint64_t>();
    in.n_rows = n_rows;
    if constexpr (kCs) {
        for (DevBuf *b : {&w.cs, &w.on_left, &w.on_right, &w.C, &w.I, &w.J}) RC_TRY(b->reserve(((size_t)n_runs + 1) * 8));
        in.text = cs.text;
        in.cs_mode = cs.mode;
        in.C = w.C.as<uint64_t>();
        in.I = w.I.as<uint64_t>();
        in.J = w.J.as<uint64_t>();
        in.bad = w.row_start.as<uint64_t>() + n_rows + 1;
        HIP_TRY(hipMemsetAsync(in.bad, 0xff, 8, s));
        paf_cs_runs_kernel<<<blocks_for(n_runs + 1), 256, 0, s>>>(in, n_runs, n, w.cs.as<uint64_t>(), w.on_left.as<uint64_t>(),
                                                                 w.on_right.as<uint64_t>());
        HIP_TRY(hipGetLastError());
        RC_TRY(w.exclusive_scan(w.cs.as<uint64_t>(), w.C.as<uint64_t>(), (size_t)n_runs + 1));
        RC_TRY(w.exclusive_scan(w.on_left.as<uint64_t>(), w.I.as<uint64_t>(), (size_t)n_runs + 1));
        RC_TRY(w.exclusive_scan(w.on_right.as<uint64_t>(), w.J.as<uint64_t>(), (size_t)n_runs + 1));
    }
    paf_rows_kernel<kCs><<<blocks_for((uint64_t)n_rows + 1), 256, 0, s>>>(in, w.head_len.as<uint32_t>(), w.fam.as<uint32_t>(),
                                                                     w.lens.as<uint64_t>());
    HIP_TRY(hipGetLastError());
    RC_TRY(w.exclusive_scan(w.lens.as<uint64_t>(), w.row_start.as<uint64_t>(), (size_t)n_rows + 1));
    RC_TRY(w.stamp(w.kPlaced));
    if constexpr (kCs) {
        uint64_t tail[2] = {0, 0};   // the size of the file and the lowest refused row, in one copy
        HIP_TRY(read_back(tail, in.row_start + n_rows, 16, s));
        if (tail[1] != ~(uint64_t)0) {
            const long long q = (long long)kept[(size_t)(tail[1] >> 2)];
            const uint64_t b = run_offsets[q], e = run_offsets[q + 1];
            if ((tail[1] & 3) == kPafBadSums) {
                uint64_t i = 0, j = 0;
                for (uint64_t t = b; t < e; ++t) {
                    if (run_op[t] != 'D') i += run_len[t];
                    if (run_op[t] != 'I') j += run_len[t];
                }
                set_error("%s: the runs of duplication %lld consume %llu and %llu bases of arms of %llu and %llu", kWhoCs, q,
                          (unsigned long long)i, (unsigned long long)j, (unsigned long long)a.sds[q].left_length,
                          (unsigned long long)a.sds[q].right_length);
            } else if ((tail[1] & 3) == kPafBadLen) {
                set_error("%s: duplication %lld has a run_len of 0 (a run of no base)", kWhoCs, q);
            } else {
                uint64_t t = b;
                while (t + 1 < e && (run_op[t] == '=' || run_op[t] == 'X' || run_op[t] == 'I' || run_op[t] == 'D')) ++t;
                set_error("%s: duplication %lld has run_op %u: an operation is one of `=`, `X`, `I`, `D`", kWhoCs, q,
                          (unsigned)run_op[t]);
            }
            return ASGART_E_ARG;
        }
        res->size = tail[0];
    } else {
        HIP_TRY(read_back(&res->size, in.row_start + n_rows, 8, s));
    }
    RC_TRY(res->file.reserve(std::max<size_t>(res->size, 16)));
    RC_TRY(w.stamp(w.kSized));
    paf_write_kernel<kCs><<<blocks_for(res->size, kStage), kThreads, 0, s>>>(in, res->size, res->file.as<uint8_t>());
    HIP_TRY(hipGetLastError());
    RC_TRY(w.stamp(w.kWritten));
    return w.finish(res);
}

}  // namespace
}  // namespace asgart

using namespace asgart;

extern "C" int32_t asgart_paf_records(int32_t device, const uint64_t *fam_offsets, int64_t n_families,
                                      const asgart_proto_sd *sds, const uint8_t *flags, const uint8_t *status,
                                      const uint32_t *distance, const int32_t *chr, const uint64_t *chr_pos, int64_t n_sd,
                                      const uint64_t *run_offsets, const uint32_t *run_len, const uint8_t *run_op,
                                      const uint8_t *name_bytes, const uint64_t *name_offsets, const uint64_t *name_length,
                                      int64_t n_names, asgart_export **out) {
    if (out) *out = nullptr;
    const ResultArg a{fam_offsets, n_families, sds, flags, chr, chr_pos, n_sd, name_bytes, name_offsets, n_names};
    std::vector<uint32_t> kept;
    RC_TRY(check_arguments(kWho, a, status, distance, run_offsets, run_len, run_op, name_length, out, kept));
    RC_TRY(use_device(kWho, device));
    return run_tool<PafWork>(out, [&](PafWork &w, asgart_export *res) {
        res->device = device;
        return run_paf<false>(w, res, CsText{nullptr, 0}, a, distance, run_offsets, run_len, run_op, name_length, kept);
    });
}

extern "C" int32_t asgart_paf_records_cs(asgart_index *idx, int32_t cs_mode, const uint64_t *fam_offsets, int64_t n_families,
                                         const asgart_proto_sd *sds, const uint8_t *flags, const uint8_t *status,
                                         const uint32_t *distance, const int32_t *chr, const uint64_t *chr_pos, int64_t n_sd,
                                         const uint64_t *run_offsets, const uint32_t *run_len, const uint8_t *run_op,
                                         const uint8_t *name_bytes, const uint64_t *name_offsets, const uint64_t *name_length,
                                         int64_t n_names, asgart_export **out) {
    if (out) *out = nullptr;
    if (cs_mode != 1 && cs_mode != 2) {
        set_error("%s: cs_mode %d: 1 is the short form, 2 the long one", kWhoCs, cs_mode);
        return ASGART_E_ARG;
    }
    if (!idx) {
        set_error("%s: bad argument (no index: the bases are its text's)", kWhoCs);
        return ASGART_E_ARG;
    }
    const ResultArg a{fam_offsets, n_families, sds, flags, chr, chr_pos, n_sd, name_bytes, name_offsets, n_names};
    std::vector<uint32_t> kept;
    RC_TRY(check_arguments(kWhoCs, a, status, distance, run_offsets, run_len, run_op, name_length, out, kept));
    const uint64_t n_text = (uint64_t)idx->n;
    for (uint32_t q : kept) {   // lev_dev.hpp's check_arms, for the duplications with a row (two empty arms are a row here)
        const asgart_proto_sd &sd = sds[q];
        if (sd.left > n_text || sd.right > n_text || sd.left_length > n_text - sd.left || sd.right_length > n_text - sd.right) {
            set_error("%s: duplication %lld reaches past the end of the text", kWhoCs, (long long)q);
            return ASGART_E_ARG;
        }
    }
    REFUSE_POISONED(idx);
    RC_TRY(use_device(kWhoCs, idx->device));
    const int32_t device = idx->device;
    return run_tool<PafWork>(out, [&](PafWork &w, asgart_export *res) {
        res->device = device;
        return run_paf<true>(w, res, CsText{idx->d_text, (uint32_t)cs_mode}, a, distance, run_offsets, run_len, run_op,
                             name_length, kept);
    });
}

extern "C" void asgart_paf_cs_geometry(uint64_t *block_threads, uint64_t *runs_per_block, uint64_t *stage_bytes,
                                       uint64_t *solo_bytes) {
    asgart_paf_geometry(block_threads, runs_per_block, stage_bytes);
    if (solo_bytes) *solo_bytes = kSolo;
}

extern "C" void asgart_paf_geometry(uint64_t *block_threads, uint64_t *runs_per_block, uint64_t *stage_bytes) {
    if (block_threads) *block_threads = kThreads;
    if (runs_per_block) *runs_per_block = kRunsMax;
    if (stage_bytes) *stage_bytes = kStage;
}
