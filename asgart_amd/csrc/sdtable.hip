// sdtable.hip -- the duplication table written on the GPU: asgart_sdtable_records, the counterpart of align.sd_table_text
// for a caller of the C ABI.
//
// What a row consists of is stated once, in sdtable_dev.hpp.  Apart from its names a row's size is bounded, so this is the
// shape of export.hip, with row and length kernels of its own (export.hip's are specialised to the three result formats):
//   lengths   one thread per row: its family by bisection of the offsets, its length by running both halves of the row
//             through a sink that counts;
//   scan      a 64-bit exclusive scan of the lengths (rocPRIM): every row's place in the file;
//   write     a workgroup owns kRows consecutive rows, so one contiguous byte range, and two threads share a row (its two
//             halves): file_writer.hpp's write_owned_range, through an LDS image of the range unless it does not fit (a
//             name of any length is legal).
// The four figures arrive as f32 arrays (align.divergence): the file does not depend on whose logarithm ran; their digits
// are f32_digits.hpp's, in display form.
#include "file_writer.hpp"
#include "sdtable_dev.hpp"

namespace asgart {
namespace {

constexpr uint32_t kThreads = 128;   // per workgroup of the write stage: two per row
constexpr uint32_t kRows = 64;       // rows per workgroup
constexpr uint32_t kStage = 24576;   // bytes of the LDS image: 384 per row (a row with short names has about 150); six
                                     // workgroups fit the 160 KiB of a CU
constexpr uint32_t kLine = 16;       // bytes per store of the copy out
static_assert(kThreads == 2 * kRows, "two threads per row");

__global__ __launch_bounds__(256) void sdtable_lengths_kernel(SdTableIn in, uint32_t *__restrict__ fam, uint32_t *__restrict__ half_at,
                                                              uint64_t *__restrict__ lens) {
    const uint32_t k = blockIdx.x * 256 + threadIdx.x;
    if (k > in.n_rows) return;
    if (k == in.n_rows) {   // the closing entry: the scan ends in the length of the body
        lens[k] = 0;
        return;
    }
    const uint32_t q = in.kept[k];
    const uint32_t f = segment_of(in.offs, in.n_fam, q);
    CountSink c;
    emit_sd_row(c, in, q, f, 0);
    const uint64_t first = c.n;
    emit_sd_row(c, in, q, f, 1);
    fam[k] = f;
    half_at[k] = (uint32_t)first;   // (names are below 2^30 bytes: the first half is below 2^32)
    lens[k] = c.n;
}

__global__ __launch_bounds__(kThreads) void sdtable_write_kernel(SdTableIn in, const uint32_t *__restrict__ fam,
                                                                 const uint32_t *__restrict__ half_at,
                                                                 const uint64_t *__restrict__ offsets, uint64_t body_at,
                                                                 uint8_t *__restrict__ out) {
    __shared__ __align__(16) uint8_t stage[kStage];
    const auto row = [&](uint8_t *dst, uint32_t k, uint32_t half) __attribute__((always_inline)) {
        ByteSink s{dst + (half ? half_at[k] : 0u)};
        emit_sd_row(s, in, in.kept[k], fam[k], half);
    };
    write_owned_range<kRows, kStage, kLine, false>(stage, offsets, body_at, in.n_rows, out, row);
}

struct SdTableWork : FileWork {
    DevBuf &kept = buf(), &counts = buf(), &figures = buf(), &pow10 = buf(), &fam = buf(), &half_at = buf(), &lens = buf(),
           &offsets = buf();
};

const char kWho[] = "asgart_sdtable_records";

int32_t run_sdtable(SdTableWork &w, asgart_export *res, const ResultArg &a, const asgart_align_counts *counts,
                    const float *const figures[4], const uint8_t *prefix, uint64_t prefix_len,
                    const std::vector<uint32_t> &kept) {
    const uint32_t n = (uint32_t)a.n_sd, n_rows = (uint32_t)kept.size();
    RC_TRY(w.open_call());
    hipStream_t s = w.s;
    if (n_rows == 0) {   // the header only
        res->size = prefix_len;
        RC_TRY(res->file.reserve(std::max<size_t>(res->size, 16)));
        if (prefix_len) HIP_TRY(hipMemcpyAsync(res->file.p, prefix, prefix_len, hipMemcpyHostToDevice, s));
        HIP_TRY(stream_sync(s));
        return 0;
    }
    RC_TRY(w.upload(a));
    RC_TRY(w.upload(w.kept, kept.data(), (size_t)n_rows * 4));
    RC_TRY(w.upload(w.counts, counts, (size_t)n * sizeof(asgart_align_counts)));
    RC_TRY(w.figures.reserve(std::max<size_t>((size_t)n * 16, 16)));
    for (int i = 0; i < 4; ++i)
        HIP_TRY(hipMemcpyAsync(w.figures.as<float>() + (size_t)i * n, figures[i], (size_t)n * 4, hipMemcpyHostToDevice, s));
    RC_TRY(w.upload(w.pow10, pow10_table(), sizeof(Pow10Entry) * kPow10Entries));
    RC_TRY(w.stamp(w.kUploaded));
    RC_TRY(w.fam.reserve((size_t)n_rows * 4));
    RC_TRY(w.half_at.reserve((size_t)n_rows * 4));
    RC_TRY(w.lens.reserve(((size_t)n_rows + 1) * 8));
    RC_TRY(w.offsets.reserve(((size_t)n_rows + 1) * 8));
    SdTableIn in{};
    static_cast<ResultView &>(in) = w.view();
    in.kept = w.kept.as<uint32_t>();
    in.counts = w.counts.as<uint64_t>();
    for (int i = 0; i < 4; ++i) in.figures[i] = w.figures.as<float>() + (size_t)i * n;
    in.pow10 = w.pow10.as<Pow10Entry>();
    in.n_rows = n_rows;
    uint64_t *lens = w.lens.as<uint64_t>(), *offsets = w.offsets.as<uint64_t>();
    sdtable_lengths_kernel<<<blocks_for((uint64_t)n_rows + 1), 256, 0, s>>>(in, w.fam.as<uint32_t>(), w.half_at.as<uint32_t>(),
                                                                          lens);
    HIP_TRY(hipGetLastError());
    RC_TRY(w.exclusive_scan(lens, offsets, (size_t)n_rows + 1));
    RC_TRY(w.stamp(w.kPlaced));
    RC_TRY(w.frame_file(res, offsets + n_rows, prefix, prefix_len, nullptr, 0));
    sdtable_write_kernel<<<blocks_for(n_rows, kRows), kThreads, 0, s>>>(in, w.fam.as<uint32_t>(), w.half_at.as<uint32_t>(),
                                                                       offsets, prefix_len, res->file.as<uint8_t>());
    HIP_TRY(hipGetLastError());
    RC_TRY(w.stamp(w.kWritten));
    return w.finish(res);
}

}  // namespace
}  // namespace asgart

using namespace asgart;

extern "C" int32_t asgart_sdtable_records(int32_t device, const uint64_t *fam_offsets, int64_t n_families,
                                          const asgart_proto_sd *sds, const uint8_t *flags, const uint8_t *status,
                                          const int32_t *chr, const uint64_t *chr_pos, int64_t n_sd, const uint8_t *name_bytes,
                                          const uint64_t *name_offsets, int64_t n_names, const asgart_align_counts *counts,
                                          const float *frac_match, const float *frac_match_indel, const float *jc_k,
                                          const float *k2_k, const uint8_t *prefix, uint64_t prefix_len, asgart_export **out) {
    if (out) *out = nullptr;
    const ResultArg a{fam_offsets, n_families, sds, flags, chr, chr_pos, n_sd, name_bytes, name_offsets, n_names};
    if (!out || a.missing() || (prefix_len && !prefix) ||
        (n_sd && (!status || !counts || !frac_match || !frac_match_indel || !jc_k || !k2_k))) {
        set_error("%s: bad argument", kWho);
        return ASGART_E_ARG;
    }
    if (n_sd >= (int64_t)1 << 31 || n_families >= (int64_t)1 << 31) {
        set_error("%s: 2^31 rows (or families) and more are not supported", kWho);
        return ASGART_E_CAP;
    }
    RC_TRY(check_result_arg(kWho, a));
    std::vector<uint32_t> kept;
    RC_TRY(check_strand_rows(kWho, sds, flags, status, chr_pos, n_sd, kept));
    RC_TRY(use_device(kWho, device));
    const float *const figures[4] = {frac_match, frac_match_indel, jc_k, k2_k};
    return run_tool<SdTableWork>(out, [&](SdTableWork &w, asgart_export *res) {
        res->device = device;
        return run_sdtable(w, res, a, counts, figures, prefix, prefix_len, kept);
    });
}

extern "C" void asgart_sdtable_geometry(uint64_t *block_threads, uint64_t *records_per_block, uint64_t *stage_bytes) {
    if (block_threads) *block_threads = kThreads;
    if (records_per_block) *records_per_block = kRows;
    if (stage_bytes) *stage_bytes = kStage;
}
