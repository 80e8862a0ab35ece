// variants_write.hip -- the two files of the variants, written on the GPU from the handles variants.hip made:
// asgart_variants_records (the pair table, one row per record; align.psv_table_text is the readable statement) and
// asgart_sites_records (VCF body rows, one per site; align.psv_vcf_text).  include/asgart_hip.h names the columns.
//
// Apart from its names a row's size is bounded, so this is the shape of sdtable.hip, once for both files (a row source
// says what a row consists of, in two halves so that two threads can share it):
//   lengths   one thread per row: its length by running both halves through a sink that counts;
//   scan      a 64-bit exclusive scan of the lengths (rocPRIM): every row's place in the file;
//   write     a workgroup owns kRows consecutive rows, so one contiguous byte range, and two threads share a row:
//             file_writer.hpp's write_owned_range, through an LDS image of the range unless it does not fit (a name of any
//             length is legal).
// The records and the sites are read where they are, on the device; only the result arrays are uploaded.
#include "file_writer.hpp"
#include "export_dev.hpp"
#include "variants_dev.hpp"

namespace asgart {
namespace {

constexpr uint32_t kThreads = 128;   // per workgroup of the write stage: two per row
constexpr uint32_t kRows = 64;       // rows per workgroup
constexpr uint32_t kStage = 16384;   // bytes of the LDS image: 256 per row (a pair row with short names has about 40); nine
                                     // workgroups fit the 160 KiB of a CU
constexpr uint32_t kLine = 16;       // bytes per store of the copy out
static_assert(kThreads == 2 * kRows, "two threads per row");

// the name and the local position of a global position on arm `side` of duplication q, and a tab behind each
template <class Sink>
__host__ __device__ inline void emit_name(Sink &s, const ResultView &in, uint32_t q, uint32_t side) {
    const int32_t id = in.chr[2 * (size_t)q + side];
    const uint64_t a = in.name_off[id];
    s.bytes(in.names + a, in.name_off[id + 1] - a);
    s.byte('\t');
}
__host__ __device__ inline uint64_t local_pos(const ResultView &in, uint32_t q, uint32_t side, uint64_t global) {
    return in.chr_pos[2 * (size_t)q + side] + (global - in.sds[4 * (size_t)q + side]);
}

// The pair table.  Half 0 of a row is the left interval (columns 1 to 3 and their tabs), half 1 the rest.
struct PairRows : ResultView {
    const asgart_variant *recs;
    uint32_t n_rows;
    template <class Sink>
    __host__ __device__ void emit(Sink &s, uint32_t k, uint32_t half) const {
        const asgart_variant r = recs[k];
        const uint32_t q = r.sd;
        const uint64_t at = local_pos(*this, q, half, half ? r.right_pos : r.left_pos);
        emit_name(s, *this, q, half);
        s.u64(at);
        s.byte('\t');
        s.u64(at + (half ? r.right_len : r.left_len));
        s.byte('\t');
        if (half == 0) return;
        s.lit("sd");
        s.u64(q);
        s.byte('\t');
        s.byte(r.op);
        s.byte('\t');
        s.byte(r.flag == 3 ? '-' : '+');
        s.byte('\t');
        s.u64(segment_of(offs, n_fam, q));
        s.byte('\t');
        s.byte(r.op == 'X' ? r.left_base : '.');
        s.byte('\t');
        s.byte(r.op == 'X' ? r.right_base : '.');
        s.byte('\n');
    }
};

// The VCF body.  Half 0 of a row is CHROM and POS, half 1 the rest.
struct SiteRows : ResultView {
    const uint64_t *pos;
    const uint32_t *pairs, *sd;
    const uint8_t *ref, *alt_mask, *side;
    uint32_t n_rows;
    template <class Sink>
    __host__ __device__ void emit(Sink &s, uint32_t k, uint32_t half) const {
        if (half == 0) {
            const uint32_t q = sd[k], arm = side[k];
            emit_name(s, *this, q, arm);
            s.u64(local_pos(*this, q, arm, pos[k]) + 1);
            return;
        }
        s.lit("\t.\t");
        s.byte(class_letter(ref[k]));
        s.byte('\t');
        bool first = true;
        for (uint32_t c = 0; c < 5; ++c)
            if (alt_mask[k] >> c & 1u) {
                if (!first) s.byte(',');
                s.byte(class_letter(c));
                first = false;
            }
        s.lit("\t.\t.\tNP=");
        s.u64(pairs[k]);
        s.byte('\n');
    }
};

template <class Rows>
__global__ __launch_bounds__(256) void variants_lengths_kernel(Rows in, uint32_t *__restrict__ half_at,
                                                               uint64_t *__restrict__ lens) {
    const uint32_t k = blockIdx.x * 256 + threadIdx.x;
    if (k > in.n_rows) return;
    if (k == in.n_rows) {   // the closing entry: the scan ends in the length of the body
        lens[k] = 0;
        return;
    }
    CountSink c;
    in.emit(c, k, 0);
    half_at[k] = (uint32_t)c.n;   // (names are below 2^30 bytes: the first half is below 2^32)
    in.emit(c, k, 1);
    lens[k] = c.n;
}

template <class Rows>
__global__ __launch_bounds__(kThreads) void variants_write_kernel(Rows in, const uint32_t *__restrict__ half_at,
                                                                  const uint64_t *__restrict__ offsets, uint64_t body_at,
                                                                  uint8_t *__restrict__ out) {
    __shared__ __align__(16) uint8_t stage[kStage];
    const auto row = [&](uint8_t *dst, uint32_t k, uint32_t half) __attribute__((always_inline)) {
        ByteSink s{dst + (half ? half_at[k] : 0u)};
        in.emit(s, k, half);
    };
    write_owned_range<kRows, kStage, kLine, false>(stage, offsets, body_at, in.n_rows, out, row);
}

struct RowsWork : FileWork {
    DevBuf &half_at = buf(), &lens = buf(), &offsets = buf();
};

// the file of `rows` (their ResultView is filled here) behind the prefix
template <class Rows>
int32_t run_rows(RowsWork &w, asgart_export *res, const ResultArg &a, Rows rows, const uint8_t *prefix, uint64_t prefix_len) {
    const uint32_t n_rows = rows.n_rows;
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
    RC_TRY(w.stamp(w.kUploaded));
    static_cast<ResultView &>(rows) = w.view();
    RC_TRY(w.half_at.reserve((size_t)n_rows * 4));
    RC_TRY(w.lens.reserve(((size_t)n_rows + 1) * 8));
    RC_TRY(w.offsets.reserve(((size_t)n_rows + 1) * 8));
    uint64_t *lens = w.lens.as<uint64_t>(), *offsets = w.offsets.as<uint64_t>();
    variants_lengths_kernel<<<blocks_for((uint64_t)n_rows + 1), 256, 0, s>>>(rows, w.half_at.as<uint32_t>(), lens);
    HIP_TRY(hipGetLastError());
    RC_TRY(w.exclusive_scan(lens, offsets, (size_t)n_rows + 1));
    RC_TRY(w.stamp(w.kPlaced));
    RC_TRY(w.frame_file(res, offsets + n_rows, prefix, prefix_len, nullptr, 0));
    variants_write_kernel<<<blocks_for(n_rows, kRows), kThreads, 0, s>>>(rows, w.half_at.as<uint32_t>(), offsets, prefix_len,
                                                                        res->file.as<uint8_t>());
    HIP_TRY(hipGetLastError());
    RC_TRY(w.stamp(w.kWritten));
    return w.finish(res);
}

// What both entry points check on the host: the arrays as asgart_sdtable_records checks them, with "a row" meaning a
// duplication with a record (var_offsets, the records' call).
int32_t check_rows(const char *who, const ResultArg &a, const std::vector<uint64_t> &var_offsets, const uint8_t *prefix,
                   uint64_t prefix_len, const void *out) {
    if (!out || a.missing() || (prefix_len && !prefix)) {
        set_error("%s: bad argument", who);
        return ASGART_E_ARG;
    }
    if (a.n_sd >= (int64_t)1 << 31 || a.n_families >= (int64_t)1 << 31) {
        set_error("%s: 2^31 rows (or families) and more are not supported", who);
        return ASGART_E_CAP;
    }
    if ((uint64_t)a.n_sd + 1 != var_offsets.size()) {
        set_error("%s: %lld duplications, and the variants were called from %llu", who, (long long)a.n_sd,
                  (unsigned long long)(var_offsets.size() - 1));
        return ASGART_E_ARG;
    }
    RC_TRY(check_result_arg(who, a));
    std::vector<uint8_t> has_rows((size_t)a.n_sd);
    for (int64_t q = 0; q < a.n_sd; ++q) has_rows[q] = var_offsets[q + 1] > var_offsets[q];
    std::vector<uint32_t> kept;
    return check_strand_rows(who, a.sds, a.flags, has_rows.data(), a.chr_pos, a.n_sd, kept);
}

const char kWhoPairs[] = "asgart_variants_records";
const char kWhoSites[] = "asgart_sites_records";

}  // namespace
}  // namespace asgart

using namespace asgart;

extern "C" int32_t asgart_variants_records(const asgart_variants *v, const uint64_t *fam_offsets, int64_t n_families,
                                           const asgart_proto_sd *sds, const uint8_t *flags, const int32_t *chr,
                                           const uint64_t *chr_pos, int64_t n_sd, const uint8_t *name_bytes,
                                           const uint64_t *name_offsets, int64_t n_names, const uint8_t *prefix,
                                           uint64_t prefix_len, asgart_export **out) {
    if (out) *out = nullptr;
    if (!v) {
        set_error("%s: bad argument (no variants)", kWhoPairs);
        return ASGART_E_ARG;
    }
    const ResultArg a{fam_offsets, n_families, sds, flags, chr, chr_pos, n_sd, name_bytes, name_offsets, n_names};
    RC_TRY(check_rows(kWhoPairs, a, v->var_offsets, prefix, prefix_len, out));
    RC_TRY(use_device(kWhoPairs, v->device));
    return run_tool<RowsWork>(out, [&](RowsWork &w, asgart_export *res) {
        res->device = v->device;
        PairRows rows{};
        rows.recs = v->records.as<asgart_variant>();
        rows.n_rows = (uint32_t)v->n_variants;
        return run_rows(w, res, a, rows, prefix, prefix_len);
    });
}

extern "C" int32_t asgart_sites_records(const asgart_sites *r, const uint64_t *fam_offsets, int64_t n_families,
                                        const asgart_proto_sd *sds, const uint8_t *flags, const int32_t *chr,
                                        const uint64_t *chr_pos, int64_t n_sd, const uint8_t *name_bytes,
                                        const uint64_t *name_offsets, int64_t n_names, const uint8_t *prefix,
                                        uint64_t prefix_len, asgart_export **out) {
    if (out) *out = nullptr;
    if (!r) {
        set_error("%s: bad argument (no sites)", kWhoSites);
        return ASGART_E_ARG;
    }
    const ResultArg a{fam_offsets, n_families, sds, flags, chr, chr_pos, n_sd, name_bytes, name_offsets, n_names};
    RC_TRY(check_rows(kWhoSites, a, r->var_offsets, prefix, prefix_len, out));
    RC_TRY(use_device(kWhoSites, r->device));
    return run_tool<RowsWork>(out, [&](RowsWork &w, asgart_export *res) {
        res->device = r->device;
        SiteRows rows{};
        rows.pos = r->pos.as<uint64_t>();
        rows.pairs = r->pairs.as<uint32_t>();
        rows.sd = r->sd.as<uint32_t>();
        rows.ref = r->ref.as<uint8_t>();
        rows.alt_mask = r->alt_mask.as<uint8_t>();
        rows.side = r->side.as<uint8_t>();
        rows.n_rows = (uint32_t)r->n_sites;
        return run_rows(w, res, a, rows, prefix, prefix_len);
    });
}

extern "C" void asgart_variants_records_geometry(uint64_t *block_threads, uint64_t *rows_per_block, uint64_t *stage_bytes) {
    if (block_threads) *block_threads = kThreads;
    if (rows_per_block) *rows_per_block = kRows;
    if (stage_bytes) *stage_bytes = kStage;
}

extern "C" void asgart_sites_records_geometry(uint64_t *block_threads, uint64_t *rows_per_block, uint64_t *stage_bytes) {
    if (block_threads) *block_threads = kThreads;
    if (rows_per_block) *rows_per_block = kRows;
    if (stage_bytes) *stage_bytes = kStage;
}
