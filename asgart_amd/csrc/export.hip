// export.hip -- result files written on the GPU: asgart_export_records and its handle, asgart_f32_shortest.
//
// Replaces, for a result held as arrays, the per-duplication part of the three exporters of reference src/exporters.rs:
// JSONExporter::save (:12-25, serde_json::to_string_pretty of the families), GFF2Exporter::save (:27-67) and
// GFF3Exporter::save (:69-113).  What a file consists of is stated once, in export_dev.hpp (units: family framing and
// records); the shortest digits of an f32 and the two forms they are printed in are in f32_digits.hpp.  Here:
//   lengths   one thread per unit: its family by bisection of the offsets, its length by running the unit through a sink that
//             counts, the digits of its identity (kept in the unit's 16-byte slot for the write stage);
//   scan      a 64-bit exclusive scan of the lengths (rocPRIM): every unit's place in the file;
//   write     a workgroup owns kUnits consecutive units, so one contiguous byte range, and two threads share a unit (its two
//             halves): file_writer.hpp's write_owned_range, through an LDS image of the range unless it does not fit (a
//             5 000-byte fragment name is legal).
#include "file_writer.hpp"
#include "export_dev.hpp"

namespace asgart {
namespace {

constexpr uint32_t kThreads = 128;    // per workgroup of the write stage: two per unit
constexpr uint32_t kUnits = 64;       // units (records and family units) per workgroup
constexpr uint32_t kStage = 40960;    // bytes of the LDS image: 640 per unit (a JSON record with short names has about 450);
                                      // four workgroups fit the 160 KiB of a CU
constexpr uint32_t kLine = 16;        // bytes per store of the copy out
static_assert(kThreads == 2 * kUnits, "two threads per unit");

__global__ __launch_bounds__(256) void export_lengths_kernel(ExportIn in, uint32_t n_units, uint4 *__restrict__ slots,
                                                             uint64_t *__restrict__ lens) {
    const uint32_t u = blockIdx.x * 256 + threadIdx.x;
    if (u > n_units) return;
    if (u == n_units) {   // the closing entry: the scan ends in the length of the body
        lens[u] = 0;
        return;
    }
    const Unit un = unit_of(in.offs, in.n_fam, u);
    CountSink c;
    F32Digits d{0, 0, 0, kF32Zero, 0};
    if (un.is_family) {
        emit_family_unit(c, in, un.fam);
    } else {
        d = f32_shortest_digits(export_identity(in, un.rec), in.pow10);
        emit_record(c, in, un.rec, un.fam, 0, d);
        emit_record(c, in, un.rec, un.fam, 1, d);
    }
    slots[u] = make_uint4(un.fam, d.digits, pack_slot_meta(d, un.is_family), un.rec);
    lens[u] = c.n;
}

// one half of the unit behind `slot` into dst, which is where the unit starts (in the image or in the file)
__device__ __forceinline__ void write_half(uint8_t *dst, const ExportIn &in, const uint4 slot, uint32_t half) {
    if (slot_is_family(slot.z)) {
        if (half == 0) {
            ByteSink s{dst};
            emit_family_unit(s, in, slot.x);
        }
        return;
    }
    const uint32_t q = slot.w;
    const F32Digits d = unpack_slot_digits(slot.y, slot.z);
    if (half == 1) {
        CountSink first;
        emit_record(first, in, q, slot.x, 0, d);
        dst += first.n;
    }
    ByteSink s{dst};
    emit_record(s, in, q, slot.x, half, d);
}

__global__ __launch_bounds__(kThreads) void export_write_kernel(ExportIn in, uint32_t n_units,
                                                                const uint4 *__restrict__ slots,
                                                                const uint64_t *__restrict__ offsets, uint64_t body_at,
                                                                uint8_t *__restrict__ out) {
    __shared__ __align__(16) uint8_t stage[kStage];
    const auto unit = [&](uint8_t *dst, uint32_t u, uint32_t half) __attribute__((always_inline)) {
        write_half(dst, in, slots[u], half);
    };
    write_owned_range<kUnits, kStage, kLine, true>(stage, offsets, body_at, n_units, out, unit);
}

__global__ __launch_bounds__(256) void f32_shortest_kernel(const float *__restrict__ values, uint64_t n, int32_t mode,
                                                           const Pow10Entry *__restrict__ pow10,
                                                           uint8_t *__restrict__ out_bytes, uint8_t *__restrict__ out_lens) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    uint8_t *text = out_bytes + i * kF32TextMax;
    ByteSink s{text};
    render_f32(s, f32_shortest_digits(values[i], pow10), mode == ASGART_F32_JSON);
    out_lens[i] = (uint8_t)(s.p - text);
}

}  // namespace
}  // namespace asgart

using namespace asgart;

namespace {

struct ExportWork : FileWork {
    DevBuf &identity = buf(), &pow10 = buf(), &slots = buf(), &lens = buf(), &offsets = buf();
};

const char kWho[] = "asgart_export_records";

// Every argument check of the call, before the device is looked at.
int32_t check_arguments(int32_t format, const ResultArg &a, const uint8_t *prefix, uint64_t prefix_len, const uint8_t *suffix,
                        uint64_t suffix_len, asgart_export **out) {
    if (!out || a.missing() || (prefix_len && !prefix) || (suffix_len && !suffix)) {
        set_error("%s: bad argument", kWho);
        return ASGART_E_ARG;
    }
    if (format != ASGART_EXPORT_JSON && format != ASGART_EXPORT_GFF2 && format != ASGART_EXPORT_GFF3) {
        set_error("%s: unknown format %d (0 JSON, 1 GFF2, 2 GFF3)", kWho, format);
        return ASGART_E_ARG;
    }
    if (a.n_sd + a.n_families >= ((int64_t)1 << 31) - 1) {
        set_error("%s: 2^31 duplications and families and more are not supported", kWho);
        return ASGART_E_CAP;
    }
    return check_result_arg(kWho, a);
}

int32_t run_export(ExportWork &w, asgart_export *res, int32_t format, const ResultArg &a, const float *identity,
                   const uint8_t *prefix, uint64_t prefix_len, const uint8_t *suffix, uint64_t suffix_len) {
    const uint32_t n = (uint32_t)a.n_sd;
    RC_TRY(w.open_call());
    hipStream_t s = w.s;
    RC_TRY(w.upload(a));
    if (identity) RC_TRY(w.upload(w.identity, identity, (size_t)n * 4));
    RC_TRY(w.upload(w.pow10, pow10_table(), sizeof(Pow10Entry) * kPow10Entries));
    RC_TRY(w.stamp(w.kUploaded));
    const uint32_t n_units = n + w.n_fam + 1;
    RC_TRY(w.slots.reserve((size_t)n_units * 16));
    RC_TRY(w.lens.reserve(((size_t)n_units + 1) * 8));
    RC_TRY(w.offsets.reserve(((size_t)n_units + 1) * 8));
    ExportIn in{};
    static_cast<ResultView &>(in) = w.view();
    in.identity = identity ? w.identity.as<float>() : nullptr;
    in.pow10 = w.pow10.as<Pow10Entry>();
    in.n = n;
    in.format = format;
    uint64_t *lens = w.lens.as<uint64_t>(), *offsets = w.offsets.as<uint64_t>();
    export_lengths_kernel<<<(unsigned)(((uint64_t)n_units + 1 + 255) / 256), 256, 0, s>>>(in, n_units, w.slots.as<uint4>(),
                                                                                          lens);
    HIP_TRY(hipGetLastError());
    RC_TRY(w.exclusive_scan(lens, offsets, (size_t)n_units + 1));
    RC_TRY(w.stamp(w.kPlaced));
    RC_TRY(w.frame_file(res, offsets + n_units, prefix, prefix_len, suffix, suffix_len));
    export_write_kernel<<<(n_units + kUnits - 1) / kUnits, kThreads, 0, s>>>(in, n_units, w.slots.as<uint4>(), offsets,
                                                                             prefix_len, res->file.as<uint8_t>());
    HIP_TRY(hipGetLastError());
    RC_TRY(w.stamp(w.kWritten));
    return w.finish(res);
}

}  // namespace

extern "C" int32_t asgart_export_records(int32_t device, int32_t format, const uint64_t *fam_offsets, int64_t n_families,
                                         const asgart_proto_sd *sds, const uint8_t *flags, const float *identity,
                                         const int32_t *chr, const uint64_t *chr_pos, int64_t n_sd,
                                         const uint8_t *name_bytes, const uint64_t *name_offsets, int64_t n_names,
                                         const uint8_t *prefix, uint64_t prefix_len, const uint8_t *suffix,
                                         uint64_t suffix_len, asgart_export **out) {
    if (out) *out = nullptr;
    const ResultArg a{fam_offsets, n_families, sds, flags, chr, chr_pos, n_sd, name_bytes, name_offsets, n_names};
    RC_TRY(check_arguments(format, a, prefix, prefix_len, suffix, suffix_len, out));
    RC_TRY(use_device(kWho, device));
    return run_tool<ExportWork>(out, [&](ExportWork &w, asgart_export *res) {
        res->device = device;
        return run_export(w, res, format, a, identity, prefix, prefix_len, suffix, suffix_len);
    });
}

extern "C" uint64_t asgart_export_size(const asgart_export *e) { return e ? e->size : 0; }

extern "C" int32_t asgart_export_copy(asgart_export *e, uint8_t *dst, uint64_t capacity) {
    if (!e || (e->size && !dst) || capacity < e->size) {
        set_error("asgart_export_copy: bad argument (the file has %llu bytes)", (unsigned long long)(e ? e->size : 0));
        return ASGART_E_ARG;
    }
    const auto t0 = std::chrono::steady_clock::now();
    HIP_TRY(hipSetDevice(e->device));
    if (e->size) HIP_TRY(hipMemcpy(dst, e->file.p, e->size, hipMemcpyDeviceToHost));
    e->ms[2] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return 0;
}

extern "C" int32_t asgart_export_timings(const asgart_export *e, double *ms3) {
    return copy_ms3("asgart_export_timings", e, ms3);
}

extern "C" void asgart_export_free(asgart_export *e) { delete e; }

extern "C" void asgart_export_geometry(uint64_t *block_threads, uint64_t *records_per_block, uint64_t *stage_bytes) {
    if (block_threads) *block_threads = kThreads;
    if (records_per_block) *records_per_block = kUnits;
    if (stage_bytes) *stage_bytes = kStage;
}

extern "C" int32_t asgart_f32_pow10_table(int32_t *k_min, int32_t *k_max, uint64_t *entries) {
    if (k_min) *k_min = kPow10Min;
    if (k_max) *k_max = kPow10Max;
    if (entries) memcpy(entries, pow10_table(), sizeof(Pow10Entry) * kPow10Entries);
    return kPow10Entries;
}

extern "C" int32_t asgart_f32_shortest(int32_t device, const float *values, int64_t n, int32_t mode, uint8_t *out_bytes,
                                       uint8_t *out_lens) {
    if (n < 0 || (n && (!values || !out_bytes || !out_lens)) || (mode != ASGART_F32_JSON && mode != ASGART_F32_DISPLAY)) {
        set_error("asgart_f32_shortest: bad argument (mode 0: serde_json's form, 1: Rust's `{}`)");
        return ASGART_E_ARG;
    }
    RC_TRY(use_device("asgart_f32_shortest", device));
    if (n == 0) return 0;
    ToolWork w;
    DevBuf &d_values = w.buf(), &pow10 = w.buf(), &bytes = w.buf(), &lens = w.buf();
    RC_TRY(w.open(0));
    RC_TRY(w.upload(d_values, values, (size_t)n * 4));
    RC_TRY(w.upload(pow10, pow10_table(), sizeof(Pow10Entry) * kPow10Entries));
    RC_TRY(bytes.reserve((size_t)n * kF32TextMax));
    RC_TRY(lens.reserve((size_t)n));
    HIP_TRY(hipMemsetAsync(bytes.p, 0, (size_t)n * kF32TextMax, w.s));
    f32_shortest_kernel<<<(unsigned)(((uint64_t)n + 255) / 256), 256, 0, w.s>>>(
        d_values.as<float>(), (uint64_t)n, mode, pow10.as<Pow10Entry>(), bytes.as<uint8_t>(), lens.as<uint8_t>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(stream_sync(w.s));
    HIP_TRY(hipMemcpyAsync(out_bytes, bytes.p, (size_t)n * kF32TextMax, hipMemcpyDeviceToHost, w.s));
    HIP_TRY(hipMemcpyAsync(out_lens, lens.p, (size_t)n, hipMemcpyDeviceToHost, w.s));
    HIP_TRY(stream_sync(w.s));
    return 0;
}
