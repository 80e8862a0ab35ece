// export.hip -- result files written on the GPU: asgart_export_records and its handle, asgart_f32_shortest.
//
// Replaces, for a result held as arrays, the per-duplication part of the three exporters of reference src/exporters.rs:
// JSONExporter::save (:12-25, serde_json::to_string_pretty of the families), GFF2Exporter::save (:27-67) and
// GFF3Exporter::save (:69-113).  What a file consists of is stated once, in export_dev.hpp (units: family framing and
// records); the shortest digits of an f32 and the two forms they are printed in are in f32_digits.hpp.  Here:
//   lengths   one thread per unit: its family by bisection of the offsets, its length by running the unit through a sink that
//             counts, the digits of its identity (kept in the unit's 16-byte slot for the write stage);
//   scan      a 64-bit exclusive scan of the lengths (rocPRIM): every unit's place in the file;
//   write     a workgroup owns kUnits consecutive units, so one contiguous byte range.  Two threads share a unit (its two
//             halves) and store its bytes into an LDS image of the range, laid out so that a 16-byte line of the file is a
//             16-byte line of the image; then all threads move the image out with one aligned 16-byte store per lane, a wave
//             1 KiB of consecutive bytes.  Only the lines the range shares with its neighbours (its head and its tail, fewer
//             than 16 bytes each) go out byte by byte.  A range that does not fit the image (a 5 000-byte fragment name is
//             legal) is stored from the threads directly: slower, never refused.
#include "tool_base.hpp"
#include "export_dev.hpp"

namespace asgart {
namespace {

constexpr uint32_t kThreads = 128;    // per workgroup of the write stage: two per unit
constexpr uint32_t kUnits = 64;       // units (records and family units) per workgroup
constexpr uint32_t kStage = 40960;    // bytes of the LDS image: 640 per unit (a JSON record with short names has about 450);
                                      // four workgroups fit the 160 KiB of a CU
constexpr uint32_t kLine = 16;        // bytes per store of the copy out

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
    const uint32_t first = blockIdx.x * kUnits;
    const uint32_t last = min(first + kUnits, n_units);
    const uint64_t g0 = body_at + offsets[first], g1 = body_at + offsets[last];   // the workgroup's bytes of the file
    const uint64_t a0 = g0 & ~(uint64_t)(kLine - 1);                              // the image starts on a line of the file
    const bool staged = g1 - a0 <= kStage;
    const uint32_t u = first + (threadIdx.x >> 1), half = threadIdx.x & 1;
    if (u < last) {
        const uint64_t at = body_at + offsets[u];
        if (staged)
            write_half(stage + (at - a0), in, slots[u], half);
        else
            write_half(out + at, in, slots[u], half);
    }
    if (!staged) return;   // (the same in every thread of the workgroup)
    __syncthreads();
    const uint32_t lines = (uint32_t)((g1 - a0 + kLine - 1) / kLine);
    for (uint32_t l = threadIdx.x; l < lines; l += kThreads) {
        const uint64_t a = a0 + (uint64_t)l * kLine;
        if (a >= g0 && a + kLine <= g1) {
            *reinterpret_cast<uint4 *>(out + a) = *reinterpret_cast<const uint4 *>(stage + l * kLine);
        } else {   // a line shared with the neighbouring range, or with the prefix or the suffix: this range's bytes only
            const uint64_t lo = max(a, g0), hi = min(a + kLine, g1);
            for (uint64_t b = lo; b < hi; ++b) out[b] = stage[b - a0];
        }
    }
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

struct ExportWork : ToolWork {
    DevBuf &offs = buf(), &sds = buf(), &flags = buf(), &identity = buf(), &chr = buf(), &chr_pos = buf(), &names = buf(),
           &name_off = buf(), &pow10 = buf(), &slots = buf(), &lens = buf(), &offsets = buf();
};

// Every argument check of the call, before the device is looked at.
int32_t check_arguments(int32_t format, const uint64_t *fam_offsets, int64_t n_families, const asgart_proto_sd *sds,
                        const uint8_t *flags, const int32_t *chr, const uint64_t *chr_pos, int64_t n_sd,
                        const uint8_t *name_bytes, const uint64_t *name_offsets, int64_t n_names, const uint8_t *prefix,
                        uint64_t prefix_len, const uint8_t *suffix, uint64_t suffix_len, asgart_export **out) {
    if (!out || !fam_offsets || n_families < 0 || n_sd < 0 || n_names < 0 || !name_offsets ||
        (n_sd && (!sds || !flags || !chr || !chr_pos)) || (prefix_len && !prefix) || (suffix_len && !suffix)) {
        set_error("asgart_export_records: bad argument");
        return ASGART_E_ARG;
    }
    if (format != ASGART_EXPORT_JSON && format != ASGART_EXPORT_GFF2 && format != ASGART_EXPORT_GFF3) {
        set_error("asgart_export_records: unknown format %d (0 JSON, 1 GFF2, 2 GFF3)", format);
        return ASGART_E_ARG;
    }
    if (n_sd + n_families >= ((int64_t)1 << 31) - 1) {
        set_error("asgart_export_records: 2^31 duplications and families and more are not supported");
        return ASGART_E_CAP;
    }
    RC_TRY(check_csr("asgart_export_records", "fam_offsets", fam_offsets, n_families, n_sd, "n_sd"));
    if (name_offsets[0] != 0 || (name_offsets[n_names] && !name_bytes) || name_offsets[n_names] >= ((uint64_t)1 << 30)) {
        set_error("asgart_export_records: name_offsets must start at 0 and end below 2^30 bytes of names");
        return ASGART_E_ARG;
    }
    for (int64_t k = 0; k < n_names; ++k)
        if (name_offsets[k] > name_offsets[k + 1]) {
            set_error("asgart_export_records: name_offsets decrease at name %lld", (long long)k);
            return ASGART_E_ARG;
        }
    return check_name_ids("asgart_export_records", chr, n_sd, n_names);
}

int32_t run_export(ExportWork &w, asgart_export *res, int32_t format, const uint64_t *fam_offsets, uint32_t nf,
                   const asgart_proto_sd *sds, const uint8_t *flags, const float *identity, const int32_t *chr,
                   const uint64_t *chr_pos, uint32_t n, const uint8_t *name_bytes, const uint64_t *name_offsets,
                   size_t n_names, const uint8_t *prefix, uint64_t prefix_len, const uint8_t *suffix, uint64_t suffix_len) {
    RC_TRY(w.open(5));
    hipStream_t s = w.s;
    HIP_TRY(hipEventRecord(w.ev[0], s));
    RC_TRY(w.upload(w.offs, fam_offsets, ((size_t)nf + 1) * 8));
    RC_TRY(w.upload(w.sds, sds, (size_t)n * sizeof(asgart_proto_sd)));
    RC_TRY(w.upload(w.flags, flags, n));
    if (identity) RC_TRY(w.upload(w.identity, identity, (size_t)n * 4));
    RC_TRY(w.upload(w.chr, chr, (size_t)n * 8));
    RC_TRY(w.upload(w.chr_pos, chr_pos, (size_t)n * 16));
    RC_TRY(w.upload(w.names, name_bytes, (size_t)name_offsets[n_names]));
    RC_TRY(w.upload(w.name_off, name_offsets, (n_names + 1) * 8));
    RC_TRY(w.upload(w.pow10, pow10_table(), sizeof(Pow10Entry) * kPow10Entries));
    HIP_TRY(hipEventRecord(w.ev[1], s));
    const uint32_t n_units = n + nf + 1;
    RC_TRY(w.slots.reserve((size_t)n_units * 16));
    RC_TRY(w.lens.reserve(((size_t)n_units + 1) * 8));
    RC_TRY(w.offsets.reserve(((size_t)n_units + 1) * 8));
    ExportIn in{};
    in.offs = w.offs.as<uint64_t>();
    in.sds = w.sds.as<uint64_t>();
    in.flags = w.flags.as<uint8_t>();
    in.identity = identity ? w.identity.as<float>() : nullptr;
    in.chr = w.chr.as<int32_t>();
    in.chr_pos = w.chr_pos.as<uint64_t>();
    in.names = w.names.as<uint8_t>();
    in.name_off = w.name_off.as<uint64_t>();
    in.pow10 = w.pow10.as<Pow10Entry>();
    in.n_fam = nf;
    in.n = n;
    in.format = format;
    uint64_t *lens = w.lens.as<uint64_t>(), *offsets = w.offsets.as<uint64_t>();
    export_lengths_kernel<<<(unsigned)(((uint64_t)n_units + 1 + 255) / 256), 256, 0, s>>>(in, n_units, w.slots.as<uint4>(),
                                                                                          lens);
    HIP_TRY(hipGetLastError());
    RC_TRY(w.exclusive_scan(lens, offsets, (size_t)n_units + 1));
    HIP_TRY(hipEventRecord(w.ev[2], s));
    uint64_t body = 0;
    HIP_TRY(read_back(&body, offsets + n_units, 8, s));
    res->size = prefix_len + body + suffix_len;
    RC_TRY(res->file.reserve(std::max<size_t>(res->size, 16)));
    uint8_t *file = res->file.as<uint8_t>();
    HIP_TRY(hipEventRecord(w.ev[3], s));
    if (prefix_len) HIP_TRY(hipMemcpyAsync(file, prefix, prefix_len, hipMemcpyHostToDevice, s));
    if (suffix_len) HIP_TRY(hipMemcpyAsync(file + prefix_len + body, suffix, suffix_len, hipMemcpyHostToDevice, s));
    export_write_kernel<<<(n_units + kUnits - 1) / kUnits, kThreads, 0, s>>>(in, n_units, w.slots.as<uint4>(), offsets,
                                                                             prefix_len, file);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(w.ev[4], s));
    HIP_TRY(stream_sync(s));
    float up = 0, a = 0, b = 0;
    HIP_TRY(hipEventElapsedTime(&up, w.ev[0], w.ev[1]));
    HIP_TRY(hipEventElapsedTime(&a, w.ev[1], w.ev[2]));
    HIP_TRY(hipEventElapsedTime(&b, w.ev[3], w.ev[4]));
    res->ms[0] = up;
    res->ms[1] = (double)a + (double)b;
    return 0;
}

}  // namespace

extern "C" int32_t asgart_export_records(int32_t device, int32_t format, const uint64_t *fam_offsets, int64_t n_families,
                                         const asgart_proto_sd *sds, const uint8_t *flags, const float *identity,
                                         const int32_t *chr, const uint64_t *chr_pos, int64_t n_sd,
                                         const uint8_t *name_bytes, const uint64_t *name_offsets, int64_t n_names,
                                         const uint8_t *prefix, uint64_t prefix_len, const uint8_t *suffix,
                                         uint64_t suffix_len, asgart_export **out) {
    if (out) *out = nullptr;
    RC_TRY(check_arguments(format, fam_offsets, n_families, sds, flags, chr, chr_pos, n_sd, name_bytes, name_offsets,
                           n_names, prefix, prefix_len, suffix, suffix_len, out));
    RC_TRY(use_device("asgart_export_records", device));
    return run_tool<ExportWork>(out, [&](ExportWork &w, asgart_export *res) {
        res->device = device;
        return run_export(w, res, format, fam_offsets, (uint32_t)n_families, sds, flags, identity, chr, chr_pos,
                          (uint32_t)n_sd, name_bytes, name_offsets, (size_t)n_names, prefix, prefix_len, suffix, suffix_len);
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
