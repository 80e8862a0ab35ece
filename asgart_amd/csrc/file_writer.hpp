// file_writer.hpp -- what the file writers (export.hip, paf.hip, sdtable.hip, variants_write.hip) are built on, on top of tool_base.hpp: the handle
// of a written file, the result arrays as they arrive at the C boundary and their checks, the device work of a writer call
// (FileWork: the common buffers, their upload, their view for the kernels, the five events of a call and its two figures),
// the way of an LDS image out to the file, the write stage of a writer whose workgroups own consecutive items, and the
// sizing and framing of the file.  What a row consists of, the length stage and the geometry are each writer's own.
#pragma once

#include "tool_base.hpp"

// The handle of a file written on the device (asgart_export_records, asgart_paf_records, asgart_paf_records_cs,
// asgart_sdtable_records, asgart_fasta_write); asgart_export_size, _copy, _timings and _free (export.hip) work on it whichever call made it.
struct asgart_export {
    int32_t device = 0;
    asgart::DevBuf file;  // the whole file, on the device
    uint64_t size = 0;
    double ms[3] = {0, 0, 0};
    ~asgart_export() {
        if (file.p && hipSetDevice(device) == hipSuccess) file.release();
    }
};

namespace asgart {

// The result arrays as a writer's entry point receives them; filled once there, read by the checks and the upload.
struct ResultArg {
    const uint64_t *fam_offsets;
    int64_t n_families;
    const asgart_proto_sd *sds;
    const uint8_t *flags;
    const int32_t *chr;
    const uint64_t *chr_pos;
    int64_t n_sd;
    const uint8_t *name_bytes;
    const uint64_t *name_offsets;
    int64_t n_names;

    // a null pointer or a negative count: part of the caller's "bad argument", which it tests before its own caps so that
    // nothing is read behind a count the caps refuse
    bool missing() const {
        return !fam_offsets || n_families < 0 || n_sd < 0 || n_names < 0 || !name_offsets ||
               (n_sd && (!sds || !flags || !chr || !chr_pos));
    }
};

// what every writer checks in the arrays themselves (behind missing() and the writer's caps): the family offsets, the name
// table, the name ids
inline int32_t check_result_arg(const char *who, const ResultArg &a) {
    RC_TRY(check_csr(who, "fam_offsets", a.fam_offsets, a.n_families, a.n_sd, "n_sd"));
    RC_TRY(check_name_table(who, a.name_bytes, a.name_offsets, a.n_names));
    return check_name_ids(who, a.chr, a.n_sd, a.n_names);
}

// The result arrays on the device, as the emit functions read them (ExportIn, SdTableIn and PafIn derive from it).
struct ResultView {
    const uint64_t *offs;      // [n_fam + 1]
    const uint64_t *sds;       // [n][4]: global left, global right, left_length, right_length
    const uint8_t *flags;      // [n]
    const int32_t *chr;        // [n][2] name ids
    const uint64_t *chr_pos;   // [n][2]
    const uint8_t *names;      // the name table: the bytes of all names, as the file prints them
    const uint64_t *name_off;  // [n_names + 1]
    uint32_t n_fam;
};

// The device work of a writer call.  A writer derives from it and names only its own buffers.
struct FileWork : ToolWork {
    DevBuf &offs = buf(), &sds = buf(), &flags = buf(), &chr = buf(), &chr_pos = buf(), &names = buf(), &name_off = buf();
    uint32_t n_fam = 0;

    using ToolWork::upload;
    int32_t upload(const ResultArg &a) {
        const size_t n = (size_t)a.n_sd;
        n_fam = (uint32_t)a.n_families;
        RC_TRY(upload(offs, a.fam_offsets, ((size_t)a.n_families + 1) * 8));
        RC_TRY(upload(sds, a.sds, n * sizeof(asgart_proto_sd)));
        RC_TRY(upload(flags, a.flags, n));
        RC_TRY(upload(chr, a.chr, n * 8));
        RC_TRY(upload(chr_pos, a.chr_pos, n * 16));
        RC_TRY(upload(names, a.name_bytes, (size_t)a.name_offsets[a.n_names]));
        return upload(name_off, a.name_offsets, ((size_t)a.n_names + 1) * 8);
    }
    ResultView view() const {
        return ResultView{offs.as<uint64_t>(), sds.as<uint64_t>(), flags.as<uint8_t>(), chr.as<int32_t>(),
                          chr_pos.as<uint64_t>(), names.as<uint8_t>(), name_off.as<uint64_t>(), n_fam};
    }

    // The five events of a call: its start, the arrays are up, every byte has its place (the last scan), the file is
    // there (sized and reserved), the file is written.
    enum Stamp { kStart, kUploaded, kPlaced, kSized, kWritten };
    int32_t open_call() {
        RC_TRY(open(5));
        return stamp(kStart);
    }
    int32_t stamp(Stamp k) {
        HIP_TRY(hipEventRecord(ev[k], s));
        return 0;
    }
    // Behind stamp(kWritten): the call's figures, ms[0] the upload, ms[1] the kernels -- up to the place of every byte and
    // from the sized file on; the read back of the size and the reservation between them are neither.
    int32_t finish(asgart_export *res) {
        HIP_TRY(stream_sync(s));
        float up = 0, a = 0, b = 0;
        HIP_TRY(hipEventElapsedTime(&up, ev[kStart], ev[kUploaded]));
        HIP_TRY(hipEventElapsedTime(&a, ev[kUploaded], ev[kPlaced]));
        HIP_TRY(hipEventElapsedTime(&b, ev[kSized], ev[kWritten]));
        res->ms[0] = up;
        res->ms[1] = (double)a + (double)b;
        return 0;
    }

    // The file of a writer whose body lies between a prefix and a suffix from the host (either may be empty): the body's
    // size is read back from *body_size (the closing entry of the scan), the file is sized and reserved, stamp(kSized), and
    // the copies of prefix and suffix are queued.  The body starts at file + prefix_len.
    int32_t frame_file(asgart_export *res, const uint64_t *body_size, const uint8_t *prefix, uint64_t prefix_len,
                       const uint8_t *suffix, uint64_t suffix_len) {
        uint64_t body = 0;
        HIP_TRY(read_back(&body, body_size, 8, s));
        res->size = prefix_len + body + suffix_len;
        RC_TRY(res->file.reserve(std::max<size_t>(res->size, 16)));
        uint8_t *file = res->file.as<uint8_t>();
        RC_TRY(stamp(kSized));
        if (prefix_len) HIP_TRY(hipMemcpyAsync(file, prefix, prefix_len, hipMemcpyHostToDevice, s));
        if (suffix_len) HIP_TRY(hipMemcpyAsync(file + prefix_len + body, suffix, suffix_len, hipMemcpyHostToDevice, s));
        return 0;
    }
};

// The image `stage` of the file's bytes [g0, g1) goes out: stage[0] is the file's byte a0, a0 <= g0 on a line of the file
// (a multiple of kLine = 16), so a 16-byte line of the file is a 16-byte line of the image and all kThreads threads of the
// workgroup move it with one aligned 16-byte store per lane, a wave 1 KiB of consecutive bytes.  Only the lines the range
// shares with its neighbours (its head and its tail, fewer than 16 bytes each) go out byte by byte: this range's bytes only.
// Behind the barrier that completes the image.
template <uint32_t kThreads, uint32_t kLine>
__device__ __forceinline__ void copy_out_image(const uint8_t *stage, uint64_t a0, uint64_t g0, uint64_t g1,
                                               uint8_t *__restrict__ out) {
    static_assert(kLine == sizeof(uint4), "a line is one 16-byte store");
    const uint32_t lines = (uint32_t)((g1 - a0 + kLine - 1) / kLine);
    for (uint32_t l = threadIdx.x; l < lines; l += kThreads) {
        const uint64_t a = a0 + (uint64_t)l * kLine;
        if (a >= g0 && a + kLine <= g1) {
            *reinterpret_cast<uint4 *>(out + a) = *reinterpret_cast<const uint4 *>(stage + l * kLine);
        } else {
            const uint64_t lo = max(a, g0), hi = min(a + kLine, g1);
            for (uint64_t b = lo; b < hi; ++b) out[b] = stage[b - a0];
        }
    }
}

// The write stage of a writer whose items (units, rows) each have a place from a scan: offsets[i] behind body_at, and
// offsets[n_items] the end.  A workgroup of 2 * kItems threads owns kItems consecutive items, so one contiguous byte range
// of the file.  Two threads share an item: each calls row(dst, item, half) with dst where the item starts, in the LDS image
// of the range (kStage bytes, starting on a line of the file) or, when the range does not fit the image (a name of any
// length is legal), in the file itself: slower, never refused.  Then the image goes out (copy_out_image).
// kRowPerSpace: row is compiled twice, once storing to LDS and once to global memory (export.hip's choice), or once, storing
// through a generic pointer (sdtable.hip's); each writer keeps the kernel it had.  A caller marks its lambda always_inline:
// left to the inliner's own order the same statements come out with other registers.
template <uint32_t kItems, uint32_t kStage, uint32_t kLine, bool kRowPerSpace, class Row>
__device__ __forceinline__ void write_owned_range(uint8_t *stage, const uint64_t *__restrict__ offsets, uint64_t body_at,
                                                  uint32_t n_items, uint8_t *__restrict__ out, Row row) {
    const uint32_t first = blockIdx.x * kItems;
    const uint32_t last = min(first + kItems, n_items);
    const uint64_t g0 = body_at + offsets[first], g1 = body_at + offsets[last];   // the workgroup's bytes of the file
    const uint64_t a0 = g0 & ~(uint64_t)(kLine - 1);                              // the image starts on a line of the file
    const bool staged = g1 - a0 <= kStage;
    const uint32_t i = first + (threadIdx.x >> 1), half = threadIdx.x & 1;
    if (i < last) {
        const uint64_t at = body_at + offsets[i];
        if (!kRowPerSpace)
            row(staged ? stage + (at - a0) : out + at, i, half);
        else if (staged)
            row(stage + (at - a0), i, half);
        else
            row(out + at, i, half);
    }
    if (!staged) return;   // (the same in every thread of the workgroup)
    __syncthreads();
    copy_out_image<2 * kItems, kLine>(stage, a0, g0, g1, out);
}

}  // namespace asgart
