// fasta_write.hip -- FASTA files written on the GPU: asgart_fasta_write, the counterpart of mask.fasta_text_host for a
// caller of the C ABI.  The strand is on the device already (an asgart_source: the raw bytes of the records), the output is
// as large as the genome, and per output byte the work is one load, one test and one store.
//
// What the file consists of is stated once, in fasta_write_dev.hpp.  A record is not of bounded size, so nothing here works
// record by record:
//   place     the host's 64-bit sum of the record sizes (header, `\n`, body): at most 2^24 records, a loop over the table it
//             has just checked; the offsets go up with the tables
//   write     a workgroup owns kWindow consecutive BYTES of the file -- not records, not lines -- so that its range starts
//             on a 16-byte line of the file whatever the records hold.  One thread finds the records of the window's first
//             and last byte by bisection of the record offsets and the intervals that can reach a base of it by bisection
//             of the interval list (fasta_window_find); all threads compose the window in an LDS image of it, byte t of
//             the window by thread t mod kThreads (fasta_window_compose); then all threads move the image out with
//             file_writer.hpp's copy_out_image, one aligned 16-byte store per lane.  A header longer than the image is
//             composed by the workgroups it spans, each its own part; there is no second path.
// kWindow = 16384 and kThreads = 256 are paf.hip's: 64 bytes of the file per thread, nine images in a CU's 160 KiB.  Design
// constants, reasoned and not measured: no sweep was run.
#include "file_writer.hpp"
#include "prep.hpp"
#include "fasta_write_dev.hpp"

namespace asgart {
namespace {

constexpr uint32_t kThreads = 256;   // per workgroup of the write stage
constexpr uint32_t kWindow = 16384;  // bytes of the file per workgroup, and of its LDS image
constexpr uint32_t kLine = 16;       // bytes per store of the copy out
constexpr int64_t kMaxIntervals = (int64_t)1 << 32;

__global__ __launch_bounds__(kThreads) void fasta_write_kernel(FastaIn in, uint64_t size, uint8_t *__restrict__ out) {
    __shared__ __align__(16) uint8_t stage[kWindow];
    __shared__ FastaWindow window;
    const uint64_t g0 = (uint64_t)blockIdx.x * kWindow;
    if (g0 >= size) return;   // (the same in every thread of the workgroup)
    const uint64_t g1 = min(g0 + kWindow, size);
    if (threadIdx.x == 0) window = fasta_window_find(in, g0, g1);
    __syncthreads();
    fasta_window_compose(in, window, g0, g1, threadIdx.x, kThreads, stage);
    __syncthreads();
    copy_out_image<kThreads, kLine>(stage, g0, g0, g1, out);
}

struct FastaWriteWork : FileWork {
    DevBuf &rec_start = buf(), &rec_len = buf(), &rec_off = buf(), &headers = buf(), &hdr_off = buf(), &iv = buf();
};

const char kWho[] = "asgart_fasta_write";

// Every argument check of the call, before the device is looked at; rec_off: where every record starts in the file.
int32_t check_arguments(const asgart_source *src, uint64_t n_src, const uint64_t *record_start, const uint64_t *record_len,
                        int64_t n_records, const uint8_t *header_bytes, const uint64_t *header_offsets,
                        const uint64_t *intervals, int64_t n_intervals, uint32_t width, uint32_t fill, asgart_export **out,
                        std::vector<uint64_t> &rec_off) {
    if (!out || !src || n_records < 0 || n_intervals < 0 || (n_records && (!record_start || !record_len || !header_offsets)) ||
        (n_intervals && !intervals)) {
        set_error("%s: bad argument (a NULL pointer or a negative count)", kWho);
        return ASGART_E_ARG;
    }
    if (fill > 255 || fill == '\n' || fill == '\r' || fill == '>') {
        set_error("%s: fill byte %u: a masked base is no line end, no `>` and one byte (0: lower case)", kWho, fill);
        return ASGART_E_ARG;
    }
    if (n_records > kMaxRecords) {
        set_error("%s: more than 2^24 records are not supported", kWho);
        return ASGART_E_CAP;
    }
    if (n_intervals > kMaxIntervals) {
        set_error("%s: more than 2^32 intervals are not supported", kWho);
        return ASGART_E_CAP;
    }
    if (n_records && (header_offsets[0] != 0 || (header_offsets[n_records] && !header_bytes))) {
        set_error("%s: header_offsets must start at 0, and header_bytes hold what they end at", kWho);
        return ASGART_E_ARG;
    }
    rec_off.assign((size_t)n_records + 1, 0);
    for (int64_t r = 0; r < n_records; ++r) {
        if (header_offsets[r] > header_offsets[r + 1]) {
            set_error("%s: header_offsets decrease at record %lld", kWho, (long long)r);
            return ASGART_E_ARG;
        }
        const size_t h_len = (size_t)(header_offsets[r + 1] - header_offsets[r]);
        if (h_len && memchr(header_bytes + header_offsets[r], '\n', h_len)) {
            set_error("%s: the header of record %lld holds a line end: it would start a line of its own", kWho, (long long)r);
            return ASGART_E_ARG;
        }
        const uint64_t end = record_start[r] + record_len[r];
        if (end < record_start[r] || end > n_src || (r + 1 < n_records && end > record_start[r + 1])) {
            set_error("%s: record %lld (start %llu, length %llu) reaches past the source's %llu bytes or into the next "
                      "record: the records must be ascending and must not overlap", kWho, (long long)r,
                      (unsigned long long)record_start[r], (unsigned long long)record_len[r], (unsigned long long)n_src);
            return ASGART_E_ARG;
        }
        const uint64_t bytes = header_offsets[r + 1] - header_offsets[r] + 1 + fasta_body_bytes(record_len[r], width);
        rec_off[r + 1] = rec_off[r] + bytes;
        if (rec_off[r + 1] < rec_off[r]) {
            set_error("%s: the file wraps past 2^64 bytes at record %lld", kWho, (long long)r);
            return ASGART_E_ARG;
        }
    }
    for (int64_t i = 0; i < n_intervals; ++i) {
        const uint64_t a = intervals[2 * i], b = intervals[2 * i + 1];
        if (a >= b || b > n_src || (i && intervals[2 * i - 1] > a)) {
            set_error("%s: interval %lld [%llu, %llu) is empty, reaches past the source's %llu bytes or starts in front of "
                      "the end of the one before it: the intervals must be ascending and disjoint", kWho, (long long)i,
                      (unsigned long long)a, (unsigned long long)b, (unsigned long long)n_src);
            return ASGART_E_ARG;
        }
    }
    return 0;
}

int32_t run_fasta_write(FastaWriteWork &w, asgart_export *res, const uint8_t *d_src, const uint64_t *record_start,
                        const uint64_t *record_len, size_t n_records, const uint8_t *header_bytes,
                        const uint64_t *header_offsets, const uint64_t *intervals, size_t n_intervals, uint32_t width,
                        uint32_t fill, const std::vector<uint64_t> &rec_off) {
    if (n_records == 0) return 0;   // an empty file: nothing to launch
    RC_TRY(w.open_call());
    hipStream_t s = w.s;
    RC_TRY(w.upload(w.rec_start, record_start, n_records * 8));
    RC_TRY(w.upload(w.rec_len, record_len, n_records * 8));
    RC_TRY(w.upload(w.rec_off, rec_off.data(), (n_records + 1) * 8));
    RC_TRY(w.upload(w.headers, header_bytes, (size_t)header_offsets[n_records]));
    RC_TRY(w.upload(w.hdr_off, header_offsets, (n_records + 1) * 8));
    RC_TRY(w.upload(w.iv, intervals, n_intervals * 16));
    RC_TRY(w.stamp(w.kUploaded));
    RC_TRY(w.stamp(w.kPlaced));   // (the host has placed the records)
    res->size = rec_off[n_records];
    RC_TRY(res->file.reserve(std::max<size_t>(res->size, 16)));
    RC_TRY(w.stamp(w.kSized));
    FastaIn in{};
    in.src = d_src;
    in.rec_start = w.rec_start.as<uint64_t>();
    in.rec_len = w.rec_len.as<uint64_t>();
    in.rec_off = w.rec_off.as<uint64_t>();
    in.headers = w.headers.as<uint8_t>();
    in.hdr_off = w.hdr_off.as<uint64_t>();
    in.iv = w.iv.as<uint64_t>();
    in.n_iv = n_intervals;
    in.n_rec = (uint32_t)n_records;
    in.width = width;
    in.fill = fill;
    const uint64_t windows = (res->size + kWindow - 1) / kWindow;
    if (windows >= (uint64_t)1 << 31) {
        set_error("%s: a file of %llu bytes has more windows than one launch takes", kWho, (unsigned long long)res->size);
        return ASGART_E_CAP;
    }
    fasta_write_kernel<<<(unsigned)windows, kThreads, 0, s>>>(in, res->size, res->file.as<uint8_t>());
    HIP_TRY(hipGetLastError());
    RC_TRY(w.stamp(w.kWritten));
    return w.finish(res);
}

}  // namespace
}  // namespace asgart

using namespace asgart;

extern "C" int32_t asgart_fasta_write(asgart_source *src, const uint64_t *record_start, const uint64_t *record_len,
                                      int64_t n_records, const uint8_t *header_bytes, const uint64_t *header_offsets,
                                      const uint64_t *intervals, int64_t n_intervals, uint32_t width, uint32_t fill,
                                      asgart_export **out) {
    if (out) *out = nullptr;
    int32_t device = 0;
    uint64_t n_src = 0;
    const uint8_t *d_src = nullptr;
    if (src) source_view(src, &device, &n_src, &d_src);
    std::vector<uint64_t> rec_off;
    RC_TRY(check_arguments(src, n_src, record_start, record_len, n_records, header_bytes, header_offsets, intervals,
                           n_intervals, width, fill, out, rec_off));
    RC_TRY(use_device(kWho, device));
    return run_tool<FastaWriteWork>(out, [&](FastaWriteWork &w, asgart_export *res) {
        res->device = device;
        return run_fasta_write(w, res, d_src, record_start, record_len, (size_t)n_records, header_bytes, header_offsets,
                               intervals, (size_t)n_intervals, width, fill, rec_off);
    });
}

extern "C" void asgart_fasta_write_geometry(uint64_t *block_threads, uint64_t *window_bytes, uint64_t *store_bytes) {
    if (block_threads) *block_threads = kThreads;
    if (window_bytes) *window_bytes = kWindow;
    if (store_bytes) *store_bytes = kLine;
}
