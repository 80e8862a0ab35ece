// prep.hpp -- what the two ways into prepare_data share (prep.hip: records in memory; fasta.hip: the bytes of FASTA
// files): the alphabet normalisation of one byte, and everything behind the upload -- the long N-runs of the
// normalised strand, the chunks they cut every record into, the index over the finished text.
#pragma once

#include "common.hpp"

namespace asgart {

constexpr uint64_t kNRunThreshold = 5000;  // reference src/bin/asgart.rs:326
constexpr int64_t kMaxRecords = 1 << 24;   // records of one prepare_data call

// (:291-301) c -> upper case unless skip_masked; then anything outside ATGCN -> N
__device__ inline uint32_t norm_byte(uint32_t c, bool skip_masked) {
    if (!skip_masked && c >= 'a' && c <= 'z') c -= 32u;
    const bool ok = c == 'A' || c == 'T' || c == 'G' || c == 'C' || c == 'N';
    return ok ? c : (uint32_t)'N';
}

// The runs of more than 5000 N of the NORMALISED strand d_text[0 .. n_bases), none across a record boundary
// (d_off: n_records + 1 record offsets on the device) -> runs: (start, end) pairs, unordered.  `who` names the entry
// point in error messages.  Synchronises s.
int32_t find_long_n_runs(const char *who, const uint8_t *d_text, uint64_t n_bases, const uint64_t *d_off,
                         int64_t n_records, hipStream_t s, std::vector<uint64_t> &runs);
// find_chunks_to_process per record (src/bin/asgart.rs:317-366) in record order (:375-395): (start, len) pairs in
// global coordinates.  off: n_records + 1 record offsets on the host; runs: what find_long_n_runs found.
void chunks_from_runs(const uint64_t *off, int64_t n_records, const std::vector<uint64_t> &runs,
                      std::vector<uint64_t> &chunks);
// '$' (:430) and the 64 zero bytes an index wants behind d_text[0 .. n_bases)
int32_t finish_text(uint8_t *d_text, uint64_t n_bases, hipStream_t s);
// an index over the finished text of n = n_bases + 1 bytes (copied), its suffixes sorted on the GPU
int32_t index_over_text(const uint8_t *d_text, uint64_t n, int32_t device, asgart_index **out);

// extract.hip: a source (asgart_source) over n bytes that are on the device already; takes `text` over on success
int32_t source_adopt(DevBuf &text, uint64_t n, int32_t device, asgart_source **out);
// extract.hip: the device of a source, its n bytes and where they lie (read, not taken over)
void source_view(const asgart_source *src, int32_t *device, uint64_t *n, const uint8_t **text);

}  // namespace asgart
