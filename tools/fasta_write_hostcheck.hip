// fasta_write_hostcheck.hip -- the write stage of asgart_fasta_write (csrc/fasta_write_dev.hpp) run on the HOST, thread by
// thread, against a plain statement of the file, on random inputs.  A stand-alone program: it launches nothing and needs no
// GPU.  Every array -- the strand, the tables, the intervals and each window's image -- is allocated to the byte, so that
// under the host's address sanitizer a read or a store one byte outside is an error:
//
//   hipcc -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         --offload-arch=gfx950 -o tools/bin/fasta_write_hostcheck tools/fasta_write_hostcheck.hip
//   tools/bin/fasta_write_hostcheck [rounds]
//
// Per round: random records (empty ones among them, gaps between them in the strand), random headers (empty, one byte,
// longer than two windows), random intervals (touching ones, one-base ones, one over everything), a width from the seams
// (0, 1, the store's 15 and 16, window - 1, window, and random ones), both fill modes; small windows (32 .. 256 bytes, so
// that a round has many) and the shipped 16384 with thread counts 1, 7, 64 and 256.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <vector>

#include "../asgart_amd/csrc/fasta_write_dev.hpp"

using namespace asgart;

namespace {

template <class T>
std::unique_ptr<T[]> exact(const std::vector<T> &v) {   // a copy with no byte behind it
    std::unique_ptr<T[]> p(new T[v.size()]);
    if (!v.empty()) memcpy(p.get(), v.data(), v.size() * sizeof(T));
    return p;
}

// the plain statement: one loop per record, one per base
std::vector<uint8_t> expected_file(const std::vector<uint8_t> &src, const std::vector<uint64_t> &rs,
                                   const std::vector<uint64_t> &rl, const std::vector<uint8_t> &headers,
                                   const std::vector<uint64_t> &hoff, const std::vector<uint64_t> &iv, uint32_t width,
                                   uint32_t fill) {
    std::vector<uint8_t> masked(src.size(), 0);
    for (size_t i = 0; i + 1 < iv.size(); i += 2)
        for (uint64_t x = iv[i]; x < iv[i + 1]; ++x) masked[x] = 1;
    std::vector<uint8_t> out;
    for (size_t r = 0; r < rs.size(); ++r) {
        out.insert(out.end(), headers.begin() + hoff[r], headers.begin() + hoff[r + 1]);
        out.push_back('\n');
        for (uint64_t b = 0; b < rl[r]; ++b) {
            uint8_t c = src[rs[r] + b];
            if (masked[rs[r] + b]) c = fill ? (uint8_t)fill : (c >= 'A' && c <= 'Z' ? (uint8_t)(c | 0x20) : c);
            out.push_back(c);
            if (b + 1 == rl[r] || (width && (b + 1) % width == 0)) out.push_back('\n');
        }
    }
    return out;
}

int fail(const char *what, uint64_t round, uint64_t at) {
    fprintf(stderr, "FAIL round %llu: %s at %llu\n", (unsigned long long)round, what, (unsigned long long)at);
    return 1;
}

}  // namespace

int main(int argc, char **argv) {
    const uint64_t rounds = argc > 1 ? strtoull(argv[1], nullptr, 10) : 300;
    std::mt19937_64 rng(20240611);
    auto below = [&](uint64_t n) { return n ? rng() % n : 0; };
    const char alphabet[] = "ACGTNacgtnRYKMryW*-0123>";
    uint64_t windows_run = 0, bytes_run = 0;
    for (uint64_t round = 0; round < rounds; ++round) {
        const uint32_t window = round % 4 == 3 ? 16384 : (uint32_t)(32 + 16 * below(15));
        const uint32_t thread_choices[] = {1, 7, 64, 256};
        const uint32_t n_threads = thread_choices[below(4)];
        const uint32_t width_choices[] = {0, 1, 15, 16, window - 1, window, 60, (uint32_t)(1 + below(3 * window)), 3, ~0u};
        const uint32_t width = width_choices[below(10)];
        const uint32_t fill = below(2) ? 0 : (below(2) ? 'N' : 'x');
        // records, with gaps between them in the strand
        const size_t n_rec = 1 + below(round % 5 == 0 ? 400 : 12);
        std::vector<uint64_t> rs, rl, hoff{0};
        std::vector<uint8_t> headers;
        uint64_t at = below(3);
        for (size_t r = 0; r < n_rec; ++r) {
            const uint64_t kind = below(8);
            const uint64_t len = n_rec > 12 ? below(3) : kind == 0 ? 0 : kind == 1 ? 1 : kind == 2 && width && width < 70000
                                 ? (uint64_t)width - 1 + below(3) : below(5 * window);
            rs.push_back(at);
            rl.push_back(len);
            at += len + (below(4) == 0 ? below(5) : 0);
            const uint64_t hk = below(10);
            const uint64_t hlen = hk == 0 ? 0 : hk == 1 ? 1 : hk == 2 ? 2 * window + below(window) : 1 + below(40);
            for (uint64_t k = 0; k < hlen; ++k) headers.push_back(k ? (uint8_t)(' ' + below(90)) : '>');
            hoff.push_back(headers.size());
        }
        std::vector<uint8_t> src(at);
        for (uint8_t &c : src) c = (uint8_t)alphabet[below(sizeof(alphabet) - 1)];
        // intervals
        std::vector<uint64_t> iv;
        const uint64_t style = below(5);
        if (style == 1 && at) {
            iv = {0, at};
        } else if (style == 2) {
            for (uint64_t x = below(2); x + 1 <= at; x += 2) { iv.push_back(x); iv.push_back(x + 1); }
        } else if (style >= 3) {
            uint64_t x = below(20);
            while (x < at) {
                const uint64_t e = std::min<uint64_t>(at, x + 1 + below(below(2) ? 8 : 2 * window));
                iv.push_back(x);
                iv.push_back(e);
                x = e + (below(3) == 0 ? 0 : below(3 * window));
            }
        }
        const std::vector<uint8_t> want = expected_file(src, rs, rl, headers, hoff, iv, width, fill);
        // where the records start, as the entry point computes it
        std::vector<uint64_t> rec_off{0};
        for (size_t r = 0; r < n_rec; ++r)
            rec_off.push_back(rec_off.back() + (hoff[r + 1] - hoff[r]) + 1 + fasta_body_bytes(rl[r], width));
        if (rec_off.back() != want.size()) return fail("the size of the file", round, rec_off.back());
        auto d_src = exact(src), d_headers = exact(headers);
        auto d_rs = exact(rs), d_rl = exact(rl), d_off = exact(rec_off), d_hoff = exact(hoff), d_iv = exact(iv);
        FastaIn in{};
        in.src = d_src.get();
        in.rec_start = d_rs.get();
        in.rec_len = d_rl.get();
        in.rec_off = d_off.get();
        in.headers = d_headers.get();
        in.hdr_off = d_hoff.get();
        in.iv = d_iv.get();
        in.n_iv = iv.size() / 2;
        in.n_rec = (uint32_t)n_rec;
        in.width = width;
        in.fill = fill;
        const uint64_t size = want.size();
        for (uint64_t g0 = 0; g0 < size; g0 += window) {
            const uint64_t g1 = std::min<uint64_t>(g0 + window, size);
            std::unique_ptr<uint8_t[]> img(new uint8_t[g1 - g0]);
            memset(img.get(), 0xEE, g1 - g0);
            const FastaWindow w = fasta_window_find(in, g0, g1);
            for (uint32_t t = 0; t < n_threads; ++t) fasta_window_compose(in, w, g0, g1, t, n_threads, img.get());
            for (uint64_t b = g0; b < g1; ++b)
                if (img[b - g0] != want[b]) {
                    fprintf(stderr, "window %u, %u threads, width %u, fill %u, %zu records, %zu intervals: got %u, want %u\n",
                            window, n_threads, width, fill, n_rec, iv.size() / 2, (unsigned)img[b - g0], (unsigned)want[b]);
                    return fail("a byte of the file", round, b);
                }
            ++windows_run;
            bytes_run += g1 - g0;
        }
    }
    printf("ok: %llu rounds, %llu windows, %llu bytes of file, every byte as the plain statement has it\n",
           (unsigned long long)rounds, (unsigned long long)windows_run, (unsigned long long)bytes_run);
    return 0;
}
