// tool_base_hostcheck.hip -- the host-callable pieces that the arm tools (rosary.hip, groups.hip, chain.hip, mask.hip) share
// through csrc/tool_base.hpp, run on the HOST against plain restatements.  A stand-alone program: it launches nothing and
// needs no GPU.  Every array is allocated to the byte, so under the host's address sanitizer a read one entry past a column
// is an error, and under the undefined-behaviour sanitizer so is a shift by the width of the type:
//
//   hipcc -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         --offload-arch=gfx950 -o tools/bin/tool_base_hostcheck tools/tool_base_hostcheck.hip
//   tools/bin/tool_base_hostcheck
//
//   first_at_least  against a linear scan, on random never-decreasing columns of 0 .. 1 000 entries with repeated and absent
//                   keys, in both element types the tools bisect (uint32_t, int32_t), for every k in 0 .. max + 2
//   bits_for        against a loop over powers of two in 128 bits, at 0, 1, 2, 3 and around 2^31 and 2^32
//   ChainGroupKey   (csrc/chain_dev.hpp) at name_bits 1 and 31 and the flag values 0 .. 3: the keys of any two duplications
//                   compare as their (cl, cr, fl) do, and no key has a bit at or above 2 * name_bits + 2
#include <hip/hip_runtime.h>

#include <cstdio>
#include <memory>
#include <random>
#include <tuple>

#include "../asgart_amd/csrc/chain_dev.hpp"
#include "../asgart_amd/csrc/tool_base.hpp"

using namespace asgart;

namespace {

template <class Key>
long check_first_at_least(std::mt19937_64 &rng, int columns) {
    long asked = 0;
    for (int c = 0; c < columns; ++c) {
        const uint32_t n = c < 4 ? (uint32_t)c : (uint32_t)(rng() % 1001);
        const uint32_t step = 1 + (uint32_t)(rng() % 4);  // (steps of 0: repeated keys; of 2 and more: absent ones)
        std::unique_ptr<Key[]> keys(new Key[n]);
        uint64_t key = rng() % 3;
        for (uint32_t i = 0; i < n; ++i) {
            key += rng() % step;
            keys[i] = (Key)key;
        }
        for (uint64_t k = 0; k <= key + 2; ++k, ++asked) {
            uint32_t want = 0;
            while (want < n && (uint64_t)keys[want] < k) ++want;
            const uint32_t got = first_at_least(keys.get(), n, k);
            if (got != want) {
                fprintf(stderr, "first_at_least: column %d of %u entries, k = %llu: %u, the scan says %u\n", c, n,
                        (unsigned long long)k, got, want);
                return -1;
            }
        }
    }
    return asked;
}

bool check_bits_for() {
    const uint64_t two31 = (uint64_t)1 << 31, two32 = (uint64_t)1 << 32;
    for (uint64_t v : {(uint64_t)0, (uint64_t)1, (uint64_t)2, (uint64_t)3, two31 - 1, two31, two31 + 1, two32, two32 + 1}) {
        unsigned want = 0;
        for (unsigned __int128 p = 1; p < v; p *= 2) ++want;   // ceil(log2(v))
        want = want < 1 ? 1 : want > 32 ? 32 : want;           // a sort has a bit, and the keys are 32-bit words
        if (bits_for(v) != want) {
            fprintf(stderr, "bits_for(%llu) = %u, the loop says %u\n", (unsigned long long)v, bits_for(v), want);
            return false;
        }
    }
    return true;
}

long check_group_key(std::mt19937_64 &rng, unsigned name_bits) {
    const uint64_t n_ids = (uint64_t)1 << name_bits;
    std::vector<int32_t> ids;
    for (uint64_t id : {(uint64_t)0, (uint64_t)1, n_ids / 2 - 1, n_ids / 2, n_ids - 2, n_ids - 1})
        if (id < n_ids) ids.push_back((int32_t)id);
    for (int r = 0; name_bits > 1 && r < 6; ++r) ids.push_back((int32_t)(rng() % n_ids));
    const size_t n = ids.size() * ids.size() * 4;  // every (cl, cr, fl)
    std::unique_ptr<int32_t[]> chr(new int32_t[2 * n]);
    std::unique_ptr<uint8_t[]> flags(new uint8_t[n]);
    size_t q = 0;
    for (int32_t cl : ids)
        for (int32_t cr : ids)
            for (uint8_t fl = 0; fl < 4; ++fl, ++q) chr[2 * q] = cl, chr[2 * q + 1] = cr, flags[q] = fl;
    const ChainGroupKey key_of{chr.get(), flags.get(), name_bits};
    const unsigned width = 2 * name_bits + 2;
    long pairs = 0;
    for (size_t a = 0; a < n; ++a) {
        const uint64_t ka = key_of((uint32_t)a);
        if (width < 64 && (ka >> width) != 0) {
            fprintf(stderr, "ChainGroupKey: name_bits %u, (%d, %d, %u): the key %llx has a bit above %u\n", name_bits,
                    chr[2 * a], chr[2 * a + 1], (unsigned)flags[a], (unsigned long long)ka, width);
            return -1;
        }
        for (size_t b = 0; b < n; ++b, ++pairs) {
            const auto ta = std::make_tuple(chr[2 * a], chr[2 * a + 1], flags[a]);
            const auto tb = std::make_tuple(chr[2 * b], chr[2 * b + 1], flags[b]);
            const uint64_t kb = key_of((uint32_t)b);
            if ((ta < tb) != (ka < kb) || (ta == tb) != (ka == kb)) {
                fprintf(stderr, "ChainGroupKey: name_bits %u: (%d, %d, %u) and (%d, %d, %u) have the keys %llx and %llx\n",
                        name_bits, chr[2 * a], chr[2 * a + 1], (unsigned)flags[a], chr[2 * b], chr[2 * b + 1],
                        (unsigned)flags[b], (unsigned long long)ka, (unsigned long long)kb);
                return -1;
            }
        }
    }
    return pairs;
}

}  // namespace

int main() {
    std::mt19937_64 rng(2024);
    const long asked_u = check_first_at_least<uint32_t>(rng, 300), asked_i = check_first_at_least<int32_t>(rng, 300);
    if (asked_u < 0 || asked_i < 0 || !check_bits_for()) return 1;
    const long pairs_1 = check_group_key(rng, 1), pairs_31 = check_group_key(rng, 31);
    if (pairs_1 < 0 || pairs_31 < 0) return 1;
    printf("first_at_least agrees with a linear scan on %ld (uint32_t) and %ld (int32_t) questions; bits_for agrees at 9 values; "
           "ChainGroupKey orders %ld pairs of triples at name_bits 1 and %ld at name_bits 31 as the triples order\n",
           asked_u, asked_i, pairs_1, pairs_31);
    return 0;
}
