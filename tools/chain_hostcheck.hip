// chain_hostcheck.hip -- the link of the chaining rule as the segment walk evaluates it (chain_link of
// csrc/chain_dev.hpp, unsigned 64-bit arithmetic split into gaps and overlaps) run on the HOST against the rule as
// include/asgart_hip.h writes it, with the signed dl and dr in 128-bit integers, on random anchors.  A stand-alone program:
// it launches nothing and needs no GPU.  It checks the arithmetic of one link, not the three sweeps of the walk.  Under
// the host's undefined-behaviour sanitizer a signed overflow in chain_link is an error:
//
//   hipcc -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         --offload-arch=gfx950 -o tools/bin/chain_hostcheck tools/chain_hostcheck.hip
//   tools/bin/chain_hostcheck [rounds]
//
// Per round: two anchors of one group with positions from four ranges (near 0, a window of 4 000 bases, the whole of u64,
// the last 2^33 below 2^64 so that position + length just does not wrap), lengths of 1 .. 2^32 - 1 skewed towards the
// short ones, both geometries, and max_gap from 0, small values, the gap itself and its neighbours, and 2^62 - 1.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <random>

#include "../asgart_amd/csrc/chain_dev.hpp"

using namespace asgart;

namespace {

typedef __int128 wide;

// the rule, literally
bool plain_link(const ChainAnchor &j, const ChainAnchor &i, bool reversed, uint64_t max_gap, wide *t) {
    const wide pl_j = j.pl, pr_j = j.pr, el_j = pl_j + j.ll, er_j = pr_j + j.rl;
    const wide pl_i = i.pl, pr_i = i.pr, el_i = pl_i + i.ll, er_i = pr_i + i.rl;
    if (!(pl_i > pl_j && el_i > el_j)) return false;
    wide dr;
    if (reversed) {
        if (!(pr_i < pr_j && er_i < er_j)) return false;
        dr = pr_j - er_i;
    } else {
        if (!(pr_i > pr_j && er_i > er_j)) return false;
        dr = pr_i - er_j;
    }
    const wide dl = pl_i - el_j, zero = 0;
    const wide gl = dl > zero ? dl : zero, gr = dr > zero ? dr : zero;
    if (gl > (wide)max_gap || gr > (wide)max_gap) return false;
    const wide new_l = (wide)i.ll - (dl < zero ? -dl : zero), new_r = (wide)i.rl - (dr < zero ? -dr : zero);
    *t = (new_l < new_r ? new_l : new_r) - (gl > gr ? gl : gr);
    return true;
}

struct Draw {
    std::mt19937_64 rng;
    uint64_t below(uint64_t n) { return n ? rng() % n : 0; }
    uint64_t length() {
        switch (below(4)) {
            case 0: return 1 + below(8);
            case 1: return 1 + below(400);
            case 2: return 1 + below(100000);
            default: return 1 + below(((uint64_t)1 << 32) - 1);
        }
    }
    uint64_t position(uint64_t len, uint64_t base) {
        const uint64_t top = ~(uint64_t)0 - len;  // the largest position that does not wrap
        uint64_t p;
        switch (below(4)) {
            case 0: p = below(16); break;
            case 1: p = base + below(4000); break;
            case 2: p = rng(); break;
            default: p = top - below((uint64_t)1 << 33); break;
        }
        return p > top ? top : p;
    }
};

}  // namespace

int main(int argc, char **argv) {
    const long rounds = argc > 1 ? atol(argv[1]) : 2000000;
    Draw d{std::mt19937_64(12345)};
    long links = 0, overlaps = 0, at_gap = 0, negative = 0;
    for (long r = 0; r < rounds; ++r) {
        const uint64_t base = d.rng() >> (1 + d.below(40));
        ChainAnchor j, i;
        j.ll = d.length(), j.rl = d.length(), i.ll = d.length(), i.rl = d.length();
        j.pl = d.position(j.ll, base), j.pr = d.position(j.rl, base);
        i.pl = d.position(i.ll, base), i.pr = d.position(i.rl, base);
        const bool reversed = d.below(2) != 0;
        uint64_t max_gap;
        const uint64_t gap = i.pl > j.pl + j.ll ? i.pl - (j.pl + j.ll) : 0;
        switch (d.below(6)) {
            case 0: max_gap = 0; break;
            case 1: max_gap = d.below(5000); break;
            case 2: max_gap = gap; break;
            case 3: max_gap = gap ? gap - 1 : 0; break;
            case 4: max_gap = gap + 1; break;
            default: max_gap = ((uint64_t)1 << 62) - 1; break;
        }
        if (max_gap >= ((uint64_t)1 << 62)) max_gap = ((uint64_t)1 << 62) - 1;
        wide want_t = 0;
        int64_t got_t = 0;
        const bool want = plain_link(j, i, reversed, max_gap, &want_t);
        const bool got = chain_link(j.pl, j.pl + j.ll, j.pr, j.pr + j.rl, i, reversed, max_gap, &got_t);
        if (want != got || (want && want_t != (wide)got_t)) {
            fprintf(stderr, "round %ld: j = (%llu, %llu, %llu, %llu), i = (%llu, %llu, %llu, %llu), reversed %d, max_gap %llu: "
                            "link %d / %d, t %lld / %lld\n", r, (unsigned long long)j.pl, (unsigned long long)j.pr,
                    (unsigned long long)j.ll, (unsigned long long)j.rl, (unsigned long long)i.pl, (unsigned long long)i.pr,
                    (unsigned long long)i.ll, (unsigned long long)i.rl, (int)reversed, (unsigned long long)max_gap, (int)want,
                    (int)got, (long long)want_t, (long long)got_t);
            return 1;
        }
        if (want) {
            ++links;
            if (i.pl < j.pl + j.ll) ++overlaps;
            if (gap == max_gap && gap) ++at_gap;
            if (got_t < 0) ++negative;
        }
    }
    printf("%ld rounds: %ld links, %ld with an overlap on the left, %ld with the left gap exactly max_gap, %ld worth less than 0; "
           "chain_link agrees with the rule\n", rounds, links, overlaps, at_gap, negative);
    return links > rounds / 100 && overlaps > 0 && at_gap > 0 && negative > 0 ? 0 : 2;
}
