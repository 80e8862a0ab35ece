// variants.hip -- the differences between the two arms of every duplication as positions in the genome, taken on the GPU
// from the runs of an alignment and the text of the index: asgart_alignment_variants (one record per base of an `X` run
// and per `I` or `D` run: the paralogous sequence variants, PSVs) and asgart_variant_sites (the distinct positions that
// the `X` records touch).  The rule is stated once, in include/asgart_hip.h; the pieces are in variants_dev.hpp;
// align.variants_host and align.sites_host are the readable statements.
//
// asgart_alignment_variants, over runs and over records, never over the runs or the bases of a row:
//   runs      one thread per run: its duplication by bisection of the run offsets; for a duplication with status 1 the two
//             checks of a run (paf_dev.hpp's codes, ONE atomic minimum names the lowest offending duplication) and what
//             the run adds to three sums: bases of the left arm, bases of the right arm, records;
//   scan      ONE exclusive scan of the three sums together (rocPRIM, 64-bit each);
//   rows      one thread per duplication, a constant of work: the runs of a duplication with status 1 must consume exactly
//             its two arms, and var_offsets[q] is the record sum in front of its first run.  The host reads the atomic
//             minimum and the number of records back; a refused call ends here, before a byte of the text is read;
//   records   record k of all finds its run by bisection of the record sums and its duplication by bisection of the run
//             offsets, both inside the few runs and duplications its workgroup's kRecords records span (found once per
//             workgroup).  Neighbouring lanes take neighbouring k: neighbouring bases of an `X` run, neighbouring bytes of
//             the text (descending ones of a reversed right arm).  A record goes out as two 16-byte stores.
// asgart_variant_sites, over records and over entries (an `X` record has up to two: its left and its right position):
//   count     one thread per record: which entries it has (variants_dev.hpp: site_entries); a wave's two ballots give
//             its number of entries;
//   scan      the waves' numbers (rocPRIM): where each wave's entries start;
//   emit      the same ballots again: entry 2k + side of record k goes to its place, so the entries stand in record order,
//             left before right; the key is the position, the value the entry's id;
//   sort      ONE stable radix sort of (position, id) pairs (rocPRIM): entries of one position stay in record order;
//   heads     an entry opens a site where its position differs from the one in front; the scan of the flags numbers the
//             sites;
//   reduce    the lanes of a wave hold consecutive entries, so sites that never decrease: the entries of one site within a
//             wave are summed and ORed through shuffles (alnstats_dev.hpp: row_sum; row_or), and the lane that opens the
//             site's part of the wave adds them: one atomicAdd and one atomicOr per site and wave.  The entry that opens
//             the site itself writes the position, the class of the text's byte there and its own (sd, side).
// Everything is integer: nothing depends on the order the atomics arrive in.
// kRecords = 1024: four records a lane, so that the workgroup's two bisections of the whole arrays are paid once per 1024
// records.  A design constant, reasoned and not measured: no sweep was run.
#include "variants_dev.hpp"

namespace asgart {
namespace {

constexpr uint32_t kThreads = 256;    // per workgroup, every kernel
constexpr uint32_t kRecords = 1024;   // records per workgroup of the records kernel
static_assert(kRecords % kThreads == 0 && kThreads % 64 == 0, "whole waves, the same number of records a lane");

__global__ __launch_bounds__(kThreads) void variants_runs_kernel(VariantsIn in) {
    const uint64_t t = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (t > in.n_runs) return;   // (t == n_runs: the closing entry, the scan ends in the totals)
    uint32_t len = 0;
    uint8_t op = 0;
    if (t < in.n_runs) {
        const uint32_t q = row_of_run(in.run_off, 0, (uint64_t)in.n_sd + 1, t);
        if (in.status[q] == 1) {
            len = in.run_len[t];
            op = in.run_op[t];
            if (!run_op_known(op) || len == 0) {
                atomicMin((unsigned long long *)in.bad,
                          (unsigned long long)((uint64_t)q << 2 | (run_op_known(op) ? kPafBadLen : kPafBadOp)));
                len = 0;
                op = 0;
            }
        }
    }
    in.S[t] = op ? RunSums{run_on_left(op, len), run_on_right(op, len), run_records(op, len)} : RunSums{0, 0, 0};
}

__global__ __launch_bounds__(kThreads) void variants_rows_kernel(VariantsIn in) {
    const uint32_t q = blockIdx.x * kThreads + threadIdx.x;
    if (q > in.n_sd) return;
    const uint64_t b = in.run_off[q];
    in.var_off[q] = in.S[b].v;   // (q == n_sd: the number of records)
    if (q == in.n_sd || in.status[q] != 1) return;
    const uint64_t e = in.run_off[q + 1];
    if (in.S[e].i - in.S[b].i != in.sds[4 * (size_t)q + 2] || in.S[e].j - in.S[b].j != in.sds[4 * (size_t)q + 3])
        atomicMin((unsigned long long *)in.bad, (unsigned long long)((uint64_t)q << 2 | kPafBadSums));
}

__global__ __launch_bounds__(kThreads) void variants_records_kernel(VariantsIn in, uint64_t n_records,
                                                                    asgart_variant *__restrict__ out,
                                                                    unsigned long long *__restrict__ n_snv) {
    // the runs and the duplications of the workgroup's first and last record: every bisection below stays between them
    const uint64_t g0 = (uint64_t)blockIdx.x * kRecords, g1 = min(g0 + kRecords, n_records);
    const uint64_t t_lo = first_records_above(in.S, 0, in.n_runs + 1, g0) - 1;
    const uint64_t t_hi = first_records_above(in.S, t_lo, in.n_runs + 1, g1 - 1);
    const uint64_t q_lo = row_of_run(in.run_off, 0, (uint64_t)in.n_sd + 1, t_lo);
    const uint64_t q_hi = first_above(in.run_off, q_lo, (uint64_t)in.n_sd + 1, t_hi - 1);
    uint32_t snv = 0;   // the wave's `X` records, the same in every lane
#pragma unroll
    for (uint32_t r = 0; r < kRecords / kThreads; ++r) {
        const uint64_t k = g0 + (uint64_t)r * kThreads + threadIdx.x;
        bool is_x = false;
        if (k < g1) {
            const uint64_t t = first_records_above(in.S, t_lo, t_hi, k) - 1;
            const uint32_t q = row_of_run(in.run_off, q_lo, q_hi, t);
            __align__(16) const asgart_variant v = variant_of(in, q, t, k - in.S[t].v);
            is_x = v.op == 'X';
            const uint4 *w = reinterpret_cast<const uint4 *>(&v);
            uint4 *dst = reinterpret_cast<uint4 *>(out + k);
            dst[0] = w[0];
            dst[1] = w[1];
        }
        snv += (uint32_t)__popcll(__ballot(is_x));
    }
    if (__lane_id() == 0 && snv) atomicAdd(n_snv, (unsigned long long)snv);
}

// ---- sites ------------------------------------------------------------------------------------------------------------

// the entries of the records a wave holds: lane l has record k0 + l, its bits from site_entries
struct WaveEntries {
    unsigned long long left, right;
    __device__ uint32_t count() const { return (uint32_t)(__popcll(left) + __popcll(right)); }
    // the entries of the wave in front of the calling lane's own
    __device__ uint32_t before(uint32_t lane) const {
        const unsigned long long below = lane ? ~0ull >> (64 - lane) : 0ull;
        return (uint32_t)(__popcll(left & below) + __popcll(right & below));
    }
};
__device__ inline WaveEntries wave_entries(uint32_t bits) {
    return WaveEntries{__ballot((bits & 1u) != 0), __ballot((bits & 2u) != 0)};
}

__global__ __launch_bounds__(kThreads) void sites_count_kernel(const asgart_variant *__restrict__ recs, uint32_t n_records,
                                                               uint32_t n_waves, uint32_t *__restrict__ wave_count) {
    const uint32_t k = blockIdx.x * kThreads + threadIdx.x, wave = k >> 6;
    const WaveEntries e = wave_entries(k < n_records ? site_entries(recs[k]) : 0u);
    // (wave n_waves, when a lane of the launch has it: the closing entry, the scan ends in the number of entries)
    if (__lane_id() == 0 && wave <= n_waves) wave_count[wave] = wave < n_waves ? e.count() : 0u;
}

__global__ __launch_bounds__(kThreads) void sites_emit_kernel(const asgart_variant *__restrict__ recs, uint32_t n_records,
                                                              const uint32_t *__restrict__ wave_at,
                                                              uint64_t *__restrict__ key, uint32_t *__restrict__ id) {
    const uint32_t k = blockIdx.x * kThreads + threadIdx.x, lane = __lane_id();
    asgart_variant r{};
    uint32_t bits = 0;
    if (k < n_records) {
        r = recs[k];
        bits = site_entries(r);
    }
    const WaveEntries e = wave_entries(bits);
    if (!bits) return;
    uint32_t at = wave_at[k >> 6] + e.before(lane);
    if (bits & 1u) {
        key[at] = r.left_pos;
        id[at] = 2 * k;
        ++at;
    }
    if (bits & 2u) {
        key[at] = r.right_pos;
        id[at] = 2 * k + 1;
    }
}

__global__ __launch_bounds__(kThreads) void sites_heads_kernel(const uint64_t *__restrict__ pos, uint32_t n_entries,
                                                               uint32_t *__restrict__ head) {
    const uint32_t e = blockIdx.x * kThreads + threadIdx.x;
    if (e > n_entries) return;
    head[e] = e < n_entries && (e == 0 || pos[e] != pos[e - 1]) ? 1u : 0u;   // (e == n_entries: the closing zero)
}

struct SitesOut {
    uint64_t *pos;
    uint32_t *pairs, *sd;
    uint8_t *ref, *side;
    uint32_t *alt_mask;   // a word per site while the atomics run; sites_pack_kernel makes the bytes
};

__global__ __launch_bounds__(kThreads) void sites_reduce_kernel(const asgart_variant *__restrict__ recs,
                                                                const uint64_t *__restrict__ pos,
                                                                const uint32_t *__restrict__ id,
                                                                const uint32_t *__restrict__ head,
                                                                const uint32_t *__restrict__ rank, uint32_t n_entries,
                                                                SitesOut out) {
    const uint32_t e = blockIdx.x * kThreads + threadIdx.x, lane = __lane_id();
    const bool is_entry = e < n_entries;
    // (the lanes behind the last entry keep a site no entry has, so that the sites still never decrease along the wave)
    uint32_t site = 0xFFFFFFFFu, alt_bit = 0;
    if (is_entry) {
        const uint32_t h = head[e], my = id[e];
        site = rank[e] + h - 1u;   // (rank is exclusive, and entry 0 is a head)
        const asgart_variant r = recs[my >> 1];
        const SiteEntry s = site_entry(r, my & 1u);
        alt_bit = 1u << s.alt;
        if (h) {
            out.pos[site] = pos[e];
            out.ref[site] = (uint8_t)s.ref;
            out.sd[site] = r.sd;
            out.side[site] = (uint8_t)(my & 1u);
        }
    }
    const uint32_t below = __shfl_up(site, 1);
    const bool opens = lane == 0 || below != site;
    const uint32_t end = row_end_lane(__ballot(opens), lane);
    const uint32_t mask = row_or(alt_bit, lane, end);
    if (opens && is_entry) {
        atomicAdd(out.pairs + site, end - lane);
        atomicOr(out.alt_mask + site, mask);
    }
}

__global__ __launch_bounds__(kThreads) void sites_pack_kernel(const uint32_t *__restrict__ words, uint32_t n_sites,
                                                              uint8_t *__restrict__ bytes) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i < n_sites) bytes[i] = (uint8_t)words[i];
}

struct VariantsWork : ToolWork {
    DevBuf &sds = buf(), &flags = buf(), &status = buf(), &run_off = buf(), &run_len = buf(), &run_op = buf(), &in_sums = buf(),
           &sums = buf(), &tail = buf(), &var_off = buf();
};

struct SitesWork : ToolWork {
    DevBuf &wave_count = buf(), &wave_at = buf(), &key = buf(), &id = buf(), &pos = buf(), &sorted_id = buf(), &head = buf(),
           &rank = buf(), &mask_words = buf();
};

const char kWho[] = "asgart_alignment_variants";
const char kWhoSites[] = "asgart_variant_sites";

int32_t run_variants(VariantsWork &w, asgart_variants *res, const uint8_t *text, const asgart_proto_sd *sds,
                     const uint8_t *flags, const uint8_t *status, uint32_t n, const uint64_t *run_offsets,
                     const uint32_t *run_len, const uint8_t *run_op) {
    const uint64_t n_runs = run_offsets[n];
    RC_TRY(w.open(4));
    hipStream_t s = w.s;
    HIP_TRY(hipEventRecord(w.ev[0], s));
    RC_TRY(w.upload(w.sds, sds, (size_t)n * sizeof(asgart_proto_sd)));
    RC_TRY(w.upload(w.flags, flags, n));
    RC_TRY(w.upload(w.status, status, n));
    RC_TRY(w.upload(w.run_off, run_offsets, ((size_t)n + 1) * 8));
    RC_TRY(w.upload(w.run_len, run_len, (size_t)n_runs * 4));
    RC_TRY(w.upload(w.run_op, run_op, (size_t)n_runs));
    HIP_TRY(hipEventRecord(w.ev[1], s));
    RC_TRY(w.in_sums.reserve(((size_t)n_runs + 1) * sizeof(RunSums)));
    RC_TRY(w.sums.reserve(((size_t)n_runs + 1) * sizeof(RunSums)));
    RC_TRY(w.tail.reserve(32));   // the refusal word, the number of records, the number of `X` records
    RC_TRY(w.var_off.reserve(((size_t)n + 1) * 8));
    HIP_TRY(hipMemsetAsync(w.tail.p, 0xff, 8, s));
    HIP_TRY(hipMemsetAsync(w.tail.as<uint64_t>() + 1, 0, 16, s));
    VariantsIn in{};
    in.sds = w.sds.as<uint64_t>();
    in.flags = w.flags.as<uint8_t>();
    in.status = w.status.as<uint8_t>();
    in.run_off = w.run_off.as<uint64_t>();
    in.run_len = w.run_len.as<uint32_t>();
    in.run_op = w.run_op.as<uint8_t>();
    in.text = text;
    in.S = w.in_sums.as<RunSums>();
    in.bad = w.tail.as<uint64_t>();
    in.var_off = w.var_off.as<uint64_t>();
    in.n_sd = n;
    in.n_runs = n_runs;
    variants_runs_kernel<<<blocks_for(n_runs + 1, kThreads), kThreads, 0, s>>>(in);
    HIP_TRY(hipGetLastError());
    {
        size_t tmp = 0;
        const RunSums *from = w.in_sums.as<RunSums>();
        RunSums *to = w.sums.as<RunSums>();
        HIP_TRY(rocprim::exclusive_scan(nullptr, tmp, from, to, RunSums{0, 0, 0}, (size_t)n_runs + 1, RunSumsPlus(), s));
        RC_TRY(w.scan_tmp.reserve(tmp + 16));
        HIP_TRY(rocprim::exclusive_scan(w.scan_tmp.p, tmp, from, to, RunSums{0, 0, 0}, (size_t)n_runs + 1, RunSumsPlus(), s));
    }
    in.S = w.sums.as<RunSums>();
    variants_rows_kernel<<<blocks_for((uint64_t)n + 1, kThreads), kThreads, 0, s>>>(in);
    HIP_TRY(hipGetLastError());
    // the lowest refused duplication and, behind it, the number of records, in one copy
    HIP_TRY(hipMemcpyAsync(in.bad + 1, in.var_off + n, 8, hipMemcpyDeviceToDevice, s));
    uint64_t tail[2] = {0, 0};
    HIP_TRY(read_back(tail, in.bad, 16, s));
    if (tail[0] != ~(uint64_t)0) return refuse_runs(kWho, tail[0], sds, run_offsets, run_len, run_op);
    if (tail[1] >= (uint64_t)1 << 31) {
        set_error("%s: %llu variants; 2^31 variants and more are not supported", kWho, (unsigned long long)tail[1]);
        return ASGART_E_CAP;
    }
    HIP_TRY(hipEventRecord(w.ev[2], s));
    res->n_variants = tail[1];
    if (tail[1]) {
        RC_TRY(res->records.reserve((size_t)tail[1] * sizeof(asgart_variant)));
        variants_records_kernel<<<blocks_for(tail[1], kRecords), kThreads, 0, s>>>(in, tail[1], res->records.as<asgart_variant>(),
                                                                                 w.tail.as<unsigned long long>() + 2);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipEventRecord(w.ev[3], s));
    HIP_TRY(stream_sync(s));
    const auto t0 = std::chrono::steady_clock::now();
    res->var_offsets.resize((size_t)n + 1);
    HIP_TRY(hipMemcpyAsync(res->var_offsets.data(), w.var_off.p, ((size_t)n + 1) * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(read_back(&res->n_snv, w.tail.as<uint64_t>() + 2, 8, s));
    float up = 0, a = 0, b = 0;
    HIP_TRY(hipEventElapsedTime(&up, w.ev[0], w.ev[1]));
    HIP_TRY(hipEventElapsedTime(&a, w.ev[1], w.ev[2]));
    HIP_TRY(hipEventElapsedTime(&b, w.ev[2], w.ev[3]));
    res->ms[0] = up;
    res->ms[1] = (double)a + (double)b;
    res->ms[2] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return 0;
}

int32_t run_sites(SitesWork &w, asgart_sites *res, const asgart_variants *v) {
    const uint32_t n_records = (uint32_t)v->n_variants;   // (below 2^31: entries below 2^32)
    const asgart_variant *recs = v->records.as<asgart_variant>();
    RC_TRY(w.open(2));
    hipStream_t s = w.s;
    HIP_TRY(hipEventRecord(w.ev[0], s));
    const uint32_t n_waves = (n_records + 63) / 64;
    RC_TRY(w.wave_count.reserve(((size_t)n_waves + 1) * 4));
    RC_TRY(w.wave_at.reserve(((size_t)n_waves + 1) * 4));
    uint32_t *wave_count = w.wave_count.as<uint32_t>(), *wave_at = w.wave_at.as<uint32_t>();
    // (a launch of whole workgroups over n_records + 64 items: some lane of it has the wave behind the last)
    sites_count_kernel<<<blocks_for((uint64_t)n_records + 64, kThreads), kThreads, 0, s>>>(recs, n_records, n_waves, wave_count);
    HIP_TRY(hipGetLastError());
    RC_TRY(w.exclusive_scan(wave_count, wave_at, (size_t)n_waves + 1));
    uint32_t n_entries = 0;
    HIP_TRY(read_back(&n_entries, wave_at + n_waves, 4, s));
    res->n_entries = n_entries;
    if (n_entries) {
        for (DevBuf *b : {&w.key, &w.pos}) RC_TRY(b->reserve((size_t)n_entries * 8));
        for (DevBuf *b : {&w.id, &w.sorted_id}) RC_TRY(b->reserve((size_t)n_entries * 4));
        for (DevBuf *b : {&w.head, &w.rank}) RC_TRY(b->reserve(((size_t)n_entries + 1) * 4));
        sites_emit_kernel<<<blocks_for(n_records, kThreads), kThreads, 0, s>>>(recs, n_records, wave_at, w.key.as<uint64_t>(),
                                                                             w.id.as<uint32_t>());
        HIP_TRY(hipGetLastError());
        RC_TRY(w.sort_pairs(w.key.as<uint64_t>(), w.pos.as<uint64_t>(), w.id.as<uint32_t>(), w.sorted_id.as<uint32_t>(),
                            n_entries, 64));
        uint32_t *head = w.head.as<uint32_t>(), *rank = w.rank.as<uint32_t>();
        sites_heads_kernel<<<blocks_for((uint64_t)n_entries + 1, kThreads), kThreads, 0, s>>>(w.pos.as<uint64_t>(), n_entries,
                                                                                            head);
        HIP_TRY(hipGetLastError());
        RC_TRY(w.exclusive_scan(head, rank, (size_t)n_entries + 1));
        uint32_t n_sites = 0;
        HIP_TRY(read_back(&n_sites, rank + n_entries, 4, s));
        if (n_sites == 0 || n_sites > n_entries) {
            set_error("%s: %u sites of %u entries", kWhoSites, n_sites, n_entries);
            return ASGART_E_HIP;
        }
        res->n_sites = n_sites;
        RC_TRY(res->pos.reserve((size_t)n_sites * 8));
        RC_TRY(res->pairs.reserve((size_t)n_sites * 4));
        RC_TRY(res->sd.reserve((size_t)n_sites * 4));
        RC_TRY(w.mask_words.reserve((size_t)n_sites * 4));
        for (DevBuf *b : {&res->ref, &res->alt_mask, &res->side}) RC_TRY(b->reserve(std::max<size_t>(n_sites, 16)));
        HIP_TRY(hipMemsetAsync(res->pairs.p, 0, (size_t)n_sites * 4, s));
        HIP_TRY(hipMemsetAsync(w.mask_words.p, 0, (size_t)n_sites * 4, s));
        const SitesOut out{res->pos.as<uint64_t>(), res->pairs.as<uint32_t>(), res->sd.as<uint32_t>(), res->ref.as<uint8_t>(),
                           res->side.as<uint8_t>(), w.mask_words.as<uint32_t>()};
        sites_reduce_kernel<<<blocks_for(n_entries, kThreads), kThreads, 0, s>>>(recs, w.pos.as<uint64_t>(),
                                                                               w.sorted_id.as<uint32_t>(), head, rank,
                                                                               n_entries, out);
        HIP_TRY(hipGetLastError());
        sites_pack_kernel<<<blocks_for(n_sites, kThreads), kThreads, 0, s>>>(w.mask_words.as<uint32_t>(), n_sites,
                                                                           res->alt_mask.as<uint8_t>());
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipEventRecord(w.ev[1], s));
    HIP_TRY(stream_sync(s));
    float kernels = 0;
    HIP_TRY(hipEventElapsedTime(&kernels, w.ev[0], w.ev[1]));
    res->ms[1] = (double)kernels;   // (nothing is uploaded; the two counts read back on the way are inside)
    return 0;
}

template <class T>
int32_t fetch(T *to, const DevBuf &from, size_t items) {
    if (to && items) HIP_TRY(hipMemcpy(to, from.p, items * sizeof(T), hipMemcpyDeviceToHost));
    return 0;
}

}  // namespace
}  // namespace asgart

using namespace asgart;

extern "C" int32_t asgart_alignment_variants(asgart_index *idx, const asgart_proto_sd *sds, const uint8_t *flags,
                                             const uint8_t *status, int64_t n_sd, const uint64_t *run_offsets,
                                             const uint32_t *run_len, const uint8_t *run_op, asgart_variants **out) {
    if (out) *out = nullptr;
    if (!out) {
        set_error("%s: bad argument", kWho);
        return ASGART_E_ARG;
    }
    RC_TRY(check_alignment_arguments(kWho, idx, sds, flags, status, n_sd, run_offsets, run_len, run_op, out));
    REFUSE_POISONED(idx);
    RC_TRY(use_device(kWho, idx->device));
    if (n_sd == 0) {   // no duplications, no records; nothing is launched
        *out = new asgart_variants;
        (*out)->device = idx->device;
        (*out)->var_offsets.assign(1, 0);
        return 0;
    }
    return run_tool<VariantsWork>(out, [&](VariantsWork &w, asgart_variants *res) {
        res->device = idx->device;
        return run_variants(w, res, idx->d_text, sds, flags, status, (uint32_t)n_sd, run_offsets, run_len, run_op);
    });
}

extern "C" void asgart_variants_counts(const asgart_variants *r, uint64_t *n_sd, uint64_t *n_variants, uint64_t *n_snv) {
    if (n_sd) *n_sd = r ? r->var_offsets.size() - 1 : 0;
    if (n_variants) *n_variants = r ? r->n_variants : 0;
    if (n_snv) *n_snv = r ? r->n_snv : 0;
}

extern "C" int32_t asgart_variants_copy(const asgart_variants *r, asgart_variant *records, uint64_t *var_offsets) {
    if (!r) {
        set_error("asgart_variants_copy: bad argument");
        return ASGART_E_ARG;
    }
    RC_TRY(use_device("asgart_variants_copy", r->device));
    if (var_offsets) memcpy(var_offsets, r->var_offsets.data(), r->var_offsets.size() * 8);
    return fetch(records, r->records, (size_t)r->n_variants);
}

extern "C" int32_t asgart_variants_timings(const asgart_variants *r, double *ms3) {
    return copy_ms3("asgart_variants_timings", r, ms3);
}

extern "C" void asgart_variants_free(asgart_variants *r) { delete r; }

extern "C" void asgart_variants_geometry(uint64_t *block_threads, uint64_t *records_per_block) {
    if (block_threads) *block_threads = kThreads;
    if (records_per_block) *records_per_block = kRecords;
}

extern "C" int32_t asgart_variant_sites(const asgart_variants *v, asgart_sites **out) {
    if (out) *out = nullptr;
    if (!v || !out) {
        set_error("%s: bad argument", kWhoSites);
        return ASGART_E_ARG;
    }
    RC_TRY(use_device(kWhoSites, v->device));
    return run_tool<SitesWork>(out, [&](SitesWork &w, asgart_sites *res) {
        res->device = v->device;
        res->var_offsets = v->var_offsets;
        return v->n_variants ? run_sites(w, res, v) : 0;
    });
}

extern "C" void asgart_sites_counts(const asgart_sites *r, uint64_t *n_sites, uint64_t *n_entries) {
    if (n_sites) *n_sites = r ? r->n_sites : 0;
    if (n_entries) *n_entries = r ? r->n_entries : 0;
}

extern "C" int32_t asgart_sites_copy(const asgart_sites *r, uint64_t *pos, uint8_t *ref, uint8_t *alt_mask, uint32_t *pairs,
                                     uint32_t *sd, uint8_t *side) {
    if (!r) {
        set_error("asgart_sites_copy: bad argument");
        return ASGART_E_ARG;
    }
    RC_TRY(use_device("asgart_sites_copy", r->device));
    const size_t n = (size_t)r->n_sites;
    RC_TRY(fetch(pos, r->pos, n));
    RC_TRY(fetch(ref, r->ref, n));
    RC_TRY(fetch(alt_mask, r->alt_mask, n));
    RC_TRY(fetch(pairs, r->pairs, n));
    RC_TRY(fetch(sd, r->sd, n));
    return fetch(side, r->side, n);
}

extern "C" int32_t asgart_sites_timings(const asgart_sites *r, double *ms3) {
    return copy_ms3("asgart_sites_timings", r, ms3);
}

extern "C" void asgart_sites_free(asgart_sites *r) { delete r; }

extern "C" void asgart_sites_geometry(uint64_t *block_threads) {
    if (block_threads) *block_threads = kThreads;
}
