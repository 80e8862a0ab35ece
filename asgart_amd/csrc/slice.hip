// slice.hip -- the filters of asgart-slice on family arrays: asgart_slice_families and its result handle.
//
// Replaces, for a result held as arrays, the per-duplication part of reference src/bin/asgart-slice.rs:126-191: the arm
// rewrite of RunResult::flatten (src/structs.rs:401-414), the retains of remove_direct .. remove_intra (:143-194) and of
// --min-length (asgart-slice.rs:150-155), max_family_members (:196-198), the retains of keep_ / restrict_ /
// exclude_fragments and their _regexp forms (:232-348), `families.retain(|f| !f.is_empty())`, and the recomputation of the
// global positions in consolidate_families (:216-227) and exclude_fragments (:311-318).  Everything that looks at a NAME
// (literal sets, regular expressions, the statistics of flatten, the reduced map) stays on the host, where it is work per
// fragment: the host hands over one small table per question, indexed by name id.  What is left per duplication is a few
// table lookups, and the whole slice is
//   stage A flags -> scan -> family sizes -> stage B flags -> scan -> family sizes -> scan over families -> one stable
//   compaction that writes every output array.
// Family sizes are differences of the scan over duplications at the family's two offsets: an empty family, one larger
// than a workgroup and one larger than 65 535 are the same case.  Survivors keep the input order (their output slot is
// their rank in the scan); the only atomic is the minimum that finds the first duplication exclude_fragments would panic on.
#include "tool_base.hpp"

namespace asgart {
namespace {

constexpr uint32_t kBlock = 256;
constexpr uint8_t kExAny = 1, kExFirst = 2, kExAbsent = 4;  // bits of tables.exclude[name]

struct SliceTables {
    const int32_t *new_id;    // nullable (no collapse)
    const uint64_t *addend;   // nullable with new_id
    const uint32_t *keep_mask, *restrict_mask;  // nullable where the option's `all` is 0
    const uint8_t *exclude;                     // nullable unless opt.exclude
    const int64_t *final_pos;                   // nullable unless opt.relocate
};

struct Arms {
    int32_t l, r;
    uint64_t pl, pr;
};

// both arms of duplication i through the collapse tables (RunResult::flatten, src/structs.rs:401-414)
__device__ inline Arms arms_of(const int2 *__restrict__ chr, const ulonglong2 *__restrict__ chr_pos, uint32_t i,
                               const SliceTables &t) {
    const int2 c = chr[i];
    const ulonglong2 p = chr_pos[i];
    Arms a{c.x, c.y, p.x, p.y};
    if (t.new_id) {
        a.pl += t.addend[c.x];
        a.pr += t.addend[c.y];
        a.l = t.new_id[c.x];
        a.r = t.new_id[c.y];
    }
    return a;
}

// stage A: the flag filters, inter / intra and --min-length; alive[i] = 1 where duplication i passes
__global__ __launch_bounds__(kBlock) void slice_stage_a_kernel(const uint4 *__restrict__ sds_v,
                                                              const uint8_t *__restrict__ flags,
                                                              const int2 *__restrict__ chr,
                                                              const ulonglong2 *__restrict__ chr_pos, uint32_t n,
                                                              SliceTables t, asgart_slice_options opt,
                                                              uint32_t *__restrict__ alive) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const uint8_t f = flags[i];
    bool ok = (f & opt.flags_set) == opt.flags_set && (f & opt.flags_clear) == 0;
    if (opt.inter_mode || opt.no_intra) {
        const Arms a = arms_of(chr, chr_pos, i, t);
        const bool same = a.l == a.r;
        if (opt.inter_mode == 1) ok = ok && same;
        if (opt.inter_mode == 2) ok = ok && (same || a.l == opt.collapsed_id || a.r == opt.collapsed_id);
        if (opt.no_intra) ok = ok && !same;
    }
    if (opt.has_min_length) {
        const uint4 v = sds_v[2 * (size_t)i + 1];  // (left_length, right_length)
        const uint64_t ll = (uint64_t)v.x | (uint64_t)v.y << 32, rl = (uint64_t)v.z | (uint64_t)v.w << 32;
        ok = ok && (ll < rl ? ll : rl) >= opt.min_length;
    }
    alive[i] = ok ? 1u : 0u;
}

// family f after stage A: dead when emptied (drop_empty) or larger than max_family_members
__global__ __launch_bounds__(kBlock) void slice_family_live_kernel(const uint64_t *__restrict__ offs, uint32_t n_fam,
                                                                  const uint32_t *__restrict__ rank_a,
                                                                  asgart_slice_options opt, uint8_t *__restrict__ live) {
    const uint32_t f = blockIdx.x * kBlock + threadIdx.x;
    if (f >= n_fam) return;
    const uint64_t size = rank_a[offs[f + 1]] - rank_a[offs[f]];
    live[f] = !((opt.drop_empty && size == 0) || (opt.has_max_family && size > opt.max_family_members));
}

// stage B: keep / restrict / exclude for the duplications of live families; *err = the first duplication that passes the
// first exclusion with an arm on a fragment the map no longer holds (the reference's unwrap, src/structs.rs:313-316)
__global__ __launch_bounds__(kBlock) void slice_stage_b_kernel(const uint64_t *__restrict__ offs, uint32_t n_fam,
                                                              const int2 *__restrict__ chr,
                                                              const ulonglong2 *__restrict__ chr_pos, uint32_t n,
                                                              SliceTables t, asgart_slice_options opt,
                                                              const uint8_t *__restrict__ live,
                                                              uint32_t *__restrict__ alive, uint32_t *__restrict__ err) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    bool ok = alive[i] != 0 && live[segment_of(offs, n_fam, i)] != 0;
    if (ok && (opt.keep_all || opt.restrict_all || opt.exclude)) {
        const Arms a = arms_of(chr, chr_pos, i, t);
        if (opt.keep_all) ok = ((t.keep_mask[a.l] | t.keep_mask[a.r]) & opt.keep_all) == opt.keep_all;
        if (ok && opt.restrict_all) ok = ((t.restrict_mask[a.l] & t.restrict_mask[a.r]) & opt.restrict_all) == opt.restrict_all;
        if (ok && opt.exclude) {
            const uint8_t e = t.exclude[a.l] | t.exclude[a.r];
            if (!(e & kExFirst) && (e & kExAbsent)) atomicMin(err, i);
            ok = !(e & kExAny);
        }
    }
    alive[i] = ok ? 1u : 0u;
}

// family f at the end: kept[f] = 1 where it is in the output
__global__ __launch_bounds__(kBlock) void slice_family_keep_kernel(const uint64_t *__restrict__ offs, uint32_t n_fam,
                                                                  const uint32_t *__restrict__ rank_b,
                                                                  const uint8_t *__restrict__ live, asgart_slice_options opt,
                                                                  uint32_t *__restrict__ kept) {
    const uint32_t f = blockIdx.x * kBlock + threadIdx.x;
    if (f >= n_fam) return;
    const uint32_t size = rank_b[offs[f + 1]] - rank_b[offs[f]];
    kept[f] = (live[f] && !(opt.drop_empty && size == 0)) ? 1u : 0u;
}

// The stable compaction.  Two lanes per duplication, each moving one aligned 16-byte half of its 32-byte asgart_proto_sd
// (lane 2i: left, right; lane 2i + 1: the two lengths), so that a wave reads 1 KiB of consecutive bytes; the even lane
// also writes chr and the flag byte, the odd lane chr_pos and the key.
__global__ __launch_bounds__(kBlock) void slice_compact_kernel(const uint4 *__restrict__ sds_v,
                                                              const uint8_t *__restrict__ flags,
                                                              const int2 *__restrict__ chr,
                                                              const ulonglong2 *__restrict__ chr_pos, uint32_t n,
                                                              SliceTables t, asgart_slice_options opt,
                                                              const uint32_t *__restrict__ alive,
                                                              const uint32_t *__restrict__ rank_b,
                                                              uint4 *__restrict__ out_sds_v, uint8_t *__restrict__ out_flags,
                                                              int2 *__restrict__ out_chr,
                                                              ulonglong2 *__restrict__ out_chr_pos,
                                                              int64_t *__restrict__ out_keys) {
    const uint64_t g = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    const uint32_t i = (uint32_t)(g >> 1), half = (uint32_t)(g & 1);
    if (i >= n || !alive[i]) return;
    const uint32_t j = rank_b[i];
    uint4 v = sds_v[g];
    const Arms a = arms_of(chr, chr_pos, i, t);
    if (half == 0) {
        if (opt.relocate) {  // consolidate_families, src/structs.rs:216-227: find_chr(..).map_or(0, ..)
            const int64_t fl = t.final_pos[a.l], fr = t.final_pos[a.r];
            const uint64_t gl = fl < 0 ? 0 : (uint64_t)fl + a.pl, gr = fr < 0 ? 0 : (uint64_t)fr + a.pr;
            v = make_uint4((uint32_t)gl, (uint32_t)(gl >> 32), (uint32_t)gr, (uint32_t)(gr >> 32));
        }
        out_chr[j] = make_int2(a.l, a.r);
        out_flags[j] = flags[i];
    } else {
        ulonglong2 p;
        p.x = a.pl;
        p.y = a.pr;
        out_chr_pos[j] = p;
        out_keys[j] = (int64_t)i;
    }
    out_sds_v[2 * (size_t)j + half] = v;
}

}  // namespace
}  // namespace asgart

using namespace asgart;

struct asgart_slice {
    std::vector<uint64_t> offs;
    std::vector<asgart_proto_sd> sds;
    std::vector<int32_t> chr;
    std::vector<uint64_t> chr_pos;
    std::vector<uint8_t> flags;
    std::vector<int64_t> keys;
    double ms[3] = {0, 0, 0};
};

namespace {

struct SliceWork : ToolWork {
    DevBuf &offs = buf(), &sds = buf(), &flags = buf(), &chr = buf(), &chr_pos = buf(), &new_id = buf(), &addend = buf(),
           &keep = buf(), &restr = buf(), &excl = buf(), &final_pos = buf();
    DevBuf &alive = buf(), &rank = buf(), &live = buf(), &kept = buf(), &fam_rank = buf(), &err = buf();
    DevBuf &o_offs = buf(), &o_sds = buf(), &o_flags = buf(), &o_chr = buf(), &o_chr_pos = buf(), &o_keys = buf();
};

// Every argument check of the call, before the device is looked at.
int32_t check_arguments(const uint64_t *fam_offsets, int64_t n_families, const asgart_proto_sd *sds, const uint8_t *flags,
                        const int32_t *chr, const uint64_t *chr_pos, int64_t n_sd, const asgart_slice_tables *tb,
                        const asgart_slice_options *opt, asgart_slice **out) {
    if (!out || !fam_offsets || !tb || !opt || n_families < 0 || n_sd < 0 || (n_sd && (!sds || !flags || !chr || !chr_pos))) {
        set_error("asgart_slice_families: bad argument");
        return ASGART_E_ARG;
    }
    if (n_sd >= ((int64_t)1 << 31) - 1 || n_families >= ((int64_t)1 << 31) - 1) {
        set_error("asgart_slice_families: 2^31 duplications or families and more are not supported");
        return ASGART_E_CAP;
    }
    RC_TRY(check_csr("asgart_slice_families", "fam_offsets", fam_offsets, n_families, n_sd, "n_sd"));
    const int64_t nn = tb->n_names;
    if (nn < 0 || (n_sd && nn == 0)) {
        set_error("asgart_slice_families: empty name table");
        return ASGART_E_ARG;
    }
    const bool collapse = tb->new_id != nullptr || tb->addend != nullptr;
    struct Need { const char *name; bool wanted; const void *p; int64_t len; };
    const Need need[6] = {{"new_id", collapse, tb->new_id, tb->table_len[0]},
                          {"addend", collapse, tb->addend, tb->table_len[1]},
                          {"keep_mask", opt->keep_all != 0, tb->keep_mask, tb->table_len[2]},
                          {"restrict_mask", opt->restrict_all != 0, tb->restrict_mask, tb->table_len[3]},
                          {"exclude", opt->exclude != 0, tb->exclude, tb->table_len[4]},
                          {"final_pos", opt->relocate != 0, tb->final_pos, tb->table_len[5]}};
    for (const Need &q : need)
        if (q.wanted && ((nn && !q.p) || (q.p ? q.len : 0) != nn)) {
            set_error("asgart_slice_families: table %s has %lld entries for %lld names", q.name,
                      (long long)(q.p ? q.len : 0), (long long)nn);
            return ASGART_E_ARG;
        }
    if (collapse)
        for (int64_t k = 0; k < nn; ++k)
            if (tb->new_id[k] < 0 || tb->new_id[k] >= nn) {
                set_error("asgart_slice_families: new_id[%lld] = %d is outside the name table (%lld names)", (long long)k,
                          tb->new_id[k], (long long)nn);
                return ASGART_E_ARG;
            }
    RC_TRY(check_name_ids("asgart_slice_families", chr, n_sd, nn));
    if (opt->inter_mode > 2 || (opt->flags_set | opt->flags_clear) > 3 || opt->collapsed_id >= nn) {
        set_error("asgart_slice_families: bad options (inter_mode 0..2, flag bits 0..3, collapsed_id inside the name table)");
        return ASGART_E_ARG;
    }
    return 0;
}

int32_t run_slice(SliceWork &w, asgart_slice *res, const uint64_t *fam_offsets, uint32_t nf, const asgart_proto_sd *sds,
                  const uint8_t *flags, const int32_t *chr, const uint64_t *chr_pos, uint32_t n,
                  const asgart_slice_tables *tb, const asgart_slice_options &opt) {
    const auto t0 = std::chrono::steady_clock::now();
    RC_TRY(w.open(4));
    hipStream_t s = w.s;
    const size_t nn = (size_t)tb->n_names;
    RC_TRY(w.upload(w.offs, fam_offsets, ((size_t)nf + 1) * 8));
    RC_TRY(w.upload(w.sds, sds, (size_t)n * sizeof(asgart_proto_sd)));
    RC_TRY(w.upload(w.flags, flags, n));
    RC_TRY(w.upload(w.chr, chr, (size_t)n * 8));
    RC_TRY(w.upload(w.chr_pos, chr_pos, (size_t)n * 16));
    SliceTables t{};
    if (tb->new_id) {
        RC_TRY(w.upload(w.new_id, tb->new_id, nn * 4));
        RC_TRY(w.upload(w.addend, tb->addend, nn * 8));
        t.new_id = w.new_id.as<int32_t>();
        t.addend = w.addend.as<uint64_t>();
    }
    if (opt.keep_all) {
        RC_TRY(w.upload(w.keep, tb->keep_mask, nn * 4));
        t.keep_mask = w.keep.as<uint32_t>();
    }
    if (opt.restrict_all) {
        RC_TRY(w.upload(w.restr, tb->restrict_mask, nn * 4));
        t.restrict_mask = w.restr.as<uint32_t>();
    }
    if (opt.exclude) {
        RC_TRY(w.upload(w.excl, tb->exclude, nn));
        t.exclude = w.excl.as<uint8_t>();
    }
    if (opt.relocate) {
        RC_TRY(w.upload(w.final_pos, tb->final_pos, nn * 8));
        t.final_pos = w.final_pos.as<int64_t>();
    }
    // alive and kept carry one closing zero, so that the exclusive scans over n + 1 / nf + 1 items end in the totals
    RC_TRY(w.alive.reserve(((size_t)n + 1) * 4));
    RC_TRY(w.rank.reserve(((size_t)n + 1) * 4));
    RC_TRY(w.live.reserve((size_t)nf + 16));
    RC_TRY(w.kept.reserve(((size_t)nf + 1) * 4));
    RC_TRY(w.fam_rank.reserve(((size_t)nf + 1) * 4));
    RC_TRY(w.err.reserve(16));
    uint32_t *alive = w.alive.as<uint32_t>(), *rank = w.rank.as<uint32_t>(), *kept = w.kept.as<uint32_t>(),
             *fam_rank = w.fam_rank.as<uint32_t>(), *err = w.err.as<uint32_t>();
    uint8_t *live = w.live.as<uint8_t>();
    const uint64_t *d_offs = w.offs.as<uint64_t>();
    const uint4 *sds_v = w.sds.as<uint4>();
    const uint8_t *d_flags = w.flags.as<uint8_t>();
    const int2 *d_chr = w.chr.as<int2>();
    const ulonglong2 *d_chr_pos = w.chr_pos.as<ulonglong2>();
    HIP_TRY(hipMemsetAsync(alive + n, 0, 4, s));
    HIP_TRY(hipMemsetAsync(kept + nf, 0, 4, s));
    HIP_TRY(hipMemsetAsync(err, 0xFF, 4, s));
    HIP_TRY(hipEventRecord(w.ev[0], s));
    if (n) {
        slice_stage_a_kernel<<<blocks_for(n), kBlock, 0, s>>>(sds_v, d_flags, d_chr, d_chr_pos, n, t, opt, alive);
        HIP_TRY(hipGetLastError());
    }
    RC_TRY(w.exclusive_scan(alive, rank, (size_t)n + 1));
    if (nf) {
        slice_family_live_kernel<<<blocks_for(nf), kBlock, 0, s>>>(d_offs, nf, rank, opt, live);
        HIP_TRY(hipGetLastError());
    }
    if (n) {
        slice_stage_b_kernel<<<blocks_for(n), kBlock, 0, s>>>(d_offs, nf, d_chr, d_chr_pos, n, t, opt, live, alive, err);
        HIP_TRY(hipGetLastError());
    }
    RC_TRY(w.exclusive_scan(alive, rank, (size_t)n + 1));
    if (nf) {
        slice_family_keep_kernel<<<blocks_for(nf), kBlock, 0, s>>>(d_offs, nf, rank, live, opt, kept);
        HIP_TRY(hipGetLastError());
    }
    RC_TRY(w.exclusive_scan(kept, fam_rank, (size_t)nf + 1));
    HIP_TRY(hipEventRecord(w.ev[1], s));
    uint32_t h_err = 0, n_out = 0, nf_out = 0;
    HIP_TRY(read_back(&h_err, err, 4, s));
    if (h_err != 0xFFFFFFFFu) {
        set_error("asgart_slice_families: duplication %u passes the exclusion with an arm on a fragment that is not in the "
                  "map (the reference unwraps find_chr there, src/structs.rs:313-316)", h_err);
        return ASGART_E_ARG;
    }
    HIP_TRY(read_back(&n_out, rank + n, 4, s));
    HIP_TRY(read_back(&nf_out, fam_rank + nf, 4, s));
    RC_TRY(w.o_offs.reserve(((size_t)nf_out + 1) * 8));
    RC_TRY(w.o_sds.reserve(std::max<size_t>((size_t)n_out * sizeof(asgart_proto_sd), 16)));
    RC_TRY(w.o_flags.reserve(std::max<size_t>(n_out, 16)));
    RC_TRY(w.o_chr.reserve(std::max<size_t>((size_t)n_out * 8, 16)));
    RC_TRY(w.o_chr_pos.reserve(std::max<size_t>((size_t)n_out * 16, 16)));
    RC_TRY(w.o_keys.reserve(std::max<size_t>((size_t)n_out * 8, 16)));
    HIP_TRY(hipEventRecord(w.ev[2], s));
    family_offsets_kernel<kBlock><<<blocks_for((uint64_t)nf + 1), kBlock, 0, s>>>(d_offs, nf, n, rank, kept, fam_rank,
                                                                                 w.o_offs.as<uint64_t>());
    HIP_TRY(hipGetLastError());
    if (n) {
        slice_compact_kernel<<<blocks_for(2 * (uint64_t)n), kBlock, 0, s>>>(
            sds_v, d_flags, d_chr, d_chr_pos, n, t, opt, alive, rank, w.o_sds.as<uint4>(), w.o_flags.as<uint8_t>(),
            w.o_chr.as<int2>(), w.o_chr_pos.as<ulonglong2>(), w.o_keys.as<int64_t>());
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipEventRecord(w.ev[3], s));
    res->offs.resize((size_t)nf_out + 1);
    res->sds.resize(n_out);
    res->chr.resize(2 * (size_t)n_out);
    res->chr_pos.resize(2 * (size_t)n_out);
    res->flags.resize(n_out);
    res->keys.resize(n_out);
    HIP_TRY(stream_sync(s));
    HIP_TRY(hipMemcpyAsync(res->offs.data(), w.o_offs.p, ((size_t)nf_out + 1) * 8, hipMemcpyDeviceToHost, s));
    if (n_out) {
        HIP_TRY(hipMemcpyAsync(res->sds.data(), w.o_sds.p, (size_t)n_out * sizeof(asgart_proto_sd), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(res->chr.data(), w.o_chr.p, (size_t)n_out * 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(res->chr_pos.data(), w.o_chr_pos.p, (size_t)n_out * 16, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(res->flags.data(), w.o_flags.p, n_out, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(res->keys.data(), w.o_keys.p, (size_t)n_out * 8, hipMemcpyDeviceToHost, s));
    }
    HIP_TRY(stream_sync(s));
    float a = 0, b = 0;
    HIP_TRY(hipEventElapsedTime(&a, w.ev[0], w.ev[1]));
    HIP_TRY(hipEventElapsedTime(&b, w.ev[2], w.ev[3]));
    res->ms[0] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    res->ms[1] = (double)a + (double)b;
    res->ms[2] = (double)b;
    return 0;
}

}  // namespace

extern "C" int32_t asgart_slice_families(int32_t device, const uint64_t *fam_offsets, int64_t n_families,
                                         const asgart_proto_sd *sds, const uint8_t *flags, const int32_t *chr,
                                         const uint64_t *chr_pos, int64_t n_sd, const asgart_slice_tables *tables,
                                         const asgart_slice_options *options, asgart_slice **out) {
    if (out) *out = nullptr;
    RC_TRY(check_arguments(fam_offsets, n_families, sds, flags, chr, chr_pos, n_sd, tables, options, out));
    RC_TRY(use_device("asgart_slice_families", device));
    return run_tool<SliceWork>(out, [&](SliceWork &w, asgart_slice *res) {
        return run_slice(w, res, fam_offsets, (uint32_t)n_families, sds, flags, chr, chr_pos, (uint32_t)n_sd, tables, *options);
    });
}

extern "C" void asgart_slice_counts(const asgart_slice *r, uint64_t *n_families, uint64_t *n_sds) {
    if (n_families) *n_families = r ? r->offs.size() - 1 : 0;
    if (n_sds) *n_sds = r ? r->sds.size() : 0;
}

extern "C" void asgart_slice_copy(const asgart_slice *r, uint64_t *fam_offsets, asgart_proto_sd *sds, int32_t *chr,
                                  uint64_t *chr_pos, uint8_t *flags, int64_t *keys) {
    if (!r) return;
    const size_t n = r->sds.size();
    if (fam_offsets) memcpy(fam_offsets, r->offs.data(), r->offs.size() * 8);
    if (!n) return;
    if (sds) memcpy(sds, r->sds.data(), n * sizeof(asgart_proto_sd));
    if (chr) memcpy(chr, r->chr.data(), n * 8);
    if (chr_pos) memcpy(chr_pos, r->chr_pos.data(), n * 16);
    if (flags) memcpy(flags, r->flags.data(), n);
    if (keys) memcpy(keys, r->keys.data(), n * 8);
}

extern "C" int32_t asgart_slice_timings(const asgart_slice *r, double *ms3) {
    return copy_ms3("asgart_slice_timings", r, ms3);
}

extern "C" void asgart_slice_free(asgart_slice *r) { delete r; }
