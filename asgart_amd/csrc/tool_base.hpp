// tool_base.hpp -- what the result tools (slice.hip, plot.hip, rosary.hip, groups.hip, mask.hip, chain.hip, alnstats.hip and, through
// file_writer.hpp, the file writers export.hip, paf.hip, sdtable.hip and fasta_write.hip) are built on: the device check of an entry point,
// the device work of one call (ToolWork: stream, events, every device buffer, the rocPRIM two-call wrappers), the host checks of offset arrays and name ids, the bisection of an offset array on the device, and the tail of an entry
// point.  extract.hip, fasta.hip and prep.hip take use_device from here.
//
// The arm tools (rosary.hip, groups.hip, chain.hip, mask.hip) share their frame as well.  An ordering is a chain of
// ToolWork::order_pass calls, one stable radix sort of the ordinals per key, the least significant key first; the key of a
// pass is a device functor of the tool's, gathered through the order so far by order_keys_kernel.  CSR rows come from
// first_at_least, a bisection of a sorted key column, and where nothing else is computed per row from row_offsets_kernel.
// The host tail is bits_for, ToolWork::fetch, give and the three figures of ToolWork::start_copy_back / figures.
#pragma once

#include "common.hpp"

#include <algorithm>
#include <deque>
#include <type_traits>

#include <rocprim/rocprim.hpp>

namespace asgart {

inline int32_t use_device(const char *who, int32_t device) {
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || device < 0 || device >= n_dev) {
        (void)hipGetLastError();
        set_error("%s: no usable device %d (there is no CPU fallback)", who, device);
        return ASGART_E_HIP;
    }
    HIP_TRY(hipSetDevice(device));
    return 0;
}

inline unsigned blocks_for(uint64_t items, uint32_t block = 256) { return (unsigned)((items + block - 1) / block); }

// the bits of a radix sort whose keys are below `values`: ceil(log2(values)), at least one, at most 32
inline unsigned bits_for(uint64_t values) {
    unsigned bits = 1;
    while (bits < 32 && ((uint64_t)1 << bits) < values) ++bits;
    return bits;
}

// ---- the segmented running maximum of groups.hip (loci: key = the name) and chain.hip (segments: key = the packed group) ----
// Record i of a sequence sorted by (key, start): its key and its end.  ToolWork::segmented_max_scan turns the ends into the
// largest end of record i and of every earlier record of its key; a record then opens a piece iff it is the first of its
// key or its start lies beyond sat(that maximum in front of it + margin).
template <class Key>
struct KeyEnd {
    uint64_t end;
    Key key;
};

// the running maximum of the ends within a key; associative where the keys never decrease from left to right
template <class Key>
struct SegmentedMax {
    __host__ __device__ KeyEnd<Key> operator()(const KeyEnd<Key> &a, const KeyEnd<Key> &b) const {
        KeyEnd<Key> r = b;
        if (a.key == b.key && a.end > b.end) r.end = a.end;
        return r;
    }
};

__host__ __device__ inline uint64_t sat_add(uint64_t a, uint64_t b) {
    const uint64_t s = a + b;
    return s < a ? ~(uint64_t)0 : s;
}

// ---- the ordering and the rows of the arm tools ----
// the first entry of keys[0 .. n), which never decrease, that is >= k; n where there is none
template <class Key>
__host__ __device__ inline uint32_t first_at_least(const Key *__restrict__ keys, uint32_t n, uint64_t k) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if ((uint64_t)keys[mid] < k) lo = mid + 1; else hi = mid;
    }
    return lo;
}

struct KeyGiven {};  // the key_of of a pass whose key column stands in memory already: only the ordinals are numbered
enum OrderSoFar { kNoOrder, kOrdered };  // a tool's first pass numbers the ordinals, every later one reads them

struct ArmName {  // the key "name of arm o" of rosary.hip and groups.hip (the host has checked: ids are not negative)
    const int32_t *__restrict__ name;
    __device__ uint32_t operator()(uint32_t o) const { return (uint32_t)name[o]; }
};

namespace {  // (internal, and templates: a file holds the instances it launches and links its own)

// The keys of one sort pass: key[i] = key_of(the record at slot i of the order so far).  Without an order so far that
// record is i, and ord[i] = i is written for the sort to carry.
template <uint32_t kThreads, class Key, class KeyOf>
__global__ __launch_bounds__(kThreads) void order_keys_kernel(KeyOf key_of, uint32_t *ord, OrderSoFar so_far, uint32_t n,
                                                              Key *__restrict__ key) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    uint32_t o = i;
    if (so_far == kOrdered) o = ord[i]; else ord[i] = i;
    if constexpr (!std::is_same<KeyOf, KeyGiven>::value) key[i] = key_of(o);
}

// offsets[k], k in [0, n_rows]: the first of the *total entries of keys, which never decrease, that is >= k
template <uint32_t kThreads, class Key>
__global__ __launch_bounds__(kThreads) void row_offsets_kernel(const Key *__restrict__ keys,
                                                               const uint32_t *__restrict__ total, uint64_t n_rows,
                                                               uint64_t *__restrict__ offsets) {
    const uint64_t k = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (k <= n_rows) offsets[k] = first_at_least(keys, *total, k);
}

}  // namespace

// what a handle's vector gives the caller's array (NULL: the caller does not want it)
template <class T>
void give(T *to, const std::vector<T> &from) {
    if (to && !from.empty()) memcpy(to, from.data(), from.size() * sizeof(T));
}

// The device work of one call: one non-blocking stream, its events and every device buffer the call uses.  A tool derives
// from it and names each of its buffers once, as a reference that buf() hands out; the destructor is the only place where
// they are released, so a call that returns early (a refusal after the launches, a failed allocation) leaves nothing.
struct ToolWork {
    hipStream_t s = nullptr;
    std::vector<hipEvent_t> ev;
    std::deque<DevBuf> bufs;  // (a deque: the references handed out stay valid while it grows)
    DevBuf &scan_tmp = buf(), &sort_tmp = buf();  // rocPRIM's scratch

    ToolWork() = default;
    ToolWork(const ToolWork &) = delete;
    ToolWork &operator=(const ToolWork &) = delete;
    ~ToolWork() {
        if (s) (void)hipStreamSynchronize(s);  // nothing is released under a kernel that still runs
        for (DevBuf &b : bufs) b.release();
        // (a released block of 256 MiB and more is kept for the next index build; without an index alive nobody wants it)
        if (BlockCache::live_indexes() == 0) BlockCache::trim();
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
        if (s) (void)hipStreamDestroy(s);
    }

    DevBuf &buf() {
        bufs.emplace_back();
        return bufs.back();
    }
    int32_t open(size_t n_events) {
        HIP_TRY(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
        ev.assign(n_events, nullptr);
        for (hipEvent_t &e : ev) HIP_TRY(hipEventCreate(&e));
        return 0;
    }
    int32_t upload(DevBuf &b, const void *src, size_t bytes) {
        RC_TRY(b.reserve(std::max<size_t>(bytes, 16)));
        if (bytes) HIP_TRY(hipMemcpyAsync(b.p, src, bytes, hipMemcpyHostToDevice, s));
        return 0;
    }
    // rocPRIM's two calls each: size query, scratch reserved, run.  (Templates all three: a file gets the rocPRIM kernels
    // of what it calls and no others.)
    template <class T>
    int32_t exclusive_scan(const T *in, T *out, size_t items) {
        size_t tmp = 0;
        HIP_TRY(rocprim::exclusive_scan(nullptr, tmp, in, out, (T)0, items, rocprim::plus<T>(), s));
        RC_TRY(scan_tmp.reserve(tmp + 16));
        HIP_TRY(rocprim::exclusive_scan(scan_tmp.p, tmp, in, out, (T)0, items, rocprim::plus<T>(), s));
        return 0;
    }
    template <class Key>
    int32_t segmented_max_scan(const KeyEnd<Key> *in, KeyEnd<Key> *out, size_t items) {
        size_t tmp = 0;
        HIP_TRY(rocprim::inclusive_scan(nullptr, tmp, in, out, items, SegmentedMax<Key>(), s));
        RC_TRY(scan_tmp.reserve(tmp + 16));
        HIP_TRY(rocprim::inclusive_scan(scan_tmp.p, tmp, in, out, items, SegmentedMax<Key>(), s));
        return 0;
    }
    template <class K>
    int32_t sort_keys(const K *in, K *out, size_t items) {
        size_t tmp = 0;
        HIP_TRY(rocprim::radix_sort_keys(nullptr, tmp, in, out, items, 0, 8 * sizeof(K), s));
        RC_TRY(sort_tmp.reserve(tmp + 16));
        HIP_TRY(rocprim::radix_sort_keys(sort_tmp.p, tmp, in, out, items, 0, 8 * sizeof(K), s));
        return 0;
    }
    template <class K>
    int32_t sort_pairs(const K *k_in, K *k_out, const uint32_t *v_in, uint32_t *v_out, size_t items, unsigned end_bit) {
        size_t tmp = 0;
        HIP_TRY(rocprim::radix_sort_pairs(nullptr, tmp, k_in, k_out, v_in, v_out, items, 0, end_bit, s));
        RC_TRY(sort_tmp.reserve(tmp + 16));
        HIP_TRY(rocprim::radix_sort_pairs(sort_tmp.p, tmp, k_in, k_out, v_in, v_out, items, 0, end_bit, s));
        return 0;
    }
    // One pass of an ordering: the n ordinals of ord, in the order so far, sorted stably into ord_out by the low end_bit
    // bits of key_of(record); the sorted keys land in sorted_key.  A later pass is the more significant key.
    template <class Key, uint32_t kThreads = 256, class KeyOf>
    int32_t order_pass(KeyOf key_of, DevBuf &key, DevBuf &sorted_key, DevBuf &ord, OrderSoFar so_far, DevBuf &ord_out,
                       uint32_t n, unsigned end_bit) {
        order_keys_kernel<kThreads><<<blocks_for(n, kThreads), kThreads, 0, s>>>(key_of, ord.as<uint32_t>(), so_far, n,
                                                                                 key.as<Key>());
        HIP_TRY(hipGetLastError());
        return sort_pairs(key.as<Key>(), sorted_key.as<Key>(), ord.as<uint32_t>(), ord_out.as<uint32_t>(), n, end_bit);
    }

    // the first `items` entries of a device buffer into a vector of the handle (waited for by the caller's stream_sync)
    template <class T>
    int32_t fetch(std::vector<T> &to, const DevBuf &from, size_t items) {
        to.resize(items);
        if (items) HIP_TRY(hipMemcpyAsync(to.data(), from.p, items * sizeof(T), hipMemcpyDeviceToHost, s));
        return 0;
    }

    // The three figures of an arm tool, which records ev[0] before its upload, ev[1] before its first kernel and ev[2]
    // behind its last: ms[0] the upload, ms[1] the kernels, ms[2] the copy back by the host's clock, from start_copy_back
    // to figures, which is called once the stream is drained.
    std::chrono::steady_clock::time_point copy_back_from;
    void start_copy_back() { copy_back_from = std::chrono::steady_clock::now(); }
    int32_t figures(double *ms) {
        ms[2] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - copy_back_from).count();
        float up = 0, kernels = 0;
        HIP_TRY(hipEventElapsedTime(&up, ev[0], ev[1]));
        HIP_TRY(hipEventElapsedTime(&kernels, ev[1], ev[2]));
        ms[0] = (double)up;
        ms[1] = (double)kernels;
        return 0;
    }
};

// offs[0 .. n_seg] are the offsets of n_seg segments over n_items items: from 0 to n_items, never decreasing
inline int32_t check_csr(const char *who, const char *name, const uint64_t *offs, int64_t n_seg, int64_t n_items,
                         const char *items_name, const char *seg_name = "family") {
    if (offs[0] != 0 || offs[n_seg] != (uint64_t)n_items) {
        set_error("%s: %s must start at 0 and end at %s = %lld (they run from %llu to %llu)", who, name, items_name,
                  (long long)n_items, (unsigned long long)offs[0], (unsigned long long)offs[n_seg]);
        return ASGART_E_ARG;
    }
    for (int64_t f = 0; f < n_seg; ++f)
        if (offs[f] > offs[f + 1]) {
            set_error("%s: %s decrease at %s %lld", who, name, seg_name, (long long)f);
            return ASGART_E_ARG;
        }
    return 0;
}

// both name ids of every duplication are rows of the name table
inline int32_t check_name_ids(const char *who, const int32_t *chr, int64_t n_sd, int64_t n_names) {
    for (int64_t q = 0; q < 2 * n_sd; ++q)
        if (chr[q] < 0 || chr[q] >= n_names) {
            set_error("%s: duplication %lld has name id %d, outside the name table (%lld names)", who, (long long)(q / 2),
                      chr[q], (long long)n_names);
            return ASGART_E_ARG;
        }
    return 0;
}

// the name table of the file writers: offsets from 0, never decreasing, below 2^30 bytes of names
inline int32_t check_name_table(const char *who, const uint8_t *name_bytes, const uint64_t *name_offsets, int64_t n_names) {
    if (name_offsets[0] != 0 || (name_offsets[n_names] && !name_bytes) || name_offsets[n_names] >= ((uint64_t)1 << 30)) {
        set_error("%s: name_offsets must start at 0 and end below 2^30 bytes of names", who);
        return ASGART_E_ARG;
    }
    for (int64_t k = 0; k < n_names; ++k)
        if (name_offsets[k] > name_offsets[k + 1]) {
            set_error("%s: name_offsets decrease at name %lld", who, (long long)k);
            return ASGART_E_ARG;
        }
    return 0;
}

// The duplications with a row (status != 0) of the PAF and table writers -> kept: each has a strand (flag 0 or 3), and
// neither of its positions + lengths wraps.
inline int32_t check_strand_rows(const char *who, const asgart_proto_sd *sds, const uint8_t *flags, const uint8_t *status,
                                 const uint64_t *chr_pos, int64_t n_sd, std::vector<uint32_t> &kept) {
    for (int64_t q = 0; q < n_sd; ++q) {
        if (!status[q]) continue;
        if (flags[q] != 0 && flags[q] != 3) {
            set_error("%s: duplication %lld has flag byte %u: a PAF row has a strand for 0 (direct, +) and 3 (reversed and "
                      "complemented, -) only", who, (long long)q, (unsigned)flags[q]);
            return ASGART_E_ARG;
        }
        for (int arm = 0; arm < 2; ++arm) {
            const uint64_t pos = chr_pos[2 * q + arm], len = arm ? sds[q].right_length : sds[q].left_length;
            if (pos + len < pos) {
                set_error("%s: duplication %lld: position %llu + length %llu wraps past 2^64", who, (long long)q,
                          (unsigned long long)pos, (unsigned long long)len);
                return ASGART_E_ARG;
            }
        }
        kept.push_back((uint32_t)q);
    }
    return 0;
}

// The tail of an entry point: the result is allocated, run(work, result) fills it, the work is gone (stream drained,
// buffers released) before the caller sees the result, and a failed call leaves no result.
template <class Work, class Result, class Run>
int32_t run_tool(Result **out, Run run) {
    std::unique_ptr<Result> res(new Result);
    {
        Work w;
        RC_TRY(run(w, res.get()));
    }
    *out = res.release();
    return 0;
}

// the three millisecond figures of a result handle (what they mean is the tool's business)
template <class Result>
int32_t copy_ms3(const char *who, const Result *r, double *ms3) {
    if (!r || !ms3) {
        set_error("%s: bad argument", who);
        return ASGART_E_ARG;
    }
    for (int k = 0; k < 3; ++k) ms3[k] = r->ms[k];
    return 0;
}

// largest f in [0, n_seg) with offs[f] <= i < offs[f + 1] (empty segments are stepped over); n_seg >= 1, i < offs[n_seg]
__device__ inline uint32_t segment_of(const uint64_t *__restrict__ offs, uint32_t n_seg, uint32_t i) {
    uint32_t lo = 0, hi = n_seg;  // first f in [0, n_seg] with offs[f] > i; offs[n_seg] > i
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (offs[mid] > i) hi = mid; else lo = mid + 1;
    }
    return lo - 1;
}

namespace {  // (internal: slice.hip and plot.hip each get their own and link into one library)

// out_offs[k] of the k-th kept family = the rank of its first duplication; thread n_fam writes the closing entry.  A template
// of the launch's block size, so that only a file that launches it holds it.
template <uint32_t kThreads>
__global__ __launch_bounds__(kThreads) void family_offsets_kernel(const uint64_t *__restrict__ offs, uint32_t n_fam,
                                                                  uint32_t n, const uint32_t *__restrict__ rank,
                                                                  const uint32_t *__restrict__ kept,
                                                                  const uint32_t *__restrict__ fam_rank,
                                                                  uint64_t *__restrict__ out_offs) {
    const uint32_t f = blockIdx.x * kThreads + threadIdx.x;
    if (f > n_fam) return;
    if (f == n_fam)
        out_offs[fam_rank[n_fam]] = rank[n];
    else if (kept[f])
        out_offs[fam_rank[f]] = rank[offs[f]];
}

}  // namespace

}  // namespace asgart
