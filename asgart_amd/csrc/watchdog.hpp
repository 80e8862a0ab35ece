// watchdog.hpp -- the waits of a search call: blocking, or with option watchdog_s polled under the heartbeats' watch.
#pragma once
#include "index.hpp"

#include <chrono>
#include <string>
#include <thread>

namespace asgart {

// Waits for everything queued on stream `st`.  With option watchdog_s > 0 the wait polls: while the heartbeat block of
// the call's extension workgroups keeps changing the device is making progress, however long it takes; a wait that
// outlasts watchdog_s seconds without any change gives up: the call returns ASGART_E_HIP naming the phase and the
// workgroups that were in flight, and the index refuses further calls (its streams may still hold the stuck work) --
// the host should report and exit, or go on in a fresh process.  (One GPU test run of round 3 sat in a call for 40
// minutes with nothing to tell where.)
struct Watchdog {
    asgart_index *idx;
    SearchCtx &cx;
    std::chrono::steady_clock::time_point t0, t_change;
    unsigned long long sig = 0;
    Watchdog(asgart_index *i, SearchCtx &c) : idx(i), cx(c), t0(std::chrono::steady_clock::now()), t_change(t0) {}
    unsigned long long signature() const {
        unsigned long long h = 1469598103934665603ull;
        if (cx.h_hb) {
            const volatile unsigned long long *p = cx.h_hb;
            for (int i = 0; i < SearchCtx::kHbTiers * SearchCtx::kHbSlots * 2; ++i) h = (h ^ p[i]) * 1099511628211ull;
        }
        return h;
    }
    // One look at the heartbeats (never blocks).  true: nothing has changed for watchdog_s seconds -- the error is set and
    // the index poisoned; the caller returns ASGART_E_HIP.
    bool expired(const char *phase) {
        const int64_t limit_s = idx->opt.watchdog_s;
        if (limit_s <= 0) return false;
        const auto now = std::chrono::steady_clock::now();
        const unsigned long long s2 = signature();
        if (s2 != sig) {
            sig = s2;
            t_change = now;
        }
        if (std::chrono::duration<double>(now - t_change).count() <= (double)limit_s) return false;
        std::string who;
        if (cx.h_hb) {
            int shown = 0;
            for (int t = 0; t < SearchCtx::kHbTiers && shown < 12; ++t)
                for (int w = 0; w < SearchCtx::kHbSlots && shown < 12; ++w) {
                    const unsigned long long a = cx.h_hb[2 * (t * SearchCtx::kHbSlots + w)], b = cx.h_hb[2 * (t * SearchCtx::kHbSlots + w) + 1];
                    if (!(a >> 63)) continue;
                    char buf[96];
                    snprintf(buf, sizeof buf, "%s tier %d wg %d: segment at probe %llu, position %llu", shown ? ";" : "", t, w,
                             a & 0xFFFFFFFFull, b);
                    who += buf;
                    ++shown;
                }
        }
        idx->poisoned.store(true);
        set_error("watchdog: no progress for %lld s while waiting for %s (%.1f s into the wait); last heartbeats:%s -- the index is "
                  "unusable from here on (option watchdog_s = 0 waits forever)", (long long)limit_s, phase,
                  std::chrono::duration<double>(now - t0).count(), who.empty() ? " none" : who.c_str());
        return true;
    }
};

// The polled wait: query() is hipStreamQuery or hipEventQuery of what is waited for.
template <class Query>
static int32_t polled_wait(asgart_index *idx, SearchCtx &cx, const char *phase, Query query) {
    Watchdog wd(idx, cx);
    for (unsigned spins = 0;; ++spins) {
        const hipError_t q = query();
        if (q == hipSuccess) return 0;
        if (q != hipErrorNotReady) HIP_TRY(q);
        (void)hipGetLastError();
        if (spins < 64) continue;                    // (short waits: no sleep at all)
        std::this_thread::sleep_for(std::chrono::microseconds(spins < 2000 ? 20 : 500));
        if ((spins & 1023u) == 0 && wd.expired(phase)) return ASGART_E_HIP;
    }
}
static int32_t wd_sync(asgart_index *idx, SearchCtx &cx, hipStream_t st, const char *phase) {
    if (idx->opt.watchdog_s > 0) return polled_wait(idx, cx, phase, [st] { return hipStreamQuery(st); });
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}
// ... for an event (a stream may have more queued behind it)
static int32_t wd_event_sync(asgart_index *idx, SearchCtx &cx, hipEvent_t ev, const char *phase) {
    if (idx->opt.watchdog_s > 0) return polled_wait(idx, cx, phase, [ev] { return hipEventQuery(ev); });
    HIP_TRY(hipEventSynchronize(ev));
    return 0;
}

}  // namespace asgart
