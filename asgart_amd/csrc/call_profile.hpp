// call_profile.hpp -- the diagnostic build's per-phase dumps of the extension kernels' cycle counters (make diag:
// ASGART_PROFILE_EXTEND); nothing in the shipped library.  The macros expand inside SearchCall's stages and use its
// members (h_ctr, d_ctr, s).
#pragma once

#ifdef ASGART_PROFILE_EXTEND
#define PROF_DUMP(tag)                                                                          \
    do {                                                                                       \
        fprintf(stderr, "[extend profile %s] stage=%llu batches=%llu | reg_cyc=%llu reg_probes=%llu | build=%llu "\
                "lds_probes=%llu match=%llu apply=%llu retire=%llu segs=%llu sumA=%llu sumCnt=%llu | longest: "   \
                "cyc=%llu g0=%llu lds_probes=%llu reg_probes=%llu sumA=%llu sumCnt=%llu stage=%llu match=%llu\n", \
                tag, h_ctr[16], h_ctr[17], h_ctr[18], h_ctr[19], h_ctr[20], h_ctr[21], h_ctr[22], h_ctr[23],  \
                h_ctr[24], h_ctr[25], h_ctr[26], h_ctr[27], h_ctr[28], h_ctr[29], h_ctr[30] >> 32,            \
                h_ctr[30] & 0xffffffffull, h_ctr[31] >> 32, h_ctr[31] & 0xffffffffull, h_ctr[32], h_ctr[33]); \
        fprintf(stderr, "    K7 steps=%llu; cycles [to barrier 1, wait, to barrier 2, wait]: control %llu %llu %llu %llu | arm wave 0 %llu %llu %llu %llu | last arm wave %llu %llu %llu %llu\n", \
                h_ctr[52], h_ctr[40], h_ctr[41], h_ctr[42], h_ctr[43], h_ctr[44], h_ctr[45], h_ctr[46], h_ctr[47], h_ctr[48], h_ctr[49], h_ctr[50], h_ctr[51]); \
        fprintf(stderr, "    K7 wave 0: extra row rounds %llu, stash rounds %llu, arms offered cooperatively %llu, resolved cooperatively %llu\n", h_ctr[53], h_ctr[56], h_ctr[54], h_ctr[55]); \
        fprintf(stderr, "    K7 wave 0 cycles: A[cmd %llu resolve %llu offers %llu] B[mid %llu create+offers %llu publish %llu next-cmd+index %llu]\n", h_ctr[57], h_ctr[58], h_ctr[59], h_ctr[60], h_ctr[61], h_ctr[62], h_ctr[63]); \
        (void)hipMemsetAsync(d_ctr + 52, 0, 13 * 8, s);                                        \
        fprintf(stderr, "    P1: arm lookups=%llu linear=%llu chain nodes=%llu accepts=%llu by level:", h_ctr[40], h_ctr[41], h_ctr[42], h_ctr[43]); \
        for (int pf_i = 0; pf_i < 8; ++pf_i) fprintf(stderr, " %llu", h_ctr[44 + pf_i]);       \
        fprintf(stderr, "\n");                                                                 \
        (void)hipMemsetAsync(d_ctr + 40, 0, 12 * 8, s);                                        \
        fprintf(stderr, "    longest slots:");                                                  \
        for (int pf_i = 0; pf_i < 12; ++pf_i) fprintf(stderr, " [%d]=%llu", pf_i, h_ctr[56 + pf_i]); \
        fprintf(stderr, "\n");                                                                 \
        fprintf(stderr, "    segments by peak arms (log2 bins):");                             \
        for (int pf_i = 0; pf_i < 16; ++pf_i) fprintf(stderr, " %llu", h_ctr[CT_HIST_PEAK + pf_i]); \
        fprintf(stderr, "\n    probes by segment length (log2 bins):");                        \
        for (int pf_i = 0; pf_i < 16; ++pf_i) fprintf(stderr, " %llu", h_ctr[CT_HIST_PROBES + pf_i]); \
        fprintf(stderr, "\n");                                                                 \
        (void)hipMemsetAsync(d_ctr + 16, 0, 18 * 8, s);                                        \
        (void)hipMemsetAsync(d_ctr + 56, 0, (CT_N1 - 56) * 8, s);                              \
    } while (0)
// one tier at a time, with its own dump (the diagnostic build gives up the overlap)
#define PROF_TIER(tag, stream, n)                                                               \
    do {                                                                                       \
        const auto pf_c0 = std::chrono::steady_clock::now();                                   \
        (void)hipStreamSynchronize(stream);                                                    \
        const double pf_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - pf_c0).count(); \
        (void)hipMemcpy(h_ctr, d_ctr, kCtrBytes, hipMemcpyDeviceToHost);                   \
        fprintf(stderr, "[tier %s] segments=%llu  %.2f ms\n", tag, (unsigned long long)(n), pf_ms); \
        PROF_DUMP(tag);                                                                        \
        (void)hipStreamSynchronize(s);                                                         \
    } while (0)
#else
#define PROF_DUMP(tag)
#define PROF_TIER(tag, stream, n)
#endif
