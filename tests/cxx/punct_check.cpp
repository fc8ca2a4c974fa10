// Host check of the puncture index arithmetic (vd_punct.h) against an enumeration of the kept positions (never
// against the header's own closed forms): pattern validation, the stage map as the kernel evaluates it (the
// group start's divmod by reciprocal, the lane's small-integer part, for stage offsets 0 .. 95 within a
// group), just below 2^32 too, and punct_len.  Every pattern of period 1 .. 7, random ones of period 8 .. 16.
// Built with hipcc and the host sanitizers by tests/test_punct.py; prints "ok" or the first mismatch.
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>
#include "vd_punct.h"

using namespace vd;

static bool kept(uint32_t mask, uint64_t t, int period) { return (mask >> (t % (uint64_t)period)) & 1u; }

// buffer index of the first value of stage g: kept positions before mother index 2g, by whole periods and a
// loop over the rest
static uint64_t index_of_stage(int period, uint32_t k0, uint32_t k1, uint64_t g)
{
    uint64_t per = 0;
    for (int i = 0; i < period; i++) per += ((k0 >> i) & 1u) + ((k1 >> i) & 1u);
    uint64_t n = g / (uint64_t)period * per;
    for (uint64_t t = g - g % (uint64_t)period; t < g; t++) n += (kept(k0, t, period) ? 1 : 0) + (kept(k1, t, period) ? 1 : 0);
    return n;
}

static int check_stage(int period, uint32_t k0, uint32_t k1, const Punct& p, uint32_t g0, uint32_t s)
{
    const uint64_t g = (uint64_t)g0 + s;
    const PunctIdx e = punct_stage(p, g0, s);
    const bool h0 = kept(k0, g, period), h1 = kept(k1, g, period);
    const uint64_t i0 = index_of_stage(period, k0, k1, g), i1 = i0 + (h0 ? 1 : 0);
    if (e.has0 != h0 || e.has1 != h1 || (h0 && e.idx0 != i0) || (h1 && e.idx1 != i1)) {
        printf("FAIL stage map (%d, 0x%x, 0x%x) g0 %u s %u: got %llu/%d %llu/%d, want %llu/%d %llu/%d\n", period, k0, k1, g0,
               s, (unsigned long long)e.idx0, (int)e.has0, (unsigned long long)e.idx1, (int)e.has1, (unsigned long long)i0,
               (int)h0, (unsigned long long)i1, (int)h1);
        return 1;
    }
    return 0;
}

static int check_pattern(int period, uint32_t k0, uint32_t k1)
{
    if (!punct_valid(period, k0, k1)) { printf("FAIL (%d, 0x%x, 0x%x) rejected\n", period, k0, k1); return 1; }
    const Punct p = punct_make(period, k0, k1);
    // divmod on its own, at the ends of the 32-bit range
    for (uint32_t g : {0u, 1u, 15u, 16u, 17u, 0x7FFFFFFFu, 0x80000000u, 0xFFFFFFF0u, 0xFFFFFFFEu, 0xFFFFFFFFu}) {
        uint32_t q, r;
        punct_divmod(p, g, q, r);
        if (q != g / (uint32_t)period || r != g % (uint32_t)period) { printf("FAIL divmod %u / %d\n", g, period); return 1; }
    }
    // the stage map: every stage 0 .. 2000 as a group start, and through group starts 31 and 95 stages before
    for (uint32_t g = 0; g <= 2000; g++) {
        if (check_stage(period, k0, k1, p, g, 0)) return 1;
        if (g >= 31 && check_stage(period, k0, k1, p, g - 31, 31)) return 1;
        if (g >= 95 && check_stage(period, k0, k1, p, g - 95, 95)) return 1;
    }
    // one group start with all its 96 offsets, at every residue of the period
    for (uint32_t g0 = 4096; g0 < 4096 + (uint32_t)period; g0++)
        for (uint32_t s = 0; s < kPunctSpan; s++)
            if (check_stage(period, k0, k1, p, g0, s)) return 1;
    // just below 2^32 (the entry points stop at kPunctMaxStages; groups read a little past the last stage)
    for (uint32_t g = 0xFFFFFFFFu - 300; g != 0; g++) {  // ends when g wraps to 0
        if (check_stage(period, k0, k1, p, g, 0)) return 1;
        if (check_stage(period, k0, k1, p, g - 95, 95)) return 1;
    }
    // punct_len: kept positions among the first 2 * (inputNum / 2), odd inputNum included
    uint64_t n = 0;  // kept among stages < inputNum / 2, extended as inputNum grows
    uint64_t stages = 0;
    for (uint64_t inputNum = 0; inputNum <= 401; inputNum++) {
        while (stages < inputNum / 2) {
            n += (kept(k0, stages, period) ? 1 : 0) + (kept(k1, stages, period) ? 1 : 0);
            stages++;
        }
        if (inputNum >= 128 && punct_len(p, inputNum) != n) {
            printf("FAIL punct_len (%d, 0x%x, 0x%x) inputNum %llu: got %llu, want %llu\n", period, k0, k1,
                   (unsigned long long)inputNum, (unsigned long long)punct_len(p, inputNum), (unsigned long long)n);
            return 1;
        }
    }
    // ... and consistent with the stage map at a large size: the index of the first stage past the data
    const uint64_t big = 2ull * 4000000123ull + 1;
    if (punct_len(p, big) != index_of_stage(period, k0, k1, big / 2)) { printf("FAIL punct_len at %llu\n", (unsigned long long)big); return 1; }
    return 0;
}

int main()
{
    // validation
    if (punct_valid(0, 0, 0) || punct_valid(0, 1, 1) || punct_valid(17, 1, 1) || punct_valid(-1, 1, 1) || punct_valid(3, 0, 0) ||
        punct_valid(3, 0x8, 0x1) || punct_valid(3, 0x1, 0x8) || punct_valid(16, 0x10000, 1) || !punct_valid(16, 0x8001, 0x7ffe) ||
        !punct_valid(1, 1, 1) || !punct_valid(1, 0, 1) || !punct_valid(3, 0, 2)) {
        printf("FAIL punct_valid\n");
        return 1;
    }
    long npat = 0;
    for (int period = 1; period <= 7; period++)
        for (uint32_t k0 = 0; k0 < (1u << period); k0++)
            for (uint32_t k1 = 0; k1 < (1u << period); k1++) {
                if (!(k0 | k1)) continue;
                if (check_pattern(period, k0, k1)) return 1;
                npat++;
            }
    std::mt19937 rng(12345);
    for (int period = 8; period <= 16; period++)
        for (int i = 0; i < 12; i++) {
            const uint32_t all = (1u << period) - 1u;
            uint32_t k0 = rng() & all, k1 = rng() & all;
            if (i == 0) { k0 = all; k1 = all; }
            if (i == 1) { k0 = 1u << (period - 1); k1 = 0; }
            if (!(k0 | k1)) k1 = 1;
            if (check_pattern(period, k0, k1)) return 1;
            npat++;
        }
    if (check_pattern(16, 0x8001, 0x7ffe)) return 1;
    if (npat != 21837 + 9 * 12) { printf("FAIL %ld patterns\n", npat); return 1; }
    printf("ok\n");
    return 0;
}
