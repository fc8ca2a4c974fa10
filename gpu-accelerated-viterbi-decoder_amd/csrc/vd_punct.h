// vd_punct.h -- index arithmetic of punctured streams (host and device, no HIP runtime calls).
//
// A puncture pattern (period, keep0, keep1): bit i of keep0 says that the first encoder output (0171, mother
// index 2t) of every stage t with t % period == i was transmitted, keep1 the same for the second output
// (0133, mother index 2t + 1).  The received buffer holds the kept values in mother order.  With
// Kp = popc(keep0) + popc(keep1) kept values per period, stage g = q * period + r has its values at
//   idx0 = q * Kp + popc(keep0 & low(r)) + popc(keep1 & low(r)),   idx1 = idx0 + ((keep0 >> r) & 1),
// low(r) = (1 << r) - 1, each present when its keep bit r is set.  A punctured value decodes as +0.0f: code 0
// of SOFT4 / SOFT8 / SOFT16 / FP32, which adds 0 to all four branch metrics of its stage.
//
// The decode kernel (vd_kernel_tg.h, channel ids kPun + format) splits the map in two: the wave-uniform
// (q0, r0) of a group's first stage g0 by punct_divmod (a 32-bit reciprocal multiply and one correction,
// scalar unit), and per lane the stage g0 + s, s < kPunctSpan, relative to float q0 * Kp by punct_rel
// (16-bit reciprocal, small integers).  punct_stage composes the two; tests/cxx/punct_check.cpp checks them
// against an enumeration of the kept positions.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define VD_PUNCT_HD __host__ __device__ inline
#else
#define VD_PUNCT_HD inline
#endif

namespace vd {

constexpr int kPunctMaxPeriod = 16;
constexpr uint32_t kPunctSpan = 96;  // punct_rel: stages past the group's first one (a 96-stage group)
// Stage indices are 32-bit.  A decode reads groups up to a few hundred stages past its last one, so the
// entry points reject inputNum / 2 above kPunctMaxStages.
constexpr uint64_t kPunctMaxStages = 0xFFFFFFFFull - 4096;

struct Punct {
    uint32_t period = 0;  // 0: not punctured
    uint32_t keep0 = 0, keep1 = 0;
    uint32_t kp = 0;      // kept values per period
    uint32_t recip = 0;   // min(floor(2^32 / period), 2^32 - 1)
    uint32_t m16 = 0;     // floor(2^16 / period) + 1
};

VD_PUNCT_HD uint32_t punct_popc(uint32_t x) { return (uint32_t)__builtin_popcount(x); }
VD_PUNCT_HD uint32_t punct_low(uint32_t r) { return (1u << r) - 1u; }  // r <= 16

VD_PUNCT_HD bool punct_valid(int period, uint32_t keep0, uint32_t keep1)
{
    if (period < 1 || period > kPunctMaxPeriod) return false;
    const uint32_t all = punct_low((uint32_t)period);
    if ((keep0 | keep1) & ~all) return false;
    return (keep0 | keep1) != 0;
}

// of a valid pattern
VD_PUNCT_HD Punct punct_make(int period, uint32_t keep0, uint32_t keep1)
{
    Punct p;
    p.period = (uint32_t)period;
    p.keep0 = keep0;
    p.keep1 = keep1;
    p.kp = punct_popc(keep0) + punct_popc(keep1);
    p.recip = period == 1 ? 0xFFFFFFFFu : (uint32_t)(0x100000000ull / (uint32_t)period);
    p.m16 = 65536u / (uint32_t)period + 1u;
    return p;
}

// kept values before position r of a period (r <= period)
VD_PUNCT_HD uint32_t punct_before(const Punct& p, uint32_t r)
{
    return punct_popc(p.keep0 & punct_low(r)) + punct_popc(p.keep1 & punct_low(r));
}

// g = q * period + r for any 32-bit g.  recip * period = 2^32 - e with 0 <= e <= period, so
// g * recip / 2^32 lies in (g / period - 1, g / period]: the estimate is floor(g / period) or one below.
VD_PUNCT_HD void punct_divmod(const Punct& p, uint32_t g, uint32_t& q, uint32_t& r)
{
    q = (uint32_t)(((uint64_t)g * p.recip) >> 32);
    r = g - q * p.period;
    if (r >= p.period) {
        q += 1;
        r -= p.period;
    }
}

// The two values of stage g0 + s (s < kPunctSpan) as float indices relative to q0 * Kp, r0 = g0 % period.
// x = r0 + s < 112: m16 * period = 2^16 + e with 0 < e <= period, so x * m16 / 2^16 = x / period + x e /
// (period 2^16) with x e < 2^16: the floor is floor(x / period).
struct PunctRel {
    uint32_t i0, i1;  // float indices (meaningful where has0 / has1)
    uint32_t has0, has1;  // 0 / 1
};
VD_PUNCT_HD PunctRel punct_rel(const Punct& p, uint32_t r0, uint32_t s)
{
    const uint32_t x = r0 + s;
    const uint32_t dq = (x * p.m16) >> 16;
    const uint32_t r = x - dq * p.period;
    PunctRel e;
    e.has0 = (p.keep0 >> r) & 1u;
    e.has1 = (p.keep1 >> r) & 1u;
    e.i0 = dq * p.kp + punct_before(p, r);
    e.i1 = e.i0 + e.has0;
    return e;
}

// the map as the kernel evaluates it: stage g0 + s through the group start g0
struct PunctIdx {
    uint64_t idx0, idx1;
    bool has0, has1;
};
VD_PUNCT_HD PunctIdx punct_stage(const Punct& p, uint32_t g0, uint32_t s = 0)
{
    uint32_t q0, r0;
    punct_divmod(p, g0, q0, r0);
    const PunctRel e = punct_rel(p, r0, s);
    const uint64_t base = (uint64_t)q0 * p.kp;
    return {base + e.i0, base + e.i1, e.has0 != 0, e.has1 != 0};
}

// received values of inputNum mother-code values: the kept positions among the first 2 * (inputNum / 2)
VD_PUNCT_HD uint64_t punct_len(const Punct& p, uint64_t inputNum)
{
    const uint64_t stages = inputNum / 2;
    return stages / p.period * p.kp + punct_before(p, (uint32_t)(stages % p.period));
}

}  // namespace vd
