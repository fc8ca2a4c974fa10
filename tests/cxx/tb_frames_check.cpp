// Host check of the tail-biting frame geometry (vd_frames.h "tail-biting frames") and its plan (vd_plan.h) against a
// plain enumeration of the extended stream (never against the header's own closed forms): for every S in 1 .. 300
// and at 2^20 - 1 and 2^20, every group start the decode of the frame reaches and the one it prefetches beyond, and
// all 96 stages of each group: the load offset is 8 ((p - 26) mod S) with the residue found by stepping, its end
// lies inside the frame's 8 S bytes, the uniform "this group wraps" predicate says exactly whether some lane leaves
// the unwrapped line 8 (p - 26), the scalar first-stage residue and the lane reduction agree with the stepping; the
// reciprocals' bounds as stated; the argument checks; the grids of plan_frames, the kernel name and the kernel
// table of launcher_frames (the tail-biting family).
// Built with hipcc and the host sanitizers by tests/test_tb_frames.py; prints "ok" or the first mismatch.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <string>
#include "vd_kernel_tg.h"
#include "vd_plan.h"
#include "frame_args.h"

using namespace vd;

struct Stub {
    using fn = void (*)();
    template <int CH, int CORE, int OB> static void tg() {}
    template <int CH, int CORE, int OB, bool SPL> static void pk() {}
};

static int check_frame(uint32_t S)
{
    uint32_t W = 0;
    while (32 * W < S) W++;
    // the decode runs W + 2 blocks of 32 stages in groups of 3, and every group head loads the next group:
    // group starts 0, 96, ... up to the one after the last group run
    const uint32_t lastRun = (W + 2 - 1) / 3 * 3 * 32, nst = lastRun + 2 * 96;
    const TbRecip rc = tb_recip(S);
    const uint64_t range = 8ull * S;
    // the frame stage of extended stage 0 by stepping back 26 times from stage 26 = frame stage 0
    uint32_t t = 0;
    for (int i = 0; i < 26; i++) t = t == 0 ? S - 1 : t - 1;
    for (uint32_t g0 = 0; g0 + 96 <= nst; g0 += 96) {
        const bool wraps = tb_wrap_group(g0, S);
        bool leaves = false;  // some lane is off the unwrapped line
        if (tb_group_r0(g0, S, rc.m32) != t) {
            printf("FAIL S %u group %u: r0 %u, want %u\n", S, g0, tb_group_r0(g0, S, rc.m32), t);
            return 1;
        }
        const uint32_t r0 = t;
        for (uint32_t s = 0; s < 96; s++) {
            const uint32_t p = g0 + s;
            leaves = leaves || p < 26 || p - 26 != t;
            const uint32_t off = tb_stage_offset(g0, s, S, rc);
            if (off != 8 * t || (uint64_t)off + 8 > range) {
                printf("FAIL S %u stage %u: offset %u, want %u (range %llu)\n", S, p, off, 8 * t, (unsigned long long)range);
                return 1;
            }
            // the wrapped form holds in every group, wrapping or not
            if (tb_lane_stage(r0, s, S, rc.m16) != t) {
                printf("FAIL S %u stage %u: lane stage %u, want %u\n", S, p, tb_lane_stage(r0, s, S, rc.m16), t);
                return 1;
            }
            if (!wraps && tb_offset_inside(g0, s) != 8 * t) {
                printf("FAIL S %u stage %u: unwrapped offset %u, want %u\n", S, p, tb_offset_inside(g0, s), 8 * t);
                return 1;
            }
            t = t + 1 == S ? 0 : t + 1;
        }
        if (wraps != leaves) {
            printf("FAIL S %u group %u: wrap predicate %d, lanes off the line %d\n", S, g0, (int)wraps, (int)leaves);
            return 1;
        }
    }
    return 0;
}

// the reciprocals: m32 and m16 as stated, tb_mod against % over the operands a decode can form and the edges
static int check_recip(uint32_t S)
{
    const TbRecip rc = tb_recip(S);
    if (rc.m32 != (uint32_t)(0xFFFFFFFFull / S)) { printf("FAIL m32 of %u\n", S); return 1; }
    if (S < 96) {
        const uint32_t e = rc.m16 * S - 65536u;  // 0 <= e <= S
        if ((uint64_t)rc.m16 * S < 65536u || e > S || rc.m16 >= (1u << 24)) { printf("FAIL m16 of %u: %u\n", S, rc.m16); return 1; }
        for (uint32_t x = 0; x < 192; x++)
            if (((x * rc.m16) >> 16) != x / S) { printf("FAIL S %u: %u / S by m16\n", S, x); return 1; }
    }
    const uint32_t xs[] = {0u, 1u, S - 1, S, S + 1, 2 * S - 1, 2 * S, 3 * S + 1, (1u << 20) + 400, (1u << 21) - 1, (1u << 31) - 1};
    for (uint32_t x : xs)
        if (tb_mod(x, S, rc.m32) != x % S) { printf("FAIL tb_mod(%u, %u) = %u\n", x, S, tb_mod(x, S, rc.m32)); return 1; }
    for (uint32_t x = 0; x < 4 * S + 500 && x < 4000; x++)
        if (tb_mod(x, S, rc.m32) != x % S) { printf("FAIL tb_mod(%u, %u) = %u\n", x, S, tb_mod(x, S, rc.m32)); return 1; }
    return 0;
}

static int check_args()
{
    struct A {
        uint64_t addr, istr, ostr, maxb;
        int nf;
        float scale;
        bool ok;
    };
    const float inf = std::numeric_limits<float>::infinity();
    const A cases[] = {
        {0, 8000, 128, 1000, 4, 40000.0f, true},
        {8, 8 * 1000, 4 * 32, 1000, 4, 1.0f, true},                   // the smallest strides
        {0, 8 * 1001, 132, 1000, 3, 40000.0f, true},                  // an odd multiple of 8
        {0, 0, 0, 1000, 1, 40000.0f, true},                           // one frame: no stride needed
        {0, 8, 4, 1, 2, 40000.0f, true},
        {0, 8ull << 20, 4ull << 15, 1u << 20, 2, 40000.0f, true},
        {0, 8000, 128, 1000, 4, 1e-30f, true},                        // no pad value to form: any finite scale > 0
        {0, 8000, 128, 1000, 4, 3e38f, true},
        {0, 8000, 128, 0, 4, 40000.0f, false},                        // maxFrameBits
        {0, 16ull << 20, 1ull << 20, (1u << 20) + 1, 4, 40000.0f, false},
        {0, 8000, 128, 1000, 0, 40000.0f, false},                     // nframes
        {0, 8000, 128, 1000, -1, 40000.0f, false},
        {0, 8000, 128, 1000, 4, 0.0f, false},                         // scale
        {0, 8000, 128, 1000, 4, -0.0f, false},
        {0, 8000, 128, 1000, 4, -1.0f, false},
        {0, 8000, 128, 1000, 4, inf, false},
        {0, 8000, 128, 1000, 4, -inf, false},
        {0, 8000, 128, 1000, 4, std::nanf(""), false},
        {4, 8000, 128, 1000, 4, 40000.0f, false},                     // alignment
        {0, 8004, 128, 1000, 4, 40000.0f, false},
        {0, 8000, 130, 1000, 4, 40000.0f, false},
        {0, 7992, 128, 1000, 4, 40000.0f, false},                     // overlapping frames
        {0, 8000, 124, 1000, 4, 40000.0f, false},
        {0, 0, 128, 1000, 2, 40000.0f, false},
    };
    int i = 0;
    for (const A& a : cases) {
        const char* why = check({false, true, false, false}, a.addr, a.istr, a.ostr, a.maxb, a.nf, kByteFramesTailbiting, a.scale);
        if ((why == nullptr) != a.ok) { printf("FAIL argument case %d: %s\n", i, why ? why : "accepted"); return 1; }
        i++;
    }
    return 0;
}

static int check_plan()
{
    const struct { uint64_t n; unsigned grid; } grids[] = {{1, 1}, {3, 1}, {4, 1}, {5, 2}, {8192, 2048}};
    for (auto g : grids) {
        const LaunchPlan p = plan_frames(0x012, g.n);
        if (!p.launches || p.form != Form::Tg || p.grid != g.grid || p.seg != kSegNone || p.stats || p.tailWG != ~0u) {
            printf("FAIL plan_frames(%llu): grid %u, want %u\n", (unsigned long long)g.n, p.grid, g.grid);
            return 1;
        }
        const std::string nm = plan_name(p, 0x012, 5);
        if (nm.rfind("vd_decode_tg<FRM+TB+SOFT8,B16,O32>", 0) != 0) { printf("FAIL name %s\n", nm.c_str()); return 1; }
    }
    if (plan_name(plan_frames(0x012, 0), 0x012, 5) != "-") { printf("FAIL empty plan\n"); return 1; }
    if (plan_name(plan_frames(0x100, 7), 0x100, 5).rfind("vd_decode_tg<FRM+TB+HARD,B32,O16>", 0) != 0) { printf("FAIL name\n"); return 1; }
    // the earlier names stay
    if (plan_name(plan_frames(0x012, 4), 0x012, 3).rfind("vd_decode_tg<FRM+SOFT8,", 0) != 0 ||
        plan_name(plan_frames(0x012, 4), 0x012, 4).rfind("vd_decode_tg<FRM+PUN+SOFT8,", 0) != 0) { printf("FAIL earlier names\n"); return 1; }
    // the table: a kernel exactly for the 12 valid (format, metric) pairs, both output widths
    int n = 0;
    for (int ch = -1; ch <= 5; ch++)
        for (int me = -1; me <= 3; me++)
            for (int o16 = 0; o16 < 2; o16++) {
                const bool want = ch >= 0 && ch < 5 && me >= 0 && me < 3 && has_kernel(Form::Tg, ch, me);
                if ((launcher_frames<Stub>({false, true, false, false}, ch, me, o16 != 0) != nullptr) != want) { printf("FAIL table %d %d %d\n", ch, me, o16); return 1; }
                n += want;
            }
    if (n != 24) { printf("FAIL %d tail-biting frame kernels\n", n); return 1; }
    // the channel ids collide with no other range
    static_assert(kFrm + kTb + HARD > kFrm + kPun + FP32 && ((kFrm + kTb) & 7) == 0, "channel id range");
    return 0;
}

int main()
{
    for (uint32_t S = 1; S <= 300; S++)
        if (check_frame(S) || check_recip(S)) return 1;
    for (uint32_t S : {(1u << 20) - 1, 1u << 20, (1u << 20) - 31, 65536u, 65535u})
        if (check_frame(S) || check_recip(S)) return 1;
    if (check_args() || check_plan()) return 1;
    printf("ok\n");
    return 0;
}
