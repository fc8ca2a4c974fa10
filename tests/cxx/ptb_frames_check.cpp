// Host check of the punctured tail-biting frame geometry (vd_frames.h "punctured tail-biting frames"), its argument
// checks and the kernel table of launcher_frames (vd_plan.h; pun + tb) against a plain enumeration (never against the
// header's own closed forms).  For a pattern and a frame of S stages the enumeration walks the frame's 2 S mother
// positions once, counting the kept ones: that gives every kept value's index in the frame's buffer and the
// buffer's length.  The extended stream is walked by stepping: stage 26 is frame stage 0, stage 0 is found by
// stepping back 26 times, and every later stage steps forward with the wrap at S.  For every group start the decode
// of the frame reaches, the one it prefetches beyond and a few groups past P, and all 96 lanes of each group, the
// two offsets of ptb_stage_offsets (ptb_group -> ptb_offsets, the chain the kernel runs) are compared with it:
//   a kept value of the frame stage lies inside the range of pfrm_bytes, at 4 x its index;
//   a punctured value lies at or above 2^31 with no 32-bit wrap of offset + 4: past any range a frame can have.
// Also: the form of every group (inside exactly when no lane leaves the unwrapped line, several turns exactly for
// a wrapping group of a frame under 96 stages), pfrm_bytes against the enumeration's length, frame_args_error case
// by case, the kernel name and the kernel table.
// Patterns: 1/2, 2/3, 3/4, (7, 0b1010001, 0b0101111), (16, 0xA5C3, 0x5A3D), (16, 0x8000, 0).  Lengths: every S in
// 1 .. 400, and 4095, 4096, 4097, 2^20 - 1, 2^20.
// Built with hipcc and the host sanitizers by tests/test_punct_tb_frames.py; prints "ok" or the first mismatch.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <string>
#include <vector>
#include "vd_kernel_tg.h"
#include "vd_plan.h"
#include "frame_args.h"

using namespace vd;

struct Stub {
    using fn = void (*)();
    template <int CH, int CORE, int OB> static void tg() {}
    template <int CH, int CORE, int OB, bool SPL> static void pk() {}
};

struct Pat {
    int period;
    uint32_t k0, k1;
};

// idx[2 t + c]: index in the frame's buffer of output c of frame stage t, or -1 when punctured; kept: their number
// (plain walk, phase 0 at stage 0)
struct Enum {
    std::vector<int32_t> idx;
    uint32_t kept = 0;
    void build(const Pat& p, uint32_t S)
    {
        idx.assign(2 * (size_t)S, -1);
        kept = 0;
        uint32_t bit = 0;
        for (uint32_t t = 0; t < S; t++) {
            if ((p.k0 >> bit) & 1u) idx[2 * (size_t)t] = (int32_t)kept++;
            if ((p.k1 >> bit) & 1u) idx[2 * (size_t)t + 1] = (int32_t)kept++;
            bit = bit + 1 == (uint32_t)p.period ? 0 : bit + 1;
        }
    }
};

static int check_frame(const Pat& p, uint32_t S)
{
    const Punct pn = punct_make(p.period, p.k0, p.k1);
    Enum en;
    en.build(p, S);
    const uint64_t range = 4ull * en.kept;
    if (pfrm_bytes(pn, S) != range || range != 4 * punct_len(pn, 2ull * S) || range > (8ull << 20)) {
        printf("FAIL (%d,0x%x,0x%x) S %u: pfrm_bytes %u, enumeration %llu\n", p.period, p.k0, p.k1, S, pfrm_bytes(pn, S),
               (unsigned long long)range);
        return 1;
    }
    uint32_t W = 0;
    while (32 * W < S) W++;
    // the decode runs W + 2 blocks of 32 stages in groups of 3, and every group head loads the next group: group
    // starts 0, 96, ... up to the one after the last group run, and three more
    const uint32_t lastRun = (W + 2 - 1) / 3 * 3 * 32, nst = lastRun + 5 * 96;
    const TbRecip rc = tb_recip(S);
    uint32_t t = 0;  // the frame stage of extended stage 0: 26 steps back from stage 26 = frame stage 0
    for (int i = 0; i < 26; i++) t = t == 0 ? S - 1 : t - 1;
    for (uint32_t g0 = 0; g0 + 96 <= nst; g0 += 96) {
        const PtbGroup g = ptb_group(pn, g0, S, rc);
        bool leaves = false;  // some lane is off the unwrapped line
        for (uint32_t s = 0; s < 96; s++) {
            const uint32_t pst = g0 + s;
            leaves = leaves || pst < 26 || pst - 26 != t;
            const PfrmOff o = ptb_stage_offsets(pn, g0, s, S, rc);
            const uint32_t off[2] = {o.o0, o.o1};
            for (int c = 0; c < 2; c++) {
                const int32_t want = en.idx[2 * (size_t)t + c];
                if (off[c] > 0xFFFFFFFBu) {
                    printf("FAIL (%d,0x%x,0x%x) S %u stage %u value %d: offset 0x%x wraps\n", p.period, p.k0, p.k1, S, pst, c, off[c]);
                    return 1;
                }
                if (want >= 0 ? off[c] != 4u * (uint32_t)want || (uint64_t)off[c] + 4 > range : off[c] < 0x80000000u) {
                    printf("FAIL (%d,0x%x,0x%x) S %u stage %u (frame stage %u) value %d: offset 0x%x, range %llu, want index %d\n",
                           p.period, p.k0, p.k1, S, pst, t, c, off[c], (unsigned long long)range, want);
                    return 1;
                }
            }
            t = t + 1 == S ? 0 : t + 1;
        }
        const uint32_t mode = !leaves ? kPtbInside : S >= 96 ? kPtbWrap : kPtbTurns;
        if (g.mode != mode) {
            printf("FAIL (%d,0x%x,0x%x) S %u group %u: form %u, want %u\n", p.period, p.k0, p.k1, S, g0, g.mode, mode);
            return 1;
        }
    }
    return 0;
}

static int check_args()
{
    struct A {
        uint64_t addr, istr, ostr, maxb;
        int nf;
        float scale;
        int period;
        uint32_t k0, k1;
        bool ok;
    };
    const float inf = std::numeric_limits<float>::infinity();
    // 3/4 keeps 4 of 6: 1000 stages -> 1334 floats (333 periods of 4, then stage 999 keeps both), 5336 bytes
    const A cases[] = {
        {0, 5336, 128, 1000, 4, 40000.0f, 3, 5, 3, true},                  // the smallest strides
        {4, 5340, 132, 1000, 4, 1.0f, 3, 5, 3, true},                      // 4-byte alignment is enough
        {12, 8000, 128, 1000, 4, 40000.0f, 1, 1, 1, true},                 // (1, 1, 1): 8 bytes a stage
        {0, 0, 0, 1000, 1, 40000.0f, 3, 5, 3, true},                       // one frame: no stride needed
        {0, 0, 4, 15, 3, 40000.0f, 16, 0x8000, 0, true},                   // frames without a kept value
        {0, 4, 4, 16, 3, 40000.0f, 16, 0x8000, 0, true},
        {0, 8ull << 20, 4ull << 15, 1u << 20, 2, 40000.0f, 1, 1, 1, true},
        {0, 5336, 128, 1000, 4, 1e-40f, 3, 5, 3, true},                    // no pad value to form: any finite scale > 0
        {0, 5336, 128, 1000, 4, 3e38f, 3, 5, 3, true},
        {0, 5336, 128, 1000, 4, 40000.0f, 0, 1, 1, false},                 // the pattern
        {0, 5336, 128, 1000, 4, 40000.0f, 17, 1, 1, false},
        {0, 5336, 128, 1000, 4, 40000.0f, -1, 1, 1, false},
        {0, 5336, 128, 1000, 4, 40000.0f, 3, 8, 3, false},                 // a bit at `period`
        {0, 5336, 128, 1000, 4, 40000.0f, 3, 5, 0x10003, false},
        {0, 5336, 128, 1000, 4, 40000.0f, 3, 0, 0, false},                 // both masks 0
        {0, 5336, 128, 0, 4, 40000.0f, 3, 5, 3, false},                    // maxFrameBits
        {0, 16ull << 20, 1ull << 20, (1u << 20) + 1, 4, 40000.0f, 3, 5, 3, false},
        {0, 5336, 128, 1000, 0, 40000.0f, 3, 5, 3, false},                 // nframes
        {0, 5336, 128, 1000, -1, 40000.0f, 3, 5, 3, false},
        {0, 5336, 128, 1000, 4, 0.0f, 3, 5, 3, false},                     // scale
        {0, 5336, 128, 1000, 4, -0.0f, 3, 5, 3, false},
        {0, 5336, 128, 1000, 4, -1.0f, 3, 5, 3, false},
        {0, 5336, 128, 1000, 4, inf, 3, 5, 3, false},
        {0, 5336, 128, 1000, 4, -inf, 3, 5, 3, false},
        {0, 5336, 128, 1000, 4, std::nanf(""), 3, 5, 3, false},
        {2, 5336, 128, 1000, 4, 40000.0f, 3, 5, 3, false},                 // alignment
        {1, 5336, 128, 1000, 4, 40000.0f, 3, 5, 3, false},
        {0, 5338, 128, 1000, 4, 40000.0f, 3, 5, 3, false},
        {0, 5336, 130, 1000, 4, 40000.0f, 3, 5, 3, false},
        {0, 5332, 128, 1000, 4, 40000.0f, 3, 5, 3, false},                 // overlapping frames
        {0, 5336, 124, 1000, 4, 40000.0f, 3, 5, 3, false},
        {0, 0, 128, 1000, 2, 40000.0f, 3, 5, 3, false},
        {0, 7996, 128, 1000, 4, 40000.0f, 1, 1, 1, false},
        {0, 0, 4, 16, 3, 40000.0f, 16, 0x8000, 0, false},
    };
    int i = 0;
    for (const A& a : cases) {
        const char* why = check({true, true, false, false}, a.addr, a.istr, a.ostr, a.maxb, a.nf, kByteFramesTailbiting, a.scale, a.period, a.k0, a.k1);
        if ((why == nullptr) != a.ok) { printf("FAIL argument case %d: %s\n", i, why ? why : "accepted"); return 1; }
        i++;
    }
    return 0;
}

static int check_table()
{
    // a kernel exactly for the 9 punctured (format, metric) pairs, both output widths; none for HARD
    int n = 0;
    for (int ch = -1; ch <= 5; ch++)
        for (int me = -1; me <= 3; me++)
            for (int o16 = 0; o16 < 2; o16++) {
                const bool want = ch >= 1 && ch < 5 && me >= 0 && me < 3 && has_kernel(Form::Tg, ch, me);
                if ((launcher_frames<Stub>({true, true, false, false}, ch, me, o16 != 0) != nullptr) != want) { printf("FAIL table %d %d %d\n", ch, me, o16); return 1; }
                if (want != (launcher_frames<Stub>({true, false, false, false}, ch, me, o16 != 0) != nullptr)) { printf("FAIL table vs FRM+PUN %d %d %d\n", ch, me, o16); return 1; }
                n += want;
            }
    if (n != 18) { printf("FAIL %d punctured tail-biting frame kernels\n", n); return 1; }
    for (int me = 0; me < 3; me++)
        if (launcher_frames<Stub>({true, true, false, false}, HARD, me, false) || launcher_frames<Stub>({true, true, false, false}, HARD, me, true)) { printf("FAIL HARD kernel\n"); return 1; }
    const std::string nm = plan_name(plan_frames(0x012, 5), 0x012, 6);
    if (nm.rfind("vd_decode_tg<FRM+TB+PUN+SOFT8,B16,O32> one frame per wave, ", 0) != 0) { printf("FAIL name %s\n", nm.c_str()); return 1; }
    if (plan_name(plan_frames(0x103, 7), 0x103, 6).rfind("vd_decode_tg<FRM+TB+PUN+SOFT16,B32,O16>", 0) != 0) { printf("FAIL name\n"); return 1; }
    if (plan_name(plan_frames(0x012, 0), 0x012, 6) != "-") { printf("FAIL empty plan\n"); return 1; }
    // the earlier names stay
    if (plan_name(plan_frames(0x012, 4), 0x012, 3).rfind("vd_decode_tg<FRM+SOFT8,", 0) != 0 ||
        plan_name(plan_frames(0x012, 4), 0x012, 4).rfind("vd_decode_tg<FRM+PUN+SOFT8,", 0) != 0 ||
        plan_name(plan_frames(0x012, 4), 0x012, 5).rfind("vd_decode_tg<FRM+TB+SOFT8,", 0) != 0) { printf("FAIL earlier names\n"); return 1; }
    // the channel ids 72 .. 76 collide with no other range (kFrm + kTb + FP32 = 60 is the highest of the others)
    static_assert(kFrm + kTb + kPun + HARD == 72 && kFrm + kTb + kPun + HARD > kFrm + kTb + FP32 && ((kFrm + kTb + kPun) & 7) == 0,
                  "channel id range");
    return 0;
}

int main()
{
    const Pat pats[] = {{1, 1, 1}, {2, 0b01, 0b11}, {3, 0b101, 0b011}, {7, 0b1010001, 0b0101111}, {16, 0xA5C3, 0x5A3D}, {16, 0x8000, 0}};
    for (const Pat& p : pats) {
        if (!punct_valid(p.period, p.k0, p.k1)) return 1;
        for (uint32_t S = 1; S <= 400; S++)
            if (check_frame(p, S)) return 1;
        for (uint32_t S : {4095u, 4096u, 4097u, (1u << 20) - 1, 1u << 20})
            if (check_frame(p, S)) return 1;
    }
    if (check_args() || check_table()) return 1;
    printf("ok\n");
    return 0;
}
