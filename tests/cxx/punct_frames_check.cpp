// Host check of the punctured-frame helpers (vd_frames.h "punctured frames") and the kernel table of
// launcher_frames (vd_plan.h; pun) against a plain enumeration of the padded, depunctured stream (never against
// the headers' own closed forms).  For a pattern and a frame of S stages the enumeration walks the frame's 2 S
// mother positions once, counting the kept ones: that gives every kept value's index in the frame's buffer and
// the buffer's length.  Then, for every group start the decode of the frame reaches (the group after the last
// group run included: every group head loads the next group) and every lane role s < 96, the two offsets of
// pfrm_group -> pfrm_base -> pfrm_offsets (the chain the kernel runs) are compared with it:
//   a kept value of a frame stage lies inside the range, at 4 x its index;
//   a punctured value, a lead stage and a stage >= S lie outside it, with no 32-bit wrap of offset + 4.
// The offsets of a lane do not depend on S (only the range does), so they are computed once per pattern and group
// and compared for every S.
// Patterns: every valid one of period 1 .. 7 (21,838) and 300 random ones of period 8 .. 16, with every S in
// 0 .. 200.  For the patterns of period 1 .. 4, the random and the named ones every (S, group, lane) is compared
// one by one; for all patterns the same comparison is made for all S at once: the enumerated length grows with S,
// so an offset is inside the range from one S on, a value of frame stage t is expected inside from S = t + 1 on,
// and a group is reached from one S on -- the two agree for every S iff the two thresholds do.
// S = 2^20 (10,925 groups; the enumeration alone walks 2^20 stages per pattern, so not every pattern takes it):
// every group for the 81 patterns of period 1 .. 3, 40 of the random ones and three named ones; the first 4
// groups, the last 8 and every 97th between for the other random ones and every 83rd pattern of period 4 .. 7.
// Near the end the lengths 2^20 - 1, - 31 and - 97 are checked too.
// Also: pfrm_bytes against the enumeration's length and punct_len, the argument checks, the kernel table.
// Built with hipcc and the host sanitizers by tests/test_punct_frames.py; prints "ok" or the first mismatch.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <random>
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

// idx[2 t + c]: index in the frame's buffer of output c of frame stage t, or -1 when punctured; cum[t]: kept
// values of the stages before t (plain walk, phase 0 at stage 0)
struct Enum {
    std::vector<int32_t> idx;
    std::vector<uint32_t> cum;
    void build(const Pat& p, uint32_t stages)
    {
        idx.assign(2 * (size_t)stages, -1);
        cum.assign((size_t)stages + 1, 0);
        uint32_t n = 0;
        for (uint32_t t = 0; t < stages; t++) {
            cum[t] = n;
            const uint32_t bit = t % (uint32_t)p.period;
            if ((p.k0 >> bit) & 1u) idx[2 * (size_t)t] = (int32_t)n++;
            if ((p.k1 >> bit) & 1u) idx[2 * (size_t)t + 1] = (int32_t)n++;
        }
        cum[stages] = n;
    }
};

static uint32_t groups_loaded(uint32_t S)  // group starts 0, 96, ...: the groups run and the one loaded after them
{
    uint32_t W = 0;
    while (32 * W < S) W++;
    return (W + 2 + 2) / 3 + 1;
}

// the offsets of all 96 lanes of group g through the kernel's chain
static void group_offsets(const Punct& pn, uint32_t g, PfrmOff* out)
{
    const PfrmGroup pg = pfrm_group(g * kFrmGroup);
    uint32_t r0;
    const uint32_t base4 = pfrm_base(pn, pg.t0, &r0);
    for (uint32_t s = 0; s < kFrmGroup; s++) out[s] = pfrm_offsets(pn, base4, r0, pg.lead, s);
}

// lane s of group g against the enumeration, for a frame of S stages
static int check_lane(const Pat& p, const Enum& en, uint32_t S, uint32_t g, uint32_t s, const PfrmOff& o)
{
    const uint64_t range = 4ull * en.cum[S];
    const uint32_t pst = g * kFrmGroup + s;  // stage of the padded stream
    const uint32_t off[2] = {o.o0, o.o1};
    for (int c = 0; c < 2; c++) {
        int64_t want = -1;  // byte offset of a kept value of a frame stage, else outside
        if (pst >= kFrmLead && pst - kFrmLead < S && en.idx[2 * (size_t)(pst - kFrmLead) + c] >= 0)
            want = 4ll * en.idx[2 * (size_t)(pst - kFrmLead) + c];
        const bool inside = (uint64_t)off[c] + 4 <= range;
        if (off[c] > 0xFFFFFFFBu) {
            printf("FAIL (%d,0x%x,0x%x) S %u stage %u value %d: offset 0x%x wraps\n", p.period, p.k0, p.k1, S, pst, c, off[c]);
            return 1;
        }
        if (inside != (want >= 0) || (inside && (int64_t)off[c] != want)) {
            printf("FAIL (%d,0x%x,0x%x) S %u stage %u value %d: offset 0x%x, range %llu, want %lld\n", p.period, p.k0, p.k1, S,
                   pst, c, off[c], (unsigned long long)range, (long long)want);
            return 1;
        }
    }
    return 0;
}

static int check_bytes(const Pat& p, const Punct& pn, const Enum& en, uint32_t S)
{
    const uint32_t b = pfrm_bytes(pn, S);
    if (b != 4u * en.cum[S] || (uint64_t)b != 4 * punct_len(pn, 2ull * S)) {
        printf("FAIL (%d,0x%x,0x%x) S %u: pfrm_bytes %u, enumeration %u, punct_len %llu\n", p.period, p.k0, p.k1, S, b,
               4u * en.cum[S], (unsigned long long)punct_len(pn, 2ull * S));
        return 1;
    }
    return 0;
}

// every S in 0 .. 200 at once, by thresholds (the header comment): lane s of group g, whose offsets are o
static int check_lane_all(const Pat& p, const Enum& en, uint32_t g, uint32_t s, const PfrmOff& o)
{
    constexpr uint32_t SMAX = 200, NEVER = SMAX + 1;
    uint32_t Sg = 0;  // the shortest frame whose decode loads group g
    while (Sg <= SMAX && groups_loaded(Sg) <= g) Sg++;
    const uint32_t pst = g * kFrmGroup + s;
    const uint32_t off[2] = {o.o0, o.o1};
    for (int c = 0; c < 2; c++) {
        if (off[c] > 0xFFFFFFFBu) { printf("FAIL (%d,0x%x,0x%x) stage %u: offset 0x%x wraps\n", p.period, p.k0, p.k1, pst, off[c]); return 1; }
        // the shortest frame whose range holds offset + 4 (the enumerated lengths en.cum[S] never shrink)
        const uint32_t need = (uint32_t)(((uint64_t)off[c] + 4 + 3) / 4);
        const uint32_t Sin = (uint32_t)(std::lower_bound(en.cum.begin(), en.cum.begin() + SMAX + 1, need) - en.cum.begin());
        uint32_t Swant = NEVER;  // the shortest frame that holds this value
        if (pst >= kFrmLead && pst - kFrmLead < SMAX && en.idx[2 * (size_t)(pst - kFrmLead) + c] >= 0) {
            Swant = pst - kFrmLead + 1;
            if (off[c] != 4u * (uint32_t)en.idx[2 * (size_t)(pst - kFrmLead) + c]) {
                printf("FAIL (%d,0x%x,0x%x) stage %u value %d: offset 0x%x, index %d\n", p.period, p.k0, p.k1, pst, c, off[c],
                       en.idx[2 * (size_t)(pst - kFrmLead) + c]);
                return 1;
            }
        }
        if (std::max(std::min(Sin, NEVER), Sg) != std::max(Swant, Sg)) {
            printf("FAIL (%d,0x%x,0x%x) stage %u value %d: offset 0x%x inside from S = %u on, want from %u on (group from %u on)\n",
                   p.period, p.k0, p.k1, pst, c, off[c], Sin, Swant, Sg);
            return 1;
        }
    }
    return 0;
}

// every S in 0 .. 200; one_by_one: every (S, group, lane) compared by itself as well
static int check_short(const Pat& p, bool one_by_one)
{
    const Punct pn = punct_make(p.period, p.k0, p.k1);
    Enum en;
    en.build(p, 200);
    const uint32_t ng = groups_loaded(200);
    std::vector<PfrmOff> off((size_t)ng * kFrmGroup);
    for (uint32_t g = 0; g < ng; g++) group_offsets(pn, g, &off[(size_t)g * kFrmGroup]);
    for (uint32_t g = 0; g < ng; g++)
        for (uint32_t s = 0; s < kFrmGroup; s++)
            if (check_lane_all(p, en, g, s, off[(size_t)g * kFrmGroup + s])) return 1;
    for (uint32_t S = 0; S <= 200; S++) {
        if (check_bytes(p, pn, en, S)) return 1;
        for (uint32_t g = 0; one_by_one && g < groups_loaded(S); g++)
            for (uint32_t s = 0; s < kFrmGroup; s++)
                if (check_lane(p, en, S, g, s, off[(size_t)g * kFrmGroup + s])) return 1;
    }
    return 0;
}

// S = 2^20 (and, for the range's sake, the lengths around it); all: every group, else the ends and a stride
static int check_long(const Pat& p, bool all)
{
    const Punct pn = punct_make(p.period, p.k0, p.k1);
    Enum en;
    en.build(p, kFrmMaxBits);
    const uint32_t lens[] = {kFrmMaxBits, kFrmMaxBits - 1, kFrmMaxBits - 31, kFrmMaxBits - 97};
    for (uint32_t S : lens)
        if (check_bytes(p, pn, en, S)) return 1;
    const uint32_t ng = groups_loaded(kFrmMaxBits);
    PfrmOff off[kFrmGroup];
    for (uint32_t g = 0; g < ng; g++) {
        const bool ends = g < 4 || g + 8 >= ng;
        if (!all && !ends && g % 97 != 0) continue;
        group_offsets(pn, g, off);
        for (uint32_t S : lens) {
            if (g >= groups_loaded(S) || (S != kFrmMaxBits && !ends)) continue;
            for (uint32_t s = 0; s < kFrmGroup; s++)
                if (check_lane(p, en, S, g, s, off[s])) return 1;
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
        {0, 5336, 128, 1000, 4, -1.0f, 3, 5, 3, false},
        {0, 5336, 128, 1000, 4, inf, 3, 5, 3, false},
        {0, 5336, 128, 1000, 4, std::nanf(""), 3, 5, 3, false},
        {0, 5336, 128, 1000, 4, 1e-40f, 3, 5, 3, false},
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
        const char* why = check({true, false, false, false}, a.addr, a.istr, a.ostr, a.maxb, a.nf, kByteFramesTerminated, a.scale, a.period, a.k0, a.k1);
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
                if ((launcher_frames<Stub>({true, false, false, false}, ch, me, o16 != 0) != nullptr) != want) { printf("FAIL table %d %d %d\n", ch, me, o16); return 1; }
                if (want != (launcher_punct<Stub>(ch, me, o16 != 0) != nullptr)) { printf("FAIL table vs PUN %d %d %d\n", ch, me, o16); return 1; }
                n += want;
            }
    if (n != 18) { printf("FAIL %d punctured frame kernels\n", n); return 1; }
    for (int me = 0; me < 3; me++)
        if (launcher_frames<Stub>({true, false, false, false}, HARD, me, false) || launcher_frames<Stub>({true, false, false, false}, HARD, me, true)) { printf("FAIL HARD kernel\n"); return 1; }
    const std::string nm = plan_name(plan_frames(0x012, 5), 0x012, 4);
    if (nm.rfind("vd_decode_tg<FRM+PUN+SOFT8,B16,O32> one frame per wave, ", 0) != 0) { printf("FAIL name %s\n", nm.c_str()); return 1; }
    if (plan_name(plan_frames(0x103, 7), 0x103, 4).rfind("vd_decode_tg<FRM+PUN+SOFT16,B32,O16>", 0) != 0) { printf("FAIL name\n"); return 1; }
    return 0;
}

int main()
{
    static_assert(pfrm_group(0).t0 == 0 && pfrm_group(0).lead == 26 && pfrm_group(96).t0 == 70 && pfrm_group(96).lead == 0, "groups");
    std::vector<Pat> small, rnd;
    for (int period = 1; period <= 7; period++)
        for (uint32_t k0 = 0; k0 < (1u << period); k0++)
            for (uint32_t k1 = 0; k1 < (1u << period); k1++)
                if (k0 | k1) small.push_back({period, k0, k1});
    std::mt19937 gen(12345);
    while (rnd.size() < 300) {
        const int period = 8 + (int)(gen() % 9);
        const uint32_t m = (1u << period) - 1u, k0 = gen() & m, k1 = gen() & m;
        if (k0 | k1) rnd.push_back({period, k0, k1});
    }
    const Pat named[] = {{16, 0x8000, 0}, {16, 0xA5C3, 0x5A3D}, {16, 0xFFFF, 0xFFFF}};
    for (size_t i = 0; i < small.size(); i++) {
        const Pat& p = small[i];
        if (!punct_valid(p.period, p.k0, p.k1) || check_short(p, p.period <= 4)) return 1;
        if ((p.period <= 3 || i % 83 == 0) && check_long(p, p.period <= 3)) return 1;
    }
    for (size_t i = 0; i < rnd.size(); i++)
        if (!punct_valid(rnd[i].period, rnd[i].k0, rnd[i].k1) || check_short(rnd[i], true) || check_long(rnd[i], i < 40)) return 1;
    for (const Pat& p : named)
        if (check_short(p, true) || check_long(p, true)) return 1;
    if (check_args() || check_table()) return 1;
    printf("ok\n");
    return 0;
}
