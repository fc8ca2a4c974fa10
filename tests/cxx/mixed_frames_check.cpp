// Host check of the mixed-frame helpers (vd_frames.h "mixed frames"), the four kernel tables of the mixed launches
// (vd_plan.h) and their names against a plain enumeration (never against the header's own closed forms).
//   records: a record is 32 bytes whose first six dwords are period, keep0, keep1, the kept values per period counted
//     bit by bit, and the two reciprocals as the kernel's index maps define them (recip: the largest 32-bit r with
//     r * period <= 2^32, found by stepping from the quotient; m16: the smallest m with m * period > 2^16), the last
//     two dwords 0;
//   mix_max_bytes: for every table and every length, the largest number of kept values of a frame, counted by walking
//     the frame's 2 S mother positions once per pattern, times the bytes of a value;
//   mixed_table_error and frame_args_error (the mixed families) message by message;
//   the 56 kernels of the four tables -- one wherever the punctured twin has one -- and the names of llr 11 .. 14.
// Arguments (tests/test_mixed_frames.py passes its lists): sizes=S,S,... pat=period,keep0,keep1 (repeated; the table
// is every prefix of them).  Built with hipcc and the host sanitizers; prints "ok" or the first mismatch.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
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

static std::vector<uint32_t> list_of(const char* s)
{
    std::vector<uint32_t> v;
    while (*s) {
        v.push_back((uint32_t)strtoul(s, (char**)&s, 0));
        if (*s == ',') s++;
    }
    return v;
}

#define FAIL(...) do { printf("FAIL " __VA_ARGS__); printf("\n"); return 1; } while (0)

// kept values of a frame of S stages, by walking its mother positions
static uint64_t kept_of(const Pat& p, uint32_t S)
{
    uint64_t kept = 0;
    uint32_t bit = 0;
    for (uint32_t t = 0; t < S; t++) {
        kept += ((p.k0 >> bit) & 1u) + ((p.k1 >> bit) & 1u);
        bit = bit + 1 == (uint32_t)p.period ? 0 : bit + 1;
    }
    return kept;
}

static int check_record(const Pat& p)
{
    const MixRecord r = mix_record(p.period, p.k0, p.k1);
    uint32_t w[8];
    static_assert(sizeof(r) == sizeof(w), "32-byte records");
    memcpy(w, &r, sizeof(w));
    uint32_t kp = 0;
    for (int i = 0; i < p.period; i++) kp += ((p.k0 >> i) & 1u) + ((p.k1 >> i) & 1u);
    uint64_t recip = 0x100000000ull / (uint64_t)p.period;
    while (recip * (uint64_t)p.period > 0x100000000ull) recip--;
    if (recip > 0xFFFFFFFFull) recip = 0xFFFFFFFFull;
    uint32_t m16 = 0;
    while ((uint64_t)m16 * (uint64_t)p.period <= 65536ull) m16++;
    const uint32_t want[8] = {(uint32_t)p.period, p.k0, p.k1, kp, (uint32_t)recip, m16, 0u, 0u};
    for (int i = 0; i < 8; i++)
        if (w[i] != want[i]) FAIL("record (%d,0x%x,0x%x) dword %d: 0x%x, want 0x%x", p.period, p.k0, p.k1, i, w[i], want[i]);
    const Punct pn = punct_make(p.period, p.k0, p.k1);
    if (memcmp(&r.pn, &pn, sizeof(pn))) FAIL("record (%d,0x%x,0x%x) differs from punct_make", p.period, p.k0, p.k1);
    return 0;
}

static int check_max_bytes(const std::vector<Pat>& pats, const std::vector<uint32_t>& sizes)
{
    std::vector<MixRecord> tab;
    for (const Pat& p : pats) tab.push_back(mix_record(p.period, p.k0, p.k1));
    for (size_t n = 0; n <= pats.size(); n++)
        for (uint32_t S : sizes) {
            uint64_t most = 0;
            for (size_t i = 0; i < n; i++) most = std::max(most, kept_of(pats[i], S));
            if (mix_max_bytes<4>(tab.data(), (int)n, S) != 4 * most || mix_max_bytes<1>(tab.data(), (int)n, S) != most)
                FAIL("mix_max_bytes of %zu patterns, S %u: %u / %u, enumeration %llu values", n, S,
                     mix_max_bytes<4>(tab.data(), (int)n, S), mix_max_bytes<1>(tab.data(), (int)n, S), (unsigned long long)most);
        }
    return 0;
}

static int check_table_error()
{
    const uint32_t good[] = {1, 1, 1, 2, 1, 3, 3, 5, 3, 16, 0x8000, 0};
    std::vector<uint32_t> many;
    for (int i = 0; i < 17; i++) many.insert(many.end(), {3u, 5u, 3u});
    struct T {
        const uint32_t* t;
        int n;
        const char* why;
    };
    const uint32_t p0[] = {0, 1, 1}, p17[] = {17, 1, 1}, pmask[] = {3, 8, 3}, pnone[] = {3, 0, 0}, phuge[] = {0x80000001u, 1, 1};
    const uint32_t second[] = {1, 1, 1, 3, 0, 0};
    const T cases[] = {{good, 4, nullptr}, {good, 0, nullptr}, {nullptr, 0, nullptr}, {many.data(), 16, nullptr},
                       {many.data(), 17, "n must be in [0, 16]"}, {good, -1, "n must be in [0, 16]"}, {nullptr, 1, "null triples"},
                       {p0, 1, "invalid puncture pattern"}, {p17, 1, "invalid puncture pattern"}, {pmask, 1, "invalid puncture pattern"},
                       {pnone, 1, "invalid puncture pattern"}, {phuge, 1, "invalid puncture pattern"}, {second, 2, "invalid puncture pattern"}};
    int i = 0;
    for (const T& c : cases) {
        const char* why = mixed_table_error(c.t, c.n);
        if (c.why ? !why || !strstr(why, c.why) : why != nullptr)
            FAIL("table case %d: %s, want %s", i, why ? why : "accepted", c.why ? c.why : "accepted");
        i++;
    }
    return 0;
}

static int check_args()
{
    // the table: 1/2, 2/3, 3/4.  1000 stages: 2000, 1500, 1334 values; the densest sets the stride rule
    const MixRecord tab[3] = {mix_record(1, 1, 1), mix_record(2, 1, 3), mix_record(3, 5, 3)};
    const MixRecord thin[1] = {mix_record(3, 5, 3)};
    struct A {
        uint64_t addr, istr;
        bool off;
        uint64_t ostr, maxb;
        int nf, kind;
        float scale;
        const MixRecord* tab;
        int n;
        uint32_t vb;
        uint64_t part;
        const char* why;  // a piece of the message, or null: accepted
    };
    const float inf = std::numeric_limits<float>::infinity();
    const A cases[] = {
        {0, 8000, false, 128, 1000, 4, 1, 1.0f, tab, 3, 4, 0, nullptr},           // the smallest strides
        {4, 8004, false, 132, 1000, 4, 0, 1.0f, tab, 3, 4, 0, nullptr},           // 4-byte alignment is enough, (1, 1, 1) included
        {12, 8000, false, 128, 1000, 4, 2, 1.0f, tab, 3, 4, 96, nullptr},
        {0, 5336, false, 128, 1000, 4, 1, 1.0f, thin, 1, 4, 0, nullptr},          // ... of the table at hand
        {1, 2001, false, 128, 1000, 4, 1, 1.0f, tab, 3, 1, 0, nullptr},           // int8: any address, any stride
        {3, 2000, false, 128, 1000, 4, 2, 0.25f, tab, 3, 1, 192, nullptr},
        {4, 0, true, 128, 1000, 4, 1, 1.0f, tab, 3, 4, 0, nullptr},               // offsets: the stride is ignored
        {4, 3, true, 128, 1000, 4, 0, 1.0f, tab, 3, 4, 0, nullptr},
        {1, 0, true, 128, 1000, 4, 2, 1.0f, tab, 3, 1, 0, nullptr},
        {0, 0, false, 0, 1000, 1, 1, 1.0f, tab, 3, 4, 0, nullptr},                // one frame: no stride needed
        {0, 8ull << 20, false, 4ull << 15, 1u << 20, 2, 1, 1.0f, tab, 3, 4, 0, nullptr},
        {0, 8000, false, 128, 1000, 4, 2, 1e-40f, tab, 3, 4, 0, nullptr},         // tail-biting: any finite scale > 0
        {0, 8000, false, 128, 1000, 4, 1, 1.0f, tab, 0, 4, 0, "pattern table is empty"},
        {0, 8000, false, 128, 1000, 4, 1, 1.0f, nullptr, 0, 4, 0, "pattern table is empty"},
        {0, 8000, false, 128, 1000, 4, 3, 1.0f, tab, 3, 4, 0, "kind must be"},
        {0, 8000, false, 128, 1000, 4, -1, 1.0f, tab, 3, 1, 0, "kind must be"},
        {0, 8000, false, 128, 0, 4, 1, 1.0f, tab, 3, 4, 0, "maxFrameBits must be in"},
        {0, 16ull << 20, false, 1ull << 20, (1u << 20) + 1, 4, 1, 1.0f, tab, 3, 4, 0, "maxFrameBits must be in"},
        {0, 8000, false, 128, 1000, 0, 1, 1.0f, tab, 3, 4, 0, "nframes must be >= 1"},
        {0, 8000, true, 128, 1000, -1, 2, 1.0f, tab, 3, 4, 0, "nframes must be >= 1"},
        {0, 8000, false, 128, 1000, 4, 1, 0.0f, tab, 3, 4, 0, "(and -65536 / scale finite)"},
        {0, 8000, false, 128, 1000, 4, 0, inf, tab, 3, 4, 0, "(and -65536 / scale finite)"},
        {0, 8000, false, 128, 1000, 4, 0, std::nanf(""), tab, 3, 1, 0, "(and -65536 / scale finite)"},
        {0, 8000, false, 128, 1000, 4, 1, 1e-40f, tab, 3, 4, 0, "(and -65536 / scale finite)"},
        {0, 8000, false, 128, 1000, 4, 2, 0.0f, tab, 3, 4, 0, "scale must be finite and > 0"},
        {0, 8000, false, 128, 1000, 4, 2, inf, tab, 3, 1, 0, "scale must be finite and > 0"},
        {2, 8000, false, 128, 1000, 4, 1, 1.0f, tab, 3, 4, 0, "rx_d must be 4-byte aligned"},
        {1, 0, true, 128, 1000, 4, 1, 1.0f, tab, 3, 4, 0, "rx_d must be 4-byte aligned"},
        {0, 8002, false, 128, 1000, 4, 1, 1.0f, tab, 3, 4, 0, "rx_stride must be a multiple of 4"},
        {0, 8000, false, 130, 1000, 4, 1, 1.0f, tab, 3, 4, 0, "output_stride must be a multiple of 4"},
        {0, 2000, true, 129, 1000, 4, 1, 1.0f, tab, 3, 1, 0, "output_stride must be a multiple of 4"},
        {0, 7996, false, 128, 1000, 4, 1, 1.0f, tab, 3, 4, 0, "rx_stride smaller than"},   // below (1, 1, 1)'s 8000 bytes
        {0, 5336, false, 128, 1000, 4, 1, 1.0f, tab, 3, 4, 0, "rx_stride smaller than"},   // enough for 3/4 only
        {0, 5332, false, 128, 1000, 4, 2, 1.0f, thin, 1, 4, 0, "rx_stride smaller than"},
        {0, 1999, false, 128, 1000, 4, 1, 1.0f, tab, 3, 1, 0, "rx_stride smaller than"},
        {0, 0, false, 128, 1000, 2, 1, 1.0f, tab, 3, 1, 0, "rx_stride smaller than"},
        {0, 8000, false, 124, 1000, 4, 1, 1.0f, tab, 3, 4, 0, "output_stride smaller than"},
        {0, 0, true, 0, 1000, 2, 2, 1.0f, tab, 3, 4, 0, "output_stride smaller than"},
        {0, 8000, false, 128, 1000, 4, 1, 1.0f, tab, 3, 4, 100, "partBits must be 0 or a multiple of 96"},
        {0, 0, true, 4ull << 15, 1u << 20, 0x7FFFFFFF, 1, 1.0f, tab, 3, 4, 96, "more than 2^31 - 1 workgroups"},
    };
    int i = 0;
    for (const A& a : cases) {
        FrameArgs c = call_of({true, a.kind == kByteFramesTailbiting, a.vb == 1, true}, a.addr, a.istr, a.ostr, a.maxb, a.nf, a.kind, a.scale);
        c.offsets = a.off;
        c.table = a.tab;
        c.tableN = a.n;
        c.partBits = a.part;
        const char* why = why_of(c);
        if (a.why ? !why || !strstr(why, a.why) : why != nullptr)
            FAIL("argument case %d: %s, want %s", i, why ? why : "accepted", a.why ? a.why : "accepted");
        i++;
    }
    // a frame's place in the host variants' buffer
    if (!mixed_frame_inside(0, 0, 0) || !mixed_frame_inside(10, 0, 10) || !mixed_frame_inside(3, 7, 10) || mixed_frame_inside(4, 7, 10) ||
        mixed_frame_inside(11, 0, 10) || mixed_frame_inside(0xFFFFFFFFFFFFFFFFull, 2, 10) || mixed_frame_inside(0, 11, 10))
        FAIL("mixed_frame_inside");
    return 0;
}

static int check_table()
{
    // a mixed kernel exactly where the punctured twin has one: 18 + 18 float, 10 + 10 int8
    int n[4] = {0, 0, 0, 0};
    for (int ch = -1; ch <= 5; ch++)
        for (int me = -1; me <= 3; me++)
            for (int o16 = 0; o16 < 2; o16++)
                for (int fam = 0; fam < 4; fam++) {
                    const bool i8 = fam & 1, tb = fam & 2;
                    const bool got = launcher_frames<Stub>({true, tb, i8, true}, ch, me, o16 != 0) != nullptr;
                    const bool twin = launcher_frames<Stub>({true, tb, i8, false}, ch, me, o16 != 0) != nullptr;
                    if (launcher_frames<Stub>({false, tb, i8, true}, ch, me, o16 != 0)) FAIL("a mixed kernel that is not a punctured one: %d %d %d", ch, me, o16);
                    const bool want = ch >= 1 && ch <= (i8 ? 2 : 4) && me >= 0 && me < 3 && has_kernel(Form::Tg, ch, me);
                    if (got != want || got != twin) FAIL("table family %d: %d %d %d", fam, ch, me, o16);
                    n[fam] += got;
                }
    if (n[0] != 18 || n[1] != 10 || n[2] != 18 || n[3] != 10) FAIL("%d + %d + %d + %d mixed kernels", n[0], n[1], n[2], n[3]);
    // the names: the punctured family's with MIX+ before PUN+ / TB+PUN+
    const char* twins[4] = {"FRM+PUN+", "FRM+TB+PUN+", "FRM+I8+PUN+", "FRM+I8+TB+PUN+"};
    const char* mixed[4] = {"FRM+MIX+PUN+", "FRM+MIX+TB+PUN+", "FRM+I8+MIX+PUN+", "FRM+I8+MIX+TB+PUN+"};
    const int twin_llr[4] = {4, 6, 8, 10};
    for (int k = 0; k < 4; k++)
        for (int o : {0x012, 0x102, 0x021, 0x001})
            for (uint32_t parts : {1u, 3u}) {
                std::string a = plan_name(plan_frames(o, 5, parts), o, twin_llr[k]);
                const std::string b = plan_name(plan_frames(o, 5, parts), o, 11 + k);
                const size_t at = a.find(twins[k]);
                if (at == std::string::npos) FAIL("name %s", a.c_str());
                a.replace(at, strlen(twins[k]), mixed[k]);
                if (a != b) FAIL("name %s, want %s", b.c_str(), a.c_str());
            }
    if (plan_name(plan_frames(0x012, 4), 0x012, 11).rfind("vd_decode_tg<FRM+MIX+PUN+SOFT8,B16,O32> one frame per wave, ", 0) != 0) FAIL("name 11");
    if (plan_name(plan_frames(0x012, 4), 0x012, 14).rfind("vd_decode_tg<FRM+I8+MIX+TB+PUN+SOFT8,B16,O32> one frame per wave, ", 0) != 0) FAIL("name 14");
    if (plan_name(plan_frames(0x012, 0), 0x012, 12) != "-") FAIL("empty plan");
    // the earlier names stay
    if (plan_name(plan_frames(0x012, 4), 0x012, 10).rfind("vd_decode_tg<FRM+I8+TB+PUN+SOFT8,", 0) != 0) FAIL("name 10");
    if (plan_name(plan_frames(0x012, 4), 0x012, 4).rfind("vd_decode_tg<FRM+PUN+SOFT8,", 0) != 0) FAIL("name 4");
    // the ids are sums: the lowest mixed id lies above the highest id there was (kI8 + kFrm + kTb + kPun + SOFT8 = 138),
    // and the flag leaves the format in the low three bits
    static_assert(kMix + kFrm + kPun + SOFT4 > kI8 + kFrm + kTb + kPun + FP32 && kMix % 8 == 0, "channel id range");
    return 0;
}

int main(int argc, char** argv)
{
    std::vector<uint32_t> sizes;
    std::vector<Pat> pats;
    for (int i = 1; i < argc; i++) {
        if (!strncmp(argv[i], "sizes=", 6)) sizes = list_of(argv[i] + 6);
        else if (!strncmp(argv[i], "pat=", 4)) {
            const std::vector<uint32_t> v = list_of(argv[i] + 4);
            if (v.size() != 3) FAIL("argument %s", argv[i]);
            pats.push_back({(int)v[0], v[1], v[2]});
        } else FAIL("argument %s", argv[i]);
    }
    if (sizes.empty() || pats.empty() || pats.size() > (size_t)kMixMaxPatterns) FAIL("usage: sizes=S,... pat=period,keep0,keep1 ...");
    for (const Pat& p : pats) {
        if (!punct_valid(p.period, p.k0, p.k1)) FAIL("pattern");
        if (check_record(p)) return 1;
    }
    for (int period = 1; period <= 16; period++)  // every period's reciprocals
        if (check_record({period, 1u << (period - 1), 1u})) return 1;
    if (check_max_bytes(pats, sizes) || check_table_error() || check_args() || check_table()) return 1;
    printf("ok %zu sizes %zu patterns\n", sizes.size(), pats.size());
    return 0;
}
