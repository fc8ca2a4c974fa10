// Host check of the frame geometry (vd_frames.h) and the frame plan (vd_plan.h) against a plain enumeration of the
// padded stream (never against the header's own closed forms): frame_words, frame_padded_stages; for every
// S in 1 .. 200 and at 2^20, terminated and open, every group start the decode of the frame reaches and all 96
// stages of each group: which stages carry the pad value, which groups take the select's branch, and where a
// stage's load lands against the frame's range of 8 S bytes; the pad value and the argument checks; the grids of
// plan_frames and the kernel table of launcher_frames.
// Built with hipcc and the host sanitizers by tests/test_frames.py; prints "ok" or the first mismatch.
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

enum Kind : int { PAD = -1, ERASED = -2 };  // or >= 0: the frame stage

static int check_frame(uint32_t S, bool term)
{
    uint32_t W = 0;
    while (32 * W < S) W++;
    const uint32_t P = 64 + 32 * W;
    if (frame_words(S) != W || frame_padded_stages(S) != P) {
        printf("FAIL S %u: words %u (want %u), padded stages %u (want %u)\n", S, frame_words(S), W, frame_padded_stages(S), P);
        return 1;
    }
    // the decode runs W + 2 blocks of 32 stages in groups of 3, and every group head loads the next group:
    // group starts 0, 96, ... up to the one after the last group run
    const uint32_t lastRun = (W + 2 - 1) / 3 * 3 * 32, nst = lastRun + 2 * 96;
    std::vector<int> kind(nst);
    for (uint32_t p = 0; p < nst; p++) kind[p] = p < 26 ? PAD : p < 26 + S ? (int)(p - 26) : term ? PAD : ERASED;
    const uint32_t end = frame_end(S, term);
    const uint64_t range = 8ull * S;
    for (uint32_t g0 = 0; g0 + 96 <= nst; g0 += 96) {
        bool any = false;
        for (uint32_t s = 0; s < 96; s++) {
            const uint32_t p = g0 + s;
            any = any || kind[p] == PAD;
            if (frame_pad_stage(p, end) != (kind[p] == PAD)) {
                printf("FAIL S %u term %d stage %u: pad predicate %d\n", S, (int)term, p, (int)frame_pad_stage(p, end));
                return 1;
            }
            const uint32_t off = frame_offset(p);
            const bool inside = (uint64_t)off + 8 <= range;
            if (off > 0xFFFFFFF7u) {  // the end of the 8-byte access must not wrap in 32 bits
                printf("FAIL S %u stage %u: offset 0x%x wraps\n", S, p, off);
                return 1;
            }
            if (inside != (kind[p] >= 0) || (inside && off != 8u * (uint32_t)kind[p])) {
                printf("FAIL S %u term %d stage %u: offset 0x%x, range %llu, want %s\n", S, (int)term, p, off,
                       (unsigned long long)range, kind[p] >= 0 ? "the frame stage" : "outside");
                return 1;
            }
        }
        if (frame_pad_group(g0, end) != any) {
            printf("FAIL S %u term %d group %u: branch %d, pad stages %d\n", S, (int)term, g0, (int)frame_pad_group(g0, end), (int)any);
            return 1;
        }
    }
    return 0;
}

static int check_pad()
{
    const float inf = std::numeric_limits<float>::infinity();
    float pad = 0.0f;
    for (float bad : {0.0f, -0.0f, -1.0f, -40000.0f, inf, -inf, std::nanf(""), 1e-40f, 1e-35f})
        if (frame_pad(bad, &pad)) { printf("FAIL frame_pad accepts scale %g\n", bad); return 1; }
    for (float sc : {1.0f, 40000.0f, 0.3f, 1e-30f, 3e38f, 7.0f, 1.0f / 3.0f, 65536.0f, 12345.678f}) {
        if (!frame_pad(sc, &pad)) { printf("FAIL frame_pad rejects scale %g\n", sc); return 1; }
        const volatile float q = pad * sc;
        if (!std::isfinite(pad) || !(q <= -32768.0f)) { printf("FAIL pad %g of scale %g: product %g\n", pad, sc, q); return 1; }
    }
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
        {0, 8000, 128, 0, 4, 40000.0f, false},                        // maxFrameBits
        {0, 16ull << 20, 1ull << 20, (1u << 20) + 1, 4, 40000.0f, false},
        {0, 8000, 128, 1000, 0, 40000.0f, false},                     // nframes
        {0, 8000, 128, 1000, -1, 40000.0f, false},
        {0, 8000, 128, 1000, 4, 0.0f, false},                         // scale
        {0, 8000, 128, 1000, 4, -1.0f, false},
        {0, 8000, 128, 1000, 4, inf, false},
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
        const char* why = check({false, false, false, false}, a.addr, a.istr, a.ostr, a.maxb, a.nf, kByteFramesTerminated, a.scale);
        if ((why == nullptr) != a.ok) { printf("FAIL argument case %d: %s\n", i, why ? why : "accepted"); return 1; }
        i++;
    }
    return 0;
}

static int check_plan()
{
    const struct { uint64_t n; unsigned grid; } grids[] = {{1, 1}, {3, 1}, {4, 1}, {5, 2}, {6400, 1600}};
    for (auto g : grids) {
        const LaunchPlan p = plan_frames(0x012, g.n);
        if (!p.launches || p.form != Form::Tg || p.grid != g.grid || p.seg != kSegNone || p.stats || p.tailWG != ~0u) {
            printf("FAIL plan_frames(%llu): grid %u, want %u\n", (unsigned long long)g.n, p.grid, g.grid);
            return 1;
        }
        const std::string nm = plan_name(p, 0x012, 3);
        if (nm.rfind("vd_decode_tg<FRM+SOFT8,B16,O32>", 0) != 0) { printf("FAIL name %s\n", nm.c_str()); return 1; }
    }
    if (plan_frames(0x012, 0).launches || plan_name(plan_frames(0x012, 0), 0x012, 3) != "-") { printf("FAIL empty plan\n"); return 1; }
    if (plan_name(plan_frames(0x103, 7), 0x103, 3).rfind("vd_decode_tg<FRM+SOFT16,B32,O16>", 0) != 0) { printf("FAIL name\n"); return 1; }
    // the table: a kernel exactly for the 12 valid (format, metric) pairs, both output widths
    int n = 0;
    for (int ch = -1; ch <= 5; ch++)
        for (int me = -1; me <= 3; me++)
            for (int o16 = 0; o16 < 2; o16++) {
                const bool want = ch >= 0 && ch < 5 && me >= 0 && me < 3 && has_kernel(Form::Tg, ch, me);
                if ((launcher_frames<Stub>({false, false, false, false}, ch, me, o16 != 0) != nullptr) != want) { printf("FAIL table %d %d %d\n", ch, me, o16); return 1; }
                n += want;
            }
    if (n != 24) { printf("FAIL %d frame kernels\n", n); return 1; }
    return 0;
}

int main()
{
    for (uint32_t S = 1; S <= 200; S++)
        for (int term = 0; term < 2; term++)
            if (check_frame(S, term != 0)) return 1;
    for (int term = 0; term < 2; term++)
        if (check_frame(1u << 20, term != 0) || check_frame((1u << 20) - 31, term != 0)) return 1;
    if (frame_words(0) != 0) { printf("FAIL frame_words(0)\n"); return 1; }
    if (check_pad() || check_args() || check_plan()) return 1;
    printf("ok\n");
    return 0;
}
