// Host check of the geometry of frames in parts (vd_frames.h "frames in parts"), its argument check and the plan of
// a parted launch (vd_plan.h plan_frames) against a plain enumeration (never against the header's own closed forms).
// For a frame of S stages and parts of Wp words:
//   the parts are found by walking the frame's words once and starting a new part every Wp words: frame_parts,
//   frame_part and the idle parts past the frame are compared with that walk, so the parts tile [0, W) exactly;
//   every group start of every part (frame_part_stage + 96 i) is a multiple of 96;
//   the padded stream (26 lead stages, the frame, the stages after it) and the extended stream (stage 26 is frame
//   stage 0, found by stepping with the wrap at S) are enumerated stage by stage, and for every group a part's decode
//   runs, the one it prefetches beyond and one more, and all 96 lanes of each, the load offsets of the four families
//   at stage start + 32 j + s -- frame_offset; pfrm_group -> pfrm_base -> pfrm_offsets; tb_stage_offset;
//   ptb_stage_offsets: the chains the kernel runs -- are compared with the enumeration: a value of the frame lies at
//   its own place inside the frame's range, everything else outside every range with no 32-bit wrap of its end;
//   the pad predicate of a lane and of its group equal the enumeration's, terminated and open.
// The wave -> (frame, part) map of a launch of 1, 3 and 5 frames of unequal lengths covers every part of every frame
// exactly once and leaves the surplus waves without words.  The argument check, the grid and the plan (the
// two-argument plan_frames unchanged) case by case.
// Patterns: (2, 1, 3), (3, 5, 3), (16, 0x8000, 0).  Lengths: every S in 1 .. 400, and 2^20 - 31, 2^20.  Parts of 3, 6,
// 9 and 32766 words.  Built with hipcc and the host sanitizers by tests/test_frame_parts.py; prints "ok" or the first
// mismatch.
#include <climits>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>
#include "vd_kernel_tg.h"
#include "vd_plan.h"

using namespace vd;

struct Pat {
    int period;
    uint32_t k0, k1;
};
static const Pat kPats[] = {{2, 1, 3}, {3, 5, 3}, {16, 0x8000, 0}};

// the frame: per pattern, idx[2 t + c] = index in the frame's buffer of output c of frame stage t, or -1 when
// punctured (plain walk, phase 0 at stage 0), and the number of kept values
struct Frame {
    uint32_t S = 0, W = 0;
    std::vector<int32_t> idx[3];
    uint32_t kept[3] = {};
    std::vector<uint32_t> ext;  // frame stage of stage p of the extended stream
    void build(uint32_t s, uint32_t nst)
    {
        S = s;
        W = 0;
        while (32 * W < S) W++;
        for (int k = 0; k < 3; k++) {
            idx[k].assign(2 * (size_t)S, -1);
            kept[k] = 0;
            uint32_t bit = 0;
            for (uint32_t t = 0; t < S; t++) {
                if ((kPats[k].k0 >> bit) & 1u) idx[k][2 * (size_t)t] = (int32_t)kept[k]++;
                if ((kPats[k].k1 >> bit) & 1u) idx[k][2 * (size_t)t + 1] = (int32_t)kept[k]++;
                bit = bit + 1 == (uint32_t)kPats[k].period ? 0 : bit + 1;
            }
        }
        ext.resize(nst);
        uint32_t t = 0;  // stage 0: 26 steps back from stage 26 = frame stage 0
        for (int i = 0; i < 26; i++) t = t == 0 ? S - 1 : t - 1;
        for (uint32_t p = 0; p < nst; p++) {
            ext[p] = t;
            t = t + 1 == S ? 0 : t + 1;
        }
    }
};

#define FAIL(...)            \
    do {                     \
        printf("FAIL ");     \
        printf(__VA_ARGS__); \
        printf("\n");        \
        return 1;            \
    } while (0)

// an offset that must load zero: at or past the range, and its access of `bytes` ends without a 32-bit wrap
static bool outside(uint32_t off, uint64_t range, uint32_t bytes) { return off >= range && off <= 0xFFFFFFFFu - bytes + 1u; }

static int check_group(const Frame& f, uint32_t g0)
{
    const uint32_t S = f.S;
    if (g0 % 96) FAIL("S %u group start %u is no multiple of 96", S, g0);
    const TbRecip rc = tb_recip(S);
    // the pad predicate, terminated and open
    for (int term = 0; term < 2; term++) {
        const uint32_t end = frame_end(S, term != 0);
        bool any = false;
        for (uint32_t s = 0; s < 96; s++) {
            const uint32_t p = g0 + s;
            const bool want = p < 26 || (term && p >= 26 + S);
            any = any || want;
            if (frame_pad_stage(p, end) != want) FAIL("S %u stage %u term %d: pad predicate", S, p, term);
        }
        if (frame_pad_group(g0, end) != any) FAIL("S %u group %u term %d: group predicate %d", S, g0, term, (int)any);
    }
    for (uint32_t s = 0; s < 96; s++) {
        const uint32_t p = g0 + s;
        const bool in = p >= 26 && p < 26 + S;
        // frames: 8 bytes at 8 (p - 26) inside the 8 S bytes, else zero through the range check
        const uint32_t o = frame_offset(p);
        if (in ? o != 8u * (p - 26) || (uint64_t)o + 8 > 8ull * S : !outside(o, 8ull * S, 8)) FAIL("S %u stage %u: frame offset 0x%x", S, p, o);
        // tail-biting frames: the wrapped frame stage, always inside
        const uint32_t t = f.ext[p], ot = tb_stage_offset(g0, s, S, rc);
        if (ot != 8u * t) FAIL("S %u stage %u: tail-biting offset %u, frame stage %u", S, p, ot, t);
    }
    for (int k = 0; k < 3; k++) {
        const Punct pn = punct_make(kPats[k].period, kPats[k].k0, kPats[k].k1);
        const uint64_t range = 4ull * f.kept[k];
        if (pfrm_bytes(pn, S) != range) FAIL("S %u pattern %d: pfrm_bytes", S, k);
        // punctured frames: the chain of the kernel's group loads
        const PfrmGroup pg = pfrm_group(g0);
        uint32_t r0;
        const uint32_t base4 = pfrm_base(pn, pg.t0, &r0);
        for (uint32_t s = 0; s < 96; s++) {
            const uint32_t p = g0 + s;
            const bool in = p >= 26 && p < 26 + S;
            const PfrmOff a = pfrm_offsets(pn, base4, r0, pg.lead, s);
            const PfrmOff b = ptb_stage_offsets(pn, g0, s, S, rc);
            const uint32_t oa[2] = {a.o0, a.o1}, ob[2] = {b.o0, b.o1};
            for (int c = 0; c < 2; c++) {
                const int32_t want = in ? f.idx[k][2 * (size_t)(p - 26) + c] : -1;
                if (want >= 0 ? oa[c] != 4u * (uint32_t)want || (uint64_t)oa[c] + 4 > range : !outside(oa[c], range, 4))
                    FAIL("S %u pattern %d stage %u value %d: punctured-frame offset 0x%x, want index %d", S, k, p, c, oa[c], want);
                const int32_t wt = f.idx[k][2 * (size_t)f.ext[p] + c];
                if (wt >= 0 ? ob[c] != 4u * (uint32_t)wt || (uint64_t)ob[c] + 4 > range : ob[c] < 0x80000000u || ob[c] > 0xFFFFFFFCu)
                    FAIL("S %u pattern %d stage %u value %d: punctured tail-biting offset 0x%x, want index %d", S, k, p, c, ob[c], wt);
            }
        }
    }
    return 0;
}

static int check_frame(Frame& f, uint32_t S, uint32_t Wp)
{
    uint32_t W = 0;
    while (32 * W < S) W++;
    if (f.S != S) f.build(S, 64 + 32 * W + 3 * 96);  // (P, and the groups a last part reads beyond it)
    if (frame_words(S) != W) FAIL("S %u: frame_words", S);
    // the walk: a new part every Wp words
    std::vector<uint32_t> first, count;
    for (uint32_t w = 0; w < W; w++) {
        if (w % Wp == 0) {
            first.push_back(w);
            count.push_back(0);
        }
        count.back()++;
    }
    const uint32_t parts = (uint32_t)first.size();
    if (frame_parts(S, Wp) != parts) FAIL("S %u Wp %u: %u parts, walk %u", S, Wp, frame_parts(S, Wp), parts);
    if (frame_parts(S, 0) != 1 || frame_part(S, 0, 0).word0 != 0 || frame_part(S, 0, 0).words != W || frame_part(S, 0, 1).words != 0)
        FAIL("S %u: whole frames", S);
    uint32_t next = 0;
    for (uint32_t j = 0; j < parts + 6; j++) {
        const FramePart fp = frame_part(S, Wp, j);
        if (j >= parts) {
            if (fp.words != 0) FAIL("S %u Wp %u part %u past the frame has %u words", S, Wp, j, fp.words);
            continue;
        }
        if (fp.word0 != first[j] || fp.words != count[j] || fp.word0 != next || fp.words < 1 || fp.words > Wp)
            FAIL("S %u Wp %u part %u: [%u, +%u), walk [%u, +%u)", S, Wp, j, fp.word0, fp.words, first[j], count[j]);
        next = fp.word0 + fp.words;
        const uint32_t start = frame_part_stage(Wp, j);
        if (start != 32 * first[j] || start % 96) FAIL("S %u Wp %u part %u: first stage %u", S, Wp, j, start);
        // the decode of the part runs words + 2 blocks in groups of 3, and every group head loads the next group
        const uint32_t groups = (fp.words + 2 + 2) / 3 + 1;
        if ((uint64_t)start + 96ull * groups > f.ext.size()) FAIL("S %u Wp %u part %u: enumeration too short", S, Wp, j);
        for (uint32_t i = 0; i < groups; i++)
            if (check_group(f, start + 96 * i)) return 1;
    }
    if (next != W) FAIL("S %u Wp %u: the parts end at word %u of %u", S, Wp, next, W);
    return 0;
}

// the waves of a launch of n frames of lengths <= Smax
static int check_waves(uint32_t Smax, uint32_t Wp, int n)
{
    const uint32_t partsMax = frame_parts(Smax, Wp), G = frame_part_groups(partsMax);
    const uint64_t grid = frame_parts_grid((uint64_t)n, Smax, 32 * Wp);
    if (partsMax <= 1) {
        if (grid != ((uint64_t)n + 3) / 4) FAIL("Smax %u Wp %u n %d: one part, grid %llu", Smax, Wp, n, (unsigned long long)grid);
        return 0;
    }
    uint32_t gwalk = 0;
    while (4 * gwalk < partsMax) gwalk++;
    if (G != gwalk || grid != (uint64_t)n * gwalk) FAIL("Smax %u Wp %u n %d: G %u grid %llu", Smax, Wp, n, G, (unsigned long long)grid);
    const uint32_t lens[5] = {Smax, 1, Smax / 2 + 1, 0, Smax > 97 ? 97u : Smax};
    std::vector<std::vector<int>> hit(n);
    for (int f = 0; f < n; f++) hit[f].assign(frame_parts(lens[f], Wp) + 1, 0);
    for (uint32_t b = 0; b < grid; b++)
        for (uint32_t wv = 0; wv < 4; wv++) {
            const FrameWave fw = frame_wave(b, wv, G);
            if (fw.frame >= (uint32_t)n || fw.frame != b / gwalk) FAIL("Smax %u Wp %u n %d: workgroup %u -> frame %u", Smax, Wp, n, b, fw.frame);
            const FramePart fp = frame_part(lens[fw.frame], Wp, fw.part);
            const uint32_t have = lens[fw.frame] ? frame_parts(lens[fw.frame], Wp) : 0;
            if ((fp.words != 0) != (fw.part < have)) FAIL("Smax %u Wp %u n %d: frame %u part %u idle?", Smax, Wp, n, fw.frame, fw.part);
            if (fw.part < have) hit[fw.frame][fw.part]++;
        }
    for (int f = 0; f < n; f++) {
        const uint32_t have = lens[f] ? frame_parts(lens[f], Wp) : 0;
        for (uint32_t j = 0; j < have; j++)
            if (hit[f][j] != 1) FAIL("Smax %u Wp %u n %d: frame %d part %u decoded %d times", Smax, Wp, n, f, j, hit[f][j]);
    }
    return 0;
}

static int check_args_and_plan()
{
    const uint64_t good[] = {0, 96, 192, 288, 3072, 98304, 1048512};
    const uint64_t bad[] = {1, 32, 48, 95, 97, 100, 128, 1u << 20, 1048512 + 96, (1ull << 32) + 96, (1ull << 32), ~0ull};
    for (uint64_t v : good)
        if (!frame_part_bits_valid(v) || frame_parts_error(1000, 4, v)) FAIL("partBits %llu refused", (unsigned long long)v);
    for (uint64_t v : bad)
        if (frame_part_bits_valid(v) || !frame_parts_error(1000, 4, v)) FAIL("partBits %llu accepted", (unsigned long long)v);
    if (1048512 % 96 || 1048512 / 32 != 32766 || frame_part_words(1048512) != 32766 || frame_part_words(96) != 3) FAIL("part words");
    // the grid: 2^20 stages in parts of 96 are 10923 parts, 2731 workgroups a frame; 786336 such frames fit, one more does not
    if (frame_parts(1u << 20, 3) != 10923 || frame_part_groups(10923) != 2731) FAIL("parts of 2^20");
    if (frame_parts_error(1u << 20, 786336, 96) || !frame_parts_error(1u << 20, 786337, 96) || !frame_parts_error(1u << 20, 1 << 20, 96) ||
        !frame_parts_error(1u << 20, INT_MAX, 96))
        FAIL("grid limit");
    if (frame_parts_error(1u << 20, INT_MAX, 0) || frame_parts_error(96, INT_MAX, 96) || frame_parts_error(1u << 20, INT_MAX, 1048512))
        FAIL("one part per frame needs ceil(nframes / 4) workgroups");
    if (frame_parts_error(0, 4, 96) || frame_parts_error(250, 0, 96)) FAIL("the family's check reports maxFrameBits and nframes");
    // the plan: two arguments as before, one part the same, more parts nframes G workgroups
    for (int o : {0x012, 0x102, 0x003, 0x024}) {
        for (uint64_t n : {1ull, 3ull, 4ull, 5ull, 6401ull}) {
            const LaunchPlan a = plan_frames(o, n), b = plan_frames(o, n, 1), c = plan_frames(o, n, 11);
            if (!a.launches || a.form != Form::Tg || a.grid != (n + 3) / 4 || a.parts != 1 || a.seg != kSegNone || a.stats) FAIL("plan of whole frames");
            if (b.grid != a.grid || b.parts != 1 || c.grid != 3 * n || c.parts != 11 || c.form != Form::Tg || c.seg != kSegNone) FAIL("plan in parts");
            for (int in = 3; in <= 6; in++) {
                const std::string na = plan_name(a, o, in), nb = plan_name(b, o, in), nc = plan_name(c, o, in);
                if (na != nb || nc != na + ", 11 parts per frame: one part per wave") FAIL("names %s | %s", na.c_str(), nc.c_str());
            }
        }
        if (plan_frames(o, 0, 11).launches) FAIL("empty plan");
    }
    if (plan_frames(0x012, 786336, 10923).grid != 2147483616u) FAIL("largest grid");
    Geom g;
    if (g.frmPartW != 0 || g.frmPartG != 1) FAIL("Geom defaults");
    return 0;
}

int main()
{
    const uint32_t wps[] = {3, 6, 9, 32766};
    Frame f;
    for (uint32_t S = 1; S <= 400; S++)
        for (uint32_t Wp : wps)
            if (check_frame(f, S, Wp)) return 1;
    for (uint32_t S : {(1u << 20) - 31, 1u << 20})
        for (uint32_t Wp : wps)
            if (check_frame(f, S, Wp)) return 1;
    for (uint32_t Smax : {1u, 96u, 97u, 250u, 400u, 1000u, 1u << 20})
        for (uint32_t Wp : wps)
            for (int n : {1, 3, 5})
                if (check_waves(Smax, Wp, n)) return 1;
    if (check_args_and_plan()) return 1;
    printf("ok\n");
    return 0;
}
