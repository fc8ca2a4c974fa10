// Host check of the int8 frame geometry (vd_frames.h "int8 frames"), its argument checks, the four kernel tables of
// the byte twins (vd_plan.h) and their names against a plain enumeration (never against the header's own closed
// forms).  For a pattern and a frame of S stages the enumeration walks the frame's 2 S mother positions once,
// counting the kept ones: that gives every kept value's index in the frame's buffer -- its byte offset -- and the
// buffer's length in bytes.  The padded stream is stage p -> frame stage p - 26 for 26 <= p < 26 + S, nothing else;
// the extended stream is walked by stepping (stage 26 is frame stage 0, back 26 steps, forward with the wrap at S).
// For every family, every part length and every part of the frame, the groups of the part's run and the one it
// prefetches beyond, up to stage P + 96, and all 96 lanes of each group, the offsets of the chain the kernel runs are
// compared with it:
//   the byte offset lies inside the range (offset + access <= range) exactly when the stage's value is a real kept
//   value of the frame; there it equals the enumeration's index (unpunctured: 2 x the frame stage), and the float
//   helper's offset is 4 x it; outside, offset + access does not wrap in 32 bits and the float helper's offset is
//   outside its range too.
// Also: frame_args_error message by message for the int8 families, the 52 kernels of the four tables and the names of llr 7 .. 10.
// Arguments (tests/test_byte_frames.py passes the lists of tests/ptb_common.py): sizes=S,S,... parts=b,b,...
// pat=period,keep0,keep1 (repeated).  Built with hipcc and the host sanitizers; prints "ok" or the first mismatch.
#include <algorithm>
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

// idx[2 t + c]: index in the frame's buffer of output c of frame stage t, or -1 when punctured; kept: their number
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

// one access of `size` bytes at offset o against a range: inside, and (outside) free of 32-bit wrap-around
static bool inside(uint32_t o, uint32_t size, uint64_t range) { return (uint64_t)o + size <= range; }
static bool wraps(uint32_t o, uint32_t size) { return (uint64_t)o + size > 0x100000000ull; }

// the group starts the decode of part j (Wp words a part, 0: whole frames) reaches: its run's groups and the one
// prefetched beyond, below limit
static std::vector<uint32_t> part_groups(uint32_t S, uint32_t Wp, uint32_t j, uint32_t limit)
{
    std::vector<uint32_t> g;
    const FramePart fp = frame_part(S, Wp, j);
    if (!fp.words) return g;
    const uint32_t fst = frame_part_stage(Wp, j), blocks = fp.words + 2, ngroups = (blocks + 2) / 3 + 1;
    for (uint32_t k = 0; k < ngroups && fst + 96 * k < limit; k++) g.push_back(fst + 96 * k);
    return g;
}

static int check_frame(const Pat& p, uint32_t S, uint32_t partBits)
{
    const bool plain = p.period == 1 && p.k0 == 1 && p.k1 == 1;  // the unpunctured families run on (1, 1, 1) only
    const Punct pn = punct_make(p.period, p.k0, p.k1);
    Enum en;
    en.build(p, S);
    const uint64_t range = en.kept, frange = 4ull * en.kept;  // bytes of the int8 frame, of the float frame
    if (pfrm_bytes<1>(pn, S) != range || range != punct_len(pn, 2ull * S) || pfrm_bytes(pn, S) != frange)
        FAIL("(%d,0x%x,0x%x) S %u: pfrm_bytes<1> %u, enumeration %llu", p.period, p.k0, p.k1, S, pfrm_bytes<1>(pn, S),
             (unsigned long long)range);
    const uint32_t W = frame_words(S), P = frame_padded_stages(S), Wp = frame_part_words(partBits);
    const uint32_t limit = P + 96;
    const TbRecip rc = tb_recip(S);
    // the frame stage of every stage of the extended stream below limit + 96, by stepping
    std::vector<uint32_t> ext(limit + 96);
    {
        uint32_t t = 0;
        for (int i = 0; i < 26; i++) t = t == 0 ? S - 1 : t - 1;
        for (uint32_t q = 0; q < ext.size(); q++) {
            ext[q] = t;
            t = t + 1 == S ? 0 : t + 1;
        }
    }
    uint32_t seen = 0;
    for (uint32_t j = 0; j < frame_parts(S, Wp) + 1; j++) {
        for (uint32_t g0 : part_groups(S, Wp, j, limit)) {
            if (g0 % 96) FAIL("S %u part %u: group start %u", S, j, g0);
            seen++;
            // the scalar values of the group, as the kernel forms them (punctured frames)
            const PfrmGroup pg = pfrm_group(g0);
            uint32_t r0b, r0f;
            const uint32_t base1 = pfrm_base<1>(pn, pg.t0, &r0b), base4 = pfrm_base(pn, pg.t0, &r0f);
            if (base4 != 4 * base1 || r0b != r0f) FAIL("S %u group %u: base %u vs %u", S, g0, base1, base4);
            for (uint32_t s = 0; s < 96; s++) {
                const uint32_t q = g0 + s;
                const bool in_frame = q >= 26 && q - 26 < S;
                if (plain) {
                    // frames: one 16-bit access per stage against 2 S bytes
                    const uint32_t o = frame_offset<1>(q), of = frame_offset(q);
                    if (wraps(o, 2)) FAIL("frames S %u stage %u: offset 0x%x wraps", S, q, o);
                    if (inside(o, 2, 2ull * S) != in_frame || inside(of, 8, 8ull * S) != in_frame)
                        FAIL("frames S %u stage %u: offsets 0x%x / 0x%x, in frame %d", S, q, o, of, (int)in_frame);
                    if (in_frame && (o != 2 * (q - 26) || of != 4 * o)) FAIL("frames S %u stage %u: offset %u (float %u)", S, q, o, of);
                    // tail-biting frames: every stage is a frame stage
                    const uint32_t ot = tb_stage_offset<1>(g0, s, S, rc), otf = tb_stage_offset(g0, s, S, rc);
                    if (ot != 2 * ext[q] || otf != 4 * ot || !inside(ot, 2, 2ull * S) || tb_offset<1>(ext[q]) != ot)
                        FAIL("tail-biting S %u stage %u (frame stage %u): offset %u (float %u)", S, q, ext[q], ot, otf);
                }
                // punctured frames and punctured tail-biting frames: one 8-bit access per value
                const PfrmOff ob = pfrm_offsets<1>(pn, base1, r0b, pg.lead, s), of = pfrm_offsets(pn, base4, r0f, pg.lead, s);
                const PfrmOff tb = ptb_stage_offsets<1>(pn, g0, s, S, rc), tf = ptb_stage_offsets(pn, g0, s, S, rc);
                const uint32_t pb[2] = {ob.o0, ob.o1}, pf[2] = {of.o0, of.o1}, xb[2] = {tb.o0, tb.o1}, xf[2] = {tf.o0, tf.o1};
                for (int c = 0; c < 2; c++) {
                    const int32_t want = in_frame ? en.idx[2 * (size_t)(q - 26) + c] : -1;
                    if (wraps(pb[c], 1) || wraps(xb[c], 1)) FAIL("punctured S %u stage %u value %d: offset wraps", S, q, c);
                    if (inside(pb[c], 1, range) != (want >= 0) || inside(pf[c], 4, frange) != (want >= 0))
                        FAIL("punctured frames (%d,0x%x,0x%x) S %u stage %u value %d: offsets 0x%x / 0x%x, range %llu, want %d", p.period,
                             p.k0, p.k1, S, q, c, pb[c], pf[c], (unsigned long long)range, want);
                    if (want >= 0 && (pb[c] != (uint32_t)want || pf[c] != 4 * pb[c]))
                        FAIL("punctured frames (%d,0x%x,0x%x) S %u stage %u value %d: offset %u (float %u), want %d", p.period, p.k0,
                             p.k1, S, q, c, pb[c], pf[c], want);
                    const int32_t wt = en.idx[2 * (size_t)ext[q] + c];
                    if (inside(xb[c], 1, range) != (wt >= 0) || inside(xf[c], 4, frange) != (wt >= 0))
                        FAIL("punctured tail-biting (%d,0x%x,0x%x) S %u stage %u value %d: offsets 0x%x / 0x%x, want %d", p.period,
                             p.k0, p.k1, S, q, c, xb[c], xf[c], wt);
                    if (wt >= 0 ? xb[c] != (uint32_t)wt || xf[c] != 4 * xb[c] : xb[c] < 0x80000000u)
                        FAIL("punctured tail-biting (%d,0x%x,0x%x) S %u stage %u (frame stage %u) value %d: offset 0x%x (float 0x%x), want %d",
                             p.period, p.k0, p.k1, S, q, ext[q], c, xb[c], xf[c], wt);
                }
            }
        }
    }
    // whole frames: every group below P + 96 was visited; in parts: the parts' groups cover the frame's words
    if (Wp == 0 && seen != std::min<uint32_t>((W + 2 + 2) / 3 + 1, (limit + 95) / 96)) FAIL("S %u: %u groups visited", S, seen);
    if (seen == 0) FAIL("S %u parts of %u: no group visited", S, partBits);
    return 0;
}

static int check_args()
{
    struct A {
        uint64_t addr, istr, ostr, maxb;
        int nf, kind;
        float scale;
        int period;
        uint32_t k0, k1;
        uint64_t part;
        const char* why;  // a piece of the message, or null: accepted
    };
    const float inf = std::numeric_limits<float>::infinity();
    // 3/4 keeps 4 of 6: 1000 stages -> 1334 bytes; (1, 1, 1): 2000 bytes
    const A cases[] = {
        {0, 2000, 128, 1000, 4, 1, 1.0f, 1, 1, 1, 0, nullptr},              // the smallest strides
        {2, 2002, 132, 1000, 4, 0, 0.25f, 1, 1, 1, 0, nullptr},             // 2-byte alignment is enough
        {6, 2006, 128, 1000, 4, 2, 4.0f, 1, 1, 1, 96, nullptr},
        {1, 1335, 128, 1000, 4, 1, 1.0f, 3, 5, 3, 0, nullptr},              // punctured: any address, any stride
        {3, 1334, 128, 1000, 4, 2, 1.0f, 3, 5, 3, 192, nullptr},
        {1, 0, 0, 1000, 1, 1, 1.0f, 3, 5, 3, 0, nullptr},                   // one frame: no stride needed
        {0, 0, 4, 15, 3, 0, 1.0f, 16, 0x8000, 0, 0, nullptr},               // frames without a kept value
        {0, 1, 4, 16, 3, 2, 1.0f, 16, 0x8000, 0, 0, nullptr},
        {0, 2ull << 20, 4ull << 15, 1u << 20, 2, 1, 1.0f, 1, 1, 1, 0, nullptr},
        {0, 2000, 128, 1000, 4, 2, 1e-40f, 1, 1, 1, 0, nullptr},            // tail-biting: any finite scale > 0
        {0, 2000, 128, 1000, 4, 2, 3e38f, 3, 5, 3, 0, nullptr},
        {0, 2000, 128, 1000, 4, 3, 1.0f, 1, 1, 1, 0, "kind must be"},       // the kind
        {0, 2000, 128, 1000, 4, -1, 1.0f, 1, 1, 1, 0, "kind must be"},
        {0, 2000, 128, 1000, 4, 1, 1.0f, 0, 1, 1, 0, "invalid puncture pattern"},
        {0, 2000, 128, 1000, 4, 1, 1.0f, 17, 1, 1, 0, "invalid puncture pattern"},
        {0, 2000, 128, 1000, 4, 1, 1.0f, 3, 8, 3, 0, "invalid puncture pattern"},
        {0, 2000, 128, 1000, 4, 1, 1.0f, 3, 0, 0, 0, "invalid puncture pattern"},
        {0, 2000, 128, 0, 4, 1, 1.0f, 1, 1, 1, 0, "maxFrameBits must be in"},
        {0, 4ull << 20, 1ull << 20, (1u << 20) + 1, 4, 1, 1.0f, 1, 1, 1, 0, "maxFrameBits must be in"},
        {0, 2000, 128, 1000, 0, 1, 1.0f, 1, 1, 1, 0, "nframes must be >= 1"},
        {0, 2000, 128, 1000, -1, 2, 1.0f, 1, 1, 1, 0, "nframes must be >= 1"},
        {0, 2000, 128, 1000, 4, 1, 0.0f, 1, 1, 1, 0, "(and -65536 / scale finite)"},  // the scale: the pad must exist
        {0, 2000, 128, 1000, 4, 0, -1.0f, 1, 1, 1, 0, "(and -65536 / scale finite)"},
        {0, 2000, 128, 1000, 4, 1, inf, 1, 1, 1, 0, "(and -65536 / scale finite)"},
        {0, 2000, 128, 1000, 4, 0, std::nanf(""), 3, 5, 3, 0, "(and -65536 / scale finite)"},
        {0, 2000, 128, 1000, 4, 1, 1e-40f, 1, 1, 1, 0, "(and -65536 / scale finite)"},
        {0, 2000, 128, 1000, 4, 2, 0.0f, 1, 1, 1, 0, "scale must be finite and > 0"},  // ... tail-biting: finite and > 0
        {0, 2000, 128, 1000, 4, 2, -0.0f, 3, 5, 3, 0, "scale must be finite and > 0"},
        {0, 2000, 128, 1000, 4, 2, inf, 1, 1, 1, 0, "scale must be finite and > 0"},
        {0, 2000, 128, 1000, 4, 2, std::nanf(""), 1, 1, 1, 0, "scale must be finite and > 0"},
        {1, 2000, 128, 1000, 4, 1, 1.0f, 1, 1, 1, 0, "multiples of 2 bytes"},  // alignment under (1, 1, 1)
        {0, 2001, 128, 1000, 4, 2, 1.0f, 1, 1, 1, 0, "multiples of 2 bytes"},
        {3, 0, 128, 1000, 1, 0, 1.0f, 1, 1, 1, 0, "multiples of 2 bytes"},
        {0, 2000, 130, 1000, 4, 1, 1.0f, 1, 1, 1, 0, "output_stride must be a multiple of 4"},
        {1, 1335, 129, 1000, 4, 1, 1.0f, 3, 5, 3, 0, "output_stride must be a multiple of 4"},
        {0, 1998, 128, 1000, 4, 1, 1.0f, 1, 1, 1, 0, "q_stride smaller than"},  // overlapping frames
        {0, 1333, 128, 1000, 4, 2, 1.0f, 3, 5, 3, 0, "q_stride smaller than"},
        {0, 0, 128, 1000, 2, 1, 1.0f, 3, 5, 3, 0, "q_stride smaller than"},
        {0, 0, 4, 16, 3, 1, 1.0f, 16, 0x8000, 0, 0, "q_stride smaller than"},
        {0, 2000, 124, 1000, 4, 1, 1.0f, 1, 1, 1, 0, "output_stride smaller than"},
        {0, 1334, 0, 1000, 2, 2, 1.0f, 3, 5, 3, 0, "output_stride smaller than"},
        {0, 2000, 128, 1000, 4, 1, 1.0f, 1, 1, 1, 100, "partBits must be 0 or a multiple of 96"},  // the part length
        {0, 2ull << 20, 4ull << 15, 1u << 20, 0x7FFFFFFF, 1, 1.0f, 1, 1, 1, 96, "more than 2^31 - 1 workgroups"},
    };
    int i = 0;
    for (const A& a : cases) {
        const char* why = check({!byte_frames_unpunctured(a.period, a.k0, a.k1), a.kind == kByteFramesTailbiting, true, false}, a.addr, a.istr, a.ostr,
                                a.maxb, a.nf, a.kind, a.scale, a.period, a.k0, a.k1, a.part);
        if (a.why ? !why || !strstr(why, a.why) : why != nullptr)
            FAIL("argument case %d: %s, want %s", i, why ? why : "accepted", a.why ? a.why : "accepted");
        i++;
    }
    return 0;
}

static int check_table()
{
    // a byte twin exactly for HARD, SOFT4 and SOFT8 (the punctured families: not HARD), both output widths: 52
    int n[4] = {0, 0, 0, 0};
    for (int ch = -1; ch <= 5; ch++)
        for (int me = -1; me <= 3; me++)
            for (int o16 = 0; o16 < 2; o16++)
                for (int fam = 0; fam < 4; fam++) {
                    const bool pun = fam & 1, tb = fam & 2;
                    const bool want = ch >= (pun ? 1 : 0) && ch <= 2 && me >= 0 && me < 3 && has_kernel(Form::Tg, ch, me);
                    const bool got = launcher_frames<Stub>({pun, tb, true, false}, ch, me, o16 != 0) != nullptr;
                    if (got != want) FAIL("table family %d: %d %d %d", fam, ch, me, o16);
                    // ... and the float twin exists wherever the byte one does
                    const bool twin = launcher_frames<Stub>({pun, tb, false, false}, ch, me, o16 != 0) != nullptr;
                    if (got && !twin) FAIL("table family %d: %d %d %d has no float twin", fam, ch, me, o16);
                    n[fam] += got;
                }
    if (n[0] != 16 || n[1] != 10 || n[2] != 16 || n[3] != 10) FAIL("%d + %d + %d + %d byte kernels", n[0], n[1], n[2], n[3]);
    // the names: the float twin's with I8+ after FRM+
    const char* twins[4] = {"FRM+", "FRM+PUN+", "FRM+TB+", "FRM+TB+PUN+"};
    const char* bytes[4] = {"FRM+I8+", "FRM+I8+PUN+", "FRM+I8+TB+", "FRM+I8+TB+PUN+"};
    for (int k = 0; k < 4; k++)
        for (int o : {0x012, 0x102, 0x021, 0x000})
            for (uint32_t parts : {1u, 3u}) {
                std::string a = plan_name(plan_frames(o, 5, parts), o, 3 + k);
                const std::string b = plan_name(plan_frames(o, 5, parts), o, 7 + k);
                const size_t at = a.find(twins[k]);
                if (at == std::string::npos) FAIL("name %s", a.c_str());
                a.replace(at, strlen(twins[k]), bytes[k]);
                if (a != b) FAIL("name %s, want %s", b.c_str(), a.c_str());
            }
    if (plan_name(plan_frames(0x012, 4), 0x012, 10).rfind("vd_decode_tg<FRM+I8+TB+PUN+SOFT8,B16,O32> one frame per wave, ", 0) != 0) FAIL("name");
    if (plan_name(plan_frames(0x012, 0), 0x012, 7) != "-") FAIL("empty plan");
    // the channel ids of the byte twins collide with no other range (kFrm + kTb + kPun + FP32 = 76 is the highest)
    static_assert(kI8 + kFrm + HARD > kFrm + kTb + kPun + FP32 && (kI8 & (kFrm | kTb | kPun | 7)) == 0, "channel id range");
    return 0;
}

int main(int argc, char** argv)
{
    std::vector<uint32_t> sizes, parts;
    std::vector<Pat> pats;
    for (int i = 1; i < argc; i++) {
        if (!strncmp(argv[i], "sizes=", 6)) sizes = list_of(argv[i] + 6);
        else if (!strncmp(argv[i], "parts=", 6)) parts = list_of(argv[i] + 6);
        else if (!strncmp(argv[i], "pat=", 4)) {
            const std::vector<uint32_t> v = list_of(argv[i] + 4);
            if (v.size() != 3) FAIL("argument %s", argv[i]);
            pats.push_back({(int)v[0], v[1], v[2]});
        } else FAIL("argument %s", argv[i]);
    }
    if (sizes.empty() || parts.empty() || pats.empty()) FAIL("usage: sizes=S,... parts=b,... pat=period,keep0,keep1 ...");
    for (const Pat& p : pats) {
        if (!punct_valid(p.period, p.k0, p.k1)) FAIL("pattern");
        for (uint32_t S : sizes)
            for (uint32_t pb : parts) {
                if (!frame_part_bits_valid(pb)) FAIL("part length %u", pb);
                if (check_frame(p, S, pb)) return 1;
            }
    }
    if (check_args() || check_table()) return 1;
    printf("ok %zu sizes %zu parts %zu patterns\n", sizes.size(), parts.size(), pats.size());
    return 0;
}
