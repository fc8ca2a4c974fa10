// vd_plan.h -- which kernel, launch form and grid a decode takes, as a pure host-side function of the option,
// the sizes, the knobs read at vd_create and the device's SIMD and segment-table counts (no HIP runtime calls,
// no decoder: tests/cxx/plan_check.cpp checks it on the CPU), with the option helpers, the list of kernels
// and the kernel names.  Shared by the C-ABI (vd_capi.hip) and the timing tools.
// Include after vd_kernel_tg.h (kSplitMinWords, kLlr, kPun, kFrm; the tools include their ablation copy of it).
#pragma once
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <string>
#include "vd_frames.h"
#include "vd_segplan.h"

namespace vd {

// ---------------------------------------------------------------- options (include/viterbi.h bit fields)
inline int ch_of(int o) { return o & 0xF; }
inline int met_of(int o) { return (o >> 4) & 0xF; }
inline int out_of(int o) { return (o >> 8) & 0xF; }
inline int comp_of(int o) { return (o >> 12) & 0xF; }
inline int bpp_of(int o) { return out_of(o) == 1 ? 16 : 32; }

inline bool valid(int o)
{
    if (o & ~0xFFFF) return false;
    int ch = ch_of(o), me = met_of(o), out = out_of(o), cm = comp_of(o);
    if (ch > 4 || me > 2 || out > 1 || cm > 1) return false;
    // OptionsValid (viterbi.h:22-41)
    if (ch == 2 && me == 2) return false;
    if (ch == 3 && me == 2) return false;
    if (ch == 3 && me == 1) return false;
    if (me == 2 && cm == 1) return false;
    return true;
}

inline size_t input_size(int o, size_t n)
{
    switch (ch_of(o)) {
    case 0: return (n + 7) / 8;
    case 1: return (n + 1) / 2;
    case 2: return n;
    case 3: return n * 2;
    case 4: return n * 4;
    }
    return 0;
}
inline size_t message_len(int o, size_t n)
{
    if (n / 2 < 64) return 0;  // the reference underflows here (size_t); rejected instead
    size_t bpp = (size_t)bpp_of(o);
    return (n / 2 - 64) / bpp * bpp;
}
// stages whose channel data lies in whole 32-bit words of the caller's buffer
inline uint64_t avail_stages(int o, size_t n)
{
    size_t words = input_size(o, n) / 4;
    uint64_t per = 0;
    switch (ch_of(o)) {
    case 0: per = words * 16; break;
    case 1: per = words * 4; break;
    case 2: per = words * 2; break;
    case 3: per = words; break;
    case 4: per = words / 2; break;
    }
    uint64_t half = n / 2;
    return per < half ? per : half;
}

// ---------------------------------------------------------------- the kernels
// The valid (format, metric) pairs, written once.  vd_decode_tg has a kernel for each (SOFT16 on int32
// patterns, TgFmt::INT); vd_decode_pk (two chunks per wave in int16 halves, vd_kernel_pk.h) for all but SOFT16.
#define VD_PK_PAIRS(X) \
    X(HARD, B32) X(HARD, B16) X(HARD, F16) X(SOFT4, B32) X(SOFT4, B16) X(SOFT4, F16) X(SOFT8, B32) X(SOFT8, B16) \
    X(FP32, B32) X(FP32, B16) X(FP32, F16)
#define VD_TG_PAIRS(X) VD_PK_PAIRS(X) X(SOFT16, B32)

// launch form, and with it the kernel family: vd_decode_tg, vd_decode_pk<.., false>, vd_decode_pk<.., true>
enum class Form : int { Tg = 0, PkBatched = 1, PkSplit = 2 };

inline bool has_kernel(Form f, int ch, int me)
{
#define VD_X(C, M) if (ch == C && me == M) return true;
    if (f == Form::Tg) { VD_TG_PAIRS(VD_X) } else { VD_PK_PAIRS(VD_X) }
#undef VD_X
    return false;
}

// The launcher of the kernel for (form, llr, format, metric, output width), null where none exists.  L gives
// the pointer type L::fn and the launchers L::tg<CH, CORE, OB> and L::pk<CH, CORE, OB, SPL>, one kernel each
// (vd_capi.hip; plan_check.cpp passes stubs): 12 pairs x {O32, O16} x {packed, LLR} of vd_decode_tg, 11 pairs
// x {O32, O16} x {batched, SPL} x {packed, LLR} of vd_decode_pk.  llr: float channel values, quantised in
// the table build (fused SoftDecisionPacker): channel ids kLlr + format.
template <class L>
typename L::fn launcher(Form f, bool llr, int ch, int me, bool o16)
{
    struct Table {
        typename L::fn at[3][2][5][3][2] = {};
        Table()
        {
            constexpr int T = (int)Form::Tg, B = (int)Form::PkBatched, S = (int)Form::PkSplit;
#define VD_ROW(F, C, M, K, ...)                                   \
    at[F][0][C][M][0] = &L::template K<C, M, 32 __VA_ARGS__>;        \
    at[F][0][C][M][1] = &L::template K<C, M, 16 __VA_ARGS__>;        \
    at[F][1][C][M][0] = &L::template K<kLlr + C, M, 32 __VA_ARGS__>; \
    at[F][1][C][M][1] = &L::template K<kLlr + C, M, 16 __VA_ARGS__>;
#define VD_X(C, M) VD_ROW(T, C, M, tg, )
            VD_TG_PAIRS(VD_X)
#undef VD_X
#define VD_X(C, M) VD_ROW(B, C, M, pk, , false) VD_ROW(S, C, M, pk, , true)
            VD_PK_PAIRS(VD_X)
#undef VD_X
#undef VD_ROW
        }
    };
    static const Table t;
    return ch >= 0 && ch < 5 && me >= 0 && me < 3 ? t.at[(int)f][llr][ch][me][o16] : nullptr;
}

// Punctured float input (channel ids kPun + format, vd_kernel_tg.h): vd_decode_tg only, every valid pair but
// HARD's (an erasure has no hard code), 9 pairs x {O32, O16}.  A table of its own: launcher<L>'s holds exactly
// the kernels of the packed and LLR plans.  Punctured decodes are planned with Knobs::pk = 0 (punct_knobs): one
// chunk per wave, batched, or a segment launch for long single batches.
#define VD_PUN_PAIRS(X) \
    X(SOFT4, B32) X(SOFT4, B16) X(SOFT4, F16) X(SOFT8, B32) X(SOFT8, B16) X(SOFT16, B32) X(FP32, B32) X(FP32, B16) X(FP32, F16)
template <class L>
typename L::fn launcher_punct(int ch, int me, bool o16)
{
    struct Table {
        typename L::fn at[5][3][2] = {};
        Table()
        {
#define VD_X(C, M)                                      \
    at[C][M][0] = &L::template tg<kPun + C, M, 32>;     \
    at[C][M][1] = &L::template tg<kPun + C, M, 16>;
            VD_PUN_PAIRS(VD_X)
#undef VD_X
        }
    };
    static const Table t;
    return ch >= 0 && ch < 5 && me >= 0 && me < 3 ? t.at[ch][me][o16] : nullptr;
}

// Frame launches (vd_frames.h; channel ids kFrm + kPun, kTb, kI8, kMix by the family's bits + format, vd_kernel_tg.h):
// vd_decode_tg only, planned by plan_frames, in one table of their own indexed by the family record.  A row per family
// that has kernels, each over a pair list x {O32, O16}:
//   frames, tail-biting frames: all 12 pairs (HARD too: a terminated frame needs no neutral code, a tail-biting one has
//     no pad and no erasure), 24 kernels each; their punctured twins: the 9 punctured pairs, 18 each;
//   the int8 twins of the four: HARD, SOFT4 and SOFT8, 8 pairs (16 kernels) unpunctured, the 5 without HARD (10)
//     punctured;
//   mixed frames, padded and tail-biting: punctured kernels (pun is set), 18 each for floats and 10 each for int8.
// 84 + 52 + 56 = 192 kernels; every other combination of the bits (mix without pun) has none and returns null.
#define VD_BYTE_PUN_PAIRS(X) X(SOFT4, B32) X(SOFT4, B16) X(SOFT4, F16) X(SOFT8, B32) X(SOFT8, B16)
#define VD_BYTE_PAIRS(X) X(HARD, B32) X(HARD, B16) X(HARD, F16) VD_BYTE_PUN_PAIRS(X)
inline constexpr int frame_family_index(FrameFamily f) { return f.pun + 2 * f.tb + 4 * f.i8 + 8 * f.mix; }
template <class L>
typename L::fn launcher_frames(FrameFamily f, int ch, int me, bool o16)
{
    struct Table {
        typename L::fn at[16][5][3][2] = {};
        Table()
        {
#define VD_X(C, M)                                        \
    at[fam][C][M][0] = &L::template tg<id + C, M, 32>;    \
    at[fam][C][M][1] = &L::template tg<id + C, M, 16>;
#define VD_FAMILY(PUN, TB, I8, MIX, PAIRS)                                                       \
    {                                                                                            \
        constexpr int fam = frame_family_index({PUN != 0, TB != 0, I8 != 0, MIX != 0});          \
        constexpr int id = kFrm + PUN * kPun + TB * kTb + I8 * kI8 + MIX * kMix;                 \
        PAIRS(VD_X)                                                                              \
    }
            VD_FAMILY(0, 0, 0, 0, VD_TG_PAIRS) VD_FAMILY(1, 0, 0, 0, VD_PUN_PAIRS)
            VD_FAMILY(0, 1, 0, 0, VD_TG_PAIRS) VD_FAMILY(1, 1, 0, 0, VD_PUN_PAIRS)
            VD_FAMILY(0, 0, 1, 0, VD_BYTE_PAIRS) VD_FAMILY(1, 0, 1, 0, VD_BYTE_PUN_PAIRS)
            VD_FAMILY(0, 1, 1, 0, VD_BYTE_PAIRS) VD_FAMILY(1, 1, 1, 0, VD_BYTE_PUN_PAIRS)
            VD_FAMILY(1, 0, 0, 1, VD_PUN_PAIRS) VD_FAMILY(1, 1, 0, 1, VD_PUN_PAIRS)
            VD_FAMILY(1, 0, 1, 1, VD_BYTE_PUN_PAIRS) VD_FAMILY(1, 1, 1, 1, VD_BYTE_PUN_PAIRS)
#undef VD_FAMILY
#undef VD_X
        }
    };
    static const Table t;
    return ch >= 0 && ch < 5 && me >= 0 && me < 3 ? t.at[frame_family_index(f)][ch][me][o16] : nullptr;
}
static_assert(kFrameHard == HARD && kFrameSoft8 == SOFT8, "vd_frames.h names the formats its refusals go by");

// ---------------------------------------------------------------- the knobs (read once, at vd_create)
struct Knobs {
    int split = 1;    // segment launches: 0 none (VD_NO_SPLIT=1), 1 pieces, 2 thirds, 3 sevenths (VD_SPLIT=...)
    int pk = 1;       // HARD/SOFT4/SOFT8/FP32 launches on vd_decode_pk (VD_NO_PK=1: on vd_decode_tg)
    int pksplit = 1;  // their single-batch launches split on vd_decode_pk (VD_PK_SPLIT=0: tg segments)
    int pktail = 1;   // ... with the tail chunks in 4-wave workgroups (VD_PK_TAIL=0: one chunk per wave)
};
inline Knobs knobs_from_env()
{
    auto is = [](const char* name, char c) { const char* v = std::getenv(name); return v && v[0] == c; };
    const char* smode = std::getenv("VD_SPLIT");
    Knobs k;
    k.split = is("VD_NO_SPLIT", '1') ? 0 : smode && !strcmp(smode, "thirds") ? 2 : smode && !strcmp(smode, "sevenths") ? 3 : 1;
    k.pk = is("VD_NO_PK", '1') ? 0 : 1;
    k.pksplit = is("VD_PK_SPLIT", '0') ? 0 : 1;
    k.pktail = is("VD_PK_TAIL", '0') ? 0 : 1;
    return k;
}
// the knobs a punctured decode is planned with: vd_decode_tg's forms only (there are no vd_decode_pk twins)
inline Knobs punct_knobs(Knobs k)
{
    k.pk = 0;
    return k;
}

// ---------------------------------------------------------------- the plan
constexpr int kSegNone = -1;
struct LaunchPlan {
    bool launches = false;  // false: packNum == 0, nothing to decode (the other fields then mean nothing)
    Form form = Form::Tg;
    unsigned grid = 0;      // workgroups of kWaves waves
    uint32_t tailWG = ~0u;  // Geom::tailWG (split launches with tail workgroups)
    int seg = kSegNone;     // the SegMode of a segment launch's table (Geom::seg)
    bool stats = false;     // Geom::stats set: segment and split launches count their re-decodes
    uint64_t packNum = 0;   // Geom::packNum
    uint32_t parts = 1;     // frame launches: the parts of the longest frame (1: one frame per wave)
};

// nbatch batches of inputNum encoded values on a device of nsimd SIMDs whose segment tables (vd_segplan.h,
// indexed by SegMode) have segWG[] workgroups, 0 for an absent table:
//  * batched launches of HARD/SOFT4/SOFT8/FP32 on vd_decode_pk, two chunks per wave: nchunks nbatch / 8 workgroups;
//  * their single batches with chunks of >= kSplitMinWords 32-bit words on vd_decode_pk's split kernel, one
//    chunk per wave cut in two halves (nchunks / 4 workgroups), the last nchunks mod nsimd chunks one per
//    workgroup of 4 waves (8 parts each): with 6400 chunks on 1024 SIMDs every SIMD then runs 6 whole-chunk
//    waves and one short one (vd_kernel_pk.h "split");
//    (SOFT8: the split kernel is 9 % faster than vd_decode_tg's segment launch on codewords and, with the
//    early-stop re-decodes, 18 % slower on noise-only input: DESIGN.md 4.3)
//  * the rest on vd_decode_tg: a segment launch for single batches when the chunks are long enough and the
//    device has a table (thirds and sevenths fall back to pieces), else one chunk per wave.
// llr (float channel values) changes the kernel, never the plan: every kernel has its LLR twin.
inline LaunchPlan plan_launch(int o, size_t inputNum, uint32_t nbatch, bool llr, const Knobs& k, int nsimd,
                              const unsigned segWG[3])
{
    (void)llr;
    LaunchPlan p;
    p.packNum = message_len(o, inputNum) / (size_t)bpp_of(o);
    p.launches = p.packNum != 0;
    if (!p.launches) return p;
    const uint32_t nch = kChunks;
    const uint64_t words32 = out_of(o) != 0 ? p.packNum / 2 : p.packNum;  // O_B16: 16-bit words
    const bool longChunks = nbatch == 1 && k.split && words32 / nch >= (uint64_t)kSplitMinWords;
    if (nbatch > 1 && k.pk && nch % (2 * kWaves) == 0 && has_kernel(Form::PkBatched, ch_of(o), met_of(o))) {
        p.form = Form::PkBatched;
        p.grid = (unsigned)((uint64_t)nch * nbatch / (2 * kWaves));
    } else if (longChunks && k.pk && k.pksplit && nch % kWaves == 0 && has_kernel(Form::PkSplit, ch_of(o), met_of(o))) {
        p.form = Form::PkSplit;
        p.stats = true;
        const uint32_t tailc = nsimd > 0 ? nch % (uint32_t)nsimd : 0u;
        p.grid = nch / kWaves;
        if (k.pktail && tailc) {
            p.tailWG = (nch - tailc) / kWaves;
            p.grid = p.tailWG + tailc;
        }
    } else {
        const int want = k.split - 1;  // the knob's SegMode
        if (longChunks) p.seg = want > kSegPieces && segWG[want] ? want : segWG[kSegPieces] ? (int)kSegPieces : kSegNone;
        p.stats = p.seg != kSegNone;
        p.grid = p.stats ? segWG[p.seg] : (unsigned)(((uint64_t)nch * nbatch + kWaves - 1) / kWaves);
    }
    return p;
}

// nframes independent frames (vd_frames.h): one frame per wave on vd_decode_tg<FRM+...>, whatever the knobs say
// (no vd_decode_pk twins, no segment launch)
// partsMax > 1 (vd_frames.h "frames in parts"): the launch's longest frame has that many parts, every frame gets
// G = frame_part_groups(partsMax) workgroups and each of their waves one part; the caller has checked
// frame_parts_error, so nframes G fits the grid
inline LaunchPlan plan_frames(int o, uint64_t nframes, uint32_t partsMax = 1)
{
    LaunchPlan p;
    p.launches = valid(o) && nframes != 0;
    p.form = Form::Tg;
    p.parts = partsMax > 1 ? partsMax : 1u;
    p.grid = p.parts > 1 ? (unsigned)(nframes * frame_part_groups(p.parts)) : (unsigned)((nframes + kWaves - 1) / kWaves);
    return p;
}

// ---------------------------------------------------------------- names
inline constexpr const char* kChNames[5] = {"HARD", "SOFT4", "SOFT8", "SOFT16", "FP32"};
inline constexpr const char* kCoreNames[3] = {"B32", "B16", "F16"};

// vd_decoder_kernel_name: the kernel and launch form of one planned launch; input: 0 packed words, 1 float
// channel values (LLR), 2 punctured float values (PUN), 3 frames of float values (FRM; a plan of plan_frames),
// 4 punctured frames (FRM+PUN; a plan of plan_frames), 5 tail-biting frames (FRM+TB; a plan of plan_frames),
// 6 punctured tail-biting frames (FRM+TB+PUN; a plan of plan_frames), 7 .. 10 the int8 twins of 3 .. 6 (FRM+I8+...),
// 11, 12 mixed frames, padded and tail-biting (FRM+MIX+PUN, FRM+MIX+TB+PUN), 13, 14 their int8 twins (FRM+I8+MIX+...)
inline std::string plan_name(const LaunchPlan& p, int o, int input)
{
    if (!p.launches) return "-";
    const bool frames = input >= 3 && input <= 14;
    const FrameFamily f = frames ? frame_family_of_input(input) : FrameFamily{};
    const std::string fam = std::string("FRM+") + (f.i8 ? "I8+" : "") + (f.mix ? "MIX+" : "") + (f.tb ? "TB+" : "") + (f.pun ? "PUN+" : "");
    const std::string args = (frames ? fam : input == 2 ? "PUN+" : input ? "LLR+" : "") + std::string(kChNames[ch_of(o)]) + "," +
                             kCoreNames[met_of(o)] + "," + (out_of(o) ? "O16" : "O32") + ">";
    if (frames)
        return "vd_decode_tg<" + args + " one frame per wave, " + (ch_of(o) == SOFT16 ? "int32 tagged patterns" : "fp32 tagged core") +
               (p.parts > 1 ? ", " + std::to_string(p.parts) + " parts per frame: one part per wave" : "");
    if (p.form == Form::PkBatched) return "vd_decode_pk<" + args + " batched: two chunks per wave, int16 halves";
    if (p.form == Form::PkSplit) return "vd_decode_pk<" + args + " split: one chunk per wave cut in two, int16 halves";
    return "vd_decode_tg<" + args + (p.seg != kSegNone ? " segment launch: one chunk or piece per wave, " : " one chunk per wave, ") +
           (ch_of(o) == SOFT16 ? "int32 tagged patterns" : "fp32 tagged core");
}

// vd_kernel_name: the kernels of an option.  The metric names the option's tie rule.  vd_decode_tg computes on
// the fp32 exact-integer tagged core (SOFT16: int32 patterns); vd_decode_pk (HARD / SOFT4 / SOFT8 / FP32) on
// exact-integer tagged int16 halves, two chunks per lane; none on fp16 arithmetic
inline std::string option_kernels(int o)
{
    static const char* ties[3] = {"M_B32", "M_B16", "M_FP16"};
    if (!valid(o)) return "-";
    const std::string fm = std::string("<") + kChNames[ch_of(o)] + "," + kCoreNames[met_of(o)] + ">";
    if (!has_kernel(Form::PkBatched, ch_of(o), met_of(o)))
        return "vd_decode_tg" + fm + " (int32 tagged patterns, " + ties[met_of(o)] + " tie rule)";
    return "vd_decode_pk" + fm + " (int16 halves" + (ch_of(o) == SOFT8 ? ", 2-stage fields" : "") +
           ": batched, two chunks per lane; single batch, one chunk cut in two) / vd_decode_tg" + fm +
           " (single batches with chunks under " + std::to_string(kSplitMinWords) + " words); " + ties[met_of(o)] + " tie rule";
}

}  // namespace vd
