// Host check of the launch plan (vd_plan.h): form, grid, tail workgroups, segment table, stats and packNum of
// plan_launch, the knobs read from the environment, the names of plan_name, the kernel table and the frame table, against
// values worked out by hand from the rules (never from plan_launch itself).  nsimd = 1024 (256 CUs) unless a
// case says otherwise; the segment tables' workgroup counts come from vd_segplan.h.
// Built with hipcc on the host by tests/test_plan.py; prints "ok" or the first mismatch.
#include <cstdio>
#include <cstdlib>
#include <sstream>
#include <string>
#include "vd_kernel_tg.h"
#include "vd_plan.h"

using namespace vd;

// stand-ins for the kernel launchers: the table's shape without instantiating a kernel
struct Stub {
    using fn = void (*)();
    template <int CH, int CORE, int OB> static void tg() {}
    template <int CH, int CORE, int OB, bool SPL> static void pk() {}
};

static const char* kEnv[] = {"VD_NO_SPLIT", "VD_SPLIT", "VD_NO_PK", "VD_PK_SPLIT", "VD_PK_TAIL"};
static Knobs knobs(const char* env)  // "NAME=value NAME=value" as a shell would set them
{
    for (const char* e : kEnv) unsetenv(e);
    std::istringstream in(env);
    for (std::string kv; in >> kv;) setenv(kv.substr(0, kv.find('=')).c_str(), kv.substr(kv.find('=') + 1).c_str(), 1);
    return knobs_from_env();
}
static LaunchPlan plan(int o, size_t n, uint32_t nbatch, bool llr, const char* env, int nsimd)
{
    unsigned wg[3];
    for (int m = 0; m < 3; m++) {
        const std::vector<uint32_t> t = seg_table(nsimd, m);
        wg[m] = t.empty() ? 0u : (unsigned)(t.size() - 1);
    }
    return plan_launch(o, n, nbatch, llr, knobs(env), nsimd, wg);
}

constexpr int HARD_B32 = 0x000, SOFT16_B32 = 0x003, SOFT8_B16_O16 = 0x112, SOFT8_B16 = 0x012, HARD_F16_O16 = 0x120;
constexpr uint32_t kNoTail = ~0u;
constexpr size_t k64M = 64000000;

struct Case {
    const char* what;
    int o;
    size_t n;
    uint32_t nbatch;
    bool llr;
    const char* env;
    int nsimd;
    Form form;
    unsigned grid;
    uint32_t tailWG;
    int seg;
    bool stats;
    uint64_t packNum;
};
static const Case kCases[] = {
    {"HARD defaults", HARD_B32, k64M, 1, false, "", 1024, Form::PkSplit, 1792, 1536, kSegNone, true, 999998},
    {"HARD VD_PK_TAIL=0", HARD_B32, k64M, 1, false, "VD_PK_TAIL=0", 1024, Form::PkSplit, 1600, kNoTail, kSegNone, true, 999998},
    {"HARD VD_PK_SPLIT=0", HARD_B32, k64M, 1, false, "VD_PK_SPLIT=0", 1024, Form::Tg, 1792, kNoTail, kSegPieces, true, 999998},
    {"HARD thirds", HARD_B32, k64M, 1, false, "VD_PK_SPLIT=0 VD_SPLIT=thirds", 1024, Form::Tg, 2048, kNoTail, kSegThirds, true, 999998},
    {"HARD sevenths", HARD_B32, k64M, 1, false, "VD_PK_SPLIT=0 VD_SPLIT=sevenths", 1024, Form::Tg, 1792, kNoTail, kSegSevenths, true, 999998},
    {"HARD VD_NO_SPLIT=1", HARD_B32, k64M, 1, false, "VD_NO_SPLIT=1", 1024, Form::Tg, 1600, kNoTail, kSegNone, false, 999998},
    {"HARD VD_NO_PK=1", HARD_B32, k64M, 1, false, "VD_NO_PK=1", 1024, Form::Tg, 1792, kNoTail, kSegPieces, true, 999998},
    {"HARD x20", HARD_B32, k64M, 20, false, "", 1024, Form::PkBatched, 16000, kNoTail, kSegNone, false, 999998},
    {"HARD x20 VD_NO_PK=1", HARD_B32, k64M, 20, false, "VD_NO_PK=1", 1024, Form::Tg, 32000, kNoTail, kSegNone, false, 999998},
    {"SOFT16", SOFT16_B32, k64M, 1, false, "", 1024, Form::Tg, 1792, kNoTail, kSegPieces, true, 999998},
    {"SOFT16 x20", SOFT16_B32, k64M, 20, false, "", 1024, Form::Tg, 32000, kNoTail, kSegNone, false, 999998},
    {"SOFT8/B16/O16", SOFT8_B16_O16, k64M, 1, false, "", 1024, Form::PkSplit, 1792, 1536, kSegNone, true, 1999996},
    {"HARD 64 words per chunk", HARD_B32, 26214528, 1, false, "", 1024, Form::PkSplit, 1792, 1536, kSegNone, true, 409600},
    {"HARD 409599 words", HARD_B32, 26214464, 1, false, "", 1024, Form::Tg, 1600, kNoTail, kSegNone, false, 409599},
    {"HARD 39 words per chunk", HARD_B32, 16000000, 1, false, "", 1024, Form::Tg, 1600, kNoTail, kSegNone, false, 249998},
    {"HARD one word", HARD_B32, 192, 1, false, "", 1024, Form::Tg, 1600, kNoTail, kSegNone, false, 1},
    {"HARD 1216 SIMDs", HARD_B32, k64M, 1, false, "", 1216, Form::PkSplit, 1840, 1520, kSegNone, true, 999998},
    {"HARD 1216 SIMDs VD_PK_SPLIT=0", HARD_B32, k64M, 1, false, "VD_PK_SPLIT=0", 1216, Form::Tg, 1600, kNoTail, kSegNone, false, 999998},
    {"LLR HARD defaults", HARD_B32, k64M, 1, true, "", 1024, Form::PkSplit, 1792, 1536, kSegNone, true, 999998},
    {"LLR HARD x20", HARD_B32, k64M, 20, true, "", 1024, Form::PkBatched, 16000, kNoTail, kSegNone, false, 999998},
    {"LLR SOFT16", SOFT16_B32, k64M, 1, true, "", 1024, Form::Tg, 1792, kNoTail, kSegPieces, true, 999998},
    {"LLR SOFT16 x20", SOFT16_B32, k64M, 20, true, "", 1024, Form::Tg, 32000, kNoTail, kSegNone, false, 999998},
};

struct NameCase {
    int o;
    size_t n;
    uint32_t nbatch;
    bool llr;
    const char* env;
    const char* name;
};
static const NameCase kNames[] = {
    {HARD_B32, k64M, 1, false, "", "vd_decode_pk<HARD,B32,O32> split: one chunk per wave cut in two, int16 halves"},
    {SOFT8_B16, k64M, 20, true, "", "vd_decode_pk<LLR+SOFT8,B16,O32> batched: two chunks per wave, int16 halves"},
    {SOFT16_B32, k64M, 1, false, "", "vd_decode_tg<SOFT16,B32,O32> segment launch: one chunk or piece per wave, int32 tagged patterns"},
    {HARD_F16_O16, k64M, 1, false, "VD_NO_SPLIT=1", "vd_decode_tg<HARD,F16,O16> one chunk per wave, fp32 tagged core"},
    {HARD_B32, 128, 1, false, "", "-"},
};

int main()
{
    for (const Case& c : kCases) {
        const LaunchPlan p = plan(c.o, c.n, c.nbatch, c.llr, c.env, c.nsimd);
        if (!p.launches || p.form != c.form || p.grid != c.grid || p.tailWG != c.tailWG || p.seg != c.seg ||
            p.stats != c.stats || p.packNum != c.packNum) {
            printf("FAIL %s: launches %d form %d grid %u tailWG %u seg %d stats %d packNum %llu\n", c.what, (int)p.launches,
                   (int)p.form, p.grid, p.tailWG, p.seg, (int)p.stats, (unsigned long long)p.packNum);
            return 1;
        }
    }
    if (plan(HARD_B32, 128, 1, false, "", 1024).launches) { printf("FAIL 128 values launch\n"); return 1; }
    for (const NameCase& c : kNames) {
        const std::string name = plan_name(plan(c.o, c.n, c.nbatch, c.llr, c.env, 1024), c.o, c.llr);
        if (name != c.name) { printf("FAIL name: got \"%s\", want \"%s\"\n", name.c_str(), c.name); return 1; }
    }
    // the kernel table: a launcher for the family of every plan, none for SOFT16 on vd_decode_pk, and exactly
    // the 12 x 4 vd_decode_tg and 11 x 8 vd_decode_pk kernels
    int nvalid = 0;
    for (int o = 0; o < 0x10000; o++) {
        if (!valid(o)) continue;
        nvalid++;
        for (uint32_t nbatch : {1u, 20u})
            for (bool llr : {false, true}) {
                const LaunchPlan p = plan(o, k64M, nbatch, llr, "", 1024);
                if (!p.launches || !has_kernel(p.form, ch_of(o), met_of(o)) ||
                    !launcher<Stub>(p.form, llr, ch_of(o), met_of(o), out_of(o) == 1)) {
                    printf("FAIL option 0x%x x%u llr %d: no kernel for form %d\n", o, nbatch, (int)llr, (int)p.form);
                    return 1;
                }
                if ((p.form == Form::Tg) != (ch_of(o) == SOFT16)) {
                    printf("FAIL option 0x%x x%u llr %d: form %d\n", o, nbatch, (int)llr, (int)p.form);
                    return 1;
                }
            }
    }
    if (nvalid != 42) { printf("FAIL %d valid options\n", nvalid); return 1; }
    int count[3] = {0, 0, 0};
    for (Form f : {Form::Tg, Form::PkBatched, Form::PkSplit})
        for (int llr = 0; llr < 2; llr++)
            for (int ch = 0; ch < 5; ch++)
                for (int me = 0; me < 3; me++)
                    for (int o16 = 0; o16 < 2; o16++) {
                        const bool have = launcher<Stub>(f, llr != 0, ch, me, o16 != 0) != nullptr;
                        count[(int)f] += have;
                        if (have != has_kernel(f, ch, me) || (have && f != Form::Tg && ch == SOFT16)) {
                            printf("FAIL kernel table: form %d llr %d format %d metric %d\n", (int)f, llr, ch, me);
                            return 1;
                        }
                    }
    if (count[0] != 48 || count[1] != 44 || count[2] != 44) {
        printf("FAIL kernel table: %d tg, %d + %d pk launchers\n", count[0], count[1], count[2]);
        return 1;
    }
    // the frame table (launcher_frames): 84 float, 52 int8 and 56 mixed kernels, and for every valid option and input code 3 .. 14 a kernel
    // exactly where vd_decoder_kernel_name names one -- not for punctured frames (4, 6) on HARD, for the int8 twins
    // (7 .. 10) on HARD, SOFT4 and SOFT8 only and the punctured ones (8, 10) not on HARD, for mixed frames (11 .. 14) not
    // on HARD and their int8 twins (13, 14) on SOFT4 and SOFT8 only
    int nframe = 0;
    for (int fam = 0; fam < 16; fam++)
        for (int ch = 0; ch < 5; ch++)
            for (int me = 0; me < 3; me++)
                for (int o16 = 0; o16 < 2; o16++)
                    nframe += launcher_frames<Stub>({(fam & 1) != 0, (fam & 2) != 0, (fam & 4) != 0, (fam & 8) != 0}, ch, me, o16 != 0) != nullptr;
    if (nframe != 84 + 52 + 56) { printf("FAIL frame table: %d kernels\n", nframe); return 1; }
    for (int o = 0; o < 0x10000; o++) {
        if (!valid(o)) continue;
        const int ch = ch_of(o);
        for (int llr = 3; llr <= 14; llr++) {
            bool none = false;
            if ((llr == 4 || llr == 6) && ch == HARD) none = true;
            if (llr >= 7 && llr <= 10 && (ch > SOFT8 || (ch == HARD && (llr == 8 || llr == 10)))) none = true;
            if (llr >= 11 && llr <= 14 && (ch == HARD || (llr >= 13 && ch > SOFT8))) none = true;
            const FrameFamily f = frame_family_of_input(llr);
            if ((launcher_frames<Stub>(f, ch, met_of(o), out_of(o) == 1) == nullptr) != none) {
                printf("FAIL frame table: option 0x%x input %d: kernel %s\n", o, llr, none ? "present" : "missing");
                return 1;
            }
            if (f.i8 != ((llr >= 7 && llr <= 10) || llr >= 13) || f.mix != (llr >= 11) || f.tb != (llr == 5 || llr == 6 || llr == 9 || llr == 10 || llr == 12 || llr == 14) ||
                f.pun != (llr == 4 || llr == 6 || llr == 8 || llr == 10 || llr >= 11)) {
                printf("FAIL family of input %d\n", llr);
                return 1;
            }
        }
    }
    printf("ok\n");
    return 0;
}
