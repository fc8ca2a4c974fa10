// Host check of the one argument check of the frame entry points (vd_frames.h frame_args_error): which error wins
// when several apply, by status code and message, for every family.  The expected outcomes are written down from the
// order callers have always seen (never from frame_args_error itself):
//   frames, punctured, punctured tail-biting frames: the argument rules, the part length, then the refusal by format;
//   tail-biting frames: the argument rules, the part length, no refusal;
//   int8 frames: the argument rules with the kind first and the part length last, then SOFT16 / FP32, HARD + open,
//     HARD + punctured;
//   mixed frames: HARD, then int8 on SOFT16 / FP32, then the argument rules with the empty table first;
// and a blocking variant's host buffer (address 0) is under no pointer rule.
// Built with hipcc and the host sanitizers by tests/test_frames.py; prints "ok" or the first mismatch.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include "vd_kernel_tg.h"
#include "vd_plan.h"
#include "frame_args.h"

using namespace vd;

constexpr int OK = 0, OPT = kFrameErrOptions, ARG = kFrameErrArg;
constexpr int O_HARD = 0x000, O_SOFT4 = 0x001, O_SOFT8 = 0x012, O_SOFT16 = 0x003, O_FP32 = 0x004;
constexpr FrameFamily FRM = {false, false, false, false}, PUN = {true, false, false, false}, TB = {false, true, false, false},
                      PTB = {true, true, false, false}, I8 = {false, false, true, false}, I8PUN = {true, false, true, false},
                      I8TB = {false, true, true, false}, MIX = {true, false, false, true}, MIXTB = {true, true, false, true},
                      I8MIX = {true, false, true, true}, I8MIXTB = {true, true, true, true};
constexpr int OPEN = kByteFramesOpen, TERM = kByteFramesTerminated, TAIL = kByteFramesTailbiting;

struct Row {
    FrameFamily fam;
    int options;
    uint64_t addr, istr;
    bool off;
    uint64_t ostr, maxb;
    int nf, kind;
    float scale;
    int period;
    uint32_t k0, k1;
    uint64_t part;
    int n;             // patterns of the table {(1, 1, 1), 2/3, 3/4} the decoder holds
    int code;
    const char* why;   // a piece of the message (null: accepted) ...
    const char* tail;  // ... and of its end, where two families' messages differ only there
};
// 1000 stages: 8000 bytes of floats, 5336 under 3/4 (3, 5, 3); 2000 and 1334 bytes of int8; 128 bytes of output
static const Row kRows[] = {
    // ---- frames
    {FRM, O_HARD, 0, 8000, false, 128, 1000, 0, OPEN, 1.0f, 1, 1, 1, 0, 0, ARG, "nframes must be >= 1", nullptr},
    {FRM, O_HARD, 0, 8000, false, 128, 1000, 4, OPEN, 1.0f, 1, 1, 1, 100, 0, ARG, "partBits must be 0 or a multiple of 96", nullptr},
    {FRM, O_HARD, 4, 8000, false, 128, 1000, 4, OPEN, 1.0f, 1, 1, 1, 0, 0, ARG, "llr_d must be 8-byte aligned", nullptr},
    {FRM, O_HARD, 0, 8000, false, 128, 1000, 4, OPEN, 1.0f, 1, 1, 1, 0, 0, OPT, "open frames on a HARD decoder", "SOFT4, SOFT8, SOFT16 or FP32"},
    {FRM, O_HARD, 0, 8000, false, 128, 1000, 4, TERM, 1.0f, 1, 1, 1, 0, 0, OK, nullptr, nullptr},
    {FRM, O_SOFT8, 4, 8004, false, 128, 1000, 4, TERM, 0.0f, 1, 1, 1, 0, 0, ARG, "(and -65536 / scale finite)", nullptr},
    {FRM, O_SOFT8, 4, 8000, false, 128, 1000, 4, TERM, 1.0f, 1, 1, 1, 0, 0, ARG, "llr_d must be 8-byte aligned", nullptr},
    {FRM, O_SOFT8, 0, 8000, false, 128, 1000, 4, TERM, 1.0f, 1, 1, 1, 0, 0, OK, nullptr, nullptr},  // the same call on a host buffer
    {FRM, O_SOFT8, 0, 8004, false, 128, 1000, 4, TERM, 1.0f, 1, 1, 1, 0, 0, ARG, "llr_stride % 8", nullptr},  // ... whose strides still count
    // ---- punctured frames
    {PUN, O_HARD, 0, 8ull << 20, false, 4ull << 15, 1u << 20, 0x7FFFFFFF, TERM, 1.0f, 3, 5, 3, 96, 0, ARG, "more than 2^31 - 1 workgroups", nullptr},
    {PUN, O_HARD, 0, 5336, false, 128, 1000, 4, TERM, 1.0f, 3, 8, 3, 0, 0, ARG, "invalid puncture pattern", nullptr},
    {PUN, O_HARD, 0, 5336, false, 128, 1000, 4, OPEN, 1.0f, 3, 5, 3, 0, 0, OPT, "punctured frames on a HARD decoder", "SOFT4, SOFT8, SOFT16 or FP32"},
    {PUN, O_SOFT4, 0, 5336, false, 128, 0, 4, TERM, 1.0f, 0, 1, 1, 0, 0, ARG, "invalid puncture pattern", nullptr},
    {PUN, O_SOFT4, 2, 5336, false, 128, 1000, 4, TERM, 1.0f, 3, 5, 3, 0, 0, ARG, "rx_d, rx_stride and output_stride must be multiples of 4", nullptr},
    {PUN, O_SOFT4, 0, 5336, false, 128, 1000, 4, TERM, 1.0f, 3, 5, 3, 0, 0, OK, nullptr, nullptr},
    // ---- tail-biting frames: every format, no refusal
    {TB, O_HARD, 0, 8000, false, 128, 1000, 4, TAIL, 1e-40f, 1, 1, 1, 0, 0, OK, nullptr, nullptr},
    {TB, O_HARD, 0, 8000, false, 128, 1000, 0, TAIL, 0.0f, 1, 1, 1, 0, 0, ARG, "nframes must be >= 1", nullptr},
    {TB, O_HARD, 0, 8000, false, 128, 1000, 4, TAIL, 1.0f, 1, 1, 1, 100, 0, ARG, "partBits must be 0 or a multiple of 96", nullptr},
    {TB, O_FP32, 4, 8000, false, 128, 1000, 4, TAIL, 1.0f, 1, 1, 1, 0, 0, ARG, "llr_d must be 8-byte aligned", nullptr},
    {TB, O_FP32, 0, 8000, false, 128, 1000, 4, TAIL, 1.0f, 1, 1, 1, 0, 0, OK, nullptr, nullptr},
    // ---- punctured tail-biting frames
    {PTB, O_HARD, 0, 5336, false, 128, 1000, 4, TAIL, 1.0f, 3, 5, 3, 0, 0, OPT, "punctured tail-biting frames on a HARD decoder", "SOFT4, SOFT8, SOFT16 or FP32"},
    {PTB, O_HARD, 0, 5336, false, 124, 1000, 4, TAIL, 1.0f, 3, 5, 3, 0, 0, ARG, "output_stride smaller than", nullptr},
    {PTB, O_SOFT16, 0, 5330, false, 128, 1000, 4, TAIL, 1.0f, 3, 5, 3, 0, 0, ARG, "rx_d, rx_stride and output_stride must be multiples of 4", nullptr},
    {PTB, O_SOFT16, 0, 5332, false, 128, 1000, 4, TAIL, 1.0f, 3, 5, 3, 0, 0, ARG, "rx_stride smaller than 4 * vd_punctured_len", nullptr},
    {PTB, O_SOFT16, 0, 5336, false, 128, 1000, 4, TAIL, 1e-40f, 3, 5, 3, 0, 0, OK, nullptr, nullptr},
    // ---- int8 frames
    {I8, O_FP32, 0, 2000, false, 128, 1000, 4, 3, 1.0f, 1, 1, 1, 0, 0, ARG, "kind must be", nullptr},
    {I8PUN, O_HARD, 0, 1334, false, 128, 1000, 4, OPEN, 1.0f, 3, 5, 3, 0, 0, OPT, "open frames on a HARD decoder", "use SOFT4 or SOFT8"},
    {I8PUN, O_HARD, 0, 1334, false, 128, 1000, 4, TERM, 1.0f, 3, 5, 3, 0, 0, OPT, "punctured frames on a HARD decoder", "use SOFT4 or SOFT8"},
    {I8, O_SOFT16, 0, 2000, false, 128, 1000, 4, TERM, 1.0f, 1, 1, 1, 100, 0, ARG, "partBits must be 0 or a multiple of 96", nullptr},
    {I8, O_SOFT16, 0, 2000, false, 128, 1000, 4, OPEN, 1.0f, 1, 1, 1, 0, 0, OPT, "int8 frames on a SOFT16 or FP32 decoder", "use HARD, SOFT4 or SOFT8"},
    {I8, O_HARD, 0, 2000, false, 128, 1000, 4, 3, 1.0f, 3, 8, 3, 0, 0, ARG, "kind must be", nullptr},
    {I8TB, O_HARD, 0, 2000, false, 128, 1000, 4, TAIL, 1.0f, 1, 1, 1, 0, 0, OK, nullptr, nullptr},
    {I8, O_SOFT8, 1, 2000, false, 128, 1000, 4, TERM, 1.0f, 1, 1, 1, 0, 0, ARG, "multiples of 2 bytes", nullptr},
    {I8, O_SOFT8, 0, 2000, false, 128, 1000, 4, TERM, 1.0f, 1, 1, 1, 0, 0, OK, nullptr, nullptr},  // the same call on a host buffer
    // ---- mixed frames
    {MIX, O_HARD, 0, 8000, false, 128, 1000, 0, TERM, 1.0f, 1, 1, 1, 0, 3, OPT, "mixed frames on a HARD decoder", "SOFT4, SOFT8, SOFT16 or FP32"},
    {MIX, O_HARD, 0, 8000, false, 128, 1000, 4, TERM, 1.0f, 1, 1, 1, 0, 0, OPT, "mixed frames on a HARD decoder", nullptr},
    {MIX, O_SOFT8, 0, 8000, false, 128, 1000, 4, 3, 1.0f, 1, 1, 1, 0, 0, ARG, "pattern table is empty", nullptr},
    {MIXTB, O_SOFT8, 0, 8000, false, 128, 0, 4, 3, 1.0f, 1, 1, 1, 0, 3, ARG, "kind must be", nullptr},
    {MIX, O_FP32, 2, 8000, false, 128, 1000, 4, OPEN, 1.0f, 1, 1, 1, 0, 3, ARG, "rx_d must be 4-byte aligned", nullptr},
    {MIX, O_FP32, 0, 8000, false, 128, 1000, 4, OPEN, 1.0f, 1, 1, 1, 0, 3, OK, nullptr, nullptr},  // the same call on a host buffer
    {MIX, O_FP32, 0, 8002, false, 128, 1000, 4, OPEN, 1.0f, 1, 1, 1, 0, 3, ARG, "rx_stride must be a multiple of 4", nullptr},
    // ---- int8 mixed frames
    {I8MIX, O_FP32, 0, 2000, false, 128, 1000, 0, TERM, 1.0f, 1, 1, 1, 0, 3, OPT, "int8 frames on a SOFT16 or FP32 decoder", "use SOFT4 or SOFT8"},
    {I8MIX, O_HARD, 0, 2000, false, 128, 1000, 4, TERM, 1.0f, 1, 1, 1, 0, 3, OPT, "mixed frames on a HARD decoder", nullptr},
    {I8MIX, O_SOFT8, 0, 2000, false, 128, 1000, 4, TERM, 1.0f, 1, 1, 1, 100, 3, ARG, "partBits must be 0 or a multiple of 96", nullptr},
    {I8MIX, O_SOFT8, 0, 2000, false, 128, 1000, 4, TERM, 1.0f, 1, 1, 1, 100, 0, ARG, "pattern table is empty", nullptr},
    {I8MIX, O_SOFT4, 3, 2001, false, 128, 1000, 4, TERM, 1.0f, 1, 1, 1, 0, 3, OK, nullptr, nullptr},
    {I8MIXTB, O_SOFT4, 3, 1, true, 128, 1000, 4, TAIL, 1e-40f, 1, 1, 1, 0, 3, OK, nullptr, nullptr},  // offsets: the stride is ignored
};

int main()
{
    const MixRecord tab[3] = {mix_record(1, 1, 1), mix_record(2, 1, 3), mix_record(3, 5, 3)};
    int i = 0;
    for (const Row& r : kRows) {
        FrameArgs a = call_of(r.fam, r.addr, r.istr, r.ostr, r.maxb, r.nf, r.kind, r.scale, r.period, r.k0, r.k1, r.part);
        a.options = r.options;
        a.offsets = r.off;
        a.table = r.n ? tab : nullptr;
        a.tableN = r.n;
        int code = 12345;
        const char* why = why_of(a, &code);
        const bool same = r.why ? why && strstr(why, r.why) && (!r.tail || (strlen(why) >= strlen(r.tail) && !strcmp(why + strlen(why) - strlen(r.tail), r.tail)))
                                : why == nullptr;
        if (!same || code != r.code) {
            printf("FAIL row %d: code %d \"%s\", want %d \"%s\" ... \"%s\"\n", i, code, why ? why : "accepted", r.code,
                   r.why ? r.why : "accepted", r.tail ? r.tail : "");
            return 1;
        }
        i++;
    }
    printf("ok\n");
    return 0;
}
