// One call of frame_args_error (vd_frames.h) as the host checks of the frame families put it: the family's call on a
// SOFT8/B16 decoder (no refusal by format) with whole frames, pattern (1, 1, 1) and an empty pattern table unless the
// case sets these; addr 0 is the host buffer of a blocking variant.
#pragma once
#include "vd_frames.h"

inline vd::FrameArgs call_of(vd::FrameFamily fam, uint64_t addr, uint64_t istr, uint64_t ostr, uint64_t maxb, int nf, int kind,
                             float scale, int period = 1, uint32_t k0 = 1, uint32_t k1 = 1, uint64_t part = 0)
{
    vd::FrameArgs a = {};
    a.fam = fam;
    a.addr = addr;
    a.stride = istr;
    a.outStride = ostr;
    a.maxFrameBits = maxb;
    a.nframes = nf;
    a.kind = kind;
    a.scale = scale;
    a.period = period;
    a.keep0 = k0;
    a.keep1 = k1;
    a.options = 0x012;
    a.partBits = part;
    return a;
}
// the message or null; *code: the status the entry point returns (0: accepted)
inline const char* why_of(const vd::FrameArgs& a, int* code = nullptr)
{
    int c = 0;
    const char* why = vd::frame_args_error(a, &c);
    if (code) *code = why ? c : 0;
    return why;
}
inline const char* check(vd::FrameFamily fam, uint64_t addr, uint64_t istr, uint64_t ostr, uint64_t maxb, int nf, int kind,
                         float scale, int period = 1, uint32_t k0 = 1, uint32_t k1 = 1, uint64_t part = 0)
{
    return why_of(call_of(fam, addr, istr, ostr, maxb, nf, kind, scale, period, k0, k1, part));
}
