// vd_frames.h -- geometry of frame decodes (host and device, no HIP runtime calls).
//
// A frame is S trellis stages (2 S float channel values, first encoder output first) of an encoder started in
// state 0 and either flushed back to state 0 by six tail zeros (terminated) or simply stopped (open).  With
// W = ceil(S / 32) and P = 64 + 32 W the frame decode is the one-chunk decode of a padded stream of P stages:
//   stages [0, 26)           the pad value twice: "both encoder outputs 0" at full confidence (26 = the
//                            reference's EXTRA_L, where the decode window starts emitting bits);
//   stages [26, 26 + S)      the frame's values;
//   stages [26 + S, P), and whatever the decode reads beyond:  the pad value (terminated) or +0.0f, an
//                            erasure (open).
// The padded stream exists only as a select in the decode kernel's loads (vd_kernel_tg.h, channel ids kFrm +
// format): a frame's buffer resource covers its 8 S bytes, stage p of the padded stream is read at byte offset
// 8 (p - 26), which falls outside the range for every virtual stage and loads zero, and the pad replaces the
// loaded pair in the lanes of a virtual stage that is not an erasure.  tests/cxx/frames_check.cpp checks the
// helpers below against a plain enumeration.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define VD_FRAMES_HD __host__ __device__ inline
#else
#define VD_FRAMES_HD inline
#endif

namespace vd {

constexpr uint32_t kFrmLead = 26;              // virtual stages before the frame (EXTRA_L of 32-bit words)
constexpr uint32_t kFrmMaxBits = 1u << 20;     // longest frame: one wave decodes a whole frame
constexpr uint32_t kFrmGroup = 96;             // stages per table build (a group of vd_decode_tg)
constexpr uint32_t kFrmNoEnd = 0xFFFFFFFFu;    // frame_end of an open frame
// Offset given to a lane whose stage lies before the frame.  8 (p - 26) wraps to 2^32 - 8 (26 - p) there, and
// for p = 25 the end of the 8-byte access, 2^32, is 0 in 32 bits: such a lane reads at 2^31 instead, whose end
// lies past every range (<= 8 * kFrmMaxBits) with no wrap-around (as kPunErased, vd_kernel_tg.h).
constexpr uint32_t kFrmOutside = 0x80000000u;

VD_FRAMES_HD uint32_t frame_words(uint32_t S) { return (S + 31u) / 32u; }                    // 32-bit words
VD_FRAMES_HD uint32_t frame_padded_stages(uint32_t S) { return 64u + 32u * frame_words(S); }  // P

// first stage of the padded stream after the frame that is a pad stage: 26 + S when terminated, none when open
VD_FRAMES_HD uint32_t frame_end(uint32_t S, bool terminated) { return terminated ? kFrmLead + S : kFrmNoEnd; }
// stage p of the padded stream carries the pad value (not a frame value, not an erasure)
VD_FRAMES_HD bool frame_pad_stage(uint32_t p, uint32_t end) { return p < kFrmLead || p >= end; }
// ... and some stage of the 96-stage group from g0 does (wave-uniform: the select's branch)
VD_FRAMES_HD bool frame_pad_group(uint32_t g0, uint32_t end) { return g0 < kFrmLead || g0 + kFrmGroup > end; }
// byte offset of stage p's two floats against a resource of 8 S bytes at the frame's first float:
// inside the range exactly for 26 <= p < 26 + S (p <= kFrmMaxBits + a few groups: 8 p stays far below 2^31)
VD_FRAMES_HD uint32_t frame_offset(uint32_t p)
{
    const uint32_t o = 8u * (p - kFrmLead);  // wraps for p < 26
    return o < kFrmOutside ? o : kFrmOutside;
}

// The pad value as a channel float: it must quantise to the format's most negative code (HARD bit 0, SOFT4 -8,
// SOFT8 -128, SOFT16 -32768, FP32 -8 after the clamp) for whatever scale the caller passes, so it is
// -65536 / scale, a finite value whose product with the scale is checked to reach -32768.  No infinity: the
// packer's narrowing path for non-finite values does not saturate in SOFT8 (vd_pack.h).
// false: scale is not finite and > 0, or so small that the pad is not finite
inline bool frame_pad(float scale, float* pad)
{
    if (!(scale > 0.0f) || !(scale <= 3.4028234663852886e38f)) return false;
    const volatile float p = -65536.0f / scale;
    if (!(p >= -3.4028234663852886e38f)) return false;
    const volatile float q = p * scale;  // the product the kernel forms
    if (!(q <= -32768.0f)) return false;
    *pad = p;
    return true;
}

// The argument checks of vd_run_device_frames (all VD_ERR_ARG): the message, or null when the arguments are good.
// llr_addr: the address of the first frame's first float.
inline const char* frame_args_error(uint64_t llr_addr, uint64_t llr_stride, uint64_t output_stride, uint64_t maxFrameBits,
                                    int nframes, float scale)
{
    float pad;
    if (maxFrameBits < 1 || maxFrameBits > kFrmMaxBits) return "maxFrameBits must be in [1, 2^20]";
    if (nframes < 1) return "nframes must be >= 1";
    if (!frame_pad(scale, &pad)) return "scale must be finite and > 0 (and -65536 / scale finite)";
    if (llr_addr & 7) return "llr_d must be 8-byte aligned";
    if ((llr_stride & 7) || (output_stride & 3)) return "llr_stride % 8 or output_stride % 4 != 0";
    if (nframes > 1 && llr_stride < 8 * maxFrameBits) return "llr_stride smaller than 8 * maxFrameBits: frames would overlap";
    if (nframes > 1 && output_stride < 4ull * frame_words((uint32_t)maxFrameBits))
        return "output_stride smaller than vd_frame_output_size(maxFrameBits): frames would overlap";
    return nullptr;
}

}  // namespace vd
