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
#include "vd_punct.h"

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
// (VB: the bytes of a channel value, 4 for floats; 1 for the int8 frames at the end of this header)
template <uint32_t VB = 4>
VD_FRAMES_HD uint32_t frame_offset(uint32_t p)
{
    const uint32_t o = 2u * VB * (p - kFrmLead);  // wraps for p < 26
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

// ---------------------------------------------------------------- punctured frames (channel ids kFrm + kPun + format)
// A punctured frame of S stages under a pattern (vd_punct.h) holds the punct_len(2 S) kept values of its 2 S
// mother-code values, the pattern's phase restarting at the frame's first stage: frame stage t uses bit
// t % period.  Its decode is the frame decode above of the depunctured frame (+0.0f at the punctured positions).
// One resource per frame, based at its first received float with a range of its received bytes.  A 96-stage group
// from padded stage g0 starts at frame stage t0 = g0 - 26 (group 0: its lanes s < 26 are lead stages, lane s >= 26
// is frame stage s - 26); (q0, r0) of t0 by punct_divmod on the scalar unit, and lane s reads its two values at
// byte 4 (q0 Kp + punct_rel(r0, s - lead)), a vector offset.  The kept indices grow with the stage, so a stage
// >= S lands at or past the range's end and loads zero by the range check alone; punctured values and lead stages
// take kFrmOutside (every other offset stays below 2^24: no 32-bit wrap of offset + 4).
// tests/cxx/punct_frames_check.cpp checks the helpers below against a plain enumeration.

// the received bytes of a punctured frame of S <= kFrmMaxBits stages: 4 punct_len(2 S), at most 8 MiB
template <uint32_t VB = 4>
VD_FRAMES_HD uint32_t pfrm_bytes(const Punct& pn, uint32_t S)
{
    uint32_t q, r;
    punct_divmod(pn, S, q, r);
    return VB * (q * pn.kp + punct_before(pn, r));
}
// the group from padded stage g0 (a multiple of kFrmGroup): its first frame stage t0, and the lanes s < lead
// that lie before the frame
struct PfrmGroup {
    uint32_t t0, lead;
};
VD_FRAMES_HD constexpr PfrmGroup pfrm_group(uint32_t g0)
{
    return g0 < kFrmLead ? PfrmGroup{0u, kFrmLead - g0} : PfrmGroup{g0 - kFrmLead, 0u};
}
// byte offset of float q0 Kp, (q0, r0) = divmod(t0, period); *r0 = t0 % period
template <uint32_t VB = 4>
VD_FRAMES_HD uint32_t pfrm_base(const Punct& pn, uint32_t t0, uint32_t* r0)
{
    uint32_t q0;
    punct_divmod(pn, t0, q0, *r0);
    return q0 * (pn.kp * VB);
}
// the byte offsets of the two values of lane s (< kFrmGroup) of the group (base4, r0, lead) against the frame's
// resource: inside the range exactly for a kept value of a frame stage < S
struct PfrmOff {
    uint32_t o0, o1;
};
// a b for a, b < 2^24: the masks change nothing and let the compiler take the full-rate 24-bit multiply
// (v_mul_u32_u24 / v_mad_u32_u24, which ignore the upper bits: the masks cost no instruction) where the 32-bit
// v_mul_lo_u32 issues at a quarter of the rate -- six of those per group were most of this path's cost
VD_FRAMES_HD uint32_t pfrm_mul24(uint32_t a, uint32_t b) { return (a & 0xFFFFFFu) * (b & 0xFFFFFFu); }
template <uint32_t VB = 4>
VD_FRAMES_HD PfrmOff pfrm_offsets(const Punct& pn, uint32_t base4, uint32_t r0, uint32_t lead, uint32_t s)
{
    const uint32_t before = s < lead ? kFrmOutside : 0u;
    // punct_rel's map of x = r0 + (s - lead) < 16 + kPunctSpan (its reciprocal proof holds unchanged), with
    // 24-bit products: x m16 < 112 (2^16 + 1) < 2^23, dq < 112
    const uint32_t x = r0 + (s < lead ? 0u : s - lead);
    const uint32_t dq = pfrm_mul24(x, pn.m16) >> 16;
    const uint32_t r = x - pfrm_mul24(dq, pn.period);
    const uint32_t has0 = (pn.keep0 >> r) & 1u, has1 = (pn.keep1 >> r) & 1u;
    const uint32_t b = base4 + pfrm_mul24(dq, VB * pn.kp) + punct_before(pn, r) * VB;
    return {b | ((has0 ^ 1u) * kFrmOutside) | before, (b + has0 * VB) | ((has1 ^ 1u) * kFrmOutside) | before};
}

// ---------------------------------------------------------------- tail-biting frames (channel ids kFrm + kTb + format)
// A tail-biting frame of S >= 1 stages: the encoder's register at the first stage holds the frame's last six
// information bits (cyclically for S < 6), so output stage t depends on bits t, t - 1, ..., t - 6 mod S, start
// state = end state, no tail.  Its decode is the one-chunk decode of the frame's extended stream of P = 64 + 32 W
// stages, stage p = frame stage (p - 26) mod S (non-negative residue, as many turns as it takes; the same rule
// for what the kernel prefetches beyond P): the interior of a periodic stream, which the fixed window decodes as
// it decodes any interior chunk.  No pad, no erasure: every format, HARD included.
// The frame's resource is the frame launch's (based at its first float, 8 S bytes), and every load offset lies
// inside it: 8 t with t < S.  A 96-stage group from g0 reads frame stages g0 - 26 + s, s < 96, unwrapped (offset
// 8 (p - 26), frame_offset without its clamp) unless it is group 0 (its lanes s < 26 lie before the frame) or
// reaches the frame's end (g0 + 96 - 26 > S): tb_wrap_group, wave-uniform.  A wrapping group reduces its first
// stage once on the scalar unit, r0 = (g0 - 26) mod S (tb_group_r0, with the wave's reciprocal of S from set-up),
// and lane s reduces x = r0 + s < S + 96 (tb_lane_stage).  tests/cxx/tb_frames_check.cpp checks the helpers
// below against a plain enumeration.

// The wave's reciprocals of its S (1 <= S <= kFrmMaxBits; one division at set-up):
//   m32 = floor((2^32 - 1) / S): (2^32 - 1) / S - 1 < m32 <= (2^32 - 1) / S, so for x < 2^31 the estimate
//     qe = floor(x m32 / 2^32) has x / S - x m32 / 2^32 < x (1 / (S 2^32) + 1 / 2^32) <= 2 x / 2^32 < 1:
//     qe is floor(x / S) or one below, and x - qe S lies in [0, 2 S): one conditional subtract (tb_mod);
//   m16 = (m32 >> 16) + 1 (used for S < 96 only): m32 >> 16 = floor((2^32 - 1) / (2^16 S)) is floor(2^16 / S),
//     or one below when S divides 2^16, so m16 S = 2^16 + e with 0 <= e <= S <= 95, and for x < 192:
//     x m16 / 2^16 = x / S + x e / (S 2^16) with x e <= 191 * 95 < 2^16, less than the 1 / S that x / S lacks
//     to the next integer at least: floor(x m16 / 2^16) = floor(x / S) exactly (punct_rel's argument).
struct TbRecip {
    uint32_t m32, m16;
};
VD_FRAMES_HD TbRecip tb_recip(uint32_t S)
{
    const uint32_t m32 = 0xFFFFFFFFu / S;
    return {m32, (m32 >> 16) + 1u};
}
// x mod S for x < 2^31 (uniform operands: one scalar multiply-high, one multiply, a subtract and a minimum)
VD_FRAMES_HD uint32_t tb_mod(uint32_t x, uint32_t S, uint32_t m32)
{
    const uint32_t r = x - (uint32_t)(((uint64_t)x * m32) >> 32) * S;  // in [0, 2 S)
    return r - S < r ? r - S : r;                                      // (r - S wraps above r when r < S)
}
// some lane of the 96-stage group from extended stage g0 (a multiple of kFrmGroup) wraps: wave-uniform
VD_FRAMES_HD bool tb_wrap_group(uint32_t g0, uint32_t S) { return g0 < kFrmLead || g0 + kFrmGroup - kFrmLead > S; }
// frame stage of the group's lane 0: (g0 - 26) mod S, non-negative (g0 <= kFrmMaxBits + a few groups; for the
// groups of a part too, "frames in parts" below: a part starts below 32 W <= S + 31 and runs its own words + 2 blocks
// and one prefetched group, so g0 - 26 < S + 32 (Wp + 2) + 96 < 2^21 + 2^20 + 200, far inside tb_mod's x < 2^31)
VD_FRAMES_HD uint32_t tb_group_r0(uint32_t g0, uint32_t S, uint32_t m32)
{
    if (g0 >= kFrmLead) return tb_mod(g0 - kFrmLead, S, m32);
    const uint32_t a = tb_mod(kFrmLead - g0, S, m32);
    return a ? S - a : 0u;
}
// frame stage of lane s (< kFrmGroup) of a wrapping group: (r0 + s) mod S, r0 < S.  x = r0 + s < S + 96: for
// S >= 96 that is below 2 S, one conditional subtract (as a minimum: no select); for S < 96, x < 192 and the
// 16-bit reciprocal is exact (above), in 24-bit products: x < 192, m16 <= 65537, x m16 < 2^24, dq < 192, S < 96
// (tb_turns_stage: that form alone, for a caller that knows S < 96)
VD_FRAMES_HD uint32_t tb_turns_stage(uint32_t x, uint32_t S, uint32_t m16) { return x - pfrm_mul24(pfrm_mul24(x, m16) >> 16, S); }
VD_FRAMES_HD uint32_t tb_lane_stage(uint32_t r0, uint32_t s, uint32_t S, uint32_t m16)
{
    const uint32_t x = r0 + s;
    if (S >= kFrmGroup) return x - S < x ? x - S : x;
    return tb_turns_stage(x, S, m16);
}
// byte offset of the two floats of frame stage t (< S) against the frame's resource: offset + 8 <= 8 S
template <uint32_t VB = 4>
VD_FRAMES_HD uint32_t tb_offset(uint32_t t) { return 2u * VB * t; }
// ... of lane s of a group that does not wrap (g0 >= 26, g0 + 96 - 26 <= S): frame stage g0 - 26 + s
template <uint32_t VB = 4>
VD_FRAMES_HD uint32_t tb_offset_inside(uint32_t g0, uint32_t s) { return 2u * VB * (g0 - kFrmLead + s); }
// the map as the kernel evaluates it: the offset of stage g0 + s of the extended stream
template <uint32_t VB = 4>
VD_FRAMES_HD uint32_t tb_stage_offset(uint32_t g0, uint32_t s, uint32_t S, const TbRecip& rc)
{
    if (!tb_wrap_group(g0, S)) return tb_offset_inside<VB>(g0, s);
    return tb_offset<VB>(tb_lane_stage(tb_group_r0(g0, S, rc.m32), s, S, rc.m16));
}

// ---------------------------------------------------------------- punctured tail-biting frames (channel ids kFrm + kTb + kPun + format)
// A punctured tail-biting frame of S >= 1 stages under a pattern holds the punct_len(2 S) kept values of its 2 S
// mother-code values, and the pattern's phase belongs to the frame stage: stage p of the extended stream is frame
// stage t = (p - 26) mod S and uses bit t % period, so the phase restarts at every wrap, whether or not the period
// divides S.  Its decode is the tail-biting decode above of the depunctured frame (+0.0f at the punctured
// positions).  One resource per frame over its pfrm_bytes, and per 96-stage group one of three wave-uniform forms
// (ptb_group), each ending in pfrm_offsets:
//   inside (no lane wraps: g0 >= 26, g0 + 96 - 26 <= S): the punctured-frame path, (base4, r0) of frame stage
//     g0 - 26 by pfrm_base and lane stage s;
//   one wrap (S >= 96: x = rs + s < S + 96 <= 2 S with rs = (g0 - 26) mod S): the lanes with x < S are frame stages
//     rs + s on the pair (base4, r0) of rs, the others frame stages x - S < 96 counted from frame stage 0: the
//     pair (0, 0) and lane stage x - S, a select per lane between two uniform pairs;
//   turns (S < 96): t = (rs + s) mod S by the 16-bit reciprocal (tb_lane_stage's argument), the pair (0, 0) and
//     lane stage t < 96.
// pfrm_offsets' argument x = r0 + lane stage < 16 + 96 holds in all three.  Every stage is a frame stage < S, so a
// kept value's offset lies inside the range (offset + 4 <= pfrm_bytes) and nothing is "past the frame's end"; a
// punctured value takes kFrmOutside (every kept offset stays below 2^24: no 32-bit wrap of offset + 4) and loads
// zero through the range check, the one thing the range check is relied on for.  A frame with no kept value has a
// range of 0 bytes and reads nothing.  tests/cxx/ptb_frames_check.cpp checks the helpers below against a plain
// enumeration.

// wave-uniform values stay in scalar registers in the kernel (a no-op on values already scalar)
#if defined(__HIP_DEVICE_COMPILE__)
#define VD_FRAMES_UNIFORM(x) ((uint32_t)__builtin_amdgcn_readfirstlane(x))
#else
#define VD_FRAMES_UNIFORM(x) ((uint32_t)(x))
#endif
constexpr uint32_t kPtbInside = 0, kPtbWrap = 1, kPtbTurns = 2;
// the uniform part of the 96-stage group from extended stage g0 (a multiple of kFrmGroup; <= kFrmMaxBits + a few
// groups) of a frame of S stages with the reciprocals rc: its form, the frame stage rs of its lane 0 (wrapping
// forms) and the pair (base4, r0) of its first frame stage (inside, one wrap)
struct PtbGroup {
    uint32_t mode, rs, base4, r0;
};
template <uint32_t VB = 4>
VD_FRAMES_HD PtbGroup ptb_group(const Punct& pn, uint32_t g0, uint32_t S, const TbRecip& rc)
{
    PtbGroup g = {kPtbTurns, 0u, 0u, 0u};
    const bool wrap = tb_wrap_group(g0, S);
    if (wrap) g.rs = VD_FRAMES_UNIFORM(tb_group_r0(g0, S, rc.m32));
    if (wrap && S < kFrmGroup) return g;
    g.mode = wrap ? kPtbWrap : kPtbInside;
    uint32_t r0;
    g.base4 = VD_FRAMES_UNIFORM(pfrm_base<VB>(pn, VD_FRAMES_UNIFORM(wrap ? g.rs : g0 - kFrmLead), &r0));
    g.r0 = VD_FRAMES_UNIFORM(r0);
    return g;
}
#undef VD_FRAMES_UNIFORM
// the byte offsets of the two values of lane s (< kFrmGroup) of the group g against the frame's resource: inside
// the range exactly for a kept value (m16: tb_recip(S).m16, used for S < 96 only)
template <uint32_t VB = 4>
VD_FRAMES_HD PfrmOff ptb_offsets(const Punct& pn, const PtbGroup& g, uint32_t s, uint32_t S, uint32_t m16)
{
    uint32_t b = g.base4, r = g.r0, ls = s;
    if (g.mode == kPtbWrap) {
        const uint32_t x = g.rs + s;  // < S + 96 <= 2 S: at most one wrap point in the group
        if (x >= S) {                 // counted from frame stage 0: x - S <= rs - S + 95 < 95
            b = 0u;
            r = 0u;
            ls = x - S;
        }
    } else if (g.mode == kPtbTurns) {
        ls = tb_turns_stage(g.rs + s, S, m16);  // tb_lane_stage for S < 96 (ptb_group): t < 96; b = r = 0
    }
    return pfrm_offsets<VB>(pn, b, r, 0u, ls);
}
// the map as the kernel evaluates it: the offsets of the two values of stage g0 + s of the extended stream
template <uint32_t VB = 4>
VD_FRAMES_HD PfrmOff ptb_stage_offsets(const Punct& pn, uint32_t g0, uint32_t s, uint32_t S, const TbRecip& rc)
{
    return ptb_offsets<VB>(pn, ptb_group<VB>(pn, g0, S, rc), s, S, rc.m16);
}

// ---------------------------------------------------------------- frames in parts (all four families)
// A decoder's part length partBits is 0 (whole frames: one frame per wave, everything above) or a multiple of 96
// in [96, 2^20].  With Wp = partBits / 32 words (a multiple of 3) a frame of S stages, W = frame_words(S), has
// ceil(W / Wp) parts; part j holds the w_j = min(Wp, W - j Wp) words from word j Wp on and is decoded by a wave
// of its own as the one-chunk decode of stages [32 j Wp, 32 j Wp + 64 + 32 w_j) of the frame's padded or extended
// stream: from equal metrics, 26 warm-up stages before its first bit and 38 traceback stages after its last, which
// are the frame's own stages where it has them and pad stages, erasures or the wrap otherwise, by the per-stage
// rules above.  32 j Wp is a multiple of 96, so every group of every part starts at a multiple of kFrmGroup of the
// stream, as the groups of a whole frame do: the helpers above take such a first stage g0 unchanged (g0 <=
// kFrmMaxBits + a few groups still holds: a part starts below 32 W).  A frame with W <= Wp is one part, the whole
// frame.  Launch geometry: partsMax = ceil(frame_words(maxFrameBits) / Wp) parts at most, G = ceil(partsMax /
// kFrmWaves) workgroups per frame, so the parts of a frame sit in neighbouring waves; wave wv of workgroup b is
// part (b % G) kFrmWaves + wv of frame b / G, and a wave whose part starts at or past its frame's W has nothing
// to do.  tests/cxx/frame_parts_check.cpp checks the helpers below against a plain enumeration.
constexpr uint32_t kFrmWaves = 4;                    // waves per workgroup (kWaves, vd_kernels.h)
constexpr uint32_t kFrmMaxGrid = 0x7FFFFFFFu;        // workgroups a launch may have

// partBits is 0 or a multiple of 96 in [96, 2^20]
VD_FRAMES_HD bool frame_part_bits_valid(uint64_t partBits)
{
    return partBits == 0 || (partBits >= kFrmGroup && partBits <= kFrmMaxBits && partBits % kFrmGroup == 0);
}
// Wp: the 32-bit words of a part (0: whole frames)
VD_FRAMES_HD uint32_t frame_part_words(uint32_t partBits) { return partBits / 32u; }
// the parts of a frame of S stages: ceil(W / Wp); 1 for whole frames (Wp = 0)
VD_FRAMES_HD uint32_t frame_parts(uint32_t S, uint32_t Wp)
{
    const uint32_t W = frame_words(S);
    return Wp == 0 || W <= Wp ? 1u : (W + Wp - 1u) / Wp;
}
// part j of a frame of S stages: its first word and its words (0: the part starts at or past the frame's W)
struct FramePart {
    uint32_t word0, words;
};
VD_FRAMES_HD FramePart frame_part(uint32_t S, uint32_t Wp, uint32_t j)
{
    const uint32_t W = frame_words(S);
    if (Wp == 0) return {0u, j == 0 ? W : 0u};
    const uint32_t w0 = j * Wp;  // j <= partsMax + kFrmWaves, Wp <= 2^15: below 2^32
    if (w0 >= W) return {w0, 0u};
    return {w0, W - w0 < Wp ? W - w0 : Wp};
}
// first stage of part j in the frame's padded or extended stream: a multiple of kFrmGroup
VD_FRAMES_HD uint32_t frame_part_stage(uint32_t Wp, uint32_t j) { return 32u * j * Wp; }
// workgroups per frame of a launch whose longest frame has partsMax parts
VD_FRAMES_HD uint32_t frame_part_groups(uint32_t partsMax) { return (partsMax + kFrmWaves - 1u) / kFrmWaves; }
// the frame and part of wave wv (< kFrmWaves) of workgroup b at G workgroups per frame
struct FrameWave {
    uint32_t frame, part;
};
VD_FRAMES_HD FrameWave frame_wave(uint32_t b, uint32_t wv, uint32_t G)
{
    const uint32_t f = b / G;
    return {f, (b - f * G) * kFrmWaves + wv};
}
// the workgroups of a launch of nframes frames of at most maxFrameBits stages in parts of partBits (64 bits: the
// caller compares with kFrmMaxGrid)
inline uint64_t frame_parts_grid(uint64_t nframes, uint32_t maxFrameBits, uint32_t partBits)
{
    const uint32_t parts = frame_parts(maxFrameBits, frame_part_words(partBits));
    if (parts <= 1) return (nframes + kFrmWaves - 1u) / kFrmWaves;
    return nframes * frame_part_groups(parts);
}
// the argument check a part length adds to every frame entry point (VD_ERR_ARG): the message, or null
inline const char* frame_parts_error(uint64_t maxFrameBits, int nframes, uint64_t partBits)
{
    if (!frame_part_bits_valid(partBits)) return "partBits must be 0 or a multiple of 96 in [96, 2^20]";
    if (maxFrameBits < 1 || maxFrameBits > kFrmMaxBits || nframes < 1) return nullptr;  // (the family's own check reports these)
    if (frame_parts_grid((uint64_t)nframes, (uint32_t)maxFrameBits, (uint32_t)partBits) > kFrmMaxGrid)
        return "nframes frames in parts of partBits need more than 2^31 - 1 workgroups";
    return nullptr;
}

// ---------------------------------------------------------------- int8 frames (channel ids kI8 + kFrm + ... + format)
// The four families above on frames of int8 channel values, one byte each in mother order and plain memory order
// (not the packed words of the stream decodes): a frame of S stages under a pattern holds punct_len(2 S) bytes, and
// its decode is the float family's decode of the frame (float)q -- the same padded or extended stream, pad value,
// erasures, phase rule and parts.  Only the byte offsets differ, the helpers above with VB = 1:
//   unpunctured (pattern (1, 1, 1)): a stage's two values are one aligned 16-bit access (first encoder output in
//     the low byte) against a resource of 2 S bytes.  Stage p of the padded stream reads at frame_offset<1>(p) =
//     2 (p - 26) with frame_offset's clamp: it wraps to 2^32 - 2 (26 - p) for p < 26, and for p = 25 the end of the
//     2-byte access, 2^32, is 0 in 32 bits as the end of the 8-byte access is, so such a lane reads at kFrmOutside,
//     whose end 2^31 + 2 lies past every range (<= 2 kFrmMaxBits) with no wrap.  For p >= 26, 2 p < 2^22.  A
//     tail-biting frame stage t reads at tb_offset<1>(t) = 2 t, offset + 2 <= 2 S;
//   punctured: single-byte accesses against a resource of pfrm_bytes<1> = punct_len(2 S) <= 2^21 bytes, at the
//     kept index itself.  The offsets are a quarter of the float ones, so what the float maps rely on holds with
//     room to spare: base4 = q0 Kp <= 2 S < 2^22 and every kept offset stay below 2^24 (the 24-bit products x m16 <
//     2^23, dq Kp < 112 * 32, dq period < 112 * 16 are those of pfrm_offsets, VB = 1 only drops a factor), a
//     punctured value or lead stage takes kFrmOutside and kFrmOutside | offset + 1 does not wrap in 32 bits, and a
//     stage >= S lands at or past the range's end since the kept indices grow with the stage.
// An out-of-range 8- or 16-bit buffer load returns zero as a dword load does; tests/test_gpu_byte_frames.py settles
// it on the device (frames of one stage, neighbours of other frames' extreme values).
// tests/cxx/byte_frames_check.cpp checks the helpers below against a plain enumeration.
constexpr int kByteFramesOpen = 0, kByteFramesTerminated = 1, kByteFramesTailbiting = 2;  // vd_capi.h VD_FRAMES_*
// the pattern that selects the unpunctured kernels (any other valid pattern, a keep-all one of a longer period
// too, selects the punctured ones)
VD_FRAMES_HD bool byte_frames_unpunctured(int period, uint32_t keep0, uint32_t keep1)
{
    return period == 1 && keep0 == 1u && keep1 == 1u;
}

// ---------------------------------------------------------------- mixed frames (channel ids kMix + a punctured frame id)
// One launch of frames at several code rates: frame f decodes under pattern rate[f] of a table of up to kMixMaxPatterns
// patterns the decoder holds on the device, and may start at its own value index off[f] of the received buffer instead
// of at f strides.  The table is an array of 32-byte records, a record the Punct of punct_make (6 dwords) and 2 dwords
// of padding: a wave reads its record once at set-up (index out of the table: the wave returns before any load of
// received values) and from there on the kernel is the punctured family's, with the wave's own pattern where the
// uniform launch has Geom::pun.  (1, 1, 1) is a legal entry and takes the same punctured path (single-value loads: no
// 8-byte or 2-byte alignment rule), whose words equal the unpunctured family's.  An offset counts values (floats, or
// bytes for int8), so every offset is aligned by construction; the frame's resource covers its pfrm_bytes from there,
// exactly as it does at f strides.  tests/cxx/mixed_frames_check.cpp checks the helpers below against a plain
// enumeration.
constexpr int kMixMaxPatterns = 16;
constexpr uint32_t kMixRecordDwords = 8;  // a record's stride in the device table
struct MixRecord {
    Punct pn;
    uint32_t pad[2] = {0u, 0u};
};
static_assert(sizeof(MixRecord) == 4 * kMixRecordDwords && sizeof(Punct) == 24, "the device table's record layout");
// the record of a valid pattern
inline MixRecord mix_record(int period, uint32_t keep0, uint32_t keep1)
{
    MixRecord r;
    r.pn = punct_make(period, keep0, keep1);
    return r;
}
// vd_set_frame_patterns' checks of n (period, keep0, keep1) triples (VD_ERR_ARG): the message, or null
inline const char* mixed_table_error(const uint32_t* triples, int n)
{
    if (n < 0 || n > kMixMaxPatterns) return "n must be in [0, 16]";
    if (n > 0 && !triples) return "null triples with n > 0";
    for (int i = 0; i < n; i++) {
        const uint32_t period = triples[3 * i];
        if (period > (uint32_t)kPunctMaxPeriod || !punct_valid((int)period, triples[3 * i + 1], triples[3 * i + 2]))
            return "invalid puncture pattern in the table: 1 <= period <= 16, keep0 and keep1 are period-bit masks, at least one bit set";
    }
    return nullptr;
}
// the received bytes of the longest frame of S stages over a table of n records
template <uint32_t VB = 4>
inline uint32_t mix_max_bytes(const MixRecord* table, int n, uint32_t S)
{
    uint32_t m = 0;
    for (int i = 0; i < n; i++) {
        const uint32_t b = pfrm_bytes<VB>(table[i].pn, S);
        m = b > m ? b : m;
    }
    return m;
}
// The blocking host variants know every frame's place: frame f (S stages, pattern index rate, out-of-table or S = 0:
// nothing read) must lie inside the total values of the buffer.  first .. first + count: the values it reads.
inline bool mixed_frame_inside(uint64_t first, uint64_t count, uint64_t total) { return count <= total && first <= total - count; }

// ---------------------------------------------------------------- the family record and the one argument check
// What a frame launch is, in four bits: pun, the frames hold the kept values of punctured frames; tb, they are
// tail-biting (no pad: terminated means nothing); i8, they hold int8 values and strides count bytes; mix, every frame
// has its own pattern of the decoder's table (always a punctured kernel: pun is set with it).  The kernel table
// (vd_plan.h launcher_frames), the names (plan_name), the argument check below and the launch (vd_capi.hip) all go
// by this record.
struct FrameFamily {
    bool pun, tb, i8, mix;
};
// the family of vd_decoder_kernel_name's input codes 3 .. 14: 3 .. 6 the float families (frames, punctured,
// tail-biting, punctured tail-biting), 7 .. 10 their int8 twins, 11 / 12 mixed frames padded / tail-biting, 13 / 14
// their int8 twins
inline FrameFamily frame_family_of_input(int llr)
{
    if (llr >= 11) return {true, (llr & 1) == 0, llr >= 13, true};
    return {((llr - 3) & 1) != 0, ((llr - 3) & 2) != 0, llr >= 7, false};
}

constexpr int kFrameErrOptions = -1, kFrameErrArg = -2;  // vd_capi.h VD_ERR_OPTIONS, VD_ERR_ARG
constexpr int kFrameHard = 0, kFrameSoft8 = 2;           // vd_kernels.h HARD, SOFT8 (the format: options & 0xF)

// One call of a frame entry point, as plain values.
struct FrameArgs {
    FrameFamily fam;            // int8 frames: pun = !byte_frames_unpunctured(pattern); tb = kind is tail-biting
    uint64_t addr;              // of the first frame's first value; 0 for the host buffers of the blocking variants
    uint64_t stride;            // bytes from a frame's values to the next frame's
    bool offsets;               // mixed: the launch has per-frame offsets (the stride is then ignored)
    uint64_t outStride;
    uint64_t maxFrameBits;      // in stages
    int nframes;
    int kind;                   // kByteFrames*
    float scale;
    int period;                 // the pattern; (1, 1, 1) for frames and tail-biting frames, unused by mixed launches
    uint32_t keep0, keep1;
    int options;                // the decoder's: its format decides the refusals
    uint64_t partBits;          // ... its part length
    const MixRecord* table;     // ... and its pattern table (mixed launches)
    int tableN;
};
// the bytes the values of a frame of S <= kFrmMaxBits stages occupy at most: under the call's (valid) pattern, or
// under the table's densest one
inline uint32_t frame_value_bytes(const FrameArgs& a, uint32_t S)
{
    if (a.fam.mix) return a.fam.i8 ? mix_max_bytes<1>(a.table, a.tableN, S) : mix_max_bytes<4>(a.table, a.tableN, S);
    const Punct pn = punct_make(a.period, a.keep0, a.keep1);
    return a.fam.i8 ? pfrm_bytes<1>(pn, S) : pfrm_bytes<4>(pn, S);
}

#define VD_HARD_PUNCTURED " on a HARD decoder: a punctured value must decode as code 0 = value 0, and HARD's v > 0 ? 1 : 0 turns it into a hard 0; use "
#define VD_HARD_OPEN "open frames on a HARD decoder: the stages after an open frame are erasures, and HARD's v > 0 ? 1 : 0 has no neutral code; terminate the frames or use "
#define VD_I8_WIDE "int8 frames on a SOFT16 or FP32 decoder: an int8 value carries nothing that a SOFT8 decoder does not use; use "
// The checks of every frame entry point behind its null-pointer check: the message and *code (kFrameErrArg or
// kFrameErrOptions), or null when the call is good.  One order for all: the argument rules (kind, pattern, maxFrameBits,
// nframes, scale, alignment, overlap of the values, overlap of the output), then frame_parts_error, then the refusals
// by the decoder's format (int8 on SOFT16 / FP32, open frames on HARD, punctured frames on HARD; none for tail-biting
// frames).  Mixed launches differ: their refusals come first and the empty table leads their argument rules.  The
// alignment rule, the overlap rule's frame bytes and the wording are the family's.
inline const char* frame_args_error(const FrameArgs& a, int* code)
{
    const FrameFamily f = a.fam;
    const int ch = a.options & 0xF;
    float pad;
    *code = kFrameErrOptions;
    if (f.mix && ch == kFrameHard) return "mixed frames" VD_HARD_PUNCTURED "SOFT4, SOFT8, SOFT16 or FP32";
    if (f.mix && f.i8 && ch > kFrameSoft8) return VD_I8_WIDE "SOFT4 or SOFT8";
    *code = kFrameErrArg;
    if (f.mix && (a.tableN < 1 || a.tableN > kMixMaxPatterns || !a.table))
        return "the decoder's pattern table is empty: call vd_set_frame_patterns first";
    if ((f.i8 || f.mix) && a.kind != kByteFramesOpen && a.kind != kByteFramesTerminated && a.kind != kByteFramesTailbiting)
        return "kind must be VD_FRAMES_OPEN, VD_FRAMES_TERMINATED or VD_FRAMES_TAILBITING";
    if (!f.mix && !punct_valid(a.period, a.keep0, a.keep1))
        return "invalid puncture pattern: 1 <= period <= 16, keep0 and keep1 are period-bit masks, at least one bit set";
    if (a.maxFrameBits < 1 || a.maxFrameBits > kFrmMaxBits) return "maxFrameBits must be in [1, 2^20]";
    if (a.nframes < 1) return "nframes must be >= 1";
    if (f.tb) {  // no pad value to form
        if (!(a.scale > 0.0f) || !(a.scale <= 3.4028234663852886e38f)) return "scale must be finite and > 0";
    } else if (!frame_pad(a.scale, &pad)) {
        return "scale must be finite and > 0 (and -65536 / scale finite)";
    }
    // alignment: of the widest access a stage's values take
    if (f.mix) {  // single values, at offsets that count values
        if (!f.i8 && (a.addr & 3)) return "rx_d must be 4-byte aligned";
        if (!f.i8 && !a.offsets && (a.stride & 3)) return "rx_stride must be a multiple of 4 bytes";
    } else if (f.i8) {
        if (!f.pun && ((a.addr | a.stride) & 1))
            return "q_d and q_stride must be multiples of 2 bytes under pattern (1, 1, 1): a stage is one 16-bit access";
    } else if (f.pun) {
        if ((a.addr | a.stride | a.outStride) & 3) return "rx_d, rx_stride and output_stride must be multiples of 4 bytes";
    } else {
        if (a.addr & 7) return "llr_d must be 8-byte aligned";
        if ((a.stride & 7) || (a.outStride & 3)) return "llr_stride % 8 or output_stride % 4 != 0";
    }
    if ((f.i8 || f.mix) && (a.outStride & 3)) return "output_stride must be a multiple of 4 bytes";
    if (a.nframes > 1 && !(f.mix && a.offsets) && a.stride < frame_value_bytes(a, (uint32_t)a.maxFrameBits))
        return f.mix   ? "rx_stride smaller than the received bytes of a maxFrameBits frame under the table's densest pattern: frames would overlap"
               : f.i8  ? "q_stride smaller than vd_punctured_len(2 * maxFrameBits): frames would overlap"
               : f.pun ? "rx_stride smaller than 4 * vd_punctured_len(2 * maxFrameBits): frames would overlap"
                       : "llr_stride smaller than 8 * maxFrameBits: frames would overlap";
    if (a.nframes > 1 && a.outStride < 4ull * frame_words((uint32_t)a.maxFrameBits))
        return "output_stride smaller than vd_frame_output_size(maxFrameBits): frames would overlap";
    if (const char* why = frame_parts_error(a.maxFrameBits, a.nframes, a.partBits)) return why;
    if (f.mix) return nullptr;
    *code = kFrameErrOptions;
    if (f.i8 && ch > kFrameSoft8) return VD_I8_WIDE "HARD, SOFT4 or SOFT8";
    if (ch == kFrameHard && a.kind == kByteFramesOpen && (f.i8 || !f.pun))
        return f.i8 ? VD_HARD_OPEN "SOFT4 or SOFT8" : VD_HARD_OPEN "SOFT4, SOFT8, SOFT16 or FP32";
    if (ch == kFrameHard && f.pun)
        return f.i8   ? "punctured frames" VD_HARD_PUNCTURED "SOFT4 or SOFT8"
               : f.tb ? "punctured tail-biting frames" VD_HARD_PUNCTURED "SOFT4, SOFT8, SOFT16 or FP32"
                      : "punctured frames" VD_HARD_PUNCTURED "SOFT4, SOFT8, SOFT16 or FP32";
    return nullptr;
}
#undef VD_HARD_PUNCTURED
#undef VD_HARD_OPEN
#undef VD_I8_WIDE

}  // namespace vd
