/*
 * vd_capi.h -- C-ABI of the MI355X-native Viterbi decoder (K=7, R=1/2, polynomials 0171/0133).
 *
 * This is the drop-in boundary for the reference's decode path
 * (alireza-md93/GPU-Accelerated-Viterbi-Decoder, class ViterbiCUDA<options>, src/viterbi/viterbi.h:43-152
 * and src/viterbi/viterbi.cu:10-139,210-262).  Plain pointers and sizes only: no HIP, CUDA or torch
 * types cross it.  include/viterbi.h rebuilds ViterbiCUDA<options> on top of these entry points;
 * INTEGRATION.md shows the bindings (C++ header, ctypes) a maintainer adds.
 *
 * Option bitmask: identical encoding to the reference (viterbi.h:7-20):
 *   channel  bits 0-3 : HARD=0 SOFT4=1 SOFT8=2 SOFT16=3 FP32=4
 *   metric   bits 4-7 : M_B32=0x00 M_B16=0x10 M_FP16=0x20
 *   output   bits 8-11: O_B32=0x000 O_B16=0x100
 *   compMode bits 12-15: REG=0x0000 DPX=0x1000  (DPX decodes identically to REG: the reference never
 *                        forwards compMode to its ACS, viterbi.cu:181,192,204)
 *
 * Status codes: every entry point that can fail returns an int (VD_OK = 0, negative on error) and
 * records a message readable with vd_last_error().  The header-only ViterbiCUDA wrapper maps a
 * non-zero status to stderr + exit(EXIT_FAILURE), the reference's HANDLE_ERROR behaviour
 * (gpuerrors.h:8-17).
 */
#ifndef VD_CAPI_H
#define VD_CAPI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VD_OK 0
#define VD_ERR_OPTIONS (-1)   /* option combination disabled by OptionsValid (viterbi.h:22-41) */
#define VD_ERR_ARG (-2)       /* null handle/pointer, or inputNum too small (< 128 encoded values) */
#define VD_ERR_DEVICE (-3)    /* HIP runtime error (message in vd_last_error) */
#define VD_ERR_NOMEM (-4)     /* device or pinned allocation failed */
#define VD_ERR_NOKERNEL (-5)  /* the gfx950 code object is missing from this build */

typedef struct vd_decoder vd_decoder;

/* ---- option / size helpers (replace ViterbiCUDA::getInputSize/getMessageLen/getOutputSize,
 *      viterbi.cu:63-92; sizes in bytes except vd_message_len, which is in decoded bits) ---- */

/* 1 when OptionsValid<options>::value is true (viterbi.h:22-41), else 0 */
int vd_options_valid(int options);
/* bytes of packed channel input for inputNum encoded values (getInputSize, viterbi.cu:63-84) */
size_t vd_input_size(int options, size_t inputNum);
/* decoded bits produced (getMessageLen, viterbi.cu:86-88); 0 when inputNum < 128 */
size_t vd_message_len(int options, size_t inputNum);
/* bytes of decoded output (getOutputSize, viterbi.cu:90-92) */
size_t vd_output_size(int options, size_t inputNum);
/* number of independent stream chunks the decode is partitioned into (6400, viterbi.cu:19) */
int vd_num_chunks(void);

/* ---- decoder objects (replace ViterbiCUDA() / ViterbiCUDA(size_t) / ~ViterbiCUDA,
 *      viterbi.cu:23-42,44-61) ---- */

/* Create a decoder for `options` on HIP device `device` (the reference hard-codes device 0,
 * viterbi.cu:132-139).  preallocInputNum > 0 reserves device buffers for that many encoded values,
 * so later runs of that size or smaller allocate nothing (the reference's pre-allocating
 * constructor, with the leak of viterbi.cu:31-36 fixed). */
int vd_create(int options, size_t preallocInputNum, int device, vd_decoder** out);
int vd_destroy(vd_decoder* dec);

/* Blocking host-to-host decode (replaces ViterbiCUDA::run, viterbi.cu:210-238): copies
 * vd_input_size(options, inputNum) bytes from input_h, decodes, copies vd_output_size bytes to
 * output_h.  kernel_ms (optional) receives the decode-kernel time in ms measured with HIP events,
 * the same scope as the reference's kernelTime (viterbi.cu:224-232). */
int vd_run(vd_decoder* dec, const void* input_h, void* output_h, size_t inputNum, float* kernel_ms);

/* Asynchronous device-to-device decode on `stream` (a hipStream_t passed as void*, NULL = the
 * null stream).  input_d / output_d are device pointers on the decoder's device, sized as above.
 * No allocation, no synchronisation: safe to capture in a hipGraph.  The stream (for NULL: the calling
 * thread's current device) must belong to the decoder's device, else VD_ERR_ARG.  Launches on any
 * number of streams may run concurrently: no launch shares device scratch with another. */
int vd_run_device(vd_decoder* dec, const void* input_d, void* output_d, size_t inputNum, void* stream);

/* nbatch independent batches of inputNum encoded values each in ONE launch (new; for batched callers):
 * batch b reads input_d + b * input_stride bytes and writes output_d + b * output_stride bytes.  Inputs are
 * only read, so input_stride is free (0: every batch decodes the same input; smaller than vd_input_size:
 * overlapping windows); output_stride >= vd_output_size unless nbatch == 1 (else VD_ERR_ARG: overlapping
 * outputs).  Each batch decodes exactly
 * as vd_run_device would (the reference's 6400-chunk partition per batch); one launch fills the GPU's
 * tail with the next batch's chunks.  Strides are multiples of 4 bytes; device pointers as above. */
int vd_run_device_batch(vd_decoder* dec, const void* input_d, size_t input_stride, void* output_d,
                        size_t output_stride, size_t inputNum, int nbatch, void* stream);

/* Batch sharding over several devices of one node: batch b (input_h[b] -> output_h[b],
 * each inputNum encoded values) is decoded by devices[b % ndev]; batches are independent, so the
 * result of each is identical to a single-device vd_run of that batch.  wall_ms (optional) is the
 * wall time from first H2D to last D2H. */
int vd_run_batches(int options, const void* const* input_h, void* const* output_h, size_t inputNum,
                   int nbatches, const int* devices, int ndev, float* wall_ms);

/* ---- streaming host pipeline (the reference allocates, copies and frees per call,
 *      viterbi.cu:210-238) ---- */

/* Pinned (page-locked) host buffers for full-rate PCIe copies; NULL on failure. */
void* vd_host_alloc(size_t bytes);
int vd_host_free(void* p);
/* Decode nbatches independent batches (input_h[b] -> output_h[b], inputNum encoded values each) on
 * the decoder's device.  Pinned buffers (vd_host_alloc, hipHostMalloc, hipHostRegister): the decode
 * kernels read the packed input from and write the decoded words to host memory directly over PCIe
 * (zero-copy, no staging).  Pageable buffers: H2D of batch b+1, decode of batch b and D2H of batch
 * b-1 overlap (two device buffer sets, three streams).  Each result equals vd_run of that batch.
 * wall_ms (optional): wall time of the whole call.  (vd_run also decodes zero-copy when both of its
 * host buffers are pinned.) */
int vd_run_stream(vd_decoder* dec, const void* const* input_h, void* const* output_h, int nbatches, size_t inputNum,
                  float* wall_ms);

/* ---- float channel values (the reference's SoftDecisionPacker stage, viterbiDF.h:98-167) ----
 * The reference packs float channel values on the host (quant(v*scale): HARD v > 0; SOFT4/SOFT8
 * (int)lrintf saturated to 4/8 bits; SOFT16 lrintf saturated to 16 bits; FP32 v*scale; MSB-first
 * words) and copies the packed words to the GPU.  These entry points take the floats on the device
 * instead; results are bit-identical to packing with SoftDecisionPacker(channel, scale) and then
 * decoding.  Float buffers must be 16-byte aligned; inputNum values. */

/* Pack inputNum float values into vd_input_size(options, inputNum) bytes of encPack_t words on the
 * device (a trailing partial word packs missing values as 0.0f). */
int vd_pack_device(int options, const float* llr_d, size_t inputNum, float scale, void* packed_d, void* stream);
/* Fused quantise + decode from device floats: the branch-metric table build quantises each value
 * (no packed intermediate, one kernel), every format. */
int vd_run_device_llr(vd_decoder* dec, const float* llr_d, void* output_d, size_t inputNum, float scale,
                      void* stream);
/* nbatch independent batches of inputNum device floats in one launch (as vd_run_device_batch): batch b
 * reads llr_d + b * llr_stride bytes and writes output_d + b * output_stride bytes (strides multiples
 * of 16 and 4 bytes; llr_stride free as input_stride, output_stride as vd_run_device_batch). */
int vd_run_device_llr_batch(vd_decoder* dec, const float* llr_d, size_t llr_stride, void* output_d,
                            size_t output_stride, size_t inputNum, float scale, int nbatch, void* stream);
/* Blocking host-to-host variant (H2D of the floats, fused decode, D2H); kernel_ms as in vd_run. */
int vd_run_llr(vd_decoder* dec, const float* llr_h, void* output_h, size_t inputNum, float scale, float* kernel_ms);

/* ---- punctured streams (rates 2/3, 3/4, ...; new, the reference decodes rate 1/2 only) ----
 * A puncture pattern is (period, keep0, keep1), 1 <= period <= 16: bit i of keep0 says that the first encoder
 * output (0171, mother index 2t) of every stage t with t % period == i was transmitted, keep1 the same for the
 * second output (0133, mother index 2t + 1); at least one bit set, none at or above bit `period`.  E.g. rate
 * 2/3: (2, 0x1, 0x3); rate 3/4: (3, 0x5, 0x3); (1, 1, 1) is the unpunctured stream.
 * inputNum keeps its meaning, the number of mother-code values (2 per stage), so the size helpers above hold
 * unchanged; the received buffer holds the kept values in mother order as floats, vd_punctured_len of them.
 * The decode equals, word for word, vd_run_device_llr of the depunctured stream: inputNum floats, the
 * received value at kept positions and +0.0f at punctured ones, same scale.  The depuncturing is an index
 * map in the loads of the branch-metric table build: no expanded copy exists.  SOFT4, SOFT8, SOFT16 and FP32
 * decoders (code 0 = value 0 adds nothing to a branch metric); a HARD decoder has no neutral code for a
 * punctured value and gets VD_ERR_OPTIONS.  An invalid pattern, or inputNum / 2 above 2^32 - 4097: VD_ERR_ARG.
 * FP32 decoders want a scale like the harness's 40000 (values saturating the metric's [-8, 7]): at scale 1 the
 * truncating FP32 branch metric loses a lone +-1 beside a punctured value. */

/* floats in the received buffer for inputNum mother-code values: the kept positions among the first
 * 2 * (inputNum / 2); 0 on an invalid pattern */
size_t vd_punctured_len(int period, uint32_t keep0, uint32_t keep1, size_t inputNum);
/* Fused depuncture + quantise + decode of device floats, under the rules of vd_run_device_llr (asynchronous, no
 * allocation, capturable, the stream on the decoder's device).  rx_d needs 4-byte alignment only (single-dword
 * loads; the 16-byte rule of the other float entry points does not apply). */
int vd_run_device_punct(vd_decoder* dec, const float* rx_d, void* output_d, size_t inputNum, float scale,
                        int period, uint32_t keep0, uint32_t keep1, void* stream);
/* nbatch independent punctured batches in one launch: batch b reads rx_d + b * rx_stride bytes and writes
 * output_d + b * output_stride bytes (both strides multiples of 4 bytes; rx_stride free as input_stride,
 * output_stride as vd_run_device_batch). */
int vd_run_device_punct_batch(vd_decoder* dec, const float* rx_d, size_t rx_stride, void* output_d,
                              size_t output_stride, size_t inputNum, float scale, int period, uint32_t keep0,
                              uint32_t keep1, int nbatch, void* stream);
/* Blocking host-to-host variant (H2D of the vd_punctured_len floats, decode, D2H); kernel_ms as in vd_run. */
int vd_run_punct(vd_decoder* dec, const float* rx_h, void* output_h, size_t inputNum, float scale, int period,
                 uint32_t keep0, uint32_t keep1, float* kernel_ms);

/* ---- independent frames, decoded from first bit to last (new; the reference decodes one long stream and
 *      never its first 26 and last 38 bits) ----
 * A frame is S trellis stages: 2 S float channel values, first encoder output first, of an encoder started in
 * state 0 and either flushed back to state 0 by six tail zeros (terminated = 1: the frame's last six
 * information bits are zeros) or simply stopped (terminated = 0, an open frame).  With W = ceil(S / 32) and
 * P = 64 + 32 W, the frame decode equals, word for word, the one-chunk decode (inputNum = 2 P) of the frame's
 * padded stream: stages [0, 26) hold the pad value twice, stages [26, 26 + S) the frame, and the stages from
 * 26 + S on the pad value (terminated) or +0.0f, an erasure (open).  The pad value is the one whose
 * quantisation is the format's most negative code, "both encoder outputs 0" at full confidence (HARD bit 0,
 * SOFT4 -8, SOFT8 -128, SOFT16 -32768, FP32 -8 after the clamp), whatever the scale.  It writes W 32-bit words
 * (O_B16: 2 W 16-bit words); decoded bit i (MSB first, as vd_count_errors reads it) is information bit i of the
 * frame, and the bits of the last word past S decode the padding (0 for a terminated frame).  The padded stream
 * is never stored: the virtual stages are a select in the loads of the branch-metric table build, one wave
 * decodes one frame, and all frames go in one launch.  Every format and metric; an open frame needs a neutral
 * code, so a HARD decoder with terminated = 0 gets VD_ERR_OPTIONS.  VD_ERR_ARG: maxFrameBits outside
 * [1, 2^20], nframes < 1, scale not finite and > 0, a misaligned pointer or stride, overlapping frames.
 * Punctured frames: vd_run_device_punct_frames below; tail-biting frames: vd_run_device_tb_frames below; punctured
 * tail-biting frames: vd_run_device_punct_tb_frames below.
 * Frames of int8 channel values are supported: vd_run_device_byte_frames below, for all four families; frames of
 * mixed code rates and per-frame offsets in one launch: vd_run_device_mixed_frames below.  The reference's MSB-first
 * packed words as frame input, int16 frames, frames longer than 2^20 stages and vd_decode_pk twins of the frame
 * kernels are not. */

/* bytes a frame of frameBits stages decodes to: 4 * ceil(frameBits / 32), for O_B32 and O_B16 alike */
size_t vd_frame_output_size(int options, size_t frameBits);
/* nframes frames in one launch, under the rules of vd_run_device_llr (asynchronous, no allocation, capturable,
 * the stream on the decoder's device).  Frame f reads 2 S_f floats at llr_d + f * llr_stride bytes and writes
 * vd_frame_output_size(S_f) bytes at output_d + f * output_stride bytes, S_f = min(frame_bits_d[f],
 * maxFrameBits), or maxFrameBits when frame_bits_d is NULL; a frame of 0 stages writes nothing, and no byte
 * outside a frame's words is written.  Nothing outside a frame's 2 S_f floats is read.  llr_d 8-byte aligned,
 * llr_stride a multiple of 8, output_stride a multiple of 4; with nframes > 1, llr_stride >= 8 * maxFrameBits
 * and output_stride >= vd_frame_output_size(maxFrameBits). */
int vd_run_device_frames(vd_decoder* dec, const float* llr_d, size_t llr_stride, void* output_d, size_t output_stride,
                         const uint32_t* frame_bits_d /* device, or NULL: every frame has maxFrameBits */,
                         size_t maxFrameBits, int nframes, int terminated, float scale, void* stream);
/* Blocking host-to-host variant over host buffers of the same layout (H2D, the launch, D2H); the output bytes
 * no frame writes keep their values.  kernel_ms as in vd_run. */
int vd_run_frames(vd_decoder* dec, const float* llr_h, size_t llr_stride, void* output_h, size_t output_stride,
                  const uint32_t* frame_bits_h, size_t maxFrameBits, int nframes, int terminated, float scale,
                  float* kernel_ms);

/* ---- punctured frames (new: the two features above in one launch, e.g. 802.11a/g packets at rate 2/3 or 3/4) ----
 * A punctured frame of S stages under a pattern (period, keep0, keep1) -- the rules of vd_punctured_len -- is stored
 * as the kept values of its 2 S mother-code values, in mother order, as floats: vd_punctured_len(period, keep0,
 * keep1, 2 S) of them.  The pattern's phase restarts at every frame's first stage: frame stage t uses bit
 * t % period.  The decode equals, word for word, vd_run_device_frames of the depunctured frame: 2 S floats, the
 * received value at kept positions and +0.0f at punctured ones, same terminated, scale and options; (1, 1, 1) is
 * the unpunctured frame and gives exactly vd_run_device_frames of the same buffer.  A frame too short to hold any
 * kept value (e.g. (16, 0x8000, 0) with S <= 15) is legal: it reads nothing and decodes as S erasures between the
 * pads.  No depunctured copy exists: the index map sits in the loads of the branch-metric table build, as in
 * vd_run_device_punct.  SOFT4, SOFT8, SOFT16 and FP32 decoders; a HARD decoder gets VD_ERR_OPTIONS, terminated or
 * open (a punctured value has no hard code).  The window limit of punctured streams carries over: rates above 3/4
 * decode exactly as defined but not error-free. */

/* nframes punctured frames in one launch, under the rules of vd_run_device_frames (asynchronous, no allocation,
 * capturable, the stream on the decoder's device).  frame_bits_d and maxFrameBits count stages (information bits
 * including any tail), not received floats: S_f = min(frame_bits_d[f], maxFrameBits), or maxFrameBits when
 * frame_bits_d is NULL.  Frame f reads exactly vd_punctured_len(period, keep0, keep1, 2 S_f) floats at rx_d + f *
 * rx_stride bytes and writes vd_frame_output_size(S_f) bytes at output_d + f * output_stride bytes, nothing else;
 * S_f = 0 writes nothing.  rx_d needs 4-byte alignment only (single-dword loads), rx_stride and output_stride are
 * multiples of 4.  VD_ERR_ARG: an invalid pattern, maxFrameBits outside [1, 2^20], nframes < 1, scale not finite
 * and > 0, a misaligned pointer or stride, and with nframes > 1 rx_stride < 4 * vd_punctured_len(period, keep0,
 * keep1, 2 * maxFrameBits) or output_stride < vd_frame_output_size(maxFrameBits). */
int vd_run_device_punct_frames(vd_decoder* dec, const float* rx_d, size_t rx_stride, void* output_d, size_t output_stride,
                               const uint32_t* frame_bits_d /* device, or NULL: every frame has maxFrameBits */,
                               size_t maxFrameBits, int nframes, int terminated, float scale, int period, uint32_t keep0,
                               uint32_t keep1, void* stream);
/* Blocking host-to-host variant over host buffers of the same layout (H2D, the launch, D2H); the output bytes
 * no frame writes keep their values.  kernel_ms as in vd_run. */
int vd_run_punct_frames(vd_decoder* dec, const float* rx_h, size_t rx_stride, void* output_h, size_t output_stride,
                        const uint32_t* frame_bits_h, size_t maxFrameBits, int nframes, int terminated, float scale,
                        int period, uint32_t keep0, uint32_t keep1, float* kernel_ms);

/* ---- tail-biting frames (new: packets whose encoder starts in the state it ends in, e.g. 802.16 OFDMA's
 *      convolutional code and many short control and burst formats) ----
 * A tail-biting frame is S >= 1 trellis stages, 2 S float channel values, first encoder output first.  The encoder's
 * register at the first stage holds the frame's last six information bits (cyclically for S < 6), so output stage
 * t depends on information bits t, t - 1, ..., t - 6, all taken mod S; no tail is sent.  With W = ceil(S / 32) and
 * P = 64 + 32 W, the frame's extended stream has P stages, and stage p holds both values of frame stage
 * (p - 26) mod S: the non-negative residue, the wrap continuing for as many turns as P needs (S = 1: every stage
 * is the frame's one stage); the same rule defines anything the kernel prefetches beyond P.  The decode equals,
 * word for word, the one-chunk decode (inputNum = 2 P, nchunks = 1, O_B16 policy 0) of the SoftDecisionPacker(
 * options, scale) packing of the extended stream.  It writes W 32-bit words (O_B16: 2 W 16-bit words); decoded
 * bit i (MSB first) with i < S is information bit i, and the remaining bits of the last word decode the wrap
 * (frame bit i mod S).  One pass with the reference's fixed window (26 warm-up stages from equal metrics, 38
 * traceback stages): the extended stream is the interior of a periodic stream, and the window decodes it as it
 * decodes the interior of any stream; no iterations, no search over start states.  No pad stages and no
 * erasures, so every format and metric is supported, HARD included.  The extended stream is never stored: the
 * wrap-around sits in the loads of the branch-metric table build, one wave decodes one frame, all frames go in
 * one launch.  Punctured tail-biting frames: vd_run_device_punct_tb_frames below. */

/* nframes tail-biting frames in one launch, under the rules of vd_run_device_frames (asynchronous, no allocation,
 * capturable, the stream on the decoder's device; the same pointers, strides and lengths array, no terminated
 * argument).  Frame f reads exactly its 2 S_f floats at llr_d + f * llr_stride bytes and writes exactly
 * vd_frame_output_size(S_f) bytes at output_d + f * output_stride bytes, S_f = min(frame_bits_d[f], maxFrameBits),
 * or maxFrameBits when frame_bits_d is NULL; S_f = 0 writes nothing.  VD_ERR_ARG: maxFrameBits outside [1, 2^20],
 * nframes < 1, scale not finite and > 0, llr_d not 8-byte aligned, llr_stride % 8 or output_stride % 4, and with
 * nframes > 1 llr_stride < 8 * maxFrameBits or output_stride < vd_frame_output_size(maxFrameBits). */
int vd_run_device_tb_frames(vd_decoder* dec, const float* llr_d, size_t llr_stride, void* output_d, size_t output_stride,
                            const uint32_t* frame_bits_d /* device, or NULL: every frame has maxFrameBits */,
                            size_t maxFrameBits, int nframes, float scale, void* stream);
/* Blocking host-to-host variant over host buffers of the same layout (H2D, the launch, D2H); the output bytes
 * no frame writes keep their values.  kernel_ms as in vd_run. */
int vd_run_tb_frames(vd_decoder* dec, const float* llr_h, size_t llr_stride, void* output_h, size_t output_stride,
                     const uint32_t* frame_bits_h, size_t maxFrameBits, int nframes, float scale, float* kernel_ms);

/* ---- punctured tail-biting frames (new: the two features above in one launch, e.g. 802.16 OFDMA's tail-biting
 *      code at rates 2/3 and 3/4) ----
 * A punctured tail-biting frame of S >= 1 stages under a pattern (period, keep0, keep1) -- the rules of
 * vd_punctured_len -- is stored as the kept values of its 2 S mother-code values, in mother order, as floats:
 * vd_punctured_len(period, keep0, keep1, 2 S) of them.  The pattern's phase belongs to the frame stage: frame stage
 * t uses bit t % period.  Stage p of the extended stream is frame stage t = (p - 26) mod S and takes the phase of
 * t, so the phase restarts at every wrap, also when S is not a multiple of period.  The decode equals, word for
 * word, vd_run_device_tb_frames of the depunctured frame: 2 S floats, the received value at kept positions and
 * +0.0f at punctured ones, same scale and options.  The pattern (1, 1, 1) gives exactly vd_run_device_tb_frames of
 * the same buffer.  A frame too short to hold any kept value (e.g. (16, 0x8000, 0) with S <= 15) is legal: it reads
 * nothing and decodes as the all-erasure frame.  Neither the depunctured frame nor the extended stream is ever
 * stored: both index maps sit in the loads of the branch-metric table build.  SOFT4, SOFT8, SOFT16 and FP32
 * decoders; a HARD decoder gets VD_ERR_OPTIONS (a punctured value has no hard code).  No pad value, so the scale
 * only has to be finite and > 0.  One pass, no iterations.  The window limit of punctured streams carries over:
 * rates above 3/4 decode exactly as defined but not error-free. */

/* nframes punctured tail-biting frames in one launch, under the rules of vd_run_device_punct_frames without its
 * terminated argument (asynchronous, no allocation, capturable, the stream on the decoder's device).  frame_bits_d
 * and maxFrameBits count stages, not received floats: S_f = min(frame_bits_d[f], maxFrameBits), or maxFrameBits
 * when frame_bits_d is NULL.  Frame f reads exactly vd_punctured_len(period, keep0, keep1, 2 S_f) floats at rx_d +
 * f * rx_stride bytes and writes exactly vd_frame_output_size(S_f) bytes at output_d + f * output_stride bytes;
 * S_f = 0 writes nothing.  rx_d, rx_stride and output_stride are multiples of 4.  VD_ERR_ARG: an invalid pattern,
 * maxFrameBits outside [1, 2^20], nframes < 1, scale not finite and > 0, a misaligned pointer or stride, and with
 * nframes > 1 rx_stride < 4 * vd_punctured_len(period, keep0, keep1, 2 * maxFrameBits) or output_stride <
 * vd_frame_output_size(maxFrameBits). */
int vd_run_device_punct_tb_frames(vd_decoder* dec, const float* rx_d, size_t rx_stride, void* output_d, size_t output_stride,
                                  const uint32_t* frame_bits_d /* device, or NULL: every frame has maxFrameBits */,
                                  size_t maxFrameBits, int nframes, float scale, int period, uint32_t keep0, uint32_t keep1,
                                  void* stream);
/* Blocking host-to-host variant over host buffers of the same layout (H2D, the launch, D2H); the output bytes
 * no frame writes keep their values.  kernel_ms as in vd_run. */
int vd_run_punct_tb_frames(vd_decoder* dec, const float* rx_h, size_t rx_stride, void* output_h, size_t output_stride,
                           const uint32_t* frame_bits_h, size_t maxFrameBits, int nframes, float scale, int period,
                           uint32_t keep0, uint32_t keep1, float* kernel_ms);

/* ---- long frames in parts spread over many waves (new: a few long frames, e.g. one DVB or CCSDS burst, would
 *      otherwise occupy a few waves of a GPU that holds thousands) ----
 * A decoder carries a part length partBits: 0 (the default: one wave decodes a whole frame, everything above) or
 * a multiple of 96 in [96, 2^20].  All eight frame entry points above, and the two int8 ones below, honour it; their signatures and argument
 * rules do not change.  With Wp = partBits / 32, a frame of S stages, W = ceil(S / 32), has ceil(W / Wp) parts,
 * and part j holds w_j = min(Wp, W - j Wp) words.  Part j decodes, word for word, as the one-chunk decode
 * (inputNum = 2 (64 + 32 w_j), nchunks = 1, O_B16 policy 0) of stages [32 j Wp, 32 j Wp + 64 + 32 w_j) of the
 * frame's padded stream (frames, punctured frames) or extended stream (tail-biting, punctured tail-biting), and
 * writes those w_j words (O_B16: 2 w_j) at word j Wp of the frame's output.  A frame with W <= Wp is one part and
 * decodes exactly as with partBits = 0.  Each part is decoded by a wave of its own from equal metrics, with 26
 * warm-up stages before it and 38 traceback stages after it: the frame's own stages where it has them, else pad
 * stages, erasures or the wrap by the same per-stage rule as above.  This is the window every stream entry point
 * uses at every chunk boundary; on noisy input a decode in parts can differ from the whole-frame decode in a few
 * words, as two chunkings of one stream can.  The bytes read and written per frame are unchanged.  The window
 * costs 64 / partBits extra stages: partBits of a few thousand keep it at 1 - 4 %.  The value is read on the host
 * when a frame entry point is called (a captured graph keeps the value it was captured with); do not call the
 * setter concurrently with launches of the same decoder.  One more VD_ERR_ARG of the frame entry points: nframes
 * frames of maxFrameBits in parts of partBits would need more than 2^31 - 1 workgroups (ceil(ceil(W_max / Wp) / 4)
 * per frame).  vd_decoder_kernel_name (llr 3 .. 6) names the parts per frame of such a launch. */

/* VD_ERR_ARG unless partBits is 0 or a multiple of 96 in [96, 2^20] */
int vd_set_frame_part_bits(vd_decoder* dec, size_t partBits);
int vd_frame_part_bits(vd_decoder* dec, size_t* partBits);

/* ---- int8 frames (new: the soft values a demapper delivers, e.g. 802.11, DVB, 802.16 or CCSDS int8 LLRs, decoded
 *      as they are: no widening pass, no float buffer four times the size of the data) ----
 * The four frame families above on frames of int8 channel values.  A frame of S stages under a pattern (period,
 * keep0, keep1) holds vd_punctured_len(period, keep0, keep1, 2 S) int8 values: the kept values of its 2 S mother-code
 * values in mother order (first encoder output first), one byte each, in plain memory order -- not the reference's
 * MSB-first packed words.  The decode equals, word for word, the float entry point of the same family on the buffer
 * (float)q, with the same scale, lengths and pattern and float strides of 4 x the byte strides:
 *   kind                   pattern (1, 1, 1)                         any other valid pattern
 *   VD_FRAMES_OPEN         vd_run_device_frames, terminated = 0      vd_run_device_punct_frames, terminated = 0
 *   VD_FRAMES_TERMINATED   vd_run_device_frames, terminated = 1      vd_run_device_punct_frames, terminated = 1
 *   VD_FRAMES_TAILBITING   vd_run_device_tb_frames                   vd_run_device_punct_tb_frames
 * Everything those contracts say carries over: the pad value -65536 / scale, erasures as +0.0f, the pattern's phase
 * restarting per frame and per wrap, S_f = min(frame_bits_d[f], maxFrameBits), S_f = 0 writing nothing, exactly the
 * frame's bytes read and exactly its words written, and the decoder's part length (vd_set_frame_part_bits).  The
 * values are multiplied by scale, rounded and saturated to the decoder's format like the floats they stand for
 * (scale 1 on a SOFT8 decoder: the values themselves).  Only the loads differ from the float kernels: pattern
 * (1, 1, 1) reads a stage's two values as one 16-bit access, so q_d and q_stride must be multiples of 2; any other
 * pattern reads single bytes at any address and any stride.  output_stride is a multiple of 4.
 * HARD, SOFT4 and SOFT8 decoders, every metric and output width.  VD_ERR_OPTIONS: a SOFT16 or FP32 decoder (an int8
 * value carries nothing that a SOFT8 decoder does not use), and a HARD decoder with VD_FRAMES_OPEN or with a pattern
 * other than (1, 1, 1), as in the float API.  VD_ERR_ARG: a kind outside 0 .. 2, an invalid pattern, maxFrameBits
 * outside [1, 2^20], nframes < 1, a scale the float family rejects (finite and > 0; open and terminated frames also
 * need -65536 / scale finite), a q_d or q_stride that is odd under (1, 1, 1), output_stride % 4, with nframes > 1 a
 * q_stride < vd_punctured_len(period, keep0, keep1, 2 * maxFrameBits) or an output_stride <
 * vd_frame_output_size(maxFrameBits), and the workgroup limit of frames in parts. */
#define VD_FRAMES_OPEN        0
#define VD_FRAMES_TERMINATED  1
#define VD_FRAMES_TAILBITING  2

/* nframes frames of int8 channel values in one launch, under the rules of vd_run_device_frames (asynchronous, no
 * allocation, capturable, the stream on the decoder's device) */
int vd_run_device_byte_frames(vd_decoder* dec, const int8_t* q_d, size_t q_stride, void* output_d, size_t output_stride,
                              const uint32_t* frame_bits_d /* device, or NULL: every frame has maxFrameBits */,
                              size_t maxFrameBits, int nframes, int kind, float scale, int period, uint32_t keep0,
                              uint32_t keep1, void* stream);
/* Blocking host-to-host variant over host buffers of the same layout (H2D, the launch, D2H); the output bytes
 * no frame writes keep their values.  kernel_ms as in vd_run. */
int vd_run_byte_frames(vd_decoder* dec, const int8_t* q_h, size_t q_stride, void* output_h, size_t output_stride,
                       const uint32_t* frame_bits_h, size_t maxFrameBits, int nframes, int kind, float scale, int period,
                       uint32_t keep0, uint32_t keep1, float* kernel_ms);

/* ---- frames of mixed code rates in one launch (new: one 802.11 slot or 802.16 burst set holds packets at rates 1/2,
 *      2/3, 3/4 and 5/6, of different lengths, their soft values back to back) ----
 * A decoder holds a table of up to 16 puncture patterns.  A mixed launch decodes nframes frames of one kind
 * (VD_FRAMES_OPEN, VD_FRAMES_TERMINATED or VD_FRAMES_TAILBITING, for the whole launch), frame f under pattern
 * rate_d[f] of the table (pattern 0 when rate_d is NULL), with S_f = min(frame_bits_d[f], maxFrameBits) stages
 * (maxFrameBits when frame_bits_d is NULL).  Frame f reads exactly vd_punctured_len(pattern_f, 2 S_f) values: at rx_d +
 * f * rx_stride bytes when rx_offsets_d is NULL, else from value index rx_offsets_d[f] of rx_d on -- an index in
 * values (floats, or bytes for int8), not a byte offset, so every offset is aligned by construction; rx_stride is
 * then ignored, the offsets may come in any order, and two frames may share input.  It writes exactly
 * vd_frame_output_size(S_f) bytes at output_d + f * output_stride.  A frame with S_f = 0 or rate_d[f] >= the
 * table's length reads nothing and writes nothing.  Frame f's words equal, word for word, those of
 * vd_run_device_punct_frames (open, terminated) or vd_run_device_punct_tb_frames (tail-biting) of that frame alone
 * under its pattern, and for int8 those of vd_run_device_byte_frames under a pattern other than (1, 1, 1).  (1, 1, 1)
 * is a legal entry -- rate-1/2 frames belong in a mixed batch -- and goes through the same punctured path with
 * single-value loads: its words equal the unpunctured family's, rx_d needs 4-byte alignment only, and the int8 twin
 * has no 2-byte alignment rule.  The decoder's part length (vd_set_frame_part_bits) applies as everywhere: the grid
 * comes from maxFrameBits, and all parts of a frame share its pattern and offset.
 * The kernels (vd_decode_tg<FRM+MIX+...>) read the table on the device when they run.  A captured graph therefore
 * decodes under the table as it stands at replay, not as it stood at capture -- unlike the part length, which is
 * read on the host when the entry point is called.
 * VD_ERR_OPTIONS: a HARD decoder (a punctured value has no hard code); a SOFT16 or FP32 decoder for the int8 twin.
 * VD_ERR_ARG: an empty table, a kind outside 0 .. 2, maxFrameBits outside [1, 2^20], nframes < 1, a scale the
 * family rejects (finite and > 0; open and terminated frames also need -65536 / scale finite), rx_d not 4-byte
 * aligned or (without offsets) rx_stride % 4 for floats, output_stride % 4, with nframes > 1 an output_stride <
 * vd_frame_output_size(maxFrameBits) or (without offsets) an rx_stride below the received bytes of a maxFrameBits
 * frame under the table's densest pattern, and the workgroup limit of frames in parts. */

/* Stores n patterns, 0 <= n <= 16, given as n (period, keep0, keep1) triples, as the decoder's table (host copy and
 * device records; the device buffer is the feature's only allocation, made by the first call and freed by vd_destroy).
 * VD_ERR_ARG: n outside [0, 16], triples NULL with n > 0, a pattern vd_punctured_len would reject; the table is then
 * unchanged.  Blocks until the copy is done.  Do not call it while launches of this decoder are in flight. */
int vd_set_frame_patterns(vd_decoder* dec, const uint32_t* triples, int n);
/* reads the table back: *n patterns, their triples into triples (room for 48 values; NULL: the count only) */
int vd_frame_patterns(vd_decoder* dec, uint32_t* triples, int* n);
/* nframes frames of float values at mixed rates in one launch, under the rules of vd_run_device_frames (asynchronous,
 * no allocation, capturable, the stream on the decoder's device) */
int vd_run_device_mixed_frames(vd_decoder* dec, const float* rx_d, size_t rx_stride,
                               const uint64_t* rx_offsets_d /* device, or NULL: frame f at f * rx_stride bytes */,
                               void* output_d, size_t output_stride,
                               const uint32_t* frame_bits_d /* device, or NULL: every frame has maxFrameBits */,
                               const uint8_t* rate_d /* device, or NULL: every frame uses pattern 0 */,
                               size_t maxFrameBits, int nframes, int kind, float scale, void* stream);
/* its int8 twin (SOFT4 and SOFT8 decoders): strides in bytes, offsets in bytes, any address */
int vd_run_device_byte_mixed_frames(vd_decoder* dec, const int8_t* q_d, size_t q_stride, const uint64_t* q_offsets_d,
                                    void* output_d, size_t output_stride, const uint32_t* frame_bits_d, const uint8_t* rate_d,
                                    size_t maxFrameBits, int nframes, int kind, float scale, void* stream);
/* Blocking host-to-host variants over host arrays of the same layout (H2D, the launch, D2H); the output bytes no frame
 * writes keep their values.  Without offsets the buffer ends with a maxFrameBits frame under the table's densest
 * pattern, as the stride rule has it; with offsets it holds rx_total values (ignored otherwise), and a frame that does
 * not lie inside them is VD_ERR_ARG.  kernel_ms as in vd_run. */
int vd_run_mixed_frames(vd_decoder* dec, const float* rx_h, size_t rx_stride, const uint64_t* rx_offsets_h, size_t rx_total,
                        void* output_h, size_t output_stride, const uint32_t* frame_bits_h, const uint8_t* rate_h,
                        size_t maxFrameBits, int nframes, int kind, float scale, float* kernel_ms);
int vd_run_byte_mixed_frames(vd_decoder* dec, const int8_t* q_h, size_t q_stride, const uint64_t* q_offsets_h, size_t q_total,
                             void* output_h, size_t output_stride, const uint32_t* frame_bits_h, const uint8_t* rate_h,
                             size_t maxFrameBits, int nframes, int kind, float scale, float* kernel_ms);

/* ---- the reference harness's channel source (RandBitGen | ConvolutionalEncoder | AddNoise |
 *      SoftDecisionPacker, viterbiDF.h:20-167), host and GPU ---- */

/* Host-side reference-harness generator (std::mt19937 bits + std::normal_distribution<float>
 * noise, exactly the reference pipeline's semantics, viterbiDF.h:20-167, main.cpp:131-137). */
int vd_simulate_host(int options, size_t N, float snr, uint32_t bitSeed, uint32_t noiseSeed,
                     uint8_t* bits, void* packed);
/* The reference harness's channel source on the GPU, bit-exact with vd_simulate_host for the same
 * seeds: RandBitGen(N, bitSeed) | ConvolutionalEncoder(7, 0171, 0133) | AddNoise(10^(-snr/5), noiseSeed)
 * (viterbiDF.h:20-95; std::mt19937 streams generated in parallel segments from a GF(2) jump-ahead,
 * libstdc++ uniform/normal and glibc logf restated).  bits_d: N bytes (0/1); values_d: 2N floats, the
 * AddNoise output.  Blocking (checks the polar method's sample count).  N <= 2^30. */
int vd_channel_device(size_t N, float snr, uint32_t bitSeed, uint32_t noiseSeed, uint8_t* bits_d, float* values_d,
                      void* stream);
/* vd_channel_device followed by SoftDecisionPacker(type, 40000) (viterbiDF.h:98-167): packed_d gets
 * vd_input_size(options, 2N) bytes, identical to vd_simulate_host's.  bits_d may be NULL.  N % 16 == 0. */
int vd_simulate_device(int options, size_t N, float snr, uint32_t bitSeed, uint32_t noiseSeed, uint8_t* bits_d,
                       void* packed_d, void* stream);
/* test hook: std::mt19937(seed)'s 624-word state array after n outputs (host GF(2) jump-ahead) */
int vd_mt_state_after(uint32_t seed, uint64_t n, uint32_t* state624);
/* bit-error count of a decoded buffer against the source bits (main.cpp:151-171) */
long long vd_count_errors(int options, const uint8_t* bits, size_t N, const void* decoded, size_t decodedBytes);

/* ---- runtime info ---- */
/* split launches (DESIGN.md §4 "load balance"): how many pieces of split chunks (vd_decode_tg segment
 * launches) or second chunk parts (vd_decode_pk split launches) were re-decoded on a device because their
 * speculative start had not converged at the boundary (all launches so far; decoded words are exact either
 * way).  VD_NO_SPLIT=1 in the environment (read at vd_create) disables splitting. */
int vd_split_redecodes(int device, uint64_t* count);
/* split launches (vd_decode_pk, single batches): waves on a device whose re-decode passes stopped at their cap
 * (2 P passes for P parts) with a part still differing.  The passes provably end within P (vd_kernel_pk.h
 * "Split"), so this stays 0; if it ever is not, the words of that launch may be wrong, and the blocking entry
 * points (vd_run, vd_run_llr, vd_run_stream) return VD_ERR_DEVICE after such a launch.  Callers of the
 * device-pointer entry points may check it after synchronising. */
int vd_split_cap_exits(int device, uint64_t* count);
/* LDS guard check (tests): enable != 0 makes every later launch of this decoder write guard words around
 * each wave's branch-metric table and survivor ring in LDS and count, at kernel exit, the guard words
 * found overwritten (an out-of-bounds LDS store); the count restarts at 0.  Off by default (one uniform
 * branch per wave when off).  VD_CHECK=1 in the environment turns it on at vd_create. */
int vd_set_guard_check(vd_decoder* dec, int enable);
/* guard words found overwritten since the check was enabled (synchronises the device) */
int vd_guard_violations(vd_decoder* dec, uint64_t* count);
const char* vd_last_error(void);
int vd_device_count(void);
/* the kernels an option combination can run, for profilers (static strings) */
const char* vd_kernel_name(int options);
/* the kernel and launch form this decoder takes for a decode of inputNum encoded values in nbatch batches
 * (vd_run_device: nbatch 1; vd_run_device_batch: nbatch) of packed (llr 0), float (llr 1) or punctured
 * float (llr 2: vd_decode_tg<PUN+...>) input, under the knobs read at vd_create (VD_NO_PK, VD_PK_SPLIT,
 * VD_NO_SPLIT); "-" when such a decode launches nothing (fewer than one output word; llr 2 on a HARD
 * decoder); llr 3: the frame launch of vd_run_device_frames (vd_decode_tg<FRM+...>), with inputNum =
 * maxFrameBits and nbatch = nframes; llr 4: the launch of vd_run_device_punct_frames (vd_decode_tg<FRM+PUN+...>),
 * inputNum and nbatch as for llr 3, "-" on a HARD decoder; llr 5: the launch of vd_run_device_tb_frames
 * (vd_decode_tg<FRM+TB+...>), inputNum and nbatch as for llr 3; llr 6: the launch of
 * vd_run_device_punct_tb_frames (vd_decode_tg<FRM+TB+PUN+...>), inputNum and nbatch as for llr 3, "-" on a HARD
 * decoder; llr 7 .. 10: the launch of vd_run_device_byte_frames that is the int8 twin of llr 3 .. 6 (the twin's name
 * with I8+ after FRM+, e.g. vd_decode_tg<FRM+I8+TB+PUN+...>), "-" where that call returns VD_ERR_OPTIONS (SOFT16 and
 * FP32 decoders; llr 8 and 10 on a HARD decoder); llr 11, 12: the launch of vd_run_device_mixed_frames for open or
 * terminated frames (vd_decode_tg<FRM+MIX+PUN+...>) and for tail-biting frames (vd_decode_tg<FRM+MIX+TB+PUN+...>), llr
 * 13, 14: those of vd_run_device_byte_mixed_frames (vd_decode_tg<FRM+I8+MIX+...>), inputNum and nbatch as for llr 3,
 * "-" where the call returns VD_ERR_OPTIONS (HARD decoders; llr 13 and 14 on SOFT16 and FP32 decoders); valid until
 * the thread's next call */
const char* vd_decoder_kernel_name(vd_decoder* dec, size_t inputNum, int nbatch, int llr);
/* build record: "<16 hex digits of the SHA-256 of the concatenated sources> <their paths, relative to the
 * package directory>"; the Python binding refuses a library whose sources have changed since (stale build) */
const char* vd_build_info(void);

#ifdef __cplusplus
}
#endif
#endif /* VD_CAPI_H */
