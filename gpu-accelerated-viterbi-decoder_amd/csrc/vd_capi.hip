// vd_capi.hip -- C-ABI runtime of the MI355X Viterbi decoder (see include/vd_capi.h).
//
// Replaces the reference's ViterbiCUDA<options> implementation (src/viterbi/viterbi.cu:10-139,210-262):
// decoder objects own reusable device buffers and a stream; vd_run is the blocking host-to-host
// call with kernel-only event timing like the reference; vd_run_device is the allocation-free,
// sync-free device path; vd_run_batches shards independent batches over the devices of a node.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <vector>
#include <chrono>

#include "../../include/vd_capi.h"
#include "vd_kernels.h"
#include "vd_kernel_tg.h"
#include "vd_kernel_pk.h"
#include "vd_pack.h"
#include "vd_mt.h"
#include "vd_mtjump.h"
#include "vd_plan.h"

using namespace vd;  // the option helpers and the plan (vd_plan.h)

namespace {

thread_local std::string g_err;

int fail(int code, const std::string& msg)
{
    g_err = msg;
    return code;
}

#define VD_HIP(expr)                                                                         \
    do {                                                                                     \
        hipError_t e_ = (expr);                                                              \
        if (e_ != hipSuccess)                                                                \
            return fail(e_ == hipErrorOutOfMemory ? VD_ERR_NOMEM : VD_ERR_DEVICE,            \
                        std::string(#expr) + ": " + hipGetErrorString(e_));                  \
    } while (0)

using launch_fn = void (*)(const void*, void*, vd::Geom, unsigned, hipStream_t);

// one launcher per kernel; vd_plan.h's launcher<Launch>() makes the table of them
struct Launch {
    using fn = launch_fn;
    template <int CH, int CORE, int OB>
    static void tg(const void* in, void* out, vd::Geom g, unsigned grid, hipStream_t s)
    {
        hipLaunchKernelGGL((vd::vd_decode_tg<CH, CORE, OB>), dim3(grid), dim3(64 * vd::kWaves), 0, s, in, out, g);
    }
    template <int CH, int CORE, int OB, bool SPL>
    static void pk(const void* in, void* out, vd::Geom g, unsigned grid, hipStream_t s)
    {
        hipLaunchKernelGGL((vd::vd_decode_pk<CH, CORE, OB, SPL>), dim3(grid), dim3(64 * vd::kWaves), 0, s, in, out, g);
    }
};

}  // namespace

// Device address of page-locked, device-mapped host memory (vd_host_alloc / hipHostMalloc /
// hipHostRegister), or null for pageable memory.  Kernels then read inputs from / write decoded words
// to such buffers directly over PCIe (zero-copy), with no staging copies at all.
static void* mapped_host(const void* p)
{
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError();
        return nullptr;
    }
    return a.type == hipMemoryTypeHost ? a.devicePointer : nullptr;
}

struct DeviceState;
struct vd_decoder {
    int options = 0;
    int device = 0;
    void* in_d = nullptr;
    void* out_d = nullptr;
    void* llr_d = nullptr;  // vd_run_llr's float input buffer
    size_t cap_in = 0, cap_out = 0, cap_llr = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    // vd_run_stream: a second buffer set and the copy-in / copy-out streams of the 3-stage pipeline
    void* in2_d = nullptr;
    void* out2_d = nullptr;
    size_t cap2_in = 0, cap2_out = 0;
    hipStream_t s_in = nullptr, s_out = nullptr;
    DeviceState* ds = nullptr;  // the device's board / segment tables (looked up once, vd_create)
    Knobs knobs;                // VD_NO_SPLIT / VD_SPLIT / VD_NO_PK / VD_PK_SPLIT / VD_PK_TAIL as read at vd_create
    uint32_t* check = nullptr;  // LDS guard violation counter (vd_set_guard_check), null = off
    uint32_t partBits = 0;      // frame launches decode frames in parts of this many stages (vd_set_frame_part_bits), 0 = whole
    // mixed frames (vd_set_frame_patterns): the pattern table, its host copy and its device records (allocated by the
    // first setter call, the only allocation of the mixed launches; the kernels read it when they run)
    MixRecord mixTab[kMixMaxPatterns];
    int mixN = 0;
    void* mixTab_d = nullptr;
};

// a device buffer of at least need bytes (contents not kept)
static int grow(void*& p, size_t& cap, size_t need)
{
    if (need <= cap) return VD_OK;
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
    VD_HIP(hipMalloc(&p, need));
    cap = need;
    return VD_OK;
}
static int ensure_capacity(vd_decoder* d, size_t inBytes, size_t outBytes)
{
    int rc = grow(d->in_d, d->cap_in, inBytes);
    return rc != VD_OK ? rc : grow(d->out_d, d->cap_out, outBytes);
}

// Per-device state shared by every decoder and stream on a device, allocated once per device:
//  * the progress board of the decode kernels' fairness controller (vd_kernels.h Fair, Geom::fair),
//    every word kFairEmpty at rest (the kernels free their slots); concurrent launches sharing it only
//    perturb issue priorities;
//  * the segment tables of segment launches (read only; vd_kernel_tg.h "segment launches");
//  * the re-decode counter of segment and split launches (vd_split_redecodes) and the split launches'
//    pass-cap counter (vd_split_cap_exits: waves that stopped re-decoding at the cap with a part still
//    differing; never expected, and vd_run / vd_run_stream fail when it is non-zero).
// Segment launches keep their boundary vectors in LDS, so launches on any number of streams share no
// scratch.  A decoder looks the state up once (vd_create), not per launch.
struct DeviceState {
    uint32_t* board = nullptr;
    int nsimd = 0;
    uint32_t* stats = nullptr;
    uint32_t* seg[3] = {};  // by SegMode: first chunk of each workgroup, then the chunk count; null = no table
    unsigned segWG[3] = {};  // ... and its workgroups
};
static DeviceState* device_state(int device)
{
    static std::mutex mu;
    static std::vector<DeviceState*> st;
    std::lock_guard<std::mutex> lk(mu);
    if ((int)st.size() <= device) st.resize(device + 1, nullptr);
    if (!st[device]) {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || cus <= 0)
            return nullptr;
        DeviceState* x = new DeviceState;
        x->nsimd = 4 * cus;
        bool ok = hipMalloc(&x->board, vd::kFairBoardWords * 4) == hipSuccess &&
                  hipMemset(x->board, 0xFF, vd::kFairBoardWords * 4) == hipSuccess &&
                  hipMalloc(&x->stats, 8) == hipSuccess && hipMemset(x->stats, 0, 8) == hipSuccess;
        for (int th = 0; th < 3 && ok; th++) {
            const std::vector<uint32_t> t = vd::seg_table(x->nsimd, th);
            if (t.empty()) continue;
            ok = hipMalloc(&x->seg[th], t.size() * 4) == hipSuccess &&
                 hipMemcpy(x->seg[th], t.data(), t.size() * 4, hipMemcpyHostToDevice) == hipSuccess;
            x->segWG[th] = (unsigned)(t.size() - 1);
        }
        if (!ok || hipDeviceSynchronize() != hipSuccess) {
            delete x;
            return nullptr;
        }
        st[device] = x;
    }
    return st[device];
}
// Which kernel, launch form and grid a decode takes: vd_plan.h, for this decoder's knobs and device
// (punct: a punctured decode, planned on vd_decode_tg's forms only)
static LaunchPlan plan_of(const vd_decoder* d, size_t inputNum, uint32_t nbatch, bool llr, bool punct = false)
{
    return plan_launch(d->options, inputNum, nbatch, llr, punct ? punct_knobs(d->knobs) : d->knobs, d->ds->nsimd,
                       d->ds->segWG);
}

// llr: in_d holds inputNum float channel values, quantised in the kernel (scale = packer scale).
// nbatch > 1: batch b at in_d + b * inStride, out_d + b * outStride, all in one launch (never split).
// pun: in_d holds the kept float values of a punctured stream (llr set; vd_punct.h), inputNum the mother-code values.
// *form: the launch form taken (the blocking entry points' split-cap check wants it)
static int launch_decode(const vd_decoder* d, const void* in_d, void* out_d, size_t inputNum, hipStream_t s,
                         Form* form = nullptr, bool llr = false, float scale = 1.0f, uint32_t nbatch = 1,
                         uint64_t inStride = 0, uint64_t outStride = 0, const Punct* pun = nullptr)
{
    const int options = d->options;
    const LaunchPlan p = plan_of(d, inputNum, nbatch, llr, pun != nullptr);
    if (form) *form = p.form;
    launch_fn f = pun ? launcher_punct<Launch>(ch_of(options), met_of(options), out_of(options) == 1)
                      : launcher<Launch>(p.form, llr, ch_of(options), met_of(options), out_of(options) == 1);
    if (!f) return fail(VD_ERR_OPTIONS, "invalid options");
    if (!p.launches) return VD_OK;
    // the launch goes to the stream's device (the null stream: the current device); the board and the
    // guard counter belong to the decoder's device
    int sdev = -1;
    if (s) VD_HIP(hipStreamGetDevice(s, &sdev));
    else VD_HIP(hipGetDevice(&sdev));
    if (sdev != d->device)
        return fail(VD_ERR_ARG, "stream on device " + std::to_string(sdev) + ", decoder on device " +
                                    std::to_string(d->device));
    vd::Geom g;
    g.packNum = p.packNum;
    g.availStages = llr ? inputNum / 2 : avail_stages(options, inputNum);
    g.nchunks = vd::kChunks;
    g.scale = scale;
    g.fair = d->ds->board;
    g.check = d->check;
    g.nbatch = nbatch;
    g.inStride = inStride;
    g.outStride = outStride;
    g.tailWG = p.tailWG;
    if (pun) {
        g.pun = *pun;
        g.punBytes = punct_len(*pun, inputNum) * sizeof(float);
    }
    if (p.seg != kSegNone) g.seg = d->ds->seg[p.seg];
    if (p.stats) g.stats = d->ds->stats;
    f(in_d, out_d, g, p.grid, s);
    VD_HIP(hipGetLastError());
    return VD_OK;
}

extern "C" {

int vd_options_valid(int options) { return valid(options) ? 1 : 0; }
size_t vd_input_size(int options, size_t n) { return input_size(options, n); }
size_t vd_message_len(int options, size_t n) { return message_len(options, n); }
size_t vd_output_size(int options, size_t n) { return message_len(options, n) / 8; }
int vd_num_chunks(void) { return vd::kChunks; }

int vd_split_redecodes(int device, uint64_t* count)
{
    if (!count) return fail(VD_ERR_ARG, "null argument");
    DeviceState* x = device_state(device);
    if (!x) return fail(VD_ERR_DEVICE, "per-device decode state unavailable");
    uint32_t v = 0;
    VD_HIP(hipMemcpy(&v, x->stats, 4, hipMemcpyDeviceToHost));
    *count = v;
    return VD_OK;
}
int vd_split_cap_exits(int device, uint64_t* count)
{
    if (!count) return fail(VD_ERR_ARG, "null argument");
    DeviceState* x = device_state(device);
    if (!x) return fail(VD_ERR_DEVICE, "per-device decode state unavailable");
    uint32_t v = 0;
    VD_HIP(hipMemcpy(&v, x->stats + 1, 4, hipMemcpyDeviceToHost));
    *count = v;
    return VD_OK;
}
const char* vd_last_error(void) { return g_err.c_str(); }
const char* vd_kernel_name(int options)
{
    static const std::vector<std::string> names = [] {
        std::vector<std::string> v;
        for (int o = 0; o < 0x100; o++) v.push_back(option_kernels(o));
        return v;
    }();
    return valid(options) ? names[options & 0xFF].c_str() : "-";
}

const char* vd_decoder_kernel_name(vd_decoder* d, size_t inputNum, int nbatch, int llr)
{
    static thread_local std::string name;
    if (!d || nbatch < 1) return "-";
    if (llr == 2 && ch_of(d->options) == HARD) return "-";  // no punctured HARD kernels
    if (llr >= 3 && llr <= 14) {  // a frame launch of the code's family (frame_family_of_input): inputNum = maxFrameBits, nbatch = nframes
        // "-" where the family has no kernel for the decoder's format (launcher_frames: no punctured HARD frames, int8
        // on HARD, SOFT4 and SOFT8 only), which is where the entry point refuses by format
        const int o = d->options;
        if (!launcher_frames<Launch>(frame_family_of_input(llr), ch_of(o), met_of(o), out_of(o) == 1)) return "-";
        if (inputNum < 1 || inputNum > kFrmMaxBits) return "-";
        if (frame_parts_error(inputNum, nbatch, d->partBits)) return "-";  // (more workgroups than a launch can have)
        name = plan_name(plan_frames(d->options, (uint64_t)nbatch, frame_parts((uint32_t)inputNum, frame_part_words(d->partBits))),
                         d->options, llr);
        return name.c_str();
    }
    name = plan_name(plan_of(d, inputNum, (uint32_t)nbatch, llr != 0, llr == 2), d->options, llr == 2 ? 2 : llr != 0);
    return name.c_str();
}

int vd_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int vd_create(int options, size_t preallocInputNum, int device, vd_decoder** out)
{
    if (!out) return fail(VD_ERR_ARG, "null output handle");
    *out = nullptr;
    if (!valid(options)) return fail(VD_ERR_OPTIONS, "options disabled by OptionsValid");
    int ndev = 0;
    VD_HIP(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) return fail(VD_ERR_ARG, "device index out of range");
    VD_HIP(hipSetDevice(device));
    vd_decoder* d = new vd_decoder();
    d->options = options;
    d->device = device;
    d->ds = device_state(device);
    if (!d->ds) {
        delete d;
        return fail(VD_ERR_NOMEM, "per-device decode state allocation failed");
    }
    d->knobs = knobs_from_env();
    const char* chk = std::getenv("VD_CHECK");
    if (chk && chk[0] == '1') {
        int rc = vd_set_guard_check(d, 1);
        if (rc != VD_OK) { vd_destroy(d); return rc; }
    }
    if (hipStreamCreateWithFlags(&d->stream, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreate(&d->ev0) != hipSuccess || hipEventCreate(&d->ev1) != hipSuccess) {
        vd_destroy(d);
        return fail(VD_ERR_DEVICE, "stream/event creation failed");
    }
    if (preallocInputNum) {
        int rc = ensure_capacity(d, input_size(options, preallocInputNum),
                                 message_len(options, preallocInputNum) / 8 + 16);
        if (rc != VD_OK) { vd_destroy(d); return rc; }
    }
    *out = d;
    return VD_OK;
}

int vd_destroy(vd_decoder* d)
{
    if (!d) return VD_OK;
    (void)hipSetDevice(d->device);
    if (d->in_d) (void)hipFree(d->in_d);
    if (d->out_d) (void)hipFree(d->out_d);
    if (d->llr_d) (void)hipFree(d->llr_d);
    if (d->in2_d) (void)hipFree(d->in2_d);
    if (d->out2_d) (void)hipFree(d->out2_d);
    if (d->s_in) (void)hipStreamDestroy(d->s_in);
    if (d->s_out) (void)hipStreamDestroy(d->s_out);
    if (d->ev0) (void)hipEventDestroy(d->ev0);
    if (d->ev1) (void)hipEventDestroy(d->ev1);
    if (d->stream) (void)hipStreamDestroy(d->stream);
    if (d->check) (void)hipFree(d->check);
    if (d->mixTab_d) (void)hipFree(d->mixTab_d);
    delete d;
    return VD_OK;
}

// vd_run / vd_run_stream (blocking): a single-batch split launch whose re-decode passes hit their cap with a part
// still differing (vd_kernel_pk.h "Split"; never expected) fails the call instead of returning wrong words
static int check_split_cap(const vd_decoder* d, Form form)
{
    if (form != Form::PkSplit) return VD_OK;
    uint32_t v = 0;
    VD_HIP(hipMemcpy(&v, d->ds->stats + 1, 4, hipMemcpyDeviceToHost));
    if (v)
        return fail(VD_ERR_DEVICE, "split launch reached its re-decode pass cap with a part still differing (" +
                                       std::to_string(v) + " waves on this device so far): decoded words may be wrong");
    return VD_OK;
}

// the blocking decode through the decoder's device buffers: in_h to in_d, the launch between the timing
// events, out_d to out_h, kernel-only time
static int run_staged(vd_decoder* d, void* in_d, const void* in_h, size_t inB, void* out_h, size_t outB, size_t inputNum,
                      bool llr, float scale, float* kernel_ms, const Punct* pun = nullptr)
{
    Form form = Form::Tg;
    VD_HIP(hipMemcpyAsync(in_d, in_h, inB, hipMemcpyHostToDevice, d->stream));
    VD_HIP(hipEventRecord(d->ev0, d->stream));
    int rc = launch_decode(d, in_d, d->out_d, inputNum, d->stream, &form, llr, scale, 1, 0, 0, pun);
    if (rc != VD_OK) return rc;
    VD_HIP(hipEventRecord(d->ev1, d->stream));
    VD_HIP(hipMemcpyAsync(out_h, d->out_d, outB, hipMemcpyDeviceToHost, d->stream));
    VD_HIP(hipStreamSynchronize(d->stream));
    if (kernel_ms) VD_HIP(hipEventElapsedTime(kernel_ms, d->ev0, d->ev1));
    return check_split_cap(d, form);
}

int vd_run(vd_decoder* d, const void* input_h, void* output_h, size_t inputNum, float* kernel_ms)
{
    if (!d || !input_h || !output_h) return fail(VD_ERR_ARG, "null argument");
    const size_t inB = input_size(d->options, inputNum), outB = message_len(d->options, inputNum) / 8;
    if (message_len(d->options, inputNum) == 0) return fail(VD_ERR_ARG, "inputNum too small");
    VD_HIP(hipSetDevice(d->device));
    void* zin = mapped_host(input_h);
    void* zout = zin ? mapped_host(output_h) : nullptr;
    if (zin && zout) {  // pinned host buffers: zero-copy decode (kernel_ms then includes the PCIe traffic)
        Form form = Form::Tg;
        VD_HIP(hipEventRecord(d->ev0, d->stream));
        int rc = launch_decode(d, zin, zout, inputNum, d->stream, &form);
        if (rc != VD_OK) return rc;
        VD_HIP(hipEventRecord(d->ev1, d->stream));
        VD_HIP(hipStreamSynchronize(d->stream));
        if (kernel_ms) VD_HIP(hipEventElapsedTime(kernel_ms, d->ev0, d->ev1));
        return check_split_cap(d, form);
    }
    int rc = ensure_capacity(d, inB, outB + 16);
    if (rc != VD_OK) return rc;
    return run_staged(d, d->in_d, input_h, inB, output_h, outB, inputNum, false, 1.0f, kernel_ms);
}

int vd_set_guard_check(vd_decoder* d, int enable)
{
    if (!d) return fail(VD_ERR_ARG, "null argument");
    VD_HIP(hipSetDevice(d->device));
    if (!enable) {
        if (d->check) VD_HIP(hipDeviceSynchronize());
        if (d->check) (void)hipFree(d->check);
        d->check = nullptr;
        return VD_OK;
    }
    // kernels still in flight on the decoder's or a caller's (non-blocking) stream may add to the counter:
    // let them finish before the reset
    if (d->check) VD_HIP(hipDeviceSynchronize());
    else VD_HIP(hipMalloc(&d->check, 4));
    VD_HIP(hipMemset(d->check, 0, 4));
    VD_HIP(hipDeviceSynchronize());
    return VD_OK;
}

int vd_guard_violations(vd_decoder* d, uint64_t* count)
{
    if (!d || !count) return fail(VD_ERR_ARG, "null argument");
    if (!d->check) return fail(VD_ERR_ARG, "guard check not enabled (vd_set_guard_check)");
    VD_HIP(hipSetDevice(d->device));
    VD_HIP(hipDeviceSynchronize());
    uint32_t v = 0;
    VD_HIP(hipMemcpy(&v, d->check, 4, hipMemcpyDeviceToHost));
    *count = v;
    return VD_OK;
}

// vd_run_device*: the argument checks, then one launch (the single-batch entry points: nbatch 1, strides 0).
// in_stride: any multiple of its alignment (0 = every batch decodes the same input); inputs are only read,
// so overlapping windows (e.g. sliding) are valid
static int run_device(vd_decoder* d, const void* in_d, void* out_d, size_t inputNum, void* stream, bool llr, float scale,
                      int nbatch, size_t in_stride, size_t output_stride, const Punct* pun = nullptr)
{
    if (!d || !in_d || !out_d) return fail(VD_ERR_ARG, "null argument");
    if (nbatch < 1) return fail(VD_ERR_ARG, "nbatch must be >= 1");
    if (message_len(d->options, inputNum) == 0) return fail(VD_ERR_ARG, "inputNum too small");
    if (nbatch > 1 && output_stride < message_len(d->options, inputNum) / 8)
        return fail(VD_ERR_ARG, "output_stride smaller than the output size: batches would overlap");
    if ((uint64_t)vd::kChunks * (uint64_t)nbatch > 0xFFFFFFFFull) return fail(VD_ERR_ARG, "nbatch too large");
    // punctured input is read by single-dword loads: 4-byte alignment, of the pointer too
    if (pun && (((uintptr_t)in_d | in_stride | output_stride) & 3))
        return fail(VD_ERR_ARG, "rx_d, rx_stride and output_stride must be multiples of 4 bytes");
    if (llr && !pun && ((in_stride & 15) || (output_stride & 3))) return fail(VD_ERR_ARG, "llr_stride % 16 or output_stride % 4 != 0");
    if (!llr && ((in_stride | output_stride) & 3)) return fail(VD_ERR_ARG, "strides must be multiples of 4 bytes");
    return launch_decode(d, in_d, out_d, inputNum, (hipStream_t)stream, nullptr, llr, scale, (uint32_t)nbatch, in_stride,
                         output_stride, pun);
}

int vd_run_device(vd_decoder* d, const void* input_d, void* output_d, size_t inputNum, void* stream)
{
    return run_device(d, input_d, output_d, inputNum, stream, false, 1.0f, 1, 0, 0);
}

int vd_run_device_batch(vd_decoder* d, const void* input_d, size_t input_stride, void* output_d, size_t output_stride,
                        size_t inputNum, int nbatch, void* stream)
{
    return run_device(d, input_d, output_d, inputNum, stream, false, 1.0f, nbatch, input_stride, output_stride);
}

static int launch_pack(int options, const float* llr_d, size_t inputNum, float scale, void* packed_d, hipStream_t s)
{
    if (((uintptr_t)llr_d & 15) != 0) return fail(VD_ERR_ARG, "llr buffer must be 16-byte aligned");
    const int ch = ch_of(options);
    const int per = ch == 0 ? 32 : ch == 1 ? 8 : ch == 2 ? 4 : ch == 3 ? 2 : 1;
    const uint64_t nw = (inputNum + per - 1) / per;
    if (nw == 0) return VD_OK;
    static void (*const kernels[5])(const float*, uint64_t, float, void*) = {
        vd::pack_llr<0>, vd::pack_llr<1>, vd::pack_llr<2>, vd::pack_llr<3>, vd::pack_llr<4>};
    if (ch < 5)
        hipLaunchKernelGGL(kernels[ch], dim3((unsigned)((nw + 255) / 256)), dim3(256), 0, s, llr_d, (uint64_t)inputNum, scale,
                           packed_d);
    VD_HIP(hipGetLastError());
    return VD_OK;
}

int vd_pack_device(int options, const float* llr_d, size_t inputNum, float scale, void* packed_d, void* stream)
{
    if (!valid(options)) return fail(VD_ERR_OPTIONS, "options disabled by OptionsValid");
    if (!llr_d || !packed_d) return fail(VD_ERR_ARG, "null argument");
    return launch_pack(options, llr_d, inputNum, scale, packed_d, (hipStream_t)stream);
}

int vd_run_device_llr(vd_decoder* d, const float* llr_d, void* output_d, size_t inputNum, float scale, void* stream)
{
    return run_device(d, llr_d, output_d, inputNum, stream, true, scale, 1, 0, 0);
}

int vd_run_device_llr_batch(vd_decoder* d, const float* llr_d, size_t llr_stride, void* output_d, size_t output_stride,
                            size_t inputNum, float scale, int nbatch, void* stream)
{
    return run_device(d, llr_d, output_d, inputNum, stream, true, scale, nbatch, llr_stride, output_stride);
}

int vd_run_llr(vd_decoder* d, const float* llr_h, void* output_h, size_t inputNum, float scale, float* kernel_ms)
{
    if (!d || !llr_h || !output_h) return fail(VD_ERR_ARG, "null argument");
    if (message_len(d->options, inputNum) == 0) return fail(VD_ERR_ARG, "inputNum too small");
    const size_t inB = inputNum * sizeof(float), outB = message_len(d->options, inputNum) / 8;
    VD_HIP(hipSetDevice(d->device));
    int rc = grow(d->llr_d, d->cap_llr, inB);
    if (rc == VD_OK) rc = grow(d->out_d, d->cap_out, outB + 16);
    if (rc != VD_OK) return rc;
    return run_staged(d, d->llr_d, llr_h, inB, output_h, outB, inputNum, true, scale, kernel_ms);
}

// ---- punctured streams (vd_punct.h; vd_decode_tg<PUN+...>) ----
// the pattern and the decoder of a punctured decode: VD_ERR_ARG / VD_ERR_OPTIONS, or *pn filled in
static int punct_args(const vd_decoder* d, int period, uint32_t keep0, uint32_t keep1, size_t inputNum, Punct* pn)
{
    if (!d) return fail(VD_ERR_ARG, "null argument");
    if (!punct_valid(period, keep0, keep1))
        return fail(VD_ERR_ARG, "invalid puncture pattern: 1 <= period <= 16, keep0 and keep1 are period-bit masks, "
                                "at least one bit set");
    if (ch_of(d->options) == HARD)
        return fail(VD_ERR_OPTIONS, "punctured input on a HARD decoder: a punctured value must decode as code 0 = value 0, "
                                    "and HARD's v > 0 ? 1 : 0 turns it into a hard 0; use SOFT4, SOFT8, SOFT16 or FP32");
    if (inputNum / 2 > kPunctMaxStages) return fail(VD_ERR_ARG, "inputNum too large: punctured decodes index stages in 32 bits");
    *pn = punct_make(period, keep0, keep1);
    return VD_OK;
}

size_t vd_punctured_len(int period, uint32_t keep0, uint32_t keep1, size_t inputNum)
{
    return punct_valid(period, keep0, keep1) ? (size_t)punct_len(punct_make(period, keep0, keep1), inputNum) : 0;
}

int vd_run_device_punct_batch(vd_decoder* d, const float* rx_d, size_t rx_stride, void* output_d, size_t output_stride,
                              size_t inputNum, float scale, int period, uint32_t keep0, uint32_t keep1, int nbatch,
                              void* stream)
{
    Punct pn;
    int rc = punct_args(d, period, keep0, keep1, inputNum, &pn);
    if (rc != VD_OK) return rc;
    return run_device(d, rx_d, output_d, inputNum, stream, true, scale, nbatch, rx_stride, output_stride, &pn);
}

int vd_run_device_punct(vd_decoder* d, const float* rx_d, void* output_d, size_t inputNum, float scale, int period,
                        uint32_t keep0, uint32_t keep1, void* stream)
{
    return vd_run_device_punct_batch(d, rx_d, 0, output_d, 0, inputNum, scale, period, keep0, keep1, 1, stream);
}

int vd_run_punct(vd_decoder* d, const float* rx_h, void* output_h, size_t inputNum, float scale, int period, uint32_t keep0,
                 uint32_t keep1, float* kernel_ms)
{
    Punct pn;
    int rc = punct_args(d, period, keep0, keep1, inputNum, &pn);
    if (rc != VD_OK) return rc;
    if (!rx_h || !output_h) return fail(VD_ERR_ARG, "null argument");
    if (message_len(d->options, inputNum) == 0) return fail(VD_ERR_ARG, "inputNum too small");
    const size_t inB = (size_t)punct_len(pn, inputNum) * sizeof(float), outB = message_len(d->options, inputNum) / 8;
    VD_HIP(hipSetDevice(d->device));
    rc = grow(d->llr_d, d->cap_llr, inB);
    if (rc == VD_OK) rc = grow(d->out_d, d->cap_out, outB + 16);
    if (rc != VD_OK) return rc;
    return run_staged(d, d->llr_d, rx_h, inB, output_h, outB, inputNum, true, scale, kernel_ms, &pn);
}

// ---- independent frames (vd_frames.h; vd_decode_tg<FRM+...>, one frame per wave) ----
size_t vd_frame_output_size(int options, size_t frameBits)
{
    (void)options;  // whole 32-bit words for O_B32 and O_B16 (two 16-bit words each) alike
    return 4 * ((frameBits + 31) / 32);
}

// frames in parts (vd_frames.h "frames in parts"): the part length every frame entry point of the decoder reads
int vd_set_frame_part_bits(vd_decoder* d, size_t partBits)
{
    if (!d) return fail(VD_ERR_ARG, "null argument");
    if (!frame_part_bits_valid(partBits)) return fail(VD_ERR_ARG, "partBits must be 0 or a multiple of 96 in [96, 2^20]");
    d->partBits = (uint32_t)partBits;
    return VD_OK;
}
int vd_frame_part_bits(vd_decoder* d, size_t* partBits)
{
    if (!d || !partBits) return fail(VD_ERR_ARG, "null argument");
    *partBits = d->partBits;
    return VD_OK;
}

static_assert(kFrameErrOptions == VD_ERR_OPTIONS && kFrameErrArg == VD_ERR_ARG && kByteFramesOpen == VD_FRAMES_OPEN &&
                  kByteFramesTerminated == VD_FRAMES_TERMINATED && kByteFramesTailbiting == VD_FRAMES_TAILBITING,
              "vd_frames.h mirrors these");

// One call of a frame entry point: what the check goes by (vd_frames.h FrameArgs, the family first) and the buffers --
// the device ones of a launch, or the host ones of a blocking variant, laid out alike.
struct FrameCall {
    FrameArgs a;
    const void* in;            // the values: floats, or int8 (a.fam.i8)
    void* out;
    const uint32_t* bits;      // the frames' lengths, or null: every frame has maxFrameBits stages
    const uint8_t* rate;       // mixed launches: the frames' pattern indices, or null: pattern 0
    const uint64_t* off;       // ... and their offsets in values, or null: frames at f strides
};
// the record of the family's entry point: plain frames and tail-biting frames carry pattern (1, 1, 1), a mixed
// launch sets its two arrays itself
static FrameCall frame_call(FrameFamily fam, const void* in, size_t stride, void* out, size_t outStride, const uint32_t* bits,
                            size_t maxFrameBits, int nframes, int kind, float scale, int period = 1, uint32_t keep0 = 1,
                            uint32_t keep1 = 1)
{
    FrameCall c = {};
    c.a.fam = fam;
    c.a.stride = stride;
    c.a.outStride = outStride;
    c.a.maxFrameBits = maxFrameBits;
    c.a.nframes = nframes;
    c.a.kind = kind;
    c.a.scale = scale;
    c.a.period = period;
    c.a.keep0 = keep0;
    c.a.keep1 = keep1;
    c.in = in;
    c.out = out;
    c.bits = bits;
    return c;
}
static FrameFamily byte_family(int kind, int period, uint32_t keep0, uint32_t keep1)
{
    return {!byte_frames_unpunctured(period, keep0, keep1), kind == kByteFramesTailbiting, true, false};
}

// The checks of every frame entry point (VD_ERR_ARG / VD_ERR_OPTIONS): a null pointer, then frame_args_error on the
// call and the decoder's format, part length and pattern table.  The part length is read here, on the host, once per
// call: a captured graph keeps the value it was captured with.  device: c.in is a device address and its alignment
// counts (the blocking variants stage into the decoder's own buffers).
static int check_frames(const vd_decoder* d, FrameCall& c, bool device)
{
    if (!d || !c.in || !c.out) return fail(VD_ERR_ARG, "null argument");
    c.a.addr = device ? (uint64_t)(uintptr_t)c.in : 0;
    c.a.offsets = c.off != nullptr;
    c.a.options = d->options;
    c.a.partBits = d->partBits;
    c.a.table = d->mixTab;
    c.a.tableN = d->mixN;
    int code = VD_OK;
    if (const char* why = frame_args_error(c.a, &code)) return fail(code, why);
    return VD_OK;
}

// the one launch of a checked call on device buffers
static int launch_frames_checked(vd_decoder* d, const FrameCall& c, hipStream_t s)
{
    const int options = d->options;
    const FrameFamily fam = c.a.fam;
    const uint32_t partBits = (uint32_t)c.a.partBits;
    const LaunchPlan p = plan_frames(options, (uint64_t)c.a.nframes,
                                     frame_parts((uint32_t)c.a.maxFrameBits, frame_part_words(partBits)));
    launch_fn f = launcher_frames<Launch>(fam, ch_of(options), met_of(options), out_of(options) == 1);
    if (!f || !p.launches) return fail(VD_ERR_OPTIONS, "invalid options");
    int sdev = -1;
    if (s) VD_HIP(hipStreamGetDevice(s, &sdev));
    else VD_HIP(hipGetDevice(&sdev));
    if (sdev != d->device)
        return fail(VD_ERR_ARG, "stream on device " + std::to_string(sdev) + ", decoder on device " +
                                    std::to_string(d->device));
    vd::Geom g;
    g.packNum = 0;
    g.availStages = 0;
    g.nchunks = 1;
    g.scale = c.a.scale;
    g.fair = d->ds->board;
    g.check = d->check;
    g.nbatch = (uint32_t)c.a.nframes;
    g.inStride = c.a.stride;
    g.outStride = c.a.outStride;
    g.frmBits = c.bits;
    g.frmMax = (uint32_t)c.a.maxFrameBits;
    g.frmTerm = c.a.kind == kByteFramesTerminated ? 1u : 0u;
    if (!fam.tb) frame_pad(c.a.scale, &g.frmPad);  // (checked)
    if (fam.mix) {  // the table as a device pointer: read by the kernel when it runs
        g.mixPat = (const uint32_t*)d->mixTab_d;
        g.mixN = (uint32_t)d->mixN;
        g.mixRate = c.rate;
        g.mixOff = c.off;
    } else if (fam.pun) {
        g.pun = punct_make(c.a.period, c.a.keep0, c.a.keep1);
    }
    if (p.parts > 1) {  // (one part: the grid and the arguments of a whole-frame launch)
        g.frmPartW = frame_part_words(partBits);
        g.frmPartG = frame_part_groups(p.parts);
    }
    f(c.in, c.out, g, p.grid, s);
    VD_HIP(hipGetLastError());
    return VD_OK;
}

// The blocking decode of a checked call on host buffers laid out like the device ones: nframes frames at the call's
// strides, the last frame's part ending with the values of a maxFrameBits frame (frame_value_bytes) and its output
// words; with offsets, total values in all.  The staging buffers are the decoder's; the offsets (8 bytes each), the
// lengths (4) and the rate indices (1) ride behind the values from the next 16-byte boundary.  Kernel-only time.
static int run_frames_staged(vd_decoder* d, FrameCall c, size_t total, float* kernel_ms)
{
    const size_t n = (size_t)c.a.nframes;
    const size_t inB = c.off ? total * (c.a.fam.i8 ? 1 : 4)
                             : (n - 1) * c.a.stride + frame_value_bytes(c.a, (uint32_t)c.a.maxFrameBits);
    const size_t outB = (n - 1) * c.a.outStride + vd_frame_output_size(d->options, c.a.maxFrameBits);
    const size_t offOff = (inB + 15) & ~(size_t)15, offB = c.off ? n * 8 : 0;
    const size_t lenOff = offOff + offB, lenB = c.bits ? n * 4 : 0;
    const size_t rateOff = lenOff + lenB, rateB = c.rate ? n : 0;
    VD_HIP(hipSetDevice(d->device));
    int rc = grow(d->llr_d, d->cap_llr, rateOff + rateB + 16);  // (+ 16: a buffer even when no frame holds a kept value)
    if (rc == VD_OK) rc = grow(d->out_d, d->cap_out, outB + 16);
    if (rc != VD_OK) return rc;
    char* const in_d = (char*)d->llr_d;
    void* const out_h = c.out;
    if (inB) VD_HIP(hipMemcpyAsync(in_d, c.in, inB, hipMemcpyHostToDevice, d->stream));
    if (c.off) VD_HIP(hipMemcpyAsync(in_d + offOff, c.off, offB, hipMemcpyHostToDevice, d->stream));
    if (c.bits) VD_HIP(hipMemcpyAsync(in_d + lenOff, c.bits, lenB, hipMemcpyHostToDevice, d->stream));
    if (c.rate) VD_HIP(hipMemcpyAsync(in_d + rateOff, c.rate, rateB, hipMemcpyHostToDevice, d->stream));
    // the words no frame writes (between the frames, of short, empty and out-of-table frames) keep the caller's values
    VD_HIP(hipMemcpyAsync(d->out_d, out_h, outB, hipMemcpyHostToDevice, d->stream));
    c.in = in_d;
    c.out = d->out_d;
    if (c.off) c.off = (const uint64_t*)(in_d + offOff);
    if (c.bits) c.bits = (const uint32_t*)(in_d + lenOff);
    if (c.rate) c.rate = (const uint8_t*)(in_d + rateOff);
    VD_HIP(hipEventRecord(d->ev0, d->stream));
    rc = launch_frames_checked(d, c, d->stream);
    if (rc != VD_OK) return rc;
    VD_HIP(hipEventRecord(d->ev1, d->stream));
    VD_HIP(hipMemcpyAsync(out_h, d->out_d, outB, hipMemcpyDeviceToHost, d->stream));
    VD_HIP(hipStreamSynchronize(d->stream));
    if (kernel_ms) VD_HIP(hipEventElapsedTime(kernel_ms, d->ev0, d->ev1));
    return VD_OK;
}

// the two ways an entry point ends: check and launch, check and run
static int launch_frames(vd_decoder* d, FrameCall c, void* stream)
{
    const int rc = check_frames(d, c, true);
    return rc != VD_OK ? rc : launch_frames_checked(d, c, (hipStream_t)stream);
}
static int run_frames(vd_decoder* d, FrameCall c, float* kernel_ms)
{
    const int rc = check_frames(d, c, false);
    return rc != VD_OK ? rc : run_frames_staged(d, c, 0, kernel_ms);
}

int vd_run_device_frames(vd_decoder* d, const float* llr_d, size_t llr_stride, void* output_d, size_t output_stride,
                         const uint32_t* frame_bits_d, size_t maxFrameBits, int nframes, int terminated, float scale,
                         void* stream)
{
    return launch_frames(d, frame_call({false, false, false, false}, llr_d, llr_stride, output_d, output_stride, frame_bits_d,
                                       maxFrameBits, nframes, terminated ? 1 : 0, scale), stream);
}
int vd_run_frames(vd_decoder* d, const float* llr_h, size_t llr_stride, void* output_h, size_t output_stride,
                  const uint32_t* frame_bits_h, size_t maxFrameBits, int nframes, int terminated, float scale,
                  float* kernel_ms)
{
    return run_frames(d, frame_call({false, false, false, false}, llr_h, llr_stride, output_h, output_stride, frame_bits_h,
                                    maxFrameBits, nframes, terminated ? 1 : 0, scale), kernel_ms);
}

// ---- punctured frames (vd_frames.h "punctured frames"; vd_decode_tg<FRM+PUN+...>) ----
int vd_run_device_punct_frames(vd_decoder* d, const float* rx_d, size_t rx_stride, void* output_d, size_t output_stride,
                               const uint32_t* frame_bits_d, size_t maxFrameBits, int nframes, int terminated, float scale,
                               int period, uint32_t keep0, uint32_t keep1, void* stream)
{
    return launch_frames(d, frame_call({true, false, false, false}, rx_d, rx_stride, output_d, output_stride, frame_bits_d,
                                       maxFrameBits, nframes, terminated ? 1 : 0, scale, period, keep0, keep1), stream);
}
int vd_run_punct_frames(vd_decoder* d, const float* rx_h, size_t rx_stride, void* output_h, size_t output_stride,
                        const uint32_t* frame_bits_h, size_t maxFrameBits, int nframes, int terminated, float scale, int period,
                        uint32_t keep0, uint32_t keep1, float* kernel_ms)
{
    return run_frames(d, frame_call({true, false, false, false}, rx_h, rx_stride, output_h, output_stride, frame_bits_h,
                                    maxFrameBits, nframes, terminated ? 1 : 0, scale, period, keep0, keep1), kernel_ms);
}

// ---- tail-biting frames (vd_frames.h "tail-biting frames"; vd_decode_tg<FRM+TB+...>) ----
int vd_run_device_tb_frames(vd_decoder* d, const float* llr_d, size_t llr_stride, void* output_d, size_t output_stride,
                            const uint32_t* frame_bits_d, size_t maxFrameBits, int nframes, float scale, void* stream)
{
    return launch_frames(d, frame_call({false, true, false, false}, llr_d, llr_stride, output_d, output_stride, frame_bits_d,
                                       maxFrameBits, nframes, kByteFramesTailbiting, scale), stream);
}
int vd_run_tb_frames(vd_decoder* d, const float* llr_h, size_t llr_stride, void* output_h, size_t output_stride,
                     const uint32_t* frame_bits_h, size_t maxFrameBits, int nframes, float scale, float* kernel_ms)
{
    return run_frames(d, frame_call({false, true, false, false}, llr_h, llr_stride, output_h, output_stride, frame_bits_h,
                                    maxFrameBits, nframes, kByteFramesTailbiting, scale), kernel_ms);
}

// ---- punctured tail-biting frames (vd_frames.h "punctured tail-biting frames"; vd_decode_tg<FRM+TB+PUN+...>) ----
int vd_run_device_punct_tb_frames(vd_decoder* d, const float* rx_d, size_t rx_stride, void* output_d, size_t output_stride,
                                  const uint32_t* frame_bits_d, size_t maxFrameBits, int nframes, float scale, int period,
                                  uint32_t keep0, uint32_t keep1, void* stream)
{
    return launch_frames(d, frame_call({true, true, false, false}, rx_d, rx_stride, output_d, output_stride, frame_bits_d,
                                       maxFrameBits, nframes, kByteFramesTailbiting, scale, period, keep0, keep1), stream);
}
int vd_run_punct_tb_frames(vd_decoder* d, const float* rx_h, size_t rx_stride, void* output_h, size_t output_stride,
                           const uint32_t* frame_bits_h, size_t maxFrameBits, int nframes, float scale, int period,
                           uint32_t keep0, uint32_t keep1, float* kernel_ms)
{
    return run_frames(d, frame_call({true, true, false, false}, rx_h, rx_stride, output_h, output_stride, frame_bits_h,
                                    maxFrameBits, nframes, kByteFramesTailbiting, scale, period, keep0, keep1), kernel_ms);
}

// ---- int8 frames (vd_frames.h "int8 frames"; vd_decode_tg<FRM+I8+...>, the byte twins of the four families) ----
int vd_run_device_byte_frames(vd_decoder* d, const int8_t* q_d, size_t q_stride, void* output_d, size_t output_stride,
                              const uint32_t* frame_bits_d, size_t maxFrameBits, int nframes, int kind, float scale,
                              int period, uint32_t keep0, uint32_t keep1, void* stream)
{
    return launch_frames(d, frame_call(byte_family(kind, period, keep0, keep1), q_d, q_stride, output_d, output_stride,
                                       frame_bits_d, maxFrameBits, nframes, kind, scale, period, keep0, keep1), stream);
}
int vd_run_byte_frames(vd_decoder* d, const int8_t* q_h, size_t q_stride, void* output_h, size_t output_stride,
                       const uint32_t* frame_bits_h, size_t maxFrameBits, int nframes, int kind, float scale, int period,
                       uint32_t keep0, uint32_t keep1, float* kernel_ms)
{
    return run_frames(d, frame_call(byte_family(kind, period, keep0, keep1), q_h, q_stride, output_h, output_stride,
                                    frame_bits_h, maxFrameBits, nframes, kind, scale, period, keep0, keep1), kernel_ms);
}

// ---- mixed frames (vd_frames.h "mixed frames"; vd_decode_tg<FRM+MIX+...>, one pattern and one place per frame) ----
int vd_set_frame_patterns(vd_decoder* d, const uint32_t* triples, int n)
{
    if (!d) return fail(VD_ERR_ARG, "null argument");
    if (const char* why = mixed_table_error(triples, n)) return fail(VD_ERR_ARG, why);
    MixRecord tab[kMixMaxPatterns] = {};  // (the records past n: period 0, never read behind mixN)
    for (int i = 0; i < n; i++) tab[i] = mix_record((int)triples[3 * i], triples[3 * i + 1], triples[3 * i + 2]);
    VD_HIP(hipSetDevice(d->device));
    if (!d->mixTab_d) VD_HIP(hipMalloc(&d->mixTab_d, sizeof(d->mixTab)));
    // blocking: hipMemcpy from pageable memory returns after the copy, so the table is in place when the call returns
    // (no launch of this decoder may be in flight: nothing else to wait for)
    VD_HIP(hipMemcpy(d->mixTab_d, tab, sizeof(tab), hipMemcpyHostToDevice));
    memcpy(d->mixTab, tab, sizeof(tab));
    d->mixN = n;
    return VD_OK;
}
int vd_frame_patterns(vd_decoder* d, uint32_t* triples, int* n)
{
    if (!d || !n) return fail(VD_ERR_ARG, "null argument");
    *n = d->mixN;
    for (int i = 0; triples && i < d->mixN; i++) {
        triples[3 * i] = d->mixTab[i].pn.period;
        triples[3 * i + 1] = d->mixTab[i].pn.keep0;
        triples[3 * i + 2] = d->mixTab[i].pn.keep1;
    }
    return VD_OK;
}

// a mixed call: a punctured family (float or int8, padded or tail-biting by the kind) with its two arrays
static FrameCall mixed_call(bool i8, const void* rx, size_t rx_stride, const uint64_t* rx_offsets, void* output, size_t output_stride,
                            const uint32_t* frame_bits, const uint8_t* rate, size_t maxFrameBits, int nframes, int kind, float scale)
{
    FrameCall c = frame_call({true, kind == kByteFramesTailbiting, i8, true}, rx, rx_stride, output, output_stride, frame_bits,
                             maxFrameBits, nframes, kind, scale);
    c.rate = rate;
    c.off = rx_offsets;
    return c;
}

int vd_run_device_mixed_frames(vd_decoder* d, const float* rx_d, size_t rx_stride, const uint64_t* rx_offsets_d, void* output_d,
                               size_t output_stride, const uint32_t* frame_bits_d, const uint8_t* rate_d, size_t maxFrameBits,
                               int nframes, int kind, float scale, void* stream)
{
    return launch_frames(d, mixed_call(false, rx_d, rx_stride, rx_offsets_d, output_d, output_stride, frame_bits_d, rate_d,
                                       maxFrameBits, nframes, kind, scale), stream);
}
int vd_run_device_byte_mixed_frames(vd_decoder* d, const int8_t* q_d, size_t q_stride, const uint64_t* q_offsets_d, void* output_d,
                                    size_t output_stride, const uint32_t* frame_bits_d, const uint8_t* rate_d, size_t maxFrameBits,
                                    int nframes, int kind, float scale, void* stream)
{
    return launch_frames(d, mixed_call(true, q_d, q_stride, q_offsets_d, output_d, output_stride, frame_bits_d, rate_d,
                                       maxFrameBits, nframes, kind, scale), stream);
}

// The blocking mixed variants know every frame's place: with offsets the buffer holds rx_total values and every frame
// must lie inside it (checked here, where the arrays are at hand).
static int run_mixed(vd_decoder* d, FrameCall c, size_t rx_total, float* kernel_ms)
{
    const int rc = check_frames(d, c, false);
    if (rc != VD_OK) return rc;
    if (c.off) {
        if (rx_total > ((size_t)1 << 40)) return fail(VD_ERR_ARG, "rx_total above 2^40 values");
        for (int f = 0; f < c.a.nframes; f++) {
            const uint32_t ri = c.rate ? c.rate[f] : 0u;
            const uint32_t S = c.bits && c.bits[f] < c.a.maxFrameBits ? c.bits[f] : (uint32_t)c.a.maxFrameBits;
            if (ri >= (uint32_t)d->mixN || S == 0) continue;  // (reads nothing)
            if (!mixed_frame_inside(c.off[f], pfrm_bytes<1>(d->mixTab[ri].pn, S), rx_total))
                return fail(VD_ERR_ARG, "frame " + std::to_string(f) + " does not lie inside the rx_total values of the buffer");
        }
    }
    return run_frames_staged(d, c, rx_total, kernel_ms);
}

int vd_run_mixed_frames(vd_decoder* d, const float* rx_h, size_t rx_stride, const uint64_t* rx_offsets_h, size_t rx_total,
                        void* output_h, size_t output_stride, const uint32_t* frame_bits_h, const uint8_t* rate_h,
                        size_t maxFrameBits, int nframes, int kind, float scale, float* kernel_ms)
{
    return run_mixed(d, mixed_call(false, rx_h, rx_stride, rx_offsets_h, output_h, output_stride, frame_bits_h, rate_h,
                                   maxFrameBits, nframes, kind, scale), rx_total, kernel_ms);
}
int vd_run_byte_mixed_frames(vd_decoder* d, const int8_t* q_h, size_t q_stride, const uint64_t* q_offsets_h, size_t q_total,
                             void* output_h, size_t output_stride, const uint32_t* frame_bits_h, const uint8_t* rate_h,
                             size_t maxFrameBits, int nframes, int kind, float scale, float* kernel_ms)
{
    return run_mixed(d, mixed_call(true, q_h, q_stride, q_offsets_h, output_h, output_stride, frame_bits_h, rate_h,
                                   maxFrameBits, nframes, kind, scale), q_total, kernel_ms);
}

void* vd_host_alloc(size_t bytes)
{
    void* p = nullptr;
    if (hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocDefault) != hipSuccess) {
        fail(VD_ERR_NOMEM, "pinned host allocation failed");
        return nullptr;
    }
    return p;
}

int vd_host_free(void* p)
{
    if (p) VD_HIP(hipHostFree(p));
    return VD_OK;
}

// Three-stage pipeline over independent batches on one device: H2D of batch b+1 (stream s_in),
// decode of batch b (the decoder's stream), D2H of batch b-1 (s_out), two device buffer sets.
// Host buffers at full PCIe rate when pinned (vd_host_alloc); pageable ones work, staged by HIP.
int vd_run_stream(vd_decoder* d, const void* const* input_h, void* const* output_h, int nbatches, size_t inputNum,
                  float* wall_ms)
{
    if (!d || !input_h || !output_h || nbatches < 0) return fail(VD_ERR_ARG, "bad arguments");
    if (message_len(d->options, inputNum) == 0) return fail(VD_ERR_ARG, "inputNum too small");
    const size_t inB = input_size(d->options, inputNum), outB = message_len(d->options, inputNum) / 8;
    VD_HIP(hipSetDevice(d->device));
    Form form = Form::Tg;  // of the launches (all alike); no launch, no split-cap check
    // all buffers pinned: the kernels stream them over PCIe themselves, back to back on one stream
    bool zc = true;
    for (int b = 0; b < nbatches && zc; b++) zc = mapped_host(input_h[b]) && mapped_host(output_h[b]);
    if (zc) {
        auto t0 = std::chrono::steady_clock::now();
        for (int b = 0; b < nbatches; b++) {
            int rc = launch_decode(d, mapped_host(input_h[b]), mapped_host(output_h[b]), inputNum, d->stream, &form);
            if (rc != VD_OK) return rc;
        }
        VD_HIP(hipStreamSynchronize(d->stream));
        if (wall_ms)
            *wall_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
        return check_split_cap(d, form);
    }
    int rc = ensure_capacity(d, inB, outB + 16);
    if (rc == VD_OK) rc = grow(d->in2_d, d->cap2_in, inB);
    if (rc == VD_OK) rc = grow(d->out2_d, d->cap2_out, outB + 16);
    if (rc != VD_OK) return rc;
    if (!d->s_in) VD_HIP(hipStreamCreateWithFlags(&d->s_in, hipStreamNonBlocking));
    if (!d->s_out) VD_HIP(hipStreamCreateWithFlags(&d->s_out, hipStreamNonBlocking));
    void* ins[2] = {d->in_d, d->in2_d};
    void* outs[2] = {d->out_d, d->out2_d};
    // per buffer set: input landed, decode done (input free, output ready), output drained
    hipEvent_t landed[2], decoded[2], drained[2];
    for (int k = 0; k < 2; k++) {
        VD_HIP(hipEventCreateWithFlags(&landed[k], hipEventDisableTiming));
        VD_HIP(hipEventCreateWithFlags(&decoded[k], hipEventDisableTiming));
        VD_HIP(hipEventCreateWithFlags(&drained[k], hipEventDisableTiming));
    }
    // Submission order matters: the runtime runs the copies of a device in submission order, so the
    // H2D of batch b+1 is enqueued BEFORE the D2H of batch b (it then overlaps decode b).
    auto h2d = [&](int b) -> int {
        const int k = b & 1;
        if (b >= 2 && hipStreamWaitEvent(d->s_in, decoded[k], 0) != hipSuccess) return fail(VD_ERR_DEVICE, "wait");
        if (hipMemcpyAsync(ins[k], input_h[b], inB, hipMemcpyHostToDevice, d->s_in) != hipSuccess ||
            hipEventRecord(landed[k], d->s_in) != hipSuccess)
            return fail(VD_ERR_DEVICE, "H2D enqueue failed");
        return VD_OK;
    };
    auto t0 = std::chrono::steady_clock::now();
    rc = nbatches > 0 ? h2d(0) : VD_OK;
    for (int b = 0; b < nbatches && rc == VD_OK; b++) {
        const int k = b & 1;
        if (hipStreamWaitEvent(d->stream, landed[k], 0) != hipSuccess ||
            (b >= 2 && hipStreamWaitEvent(d->stream, drained[k], 0) != hipSuccess)) {
            rc = fail(VD_ERR_DEVICE, "pipeline enqueue failed");
            break;
        }
        rc = launch_decode(d, ins[k], outs[k], inputNum, d->stream, &form);
        if (rc != VD_OK) break;
        if (hipEventRecord(decoded[k], d->stream) != hipSuccess) { rc = fail(VD_ERR_DEVICE, "record"); break; }
        if (b + 1 < nbatches && (rc = h2d(b + 1)) != VD_OK) break;
        if (hipStreamWaitEvent(d->s_out, decoded[k], 0) != hipSuccess ||
            hipMemcpyAsync(output_h[b], outs[k], outB, hipMemcpyDeviceToHost, d->s_out) != hipSuccess ||
            hipEventRecord(drained[k], d->s_out) != hipSuccess) {
            rc = fail(VD_ERR_DEVICE, "pipeline enqueue failed");
            break;
        }
    }
    const hipError_t e1 = hipStreamSynchronize(d->s_out), e2 = hipStreamSynchronize(d->stream),
                     e3 = hipStreamSynchronize(d->s_in);
    auto t1 = std::chrono::steady_clock::now();
    for (int k = 0; k < 2; k++) {
        (void)hipEventDestroy(landed[k]);
        (void)hipEventDestroy(decoded[k]);
        (void)hipEventDestroy(drained[k]);
    }
    if (rc != VD_OK) return rc;
    if (e1 != hipSuccess || e2 != hipSuccess || e3 != hipSuccess) return fail(VD_ERR_DEVICE, "pipeline failed");
    if (wall_ms) *wall_ms = std::chrono::duration<float, std::milli>(t1 - t0).count();
    return check_split_cap(d, form);
}

int vd_run_batches(int options, const void* const* input_h, void* const* output_h, size_t inputNum,
                   int nbatches, const int* devices, int ndev, float* wall_ms)
{
    if (!valid(options)) return fail(VD_ERR_OPTIONS, "options disabled by OptionsValid");
    if (!input_h || !output_h || !devices || ndev <= 0 || nbatches < 0) return fail(VD_ERR_ARG, "bad arguments");
    std::vector<vd_decoder*> decs(ndev, nullptr);
    for (int i = 0; i < ndev; i++) {
        int rc = vd_create(options, inputNum, devices[i], &decs[i]);
        if (rc != VD_OK) {
            for (auto* x : decs) vd_destroy(x);
            return rc;
        }
    }
    std::vector<int> rcs(ndev, VD_OK);
    std::vector<std::string> errs(ndev);
    auto t0 = std::chrono::steady_clock::now();
    std::vector<std::thread> th;
    for (int i = 0; i < ndev; i++) {
        th.emplace_back([&, i]() {
            for (int b = i; b < nbatches; b += ndev) {
                int rc = vd_run(decs[i], input_h[b], output_h[b], inputNum, nullptr);
                if (rc != VD_OK) { rcs[i] = rc; errs[i] = g_err; return; }
            }
        });
    }
    for (auto& t : th) t.join();
    auto t1 = std::chrono::steady_clock::now();
    for (auto* x : decs) vd_destroy(x);
    for (int i = 0; i < ndev; i++)
        if (rcs[i] != VD_OK) return fail(rcs[i], errs[i]);
    if (wall_ms) *wall_ms = std::chrono::duration<float, std::milli>(t1 - t0).count();
    return VD_OK;
}

}  // extern "C"

// ---------------------------------------------------------------- reference-exact channel source
namespace {
constexpr uint64_t kMtL = 65536;  // engine outputs per parallel segment
constexpr int kMtR = 8;           // radix of the jump tree
constexpr int kMtLevels = 6;      // jump polynomials for trees of up to R^6 = 262144 segments (2^34 outputs)
int mt_levels(uint64_t T)
{
    int k = 0;
    for (uint64_t p = 1; p < T; p *= kMtR) k++;
    return k;
}
// segment-start states of std::mt19937(seed) for T segments of kMtL outputs: st[m] = the state after
// m * kMtL outputs.  Jump tree, top level first: every state at a multiple of R^(k+1) generates its
// raw words (mt_xseq), then the R-1 children at +c R^k are XOR-accumulated from them (mt_jump).
// jump polynomials on the current device (uploaded once per device, kept for the process)
int mt_polys_device(const uint32_t** out)
{
    static std::mutex mu;
    static std::vector<uint32_t*> per_dev;
    int dev = 0;
    VD_HIP(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lk(mu);
    if ((int)per_dev.size() <= dev) per_dev.resize(dev + 1, nullptr);
    if (!per_dev[dev]) {
        const std::vector<uint32_t>* polys;
        try {
            polys = &vd::mtj::jump_polys(kMtL, kMtR, kMtLevels);
        } catch (const std::exception& e) {
            return fail(VD_ERR_DEVICE, std::string("mt19937 jump polynomials: ") + e.what());
        }
        uint32_t* p = nullptr;
        VD_HIP(hipMalloc(&p, polys->size() * 4));
        VD_HIP(hipMemcpy(p, polys->data(), polys->size() * 4, hipMemcpyHostToDevice));
        per_dev[dev] = p;
    }
    *out = per_dev[dev];
    return VD_OK;
}
int mt_states(uint32_t seed, uint64_t T, uint32_t* st, uint32_t* xs, hipStream_t s)
{
    using namespace vd::mt;
    VD_HIP(hipMemsetAsync(st, 0, T * kN * 4, s));
    hipLaunchKernelGGL(mt_seed, dim3(1), dim3(64), 0, s, seed, st);
    VD_HIP(hipGetLastError());
    const int levels = mt_levels(T);
    if (!levels) return VD_OK;
    if (levels > kMtLevels) return fail(VD_ERR_ARG, "mt19937 stream longer than the jump tree");
    const uint32_t* polys_d = nullptr;  // level k's polynomials do not depend on the tree depth
    int rc = mt_polys_device(&polys_d);
    if (rc) return rc;
    uint64_t step = 1;
    for (int k = 0; k < levels; k++) step *= kMtR;  // R^levels
    for (int k = levels - 1; k >= 0; k--) {
        const uint64_t dstStep = step / kMtR, nsrc = (T + step - 1) / step;
        hipLaunchKernelGGL(mt_xseq, dim3((unsigned)nsrc), dim3(kThreads), 0, s, st, (uint32_t)step, xs);
        VD_HIP(hipGetLastError());
        // slice width: enough workgroups (>= ~4096) on narrow levels, 64 poly words at most
        const uint64_t jumps = nsrc * (kMtR - 1);
        int sw = (int)std::min<uint64_t>(kSliceWords, std::max<uint64_t>(4, jumps * kQW / 4096));
        const unsigned nsl = (unsigned)((kQW + sw - 1) / sw);
        hipLaunchKernelGGL(mt_jump, dim3((unsigned)nsrc, kMtR - 1, nsl), dim3(64), 0, s, xs,
                           polys_d + (size_t)k * (kMtR - 1) * kQW, (uint32_t)step, (uint32_t)dstStep, (uint32_t)T, sw, st);
        VD_HIP(hipGetLastError());
        step = dstStep;
    }
    return VD_OK;
}
struct DevBuf {  // stream-ordered scratch
    void* p = nullptr;
    hipStream_t s;
    explicit DevBuf(hipStream_t s_) : s(s_) {}
    hipError_t alloc(size_t n) { return hipMallocAsync(&p, n ? n : 4, s); }
    ~DevBuf() { if (p) (void)hipFreeAsync(p, s); }
};
}  // namespace

extern "C" {

int vd_channel_device(size_t N, float snr, uint32_t bitSeed, uint32_t noiseSeed, uint8_t* bits_d, float* values_d,
                      void* stream)
{
    using namespace vd::mt;
    if (!bits_d || !values_d) return fail(VD_ERR_ARG, "null argument");
    if (N == 0) return VD_OK;
    if (N > (1ull << 30)) return fail(VD_ERR_ARG, "N above 2^30 bits");
    hipStream_t s = (hipStream_t)stream;
    const float sigma = (float)std::pow(10, -snr / 5.0);  // AddNoise(pow(10, -snr/5.0)), main.cpp:135
    const uint64_t nval = 2 * (uint64_t)N;
    // message bits
    const uint64_t Tb = (N + kMtL - 1) / kMtL;
    const uint64_t attempts = std::isinf(sigma) ? 0 : (uint64_t)(1.30 * (double)N) + 4096;  // E = 4/pi N
    const uint64_t Tn = (2 * attempts + kMtL - 1) / kMtL;
    const uint64_t Tmax = std::max(Tb, Tn);
    const uint64_t nxs = (Tmax + kMtR - 1) / kMtR;
    DevBuf stb(s), stn(s), xs(s), cnt(s);
    VD_HIP(stb.alloc(Tb * kN * 4));
    VD_HIP(xs.alloc(nxs * kNX * 4));
    int rc = mt_states(bitSeed, Tb, (uint32_t*)stb.p, (uint32_t*)xs.p, s);
    if (rc) return rc;
    hipLaunchKernelGGL(mt_bits, dim3((unsigned)Tb), dim3(kThreads), 0, s, (const uint32_t*)stb.p, kMtL, (uint64_t)N, bits_d);
    VD_HIP(hipGetLastError());
    if (std::isinf(sigma)) {  // AddNoise's stddev = +inf branch (viterbiDF.h:79-85)
        hipLaunchKernelGGL(mt_add_base<false>, dim3((unsigned)((nval + 1023) / 1024)), dim3(256), 0, s,
                           (const uint8_t*)bits_d, nval, values_d);
        VD_HIP(hipGetLastError());
        return VD_OK;
    }
    VD_HIP(stn.alloc(Tn * kN * 4));
    VD_HIP(cnt.alloc((Tn + 1) * 4));
    rc = mt_states(noiseSeed, Tn, (uint32_t*)stn.p, (uint32_t*)xs.p, s);
    if (rc) return rc;
    uint32_t* counts = (uint32_t*)cnt.p;
    hipLaunchKernelGGL(mt_noise<0>, dim3((unsigned)Tn), dim3(kThreads), 0, s, (const uint32_t*)stn.p, kMtL, counts,
                       nval, sigma, values_d);
    VD_HIP(hipGetLastError());
    hipLaunchKernelGGL(scan_counts, dim3(1), dim3(1024), 0, s, counts, (uint32_t)Tn);
    VD_HIP(hipGetLastError());
    hipLaunchKernelGGL(mt_noise<1>, dim3((unsigned)Tn), dim3(kThreads), 0, s, (const uint32_t*)stn.p, kMtL, counts,
                       nval, sigma, values_d);
    VD_HIP(hipGetLastError());
    hipLaunchKernelGGL(mt_add_base<true>, dim3((unsigned)((nval + 1023) / 1024)), dim3(256), 0, s,
                       (const uint8_t*)bits_d, nval, values_d);
    VD_HIP(hipGetLastError());
    uint32_t total = 0;
    VD_HIP(hipMemcpyAsync(&total, counts + Tn, 4, hipMemcpyDeviceToHost, s));
    VD_HIP(hipStreamSynchronize(s));
    if (total < N) return fail(VD_ERR_DEVICE, "polar method: too few accepted pairs generated");
    return VD_OK;
}

int vd_simulate_device(int options, size_t N, float snr, uint32_t bitSeed, uint32_t noiseSeed, uint8_t* bits_d,
                       void* packed_d, void* stream)
{
    if (!valid(options)) return fail(VD_ERR_OPTIONS, "options disabled by OptionsValid");
    if (!packed_d || N % 16) return fail(VD_ERR_ARG, "null argument or N not a multiple of 16");
    hipStream_t s = (hipStream_t)stream;
    DevBuf bb(s), vb(s);
    if (!bits_d) {
        VD_HIP(bb.alloc(N));
        bits_d = (uint8_t*)bb.p;
    }
    VD_HIP(vb.alloc(2 * N * sizeof(float)));
    int rc = vd_channel_device(N, snr, bitSeed, noiseSeed, bits_d, (float*)vb.p, stream);
    if (rc) return rc;
    return launch_pack(options, (const float*)vb.p, 2 * N, 40000.0f, packed_d, s);  // SoftDecisionPacker(type, 40000)
}

}  // extern "C"

