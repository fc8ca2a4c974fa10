"""vitdec -- Python binding of the MI355X Viterbi decoder's C-ABI (include/vd_capi.h).

Mirrors the reference's decoder interface `ViterbiCUDA<options>` (src/viterbi/viterbi.h:43-152):
the same option bitmask, the same constexpr members (constLen, polyn1, polyn2, extraL, extraR,
bitsPerPack, encDataPerPack, ...), the same size helpers and the same `run(input, output, inputNum)`
call returning the kernel time in ms.  Errors raise VitdecError (the reference exits the process,
gpuerrors.h:8-17; the C++ header include/viterbi.h keeps that behaviour).

Device-side entry points (`run_device`, `simulate_device`) take raw device pointers, e.g.
`tensor.data_ptr()` of a torch tensor on the decoder's device, and a HIP stream handle
(`torch.cuda.current_stream().cuda_stream`).  torch is only plumbing for memory and streams.

There is no CPU fallback: if lib/libvitdec.so is missing or no GPU is visible, decoding raises.
"""
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# VITDEC_LIB (tests only): another build of the same C-ABI, e.g. the deliberately broken scratch build
# tests/test_gpu_guard.py uses to show the LDS guard check catches a real bug
LIB_PATH = os.environ.get("VITDEC_LIB") or os.path.join(_HERE, "lib", "libvitdec.so")

# ---- option bitmask (reference src/viterbi/viterbi.h:7-20) ----
CHANNEL_MASK, METRIC_MASK, DECODE_MASK, COMP_MASK = 0xF, 0xF0, 0xF00, 0xF000
HARD, SOFT4, SOFT8, SOFT16, FP32 = 0x0, 0x1, 0x2, 0x3, 0x4
M_B32, M_B16, M_FP16 = 0x00, 0x10, 0x20
O_B32, O_B16 = 0x000, 0x100
REG, DPX = 0x0000, 0x1000

INPUT_NAMES = {"HARD": HARD, "h": HARD, "SOFT4": SOFT4, "s4": SOFT4, "SOFT8": SOFT8, "s8": SOFT8,
               "SOFT16": SOFT16, "s16": SOFT16, "FP32": FP32, "f": FP32}
METRIC_NAMES = {"b16": M_B16, "b32": M_B32, "f16": M_FP16}
OUTPUT_NAMES = {"b16": O_B16, "b32": O_B32}
COMP_NAMES = {"REG": REG, "reg": REG, "DPX": DPX, "dpx": DPX}

VD_OK = 0
_ERRNAMES = {-1: "VD_ERR_OPTIONS", -2: "VD_ERR_ARG", -3: "VD_ERR_DEVICE", -4: "VD_ERR_NOMEM",
             -5: "VD_ERR_NOKERNEL"}

# every entry point declared in include/vd_capi.h (tests check the library exports all of them)
EXPORTS = ["vd_options_valid", "vd_input_size", "vd_message_len", "vd_output_size", "vd_num_chunks",
           "vd_create", "vd_destroy", "vd_run", "vd_run_device", "vd_run_device_batch", "vd_run_batches",
           "vd_simulate_host", "vd_count_errors", "vd_last_error", "vd_device_count", "vd_kernel_name",
           "vd_pack_device", "vd_run_device_llr", "vd_run_llr", "vd_host_alloc", "vd_host_free",
           "vd_run_stream", "vd_channel_device", "vd_simulate_device", "vd_mt_state_after", "vd_split_redecodes",
           "vd_split_cap_exits", "vd_set_guard_check", "vd_guard_violations", "vd_run_device_llr_batch", "vd_build_info",
           "vd_decoder_kernel_name", "vd_punctured_len", "vd_run_device_punct", "vd_run_device_punct_batch",
           "vd_run_punct", "vd_frame_output_size", "vd_run_device_frames", "vd_run_frames",
           "vd_run_device_punct_frames", "vd_run_punct_frames", "vd_run_device_tb_frames", "vd_run_tb_frames",
           "vd_run_device_punct_tb_frames", "vd_run_punct_tb_frames", "vd_set_frame_part_bits", "vd_frame_part_bits",
           "vd_run_device_byte_frames", "vd_run_byte_frames", "vd_set_frame_patterns", "vd_frame_patterns",
           "vd_run_device_mixed_frames", "vd_run_device_byte_mixed_frames", "vd_run_mixed_frames",
           "vd_run_byte_mixed_frames"]

# puncture patterns (period, keep0, keep1): bit i of keep0 / keep1 = the first (0171) / second (0133) encoder
# output of the stages t with t % period == i is transmitted.  Any valid masks decode (and equal the rate-1/2
# decode of the depunctured stream); these three are the ones the fixed decode window is long enough for
# (DESIGN.md "Punctured streams")
# the kind of an int8 frame launch (vd_capi.h VD_FRAMES_*)
FRAMES_OPEN, FRAMES_TERMINATED, FRAMES_TAILBITING = 0, 1, 2

PUNCTURE = {"1/2": (1, 1, 1), "2/3": (2, 0b01, 0b11), "3/4": (3, 0b101, 0b011)}


class VitdecError(RuntimeError):
    pass


_lib = None


def lib():
    """Load lib/libvitdec.so (raises if the HIP extension has not been built)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise VitdecError(f"{LIB_PATH} not built: run `make -C {_HERE}` (or __graft_entry__.build())")
    L = ctypes.CDLL(LIB_PATH)
    if not os.environ.get("VITDEC_LIB"):  # the product library must be built from the sources in this tree
        if not hasattr(L, "vd_build_info"):
            raise VitdecError(f"{LIB_PATH} predates the build record (no vd_build_info): rebuild it with "
                              f"`make -C {_HERE}`")
        L.vd_build_info.restype = ctypes.c_char_p
        stale = build_mismatch(L.vd_build_info().decode())
        if stale:
            raise VitdecError(f"{LIB_PATH} is stale ({stale}): rebuild it with `make -C {_HERE}`")
    sz, vp, i, f = ctypes.c_size_t, ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    # name: (argtypes, restype or None)
    sig = {"vd_options_valid": ([i], None),
           "vd_input_size": ([i, sz], sz), "vd_message_len": ([i, sz], sz), "vd_output_size": ([i, sz], sz),
           "vd_create": ([i, sz, i, ctypes.POINTER(vp)], None), "vd_destroy": ([vp], None),
           "vd_run": ([vp, vp, vp, sz, ctypes.POINTER(f)], None), "vd_run_device": ([vp, vp, vp, sz, vp], None),
           "vd_run_device_batch": ([vp, vp, sz, vp, sz, sz, ctypes.c_int, vp], None),
           "vd_run_batches": ([i, ctypes.POINTER(vp), ctypes.POINTER(vp), sz, i, ctypes.POINTER(i), i,
                               ctypes.POINTER(f)], None),
           "vd_simulate_host": ([i, sz, f, ctypes.c_uint32, ctypes.c_uint32, vp, vp], None),
           "vd_channel_device": ([sz, f, ctypes.c_uint32, ctypes.c_uint32, vp, vp, vp], None),
           "vd_simulate_device": ([i, sz, f, ctypes.c_uint32, ctypes.c_uint32, vp, vp, vp], None),
           "vd_mt_state_after": ([ctypes.c_uint32, ctypes.c_uint64, vp], None),
           "vd_split_redecodes": ([i, ctypes.POINTER(ctypes.c_uint64)], None),
           "vd_split_cap_exits": ([i, ctypes.POINTER(ctypes.c_uint64)], None),
           "vd_set_guard_check": ([vp, i], None), "vd_guard_violations": ([vp, ctypes.POINTER(ctypes.c_uint64)], None),
           "vd_count_errors": ([i, vp, sz, vp, sz], ctypes.c_longlong), "vd_last_error": (None, ctypes.c_char_p),
           "vd_pack_device": ([i, vp, sz, f, vp, vp], None), "vd_host_alloc": ([sz], vp), "vd_host_free": ([vp], None),
           "vd_run_stream": ([vp, ctypes.POINTER(vp), ctypes.POINTER(vp), i, sz, ctypes.POINTER(f)], None),
           "vd_run_device_llr": ([vp, vp, vp, sz, f, vp], None),
           "vd_run_llr": ([vp, vp, vp, sz, f, ctypes.POINTER(f)], None),
           "vd_run_device_llr_batch": ([vp, vp, sz, vp, sz, sz, f, ctypes.c_int, vp], None),
           "vd_punctured_len": ([i, ctypes.c_uint32, ctypes.c_uint32, sz], sz),
           "vd_run_device_punct": ([vp, vp, vp, sz, f, i, ctypes.c_uint32, ctypes.c_uint32, vp], None),
           "vd_run_device_punct_batch": ([vp, vp, sz, vp, sz, sz, f, i, ctypes.c_uint32, ctypes.c_uint32, i, vp], None),
           "vd_run_punct": ([vp, vp, vp, sz, f, i, ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(f)], None),
           "vd_frame_output_size": ([i, sz], sz),
           "vd_run_device_frames": ([vp, vp, sz, vp, sz, vp, sz, i, i, f, vp], None),
           "vd_run_frames": ([vp, vp, sz, vp, sz, vp, sz, i, i, f, ctypes.POINTER(f)], None),
           "vd_run_device_punct_frames": ([vp, vp, sz, vp, sz, vp, sz, i, i, f, i, ctypes.c_uint32, ctypes.c_uint32, vp], None),
           "vd_run_punct_frames": ([vp, vp, sz, vp, sz, vp, sz, i, i, f, i, ctypes.c_uint32, ctypes.c_uint32,
                                    ctypes.POINTER(f)], None),
           "vd_run_device_tb_frames": ([vp, vp, sz, vp, sz, vp, sz, i, f, vp], None),
           "vd_run_tb_frames": ([vp, vp, sz, vp, sz, vp, sz, i, f, ctypes.POINTER(f)], None),
           "vd_run_device_punct_tb_frames": ([vp, vp, sz, vp, sz, vp, sz, i, f, i, ctypes.c_uint32, ctypes.c_uint32, vp], None),
           "vd_run_punct_tb_frames": ([vp, vp, sz, vp, sz, vp, sz, i, f, i, ctypes.c_uint32, ctypes.c_uint32,
                                       ctypes.POINTER(f)], None),
           "vd_run_device_byte_frames": ([vp, vp, sz, vp, sz, vp, sz, i, i, f, i, ctypes.c_uint32, ctypes.c_uint32, vp], None),
           "vd_run_byte_frames": ([vp, vp, sz, vp, sz, vp, sz, i, i, f, i, ctypes.c_uint32, ctypes.c_uint32,
                                   ctypes.POINTER(f)], None),
           "vd_set_frame_part_bits": ([vp, sz], None), "vd_frame_part_bits": ([vp, ctypes.POINTER(sz)], None),
           "vd_set_frame_patterns": ([vp, vp, i], None), "vd_frame_patterns": ([vp, vp, ctypes.POINTER(i)], None),
           "vd_run_device_mixed_frames": ([vp, vp, sz, vp, vp, sz, vp, vp, sz, i, i, f, vp], None),
           "vd_run_device_byte_mixed_frames": ([vp, vp, sz, vp, vp, sz, vp, vp, sz, i, i, f, vp], None),
           "vd_run_mixed_frames": ([vp, vp, sz, vp, sz, vp, sz, vp, vp, sz, i, i, f, ctypes.POINTER(f)], None),
           "vd_run_byte_mixed_frames": ([vp, vp, sz, vp, sz, vp, sz, vp, vp, sz, i, i, f, ctypes.POINTER(f)], None),
           "vd_kernel_name": ([i], ctypes.c_char_p),
           "vd_decoder_kernel_name": ([vp, sz, i, i], ctypes.c_char_p)}
    for name, (args, res) in sig.items():
        if not hasattr(L, name):
            if os.environ.get("VITDEC_LIB"):  # an earlier round's build in a same-box A/B: fewer entry points
                continue
            raise VitdecError(f"{LIB_PATH} does not export {name}")
        fn = getattr(L, name)
        if args is not None:
            fn.argtypes = args
        if res is not None:
            fn.restype = res
    _lib = L
    return L


def build_mismatch(info):
    """None when the sources named in the library's build record hash to the recorded value, else why not."""
    import hashlib
    parts = info.split()
    if len(parts) < 2:
        return "no build record"
    h = hashlib.sha256()
    for rel in parts[1:]:
        p = os.path.join(_HERE, rel)
        if not os.path.exists(p):
            return f"source {rel} missing"
        with open(p, "rb") as fh:
            h.update(fh.read())
    return None if h.hexdigest()[:16] == parts[0] else "sources changed since the build"


def _check(rc):
    if rc != VD_OK:
        msg = lib().vd_last_error().decode(errors="replace")
        raise VitdecError(f"{_ERRNAMES.get(rc, rc)}: {msg}")


def parse_options(input="HARD", metric="b32", output="b32", comp="REG"):
    """CLI-style names (reference src/main.cpp:174-264) -> options bitmask."""
    return INPUT_NAMES[input] | METRIC_NAMES[metric] | OUTPUT_NAMES[output] | COMP_NAMES[comp]


def options_valid(options):
    return bool(lib().vd_options_valid(options))


def device_count():
    return lib().vd_device_count()


def kernel_name(options):
    return lib().vd_kernel_name(options).decode()


class ViterbiCUDA:
    """The reference's ViterbiCUDA<options> (viterbi.h:43-152) over the C-ABI."""

    constLen = 7
    polyn1 = 0o171
    polyn2 = 0o133
    extraL_raw = extraR_raw = slideSize_raw = 32
    bmMemWidth = 32
    blockDimY = 2
    FPprecision = 4

    def __init__(self, options, inputNum=0, device=0):
        if not options_valid(options):
            raise VitdecError(f"options 0x{options:x} disabled by OptionsValid")
        self.options = options
        self.inputType = options & CHANNEL_MASK
        self.metricType = options & METRIC_MASK
        self.outputType = options & DECODE_MASK
        self.compMode = options & COMP_MASK
        self.bitsPerMetric = {M_B16: 16, M_B32: 32}.get(self.metricType, 11)
        self.bitsPerPack = 16 if self.outputType == O_B16 else 32
        rnd = lambda a, b: (a + b - 1) // b * b
        self.extraL = rnd(32, self.bitsPerPack) - (self.constLen - 1)
        self.extraR = rnd(32, self.bitsPerPack) + (self.constLen - 1)
        self.slideSize = rnd(32, self.bitsPerPack)
        self.forwardLen = self.extraL + self.slideSize + self.extraR
        self.encDataPerPack = {HARD: 32, SOFT4: 8, SOFT8: 4, SOFT16: 2, FP32: 1}[self.inputType]
        self.encDataWidth = {HARD: 1, SOFT4: 4, SOFT8: 8, SOFT16: 16, FP32: self.FPprecision}[self.inputType]
        self.encPack_t = np.float32 if self.inputType == FP32 else np.int32
        self.decPack_t = np.uint16 if self.outputType == O_B16 else np.uint32
        self.device = device
        h = ctypes.c_void_p()
        _check(lib().vd_create(options, inputNum, device, ctypes.byref(h)))
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            lib().vd_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # size helpers (viterbi.cu:63-92)
    def getInputSize(self, inputNum):
        return lib().vd_input_size(self.options, inputNum)

    def getMessageLen(self, inputNum):
        return lib().vd_message_len(self.options, inputNum)

    def getOutputSize(self, inputNum):
        return lib().vd_output_size(self.options, inputNum)

    def run(self, input_h, output_h=None, inputNum=None):
        """Blocking host decode (viterbi.cu:210-238). Returns (output array, kernel ms)."""
        input_h = np.ascontiguousarray(input_h)
        if inputNum is None:
            inputNum = input_h.size * self.encDataPerPack
        if input_h.nbytes < self.getInputSize(inputNum):
            raise VitdecError("input buffer smaller than getInputSize(inputNum)")
        if output_h is None:
            output_h = np.zeros(self.getOutputSize(inputNum) // np.dtype(self.decPack_t).itemsize,
                                dtype=self.decPack_t)
        if output_h.nbytes < self.getOutputSize(inputNum):
            raise VitdecError("output buffer smaller than getOutputSize(inputNum)")
        ms = ctypes.c_float(0.0)
        _check(lib().vd_run(self._h, input_h.ctypes.data, output_h.ctypes.data, inputNum, ctypes.byref(ms)))
        return output_h, ms.value

    def run_device(self, input_ptr, output_ptr, inputNum, stream=0):
        """Async device decode: raw device pointers on self.device, HIP stream handle (int)."""
        _check(lib().vd_run_device(self._h, ctypes.c_void_p(input_ptr), ctypes.c_void_p(output_ptr), inputNum,
                                   ctypes.c_void_p(stream)))

    def run_device_batch(self, input_ptr, input_stride, output_ptr, output_stride, inputNum, nbatch, stream=0):
        """nbatch independent batches in one launch: batch b at input_ptr + b * input_stride bytes (0: the
        same input each time) -> output_ptr + b * output_stride bytes (vd_run_device_batch)."""
        _check(lib().vd_run_device_batch(self._h, ctypes.c_void_p(input_ptr), input_stride, ctypes.c_void_p(output_ptr),
                                         output_stride, inputNum, nbatch, ctypes.c_void_p(stream)))

    def kernel_for(self, inputNum, nbatch=1, llr=False):
        """the kernel and launch form this decoder runs for nbatch batches of inputNum values
        (vd_decoder_kernel_name: follows VD_NO_PK / VD_PK_SPLIT / VD_NO_SPLIT as read at creation); llr: False /
        0 packed input, True / 1 float channel values, 2 punctured float values, 3 a frame launch (inputNum =
        maxFrameBits, nbatch = nframes), 4 a launch of punctured frames (likewise), 5 a launch of tail-biting
        frames (likewise), 6 a launch of punctured tail-biting frames (likewise; "-" on a HARD decoder), 7 .. 10 the
        int8 twins of 3 .. 6 (run_device_byte_frames; "-" where that call is refused), 11 / 12 a mixed launch of
        open or terminated / of tail-biting frames (run_device_mixed_frames), 13 / 14 their int8 twins (likewise "-"
        where the call is refused)"""
        return lib().vd_decoder_kernel_name(self._h, inputNum, nbatch, int(llr)).decode()

    def set_guard_check(self, enable=True):
        """LDS guard words around every wave's table and ring, counted at kernel exit when overwritten
        (vd_set_guard_check; the count restarts at 0)."""
        _check(lib().vd_set_guard_check(self._h, 1 if enable else 0))

    def guard_violations(self):
        """guard words found overwritten since set_guard_check(True) (synchronises the device)"""
        v = ctypes.c_uint64(0)
        _check(lib().vd_guard_violations(self._h, ctypes.byref(v)))
        return v.value

    def run_stream(self, inputs, inputNum=None, outputs=None):
        """Pipelined decode of independent batches (host copies overlapped with decoding).
        Returns (list of outputs, wall ms).  Pass PinnedArray(...).array buffers (inputs and outputs) for the zero-copy path."""
        inputs = [np.ascontiguousarray(a) for a in inputs]
        if inputNum is None:
            inputNum = inputs[0].size * self.encDataPerPack
        n_out = self.getOutputSize(inputNum) // np.dtype(self.decPack_t).itemsize
        if outputs is None:
            outputs = [np.zeros(n_out, dtype=self.decPack_t) for _ in inputs]
        for a in inputs:
            if a.nbytes < self.getInputSize(inputNum):
                raise VitdecError("input buffer smaller than getInputSize(inputNum)")
        ins = (ctypes.c_void_p * len(inputs))(*[a.ctypes.data for a in inputs])
        outs = (ctypes.c_void_p * len(outputs))(*[o.ctypes.data for o in outputs])
        ms = ctypes.c_float(0.0)
        _check(lib().vd_run_stream(self._h, ins, outs, len(inputs), inputNum, ctypes.byref(ms)))
        return outputs, ms.value

    # ---- float channel values (SoftDecisionPacker(channel, scale) fused into the decode) ----
    def run_llr(self, llr_h, scale=40000.0, output_h=None):
        """Blocking decode of float channel values (viterbiDF.h:98-167 packer fused). Returns (out, ms)."""
        llr_h = np.ascontiguousarray(llr_h, dtype=np.float32)
        inputNum = llr_h.size
        if output_h is None:
            output_h = np.zeros(self.getOutputSize(inputNum) // np.dtype(self.decPack_t).itemsize,
                                dtype=self.decPack_t)
        ms = ctypes.c_float(0.0)
        _check(lib().vd_run_llr(self._h, llr_h.ctypes.data, output_h.ctypes.data, inputNum, scale, ctypes.byref(ms)))
        return output_h, ms.value

    def run_device_llr(self, llr_ptr, output_ptr, inputNum, scale=40000.0, stream=0):
        """Async fused decode of inputNum device floats (16-byte aligned)."""
        _check(lib().vd_run_device_llr(self._h, ctypes.c_void_p(llr_ptr), ctypes.c_void_p(output_ptr), inputNum,
                                       scale, ctypes.c_void_p(stream)))

    def run_device_llr_batch(self, llr_ptr, llr_stride, output_ptr, output_stride, inputNum, nbatch, scale=40000.0,
                             stream=0):
        """nbatch fused decodes of inputNum device floats each in one launch (vd_run_device_llr_batch)."""
        _check(lib().vd_run_device_llr_batch(self._h, ctypes.c_void_p(llr_ptr), llr_stride, ctypes.c_void_p(output_ptr),
                                             output_stride, inputNum, scale, nbatch, ctypes.c_void_p(stream)))

    # ---- punctured streams: the kept float values only, depunctured in the decode's loads ----
    def run_punct(self, rx_h, pattern, inputNum, scale=40000.0, output_h=None):
        """Blocking decode of a punctured stream: rx_h = puncture(values, pattern), the punctured_len(pattern,
        inputNum) kept floats of inputNum mother-code values; pattern = (period, keep0, keep1), e.g.
        PUNCTURE["3/4"].  Equals run_llr(depuncture(rx_h, pattern, inputNum), scale) word for word.  SOFT4,
        SOFT8, SOFT16 and FP32 decoders (HARD: VD_ERR_OPTIONS, a hard decision has no neutral code for a
        punctured value).  FP32 decoders need a scale like the harness's 40000: at scale 1 the truncating
        FP32 branch metric loses a lone +-1 beside a punctured value (rate 3/4 then decodes with errors in a
        third of the bits on a nearly noiseless stream).  Returns (out, ms)."""
        rx_h = np.ascontiguousarray(rx_h, dtype=np.float32)
        need = punctured_len(pattern, inputNum)  # (0: an invalid pattern, which the call below reports)
        if rx_h.size < need:
            raise VitdecError(f"{rx_h.size} received values given, punctured_len{pattern} of {inputNum} is {need}")
        if output_h is None:
            output_h = np.zeros(self.getOutputSize(inputNum) // np.dtype(self.decPack_t).itemsize,
                                dtype=self.decPack_t)
        ms = ctypes.c_float(0.0)
        _check(lib().vd_run_punct(self._h, rx_h.ctypes.data, output_h.ctypes.data, inputNum, scale, *pattern,
                                  ctypes.byref(ms)))
        return output_h, ms.value

    def run_device_punct(self, rx_ptr, output_ptr, inputNum, pattern, scale=40000.0, stream=0):
        """Async decode of punctured_len(pattern, inputNum) device floats (4-byte aligned)."""
        _check(lib().vd_run_device_punct(self._h, ctypes.c_void_p(rx_ptr), ctypes.c_void_p(output_ptr), inputNum, scale,
                                         *pattern, ctypes.c_void_p(stream)))

    def run_device_punct_batch(self, rx_ptr, rx_stride, output_ptr, output_stride, inputNum, nbatch, pattern,
                               scale=40000.0, stream=0):
        """nbatch punctured decodes in one launch: batch b at rx_ptr + b * rx_stride bytes -> output_ptr + b *
        output_stride bytes (strides multiples of 4 bytes; vd_run_device_punct_batch)."""
        _check(lib().vd_run_device_punct_batch(self._h, ctypes.c_void_p(rx_ptr), rx_stride, ctypes.c_void_p(output_ptr),
                                               output_stride, inputNum, scale, *pattern, nbatch, ctypes.c_void_p(stream)))

    # ---- long frames in parts spread over many waves (vd_capi.h "long frames in parts") ----
    def set_frame_part_bits(self, part_bits):
        """Every frame entry point of this decoder decodes frames in parts of part_bits stages, one wave per part:
        0 (the default) whole frames, else a multiple of 96 in [96, 2^20].  Part j of a frame equals, word for word,
        the one-chunk decode of sub-stream j of frame_parts(the frame's padded or extended stream, part_bits).  Read
        on the host at each call; not to be called while launches of this decoder are being issued."""
        _check(lib().vd_set_frame_part_bits(self._h, part_bits))

    def frame_part_bits(self):
        v = ctypes.c_size_t(0)
        _check(lib().vd_frame_part_bits(self._h, ctypes.byref(v)))
        return v.value

    # ---- independent frames, decoded from first bit to last (vd_capi.h "independent frames") ----
    def _run_frames_host(self, who, nframes, maxFrameBits, frame_bits, call):
        """What the blocking frame wrappers share: the output array, the lengths as uint32 (one per frame), the timing
        float and the call, call(out_ptr, row_bytes, frame_bits_ptr, ms_ref) -> status.  Returns (out, ms)."""
        row = frame_output_size(self.options, maxFrameBits)
        out = np.zeros((nframes, row // np.dtype(self.decPack_t).itemsize), dtype=self.decPack_t)
        fb = None
        if frame_bits is not None:
            fb = np.ascontiguousarray(frame_bits, dtype=np.uint32)
            if fb.shape != (nframes,):
                raise VitdecError(f"{who}: frame_bits must hold one length per frame")
        ms = ctypes.c_float(0.0)
        _check(call(out.ctypes.data, row, fb.ctypes.data if fb is not None else None, ctypes.byref(ms)))
        return out, ms.value

    def run_frames(self, llr_h, terminated=True, scale=40000.0, frame_bits=None):
        """Blocking decode of nframes frames in one launch.  llr_h: float array [nframes, 2 * maxFrameBits], frame f
        in row f (first encoder output first, encoder started in state 0); frame_bits: the stages of each frame
        (values above maxFrameBits count as maxFrameBits, 0 decodes nothing), default maxFrameBits each;
        terminated: the frames end with six tail zeros (else open frames: not on HARD decoders).  Frame f
        equals, word for word, the one-chunk decode of pad_frame(its values, ...).  Returns (out, ms): out
        [nframes, words] of decPack_t, 4 * ceil(maxFrameBits / 32) bytes a row, bit i of a row (MSB first)
        information bit i of the frame; the words past a shorter frame's own stay 0."""
        llr_h = np.ascontiguousarray(llr_h, dtype=np.float32)
        if llr_h.ndim != 2 or llr_h.shape[1] % 2:
            raise VitdecError("run_frames: llr_h must be [nframes, 2 * maxFrameBits]")
        nframes, max_bits = llr_h.shape[0], llr_h.shape[1] // 2
        return self._run_frames_host(
            "run_frames", nframes, max_bits, frame_bits, lambda out, row, bits, ms: lib().vd_run_frames(
                self._h, llr_h.ctypes.data, 8 * max_bits, out, row, bits, max_bits, nframes, 1 if terminated else 0,
                scale, ms))

    def run_device_frames(self, llr_ptr, llr_stride, output_ptr, output_stride, maxFrameBits, nframes, terminated=True,
                          scale=40000.0, frame_bits_ptr=0, stream=0):
        """Async decode of nframes frames in one launch (vd_run_device_frames): frame f reads its 2 S_f floats at
        llr_ptr + f * llr_stride bytes (8-byte aligned) and writes 4 * ceil(S_f / 32) bytes at output_ptr + f *
        output_stride; S_f = min(lengths[f], maxFrameBits) with frame_bits_ptr a device array of uint32 lengths,
        or maxFrameBits when it is 0."""
        _check(lib().vd_run_device_frames(self._h, ctypes.c_void_p(llr_ptr), llr_stride, ctypes.c_void_p(output_ptr),
                                          output_stride, ctypes.c_void_p(frame_bits_ptr) if frame_bits_ptr else None,
                                          maxFrameBits, nframes, 1 if terminated else 0, scale, ctypes.c_void_p(stream)))

    # ---- punctured frames: the kept float values of every frame, depunctured in the frame launch's loads ----
    def run_punct_frames(self, rx_h, pattern, maxFrameBits, terminated=True, scale=40000.0, frame_bits=None):
        """Blocking decode of nframes punctured frames in one launch.  rx_h: float array [nframes, L], L >=
        punctured_len(pattern, 2 * maxFrameBits): row f starts with puncture(frame f's values, pattern), the
        pattern's phase at 0 at the frame's first stage (the row pitch is the stride); pattern = (period, keep0,
        keep1), e.g. PUNCTURE["3/4"]; frame_bits: the stages of each frame (information bits including any tail,
        not received floats), as in run_frames.  Frame f equals, word for word, run_frames of depuncture(its
        received values, pattern, 2 S_f).  SOFT4, SOFT8, SOFT16 and FP32 decoders (HARD: VD_ERR_OPTIONS).
        Returns (out, ms) shaped as run_frames does."""
        rx_h = np.ascontiguousarray(rx_h, dtype=np.float32)
        if rx_h.ndim != 2:
            raise VitdecError("run_punct_frames: rx_h must be [nframes, L]")
        need = punctured_len(pattern, 2 * maxFrameBits)  # (0 too for an invalid pattern, which the call below reports)
        if rx_h.shape[1] < need:
            raise VitdecError(f"run_punct_frames: rows of {rx_h.shape[1]} received values, punctured_len{tuple(pattern)} "
                              f"of {2 * maxFrameBits} is {need}")
        nframes = rx_h.shape[0]
        return self._run_frames_host(
            "run_punct_frames", nframes, maxFrameBits, frame_bits, lambda out, row, bits, ms: lib().vd_run_punct_frames(
                self._h, rx_h.ctypes.data, 4 * rx_h.shape[1], out, row, bits, maxFrameBits, nframes,
                1 if terminated else 0, scale, *pattern, ms))

    def run_device_punct_frames(self, rx_ptr, rx_stride, output_ptr, output_stride, maxFrameBits, nframes, pattern,
                                terminated=True, scale=40000.0, frame_bits_ptr=0, stream=0):
        """Async decode of nframes punctured frames in one launch (vd_run_device_punct_frames): frame f reads its
        punctured_len(pattern, 2 S_f) floats at rx_ptr + f * rx_stride bytes (4-byte aligned) and writes 4 *
        ceil(S_f / 32) bytes at output_ptr + f * output_stride; S_f = min(lengths[f], maxFrameBits) stages with
        frame_bits_ptr a device array of uint32 lengths, or maxFrameBits when it is 0."""
        _check(lib().vd_run_device_punct_frames(self._h, ctypes.c_void_p(rx_ptr), rx_stride, ctypes.c_void_p(output_ptr),
                                                output_stride, ctypes.c_void_p(frame_bits_ptr) if frame_bits_ptr else None,
                                                maxFrameBits, nframes, 1 if terminated else 0, scale, *pattern,
                                                ctypes.c_void_p(stream)))

    # ---- tail-biting frames: the wrap-around of every frame in the frame launch's loads (vd_capi.h) ----
    def run_tb_frames(self, llr_h, scale=40000.0, frame_bits=None):
        """Blocking decode of nframes tail-biting frames in one launch.  llr_h: float array [nframes, 2 *
        maxFrameBits], frame f in row f (first encoder output first, the encoder preloaded with the frame's last six
        information bits); frame_bits: the stages of each frame as in run_frames.  Frame f equals, word for word,
        the one-chunk decode of wrap_frame(its values).  Every format, HARD included.  Returns (out, ms) shaped as
        run_frames does: bit i of a row (MSB first), i < S_f, is information bit i of the frame, the rest of its
        last word decodes the wrap (frame bit i mod S_f)."""
        llr_h = np.ascontiguousarray(llr_h, dtype=np.float32)
        if llr_h.ndim != 2 or llr_h.shape[1] % 2:
            raise VitdecError("run_tb_frames: llr_h must be [nframes, 2 * maxFrameBits]")
        nframes, max_bits = llr_h.shape[0], llr_h.shape[1] // 2
        return self._run_frames_host(
            "run_tb_frames", nframes, max_bits, frame_bits, lambda out, row, bits, ms: lib().vd_run_tb_frames(
                self._h, llr_h.ctypes.data, 8 * max_bits, out, row, bits, max_bits, nframes, scale, ms))

    def run_device_tb_frames(self, llr_ptr, llr_stride, output_ptr, output_stride, maxFrameBits, nframes, scale=40000.0,
                             frame_bits_ptr=0, stream=0):
        """Async decode of nframes tail-biting frames in one launch (vd_run_device_tb_frames): pointers, strides and
        lengths as run_device_frames; frame f reads exactly its 2 S_f floats and writes 4 * ceil(S_f / 32) bytes."""
        _check(lib().vd_run_device_tb_frames(self._h, ctypes.c_void_p(llr_ptr), llr_stride, ctypes.c_void_p(output_ptr),
                                             output_stride, ctypes.c_void_p(frame_bits_ptr) if frame_bits_ptr else None,
                                             maxFrameBits, nframes, scale, ctypes.c_void_p(stream)))

    # ---- punctured tail-biting frames: the kept float values of every frame, both index maps in the loads ----
    def run_punct_tb_frames(self, rx_h, pattern, maxFrameBits, scale=40000.0, frame_bits=None):
        """Blocking decode of nframes punctured tail-biting frames in one launch.  rx_h: float array [nframes, L], L >=
        punctured_len(pattern, 2 * maxFrameBits): row f starts with puncture(frame f's values, pattern), the
        pattern's phase at 0 at the frame's first stage and restarting at every wrap (the row pitch is the stride);
        pattern = (period, keep0, keep1), e.g. PUNCTURE["3/4"]; frame_bits: the stages of each frame (not received
        floats), as in run_frames.  Frame f equals, word for word, run_tb_frames of depuncture(its received values,
        pattern, 2 S_f): the one-chunk decode of wrap_frame(depuncture(...)).  SOFT4, SOFT8, SOFT16 and FP32
        decoders (HARD: VD_ERR_OPTIONS).  Returns (out, ms) shaped as run_tb_frames does."""
        rx_h = np.ascontiguousarray(rx_h, dtype=np.float32)
        if rx_h.ndim != 2:
            raise VitdecError("run_punct_tb_frames: rx_h must be [nframes, L]")
        need = punctured_len(pattern, 2 * maxFrameBits)  # (0 too for an invalid pattern, which the call below reports)
        if rx_h.shape[1] < need:
            raise VitdecError(f"run_punct_tb_frames: rows of {rx_h.shape[1]} received values, punctured_len{tuple(pattern)} "
                              f"of {2 * maxFrameBits} is {need}")
        nframes = rx_h.shape[0]
        return self._run_frames_host(
            "run_punct_tb_frames", nframes, maxFrameBits, frame_bits, lambda out, row, bits, ms: lib().vd_run_punct_tb_frames(
                self._h, rx_h.ctypes.data, 4 * rx_h.shape[1], out, row, bits, maxFrameBits, nframes, scale, *pattern,
                ms))

    def run_device_punct_tb_frames(self, rx_ptr, rx_stride, output_ptr, output_stride, maxFrameBits, nframes, pattern,
                                   scale=40000.0, frame_bits_ptr=0, stream=0):
        """Async decode of nframes punctured tail-biting frames in one launch (vd_run_device_punct_tb_frames):
        pointers, strides and lengths as run_device_punct_frames; frame f reads exactly its punctured_len(pattern,
        2 S_f) floats and writes 4 * ceil(S_f / 32) bytes."""
        _check(lib().vd_run_device_punct_tb_frames(self._h, ctypes.c_void_p(rx_ptr), rx_stride, ctypes.c_void_p(output_ptr),
                                                   output_stride, ctypes.c_void_p(frame_bits_ptr) if frame_bits_ptr else None,
                                                   maxFrameBits, nframes, scale, *pattern, ctypes.c_void_p(stream)))

    # ---- int8 frames: the four families above on int8 channel values, byte-wide loads (vd_capi.h "int8 frames") ----
    def run_byte_frames(self, q_h, kind, pattern=(1, 1, 1), maxFrameBits=None, scale=1.0, frame_bits=None):
        """Blocking decode of nframes frames of int8 channel values in one launch.  q_h: int8 array [nframes, L], row f
        starts with frame f's kept values in mother order, one byte each (the row pitch is the stride); kind:
        FRAMES_OPEN, FRAMES_TERMINATED or FRAMES_TAILBITING; pattern = (period, keep0, keep1), (1, 1, 1) for
        unpunctured frames (then L must be even, and maxFrameBits defaults to L // 2; with any other pattern
        maxFrameBits must be given and L >= punctured_len(pattern, 2 * maxFrameBits)); frame_bits: the stages of each
        frame, as in run_frames.  Frame f equals, word for word, the float family's decode (run_frames,
        run_punct_frames, run_tb_frames, run_punct_tb_frames) of q_h.astype(float32) with the same scale.  HARD (not
        open, not punctured), SOFT4 and SOFT8 decoders; SOFT16 and FP32: VD_ERR_OPTIONS.  Returns (out, ms) shaped as
        run_frames does."""
        q_h = np.ascontiguousarray(q_h, dtype=np.int8)
        if q_h.ndim != 2:
            raise VitdecError("run_byte_frames: q_h must be [nframes, L]")
        if maxFrameBits is None:
            if tuple(pattern) != (1, 1, 1):
                raise VitdecError("run_byte_frames: maxFrameBits must be given with a puncture pattern")
            maxFrameBits = q_h.shape[1] // 2
        need = punctured_len(pattern, 2 * maxFrameBits)  # (0 too for an invalid pattern, which the call below reports)
        if q_h.shape[1] < need:
            raise VitdecError(f"run_byte_frames: rows of {q_h.shape[1]} values, punctured_len{tuple(pattern)} of "
                              f"{2 * maxFrameBits} is {need}")
        nframes = q_h.shape[0]
        return self._run_frames_host(
            "run_byte_frames", nframes, maxFrameBits, frame_bits, lambda out, row, bits, ms: lib().vd_run_byte_frames(
                self._h, q_h.ctypes.data, q_h.shape[1], out, row, bits, maxFrameBits, nframes, kind, scale, *pattern,
                ms))

    def run_device_byte_frames(self, q_ptr, q_stride, output_ptr, output_stride, maxFrameBits, nframes, kind,
                               pattern=(1, 1, 1), scale=1.0, frame_bits_ptr=0, stream=0):
        """Async decode of nframes frames of int8 channel values in one launch (vd_run_device_byte_frames): frame f
        reads its punctured_len(pattern, 2 S_f) bytes at q_ptr + f * q_stride bytes (pattern (1, 1, 1): both multiples
        of 2; else any address and stride) and writes 4 * ceil(S_f / 32) bytes at output_ptr + f * output_stride; S_f =
        min(lengths[f], maxFrameBits) stages with frame_bits_ptr a device array of uint32 lengths, or maxFrameBits
        when it is 0."""
        _check(lib().vd_run_device_byte_frames(self._h, ctypes.c_void_p(q_ptr), q_stride, ctypes.c_void_p(output_ptr),
                                               output_stride, ctypes.c_void_p(frame_bits_ptr) if frame_bits_ptr else None,
                                               maxFrameBits, nframes, kind, scale, *pattern, ctypes.c_void_p(stream)))

    # ---- frames of mixed code rates in one launch (vd_capi.h "frames of mixed code rates") ----
    def set_frame_patterns(self, patterns):
        """The decoder's table of up to 16 puncture patterns (period, keep0, keep1), which the mixed launches index per
        frame; (1, 1, 1) is a legal entry.  Blocks until the device copy is done; the kernels read the table when they
        run (a replayed graph sees the table as it stands then).  Not to be called while launches of this decoder
        are in flight."""
        t = np.ascontiguousarray(patterns, dtype=np.uint32).reshape(-1)
        if t.size % 3:
            raise VitdecError("set_frame_patterns: patterns must be (period, keep0, keep1) triples")
        _check(lib().vd_set_frame_patterns(self._h, t.ctypes.data if t.size else None, t.size // 3))

    def frame_patterns(self):
        """the table as a list of (period, keep0, keep1)"""
        t = np.zeros(48, dtype=np.uint32)
        n = ctypes.c_int(0)
        _check(lib().vd_frame_patterns(self._h, t.ctypes.data, ctypes.byref(n)))
        return [tuple(int(x) for x in t[3 * k:3 * k + 3]) for k in range(n.value)]

    def _run_mixed(self, fn, who, dtype, rx_h, kind, maxFrameBits, scale, frame_bits, rates, offsets):
        rx_h = np.ascontiguousarray(rx_h, dtype=dtype)
        if offsets is None:
            if rx_h.ndim != 2:
                raise VitdecError(f"{who}: rx_h must be [nframes, L] without offsets")
            nframes, stride, total, off = rx_h.shape[0], rx_h.shape[1] * rx_h.itemsize, 0, None
            need = max([punctured_len(p, 2 * maxFrameBits) for p in self.frame_patterns()] or [0])
            if rx_h.shape[1] < need:
                raise VitdecError(f"{who}: rows of {rx_h.shape[1]} values, the table's densest pattern needs {need} for "
                                  f"{maxFrameBits} stages")
        else:
            off = np.ascontiguousarray(offsets, dtype=np.uint64)
            if off.ndim != 1 or rx_h.ndim != 1:
                raise VitdecError(f"{who}: with offsets rx_h is one flat buffer and offsets holds one index per frame")
            nframes, stride, total = off.size, 0, rx_h.size

        def call(out, row, bits, ms):  # (the rates are checked after the lengths)
            rt = None
            if rates is not None:
                rt = np.ascontiguousarray(rates, dtype=np.uint8)
                if rt.shape != (nframes,):
                    raise VitdecError(f"{who}: rates must hold one pattern index per frame")
            rx = rx_h if rx_h.size else np.zeros(4, dtype=dtype)  # (a buffer to point at: no frame reads a value)
            return fn(self._h, rx.ctypes.data, stride, off.ctypes.data if off is not None else None, total, out, row, bits,
                      rt.ctypes.data if rt is not None else None, maxFrameBits, nframes, kind, scale, ms)
        return self._run_frames_host(who, nframes, maxFrameBits, frame_bits, call)

    def run_mixed_frames(self, rx_h, kind, maxFrameBits, scale=40000.0, frame_bits=None, rates=None, offsets=None):
        """Blocking decode of nframes frames at mixed code rates in one launch.  Frame f decodes under pattern rates[f]
        of set_frame_patterns' table (default: pattern 0) with min(frame_bits[f], maxFrameBits) stages; kind:
        FRAMES_OPEN, FRAMES_TERMINATED or FRAMES_TAILBITING for all of them.  Without offsets rx_h is a float array
        [nframes, L] with frame f's received values at the start of row f; with offsets it is one flat float buffer and
        frame f's values start at index offsets[f] (mixed_layout gives back-to-back offsets).  Frame f equals, word
        for word, run_punct_frames / run_punct_tb_frames of that frame alone under its pattern; a frame of 0 stages or
        with a rate index outside the table decodes nothing.  SOFT4, SOFT8, SOFT16 and FP32 decoders.  Returns (out,
        ms) shaped as run_frames does."""
        return self._run_mixed(lib().vd_run_mixed_frames, "run_mixed_frames", np.float32, rx_h, kind, maxFrameBits, scale,
                               frame_bits, rates, offsets)

    def run_byte_mixed_frames(self, q_h, kind, maxFrameBits, scale=1.0, frame_bits=None, rates=None, offsets=None):
        """run_mixed_frames on int8 channel values (row pitch and offsets in bytes): frame f equals run_byte_frames of
        that frame alone under its pattern -- the punctured path, also for (1, 1, 1), whose words equal the unpunctured
        one's.  SOFT4 and SOFT8 decoders."""
        return self._run_mixed(lib().vd_run_byte_mixed_frames, "run_byte_mixed_frames", np.int8, q_h, kind, maxFrameBits,
                               scale, frame_bits, rates, offsets)

    def run_device_mixed_frames(self, rx_ptr, rx_stride, output_ptr, output_stride, maxFrameBits, nframes, kind,
                                scale=40000.0, frame_bits_ptr=0, rate_ptr=0, offsets_ptr=0, stream=0):
        """Async decode of nframes frames at mixed code rates in one launch (vd_run_device_mixed_frames): frame f reads
        its punctured_len(pattern rate[f], 2 S_f) floats at rx_ptr + f * rx_stride bytes, or with offsets_ptr (a
        device array of uint64 value indices) from float offsets[f] of rx_ptr on, and writes 4 * ceil(S_f / 32) bytes
        at output_ptr + f * output_stride.  rate_ptr: a device array of uint8 pattern indices (0: pattern 0 for all);
        frame_bits_ptr as in run_device_frames."""
        vp = ctypes.c_void_p
        _check(lib().vd_run_device_mixed_frames(self._h, vp(rx_ptr), rx_stride, vp(offsets_ptr) if offsets_ptr else None,
                                                vp(output_ptr), output_stride, vp(frame_bits_ptr) if frame_bits_ptr else None,
                                                vp(rate_ptr) if rate_ptr else None, maxFrameBits, nframes, kind, scale,
                                                vp(stream)))

    def run_device_byte_mixed_frames(self, q_ptr, q_stride, output_ptr, output_stride, maxFrameBits, nframes, kind,
                                     scale=1.0, frame_bits_ptr=0, rate_ptr=0, offsets_ptr=0, stream=0):
        """run_device_mixed_frames on int8 channel values (vd_run_device_byte_mixed_frames): strides and offsets in
        bytes, any address."""
        vp = ctypes.c_void_p
        _check(lib().vd_run_device_byte_mixed_frames(self._h, vp(q_ptr), q_stride, vp(offsets_ptr) if offsets_ptr else None,
                                                     vp(output_ptr), output_stride,
                                                     vp(frame_bits_ptr) if frame_bits_ptr else None,
                                                     vp(rate_ptr) if rate_ptr else None, maxFrameBits, nframes, kind, scale,
                                                     vp(stream)))


class PinnedArray:
    """A numpy view of page-locked host memory from vd_host_alloc (freed with the object)."""

    def __init__(self, shape, dtype):
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        self._p = lib().vd_host_alloc(n)
        if not self._p:
            raise VitdecError("vd_host_alloc failed")
        buf = (ctypes.c_char * n).from_address(self._p)
        self.array = np.frombuffer(buf, dtype=dtype).reshape(shape)

    def __del__(self):
        if getattr(self, "_p", None):
            lib().vd_host_free(self._p)
            self._p = None


def pack_device(options, llr_ptr, inputNum, packed_ptr, scale=40000.0, stream=0):
    """The reference's SoftDecisionPacker on device floats -> vd_input_size(options, inputNum) bytes."""
    _check(lib().vd_pack_device(options, ctypes.c_void_p(llr_ptr), inputNum, scale, ctypes.c_void_p(packed_ptr),
                                ctypes.c_void_p(stream)))


def punctured_len(pattern, inputNum):
    """received values of inputNum mother-code values under pattern (vd_punctured_len; 0: invalid pattern)"""
    return lib().vd_punctured_len(*pattern, inputNum)


def _kept(pattern, inputNum):
    """which of the first 2 * (inputNum // 2) mother positions pattern = (period, keep0, keep1) transmits"""
    period, keep0, keep1 = pattern
    r = np.arange(inputNum // 2) % period
    return np.stack([(keep0 >> r) & 1, (keep1 >> r) & 1], axis=1).reshape(-1).astype(bool)


def puncture(values, pattern):
    """the kept values of a rate-1/2 stream, in mother order (host helper: the transmitter's puncturer)"""
    v = np.ascontiguousarray(values, dtype=np.float32).reshape(-1)
    kept = _kept(pattern, v.size)
    return v[:kept.size][kept]


def depuncture(rx, pattern, inputNum):
    """the rate-1/2 stream of inputNum values a punctured decode is defined by: rx at the kept positions,
    +0.0 at the punctured ones"""
    kept = _kept(pattern, inputNum)
    out = np.zeros(inputNum, dtype=np.float32)
    out[:kept.size][kept] = np.asarray(rx, dtype=np.float32).reshape(-1)[:int(kept.sum())]
    return out


def mixed_layout(lengths, rates, patterns):
    """(offsets, total) of frames laid back to back in one received buffer: frame f of lengths[f] stages under
    patterns[rates[f]] holds punctured_len(that pattern, 2 * lengths[f]) values from index offsets[f] on; a frame whose
    rate index lies outside patterns holds none.  offsets: uint64 array, total: the values of the buffer."""
    offs, at = np.zeros(len(lengths), dtype=np.uint64), 0
    for f, (S, r) in enumerate(zip(lengths, rates)):
        offs[f] = at
        if 0 <= int(r) < len(patterns):
            period, keep0, keep1 = patterns[int(r)]
            kp = bin(keep0).count("1") + bin(keep1).count("1")
            low = (1 << (int(S) % period)) - 1
            at += int(S) // period * kp + bin(keep0 & low).count("1") + bin(keep1 & low).count("1")
    return offs, at


def frame_output_size(options, frameBits):
    """bytes a frame of frameBits stages decodes to: 4 * ceil(frameBits / 32) (vd_frame_output_size)"""
    return lib().vd_frame_output_size(options, frameBits)


FRAME_LEAD = 26  # pad stages before a frame: the reference's extraL, where a decode window starts emitting bits


def pad_frame(values, terminated, scale, opt):
    """The padded stream that defines a frame decode (host helper; the contract the tests feed to the oracle).

    values: the 2 S floats of a frame of S stages.  Returns the 2 P floats, P = 64 + 32 ceil(S / 32), of
    26 pad stages, the frame, and pad stages (terminated) or +0.0 erasures (open frame) up to P; the frame
    decode equals the one-chunk decode (nchunks = 1, inputNum = 2 P) of its SoftDecisionPacker(opt, scale)
    packing, and decoded bit i is information bit i of the frame.  The pad float is -32768 / scale rounded
    away from zero, so that it quantises to the most negative code of every format (HARD bit 0, SOFT4 -8,
    SOFT8 -128, SOFT16 -32768, FP32 -8 after the clamp): the same code as the decode kernel's own pad value
    (-65536 / scale), hence the same branch metrics.  Open frames need a neutral code: not with HARD."""
    v = np.ascontiguousarray(values, dtype=np.float32).reshape(-1)
    if v.size % 2:
        raise VitdecError("pad_frame: two values per stage")
    if not terminated and (opt & CHANNEL_MASK) == HARD:
        raise VitdecError("pad_frame: an open frame needs a neutral code, HARD has none")
    sc = np.float32(scale)
    with np.errstate(all="ignore"):
        ok = np.isfinite(sc) and sc > 0 and np.isfinite(np.float32(-65536.0) / sc)
    if not ok:  # (the entry points' rule, VD_ERR_ARG there)
        raise VitdecError("pad_frame: scale must be finite and > 0 (and -65536 / scale finite)")
    pad = np.float32(-32768.0) / sc
    if pad * sc > np.float32(-32768.0):
        pad = np.nextafter(pad, np.float32(-np.inf))
    S = v.size // 2
    P = 64 + 32 * ((S + 31) // 32)
    out = np.full(2 * P, pad if terminated else 0.0, dtype=np.float32)
    out[:2 * FRAME_LEAD] = pad
    out[2 * FRAME_LEAD:2 * (FRAME_LEAD + S)] = v
    return out


def wrap_frame(values):
    """The extended stream that defines a tail-biting frame decode (host helper; the contract the tests feed to
    the oracle).

    values: the 2 S floats of a tail-biting frame of S >= 1 stages.  Returns the 2 P floats, P = 64 + 32 ceil(S /
    32), with stage p holding both values of frame stage (p - 26) mod S (the non-negative residue, as many turns
    as P takes); the frame decode equals the one-chunk decode (nchunks = 1, inputNum = 2 P) of its
    SoftDecisionPacker(opt, scale) packing, and decoded bit i < S is information bit i of the frame."""
    v = np.ascontiguousarray(values, dtype=np.float32).reshape(-1)
    if v.size % 2 or v.size == 0:
        raise VitdecError("wrap_frame: two values per stage, at least one stage")
    S = v.size // 2
    P = 64 + 32 * ((S + 31) // 32)
    return v.reshape(S, 2)[(np.arange(P) - FRAME_LEAD) % S].reshape(-1).copy()


def frame_parts(stream, part_bits):
    """The sub-streams that define a frame decode in parts (host helper; the contract the tests feed to the oracle).

    stream: the 2 P floats, P = 64 + 32 W, of a frame's padded stream (pad_frame) or extended stream (wrap_frame);
    part_bits: 0 (whole frames) or a multiple of 96 in [96, 2^20].  Yields (word0, words, sub) for part j = 0, 1,
    ...: with Wp = part_bits / 32, word0 = j Wp, words = w_j = min(Wp, W - j Wp), and sub the 2 (64 + 32 w_j)
    floats of stages [32 j Wp, 32 j Wp + 64 + 32 w_j) of the stream.  Part j of the frame decode equals the
    one-chunk decode (nchunks = 1, inputNum = sub.size) of sub's SoftDecisionPacker packing, written at word word0
    of the frame's output (O_B16: 16-bit words 2 word0 .. 2 word0 + 2 w_j - 1).  part_bits = 0, or >= 32 W, yields
    the stream itself."""
    v = np.ascontiguousarray(stream, dtype=np.float32).reshape(-1)
    if v.size % 64 or v.size < 2 * 96:
        raise VitdecError("frame_parts: a stream of 2 (64 + 32 W) floats, W >= 1")
    if part_bits != 0 and (part_bits % 96 or not 96 <= part_bits <= 1 << 20):
        raise VitdecError("frame_parts: part_bits must be 0 or a multiple of 96 in [96, 2^20]")
    W = v.size // 64 - 2
    Wp = part_bits // 32 if part_bits else W
    for w0 in range(0, W, Wp):
        w = min(Wp, W - w0)
        yield w0, w, v[64 * w0:64 * w0 + 2 * (64 + 32 * w)]


def simulate_host(options, n_bits, snr, bit_seed, noise_seed):
    """Reference harness pipeline on the host (std::mt19937 + std::normal_distribution<float>)."""
    bits = np.zeros(n_bits, dtype=np.uint8)
    nbytes = lib().vd_input_size(options, 2 * n_bits)
    packed = np.zeros(nbytes // 4, dtype=np.float32 if (options & CHANNEL_MASK) == FP32 else np.int32)
    _check(lib().vd_simulate_host(options, n_bits, snr, bit_seed, noise_seed, bits.ctypes.data, packed.ctypes.data))
    return bits, packed


def channel_device(n_bits, snr, bit_seed, noise_seed, bits_ptr, values_ptr, stream=0):
    """The reference harness's RandBitGen | ConvolutionalEncoder | AddNoise on the GPU, bit-exact with
    simulate_host for the same seeds: n_bits bytes of message bits, 2 n_bits float channel values."""
    _check(lib().vd_channel_device(n_bits, snr, bit_seed, noise_seed, ctypes.c_void_p(bits_ptr),
                                   ctypes.c_void_p(values_ptr), ctypes.c_void_p(stream)))


def simulate_device(options, n_bits, snr, bit_seed, noise_seed, bits_ptr, packed_ptr, stream=0):
    """channel_device + SoftDecisionPacker(type, 40000): the packed input simulate_host makes, on the GPU."""
    _check(lib().vd_simulate_device(options, n_bits, snr, bit_seed, noise_seed,
                                    ctypes.c_void_p(bits_ptr) if bits_ptr else None, ctypes.c_void_p(packed_ptr),
                                    ctypes.c_void_p(stream)))


def split_redecodes(device=0):
    """split chunks re-decoded whole on a device so far (a speculative piece start did not converge)"""
    v = ctypes.c_uint64(0)
    _check(lib().vd_split_redecodes(device, ctypes.byref(v)))
    return v.value


def split_cap_exits(device=0):
    """split-launch waves that stopped re-decoding at the pass cap with a part still differing (always 0: the
    passes provably end within P; run / run_llr / run_stream raise if it is ever not)"""
    v = ctypes.c_uint64(0)
    _check(lib().vd_split_cap_exits(device, ctypes.byref(v)))
    return v.value


def mt_state_after(seed, n):
    """std::mt19937(seed)'s state array after n outputs (host GF(2) jump-ahead used by channel_device)."""
    st = np.zeros(624, dtype=np.uint32)
    _check(lib().vd_mt_state_after(seed, n, st.ctypes.data))
    return st


def count_errors(options, bits, decoded):
    return int(lib().vd_count_errors(options, bits.ctypes.data, bits.size, decoded.ctypes.data, decoded.nbytes))


def run_batches(options, inputs, inputNum, devices):
    """Independent batches sharded over `devices` (vd_run_batches). Returns (outputs, wall ms)."""
    n = len(inputs)
    dt = np.uint16 if (options & DECODE_MASK) == O_B16 else np.uint32
    outs = [np.zeros(lib().vd_output_size(options, inputNum) // np.dtype(dt).itemsize, dtype=dt) for _ in range(n)]
    ins = (ctypes.c_void_p * n)(*[x.ctypes.data for x in inputs])
    ous = (ctypes.c_void_p * n)(*[x.ctypes.data for x in outs])
    devs = (ctypes.c_int * len(devices))(*devices)
    ms = ctypes.c_float(0.0)
    _check(lib().vd_run_batches(options, ins, ous, inputNum, n, devs, len(devices), ctypes.byref(ms)))
    return outs, ms.value
