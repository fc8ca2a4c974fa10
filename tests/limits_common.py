"""Frame launches at the limits of the API (test helper for test_frames_limits.py and test_gpu_frames_limits.py): one
description of a launch for the three frame families -- independent frames (frm), punctured frames (pun), tail-biting
frames (tb) -- so that a test is written once for all of them, and the long frames of the length-limit tests with
their oracle words, computed once per case and read-only.  The contract is the existing one: frames_common.oracle_frame
(vitdec.pad_frame), the same of depuncture(received values), and tb_common.oracle_tb_frame (vitdec.wrap_frame)."""
import collections
import ctypes
import functools

import numpy as np

import vd_oracle as vo
from frames_common import OPTIONS6, SCALE, SIGMA, encode, frame_bits, frames, oracle_frame
from tb_common import oracle_tb_frame, tb_encode, tb_frames

P34 = (3, 0b101, 0b011)
P78 = (7, 0b1010001, 0b0101111)
P16 = (16, 0xA5C3, 0x5A3D)
S8 = vo.SOFT8 | vo.M_B16
HARD = vo.HARD

# fam: "frm", "pun" or "tb"; term: terminated (frm, pun; None for tb); pat: the puncture pattern (pun; else None)
Case = collections.namedtuple("Case", "fam opt term pat")


def _cases():
    out = [Case("frm", o, t, None) for o in OPTIONS6 for t in (True, False) if t or (o & 0xF) != HARD]
    # every pattern with SOFT8 | M_B16, 3/4 with the other options; no punctured frames on HARD decoders
    out += [Case("pun", o, t, p) for o in OPTIONS6 if (o & 0xF) != HARD for t in (True, False)
            for p in ((P34, P78, P16) if o == S8 else (P34,))]
    out += [Case("tb", o, None, None) for o in OPTIONS6]
    return out


CASES = _cases()
# one SOFT8 | M_B16 launch per family (the blocking entry points, the offsets past 4 GiB, the streams)
S8_CASES = [Case("frm", S8, True, None), Case("pun", S8, False, P34), Case("tb", S8, None, None)]


def cid(c):
    s = f"{c.fam}-0x{c.opt:03x}"
    if c.term is not None:
        s += "-terminated" if c.term else "-open"
    if c.pat is not None:
        s += f"-p{c.pat[0]}-{c.pat[1]:x}-{c.pat[2]:x}"
    return s


def small_frames(c, n, S, seed):
    """(bits [n, S], values [n, 2 S]) of n noisy frames of the case's kind (the cached draws of frames_common /
    tb_common, read-only)"""
    return tb_frames(n, S, seed=seed) if c.fam == "tb" else frames(n, S, c.term, seed=seed)


def row_of(vd, c, values):
    """the floats a launch of the case reads for a frame of these values: the kept ones for punctured frames"""
    return vd.puncture(values, c.pat) if c.fam == "pun" else np.asarray(values, dtype=np.float32)


def row_bytes(vd, c, S):
    """bytes of a frame of S stages in the input buffer (the smallest legal stride)"""
    return 4 * vd.punctured_len(c.pat, 2 * S) if c.fam == "pun" else 8 * S


def oracle_row(vd, c, row, S, scale=SCALE):
    """the words that define the decode of a frame of S stages given as the floats the launch reads"""
    if c.fam == "tb":
        return oracle_tb_frame(vd, c.opt, row, scale)
    if c.fam == "pun":
        return oracle_frame(vd, c.opt, vd.depuncture(row, c.pat, 2 * S), c.term, scale)
    return oracle_frame(vd, c.opt, row, c.term, scale)


def frame_nbytes(S):
    return 4 * ((S + 31) // 32)


def launch_device(d, c, in_ptr, in_stride, out_ptr, out_stride, max_bits, n, scale=SCALE, lens_ptr=0, stream=0):
    """the device entry point of the case's family (asynchronous)"""
    if c.fam == "tb":
        d.run_device_tb_frames(in_ptr, in_stride, out_ptr, out_stride, max_bits, n, scale, frame_bits_ptr=lens_ptr, stream=stream)
    elif c.fam == "pun":
        d.run_device_punct_frames(in_ptr, in_stride, out_ptr, out_stride, max_bits, n, c.pat, c.term, scale,
                                  frame_bits_ptr=lens_ptr, stream=stream)
    else:
        d.run_device_frames(in_ptr, in_stride, out_ptr, out_stride, max_bits, n, c.term, scale, frame_bits_ptr=lens_ptr,
                            stream=stream)


def launch_host(vd, d, c, in_h, in_stride, out_h, out_offset, out_stride, lens_h, max_bits, n, scale=SCALE):
    """the blocking host entry point of the case's family over host buffers of any layout (the binding's run_*frames
    methods take contiguous rows only): frame f's floats at in_h + f * in_stride bytes, its words at out_h +
    out_offset + f * out_stride bytes.  Returns kernel_ms."""
    ms = ctypes.c_float(0.0)
    lens = lens_h.ctypes.data if lens_h is not None else None
    inp, out = in_h.ctypes.data, out_h.ctypes.data + out_offset
    if c.fam == "tb":
        rc = vd.lib().vd_run_tb_frames(d._h, inp, in_stride, out, out_stride, lens, max_bits, n, scale, ctypes.byref(ms))
    elif c.fam == "pun":
        rc = vd.lib().vd_run_punct_frames(d._h, inp, in_stride, out, out_stride, lens, max_bits, n, 1 if c.term else 0, scale,
                                          *c.pat, ctypes.byref(ms))
    else:
        rc = vd.lib().vd_run_frames(d._h, inp, in_stride, out, out_stride, lens, max_bits, n, 1 if c.term else 0, scale,
                                    ctypes.byref(ms))
    vd._check(rc)
    return ms.value


def expected_bytes(size, offset, out_stride, words, sentinel=0xA5):
    """the output buffer a launch must leave: sentinel bytes, and frame f's words (None: an empty frame) at offset +
    f * out_stride"""
    want = np.full(size, sentinel, dtype=np.uint8)
    for f, w in enumerate(words):
        if w is not None:
            b = np.ascontiguousarray(w).view(np.uint8)
            want[offset + f * out_stride: offset + f * out_stride + b.size] = b
    return want


def first_difference(got, want, offset, out_stride, n):
    """where two output buffers differ, for an assertion message: (frame, 32-bit word in the frame) of the first few
    differing bytes inside the frames' rows, or the byte offsets of those outside"""
    bad = np.flatnonzero(got != want)
    if bad.size == 0:
        return None
    rel = bad[:6] - offset
    return [(int(r // out_stride), int(r % out_stride) // 4) if 0 <= r < n * out_stride else int(r + offset) for r in rel], int(bad.size)


# ---------------------------------------------------------------- long frames: every boundary up to the limit
LONG_MAX = 1 << 20
# the limit, the last length with a partial final word, both sides of 2^16 (the 16-bit reciprocal, the 24-bit
# products), a length just past a 4096-stage boundary, and short frames beside them in the same workgroups
LONG_LENGTHS = [1 << 20, (1 << 20) - 31, 65536 + 33, 65535, 4097, 97, 0, 1]
LONG_SEED = 7          # frame f: default_rng(LONG_SEED + f), the bits first, then the noise
LONG_CHECKED = 4096    # frames from this length on decode with 0 bit errors through the oracle (terminated, tail-biting)
LONG_OUT_STRIDE = 4 * 32768 + 8
LONG_OUT_OFFSET = 8


@functools.lru_cache(maxsize=None)
def long_frames(kind):
    """kind "terminated", "open" or "tb": [(bits, values) or None for the empty frame] for LONG_LENGTHS, read-only"""
    out = []
    for f, S in enumerate(LONG_LENGTHS):
        if S == 0:
            out.append(None)
            continue
        rng = np.random.default_rng(LONG_SEED + f)
        if kind == "tb":
            bits = rng.integers(0, 2, S, dtype=np.uint8)
            clean = tb_encode(bits)[0]
        else:
            bits = frame_bits(1, S, kind == "terminated", rng)[0]
            clean = encode(bits)
        vals = (clean + rng.normal(0.0, SIGMA, 2 * S).astype(np.float32)).astype(np.float32)
        bits.setflags(write=False)
        vals.setflags(write=False)
        out.append((bits, vals))
    return out


def long_kind(c):
    return "tb" if c.fam == "tb" else "terminated" if c.term else "open"


_LONG_ROWS = {}


def long_rows(vd, c):
    """the floats of every long frame as a launch of the case reads them (None: the empty frame), read-only"""
    key = (c.fam, c.term, c.pat)
    if key not in _LONG_ROWS:
        rows = []
        for fr in long_frames(long_kind(c)):
            r = None if fr is None else np.array(row_of(vd, c, fr[1]))
            if r is not None:
                r.setflags(write=False)
            rows.append(r)
        _LONG_ROWS[key] = rows
    return _LONG_ROWS[key]


_LONG_REFS = {}


def long_refs(vd, c):
    """the oracle's words of every long frame of the case (None: the empty frame), computed once, read-only"""
    if c not in _LONG_REFS:
        refs = []
        for S, r in zip(LONG_LENGTHS, long_rows(vd, c)):
            w = None if r is None else oracle_row(vd, c, r, S)
            if w is not None:
                w.setflags(write=False)
            refs.append(w)
        _LONG_REFS[c] = refs
    return _LONG_REFS[c]


def long_in_stride(vd, c):
    """8 << 20 bytes, or for punctured frames the bytes of a frame of 2^20 stages"""
    return row_bytes(vd, c, LONG_MAX)
