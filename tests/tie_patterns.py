"""Tie-dense and degenerate channel inputs (test helper): on them most add-compare-selects are ties, so the decoded
words are the metric core's tie rule (vd_oracle.c decode_chunk) and hardly anything else -- an all-zero soft
input decodes to 0xf83f83f8 (M_B32), 0xf03f03f0 (M_B16) or 0 (M_FP16) in every word.

pattern(opt, kind, n): the packed input of n encoded values as the decoders read it (int32 words; FP32: floats).
llr_pattern(opt, kind, n): float channel values for the fused-LLR launches (packed by the decoder with `scale`).
reference(opt, kind, nbits): the oracle's words and its range flag, computed once per session and read-only.
Random draws come from np.random.default_rng(7), one generator per call.
"""
import functools

import numpy as np

import vd_oracle as vo

PATTERNS = ["zeros", "all_min", "all_max", "saturated", "ternary", "sparse", "random"]
LLR_PATTERNS = ["zeros", "ternary", "sparse"]
LLR_SCALE = 40000.0
SEED = 7
_BITS = {vo.SOFT4: 4, vo.SOFT8: 8, vo.SOFT16: 16}


def _soft_values(kind, n, bits, rng):
    lo, hi = -(1 << (bits - 1)), (1 << (bits - 1)) - 1
    if kind == "zeros":
        return np.zeros(n, np.int64)
    if kind == "all_min":
        return np.full(n, lo, np.int64)
    if kind == "all_max":
        return np.full(n, hi, np.int64)
    if kind == "saturated":
        return np.where(rng.integers(0, 2, n) == 1, hi, lo).astype(np.int64)
    if kind == "ternary":
        return rng.integers(-1, 2, n)
    if kind == "sparse":
        v = np.zeros(n, np.int64)
        hit = rng.random(n) < 0.02
        v[hit] = rng.integers(lo, hi + 1, int(hit.sum()))
        return v
    if kind == "random":
        return rng.integers(lo, hi + 1, n)
    raise ValueError(kind)


def _pack_soft(v, bits):
    """the first value in the most significant bits of each 32-bit word (viterbiDF.h SoftDecisionPacker)"""
    per = 32 // bits
    u = np.zeros((v.size + per - 1) // per * per, np.uint64)
    u[:v.size] = v.astype(np.int64) & ((1 << bits) - 1)
    u = u.reshape(-1, per)
    w = np.zeros(u.shape[0], np.uint64)
    for i in range(per):
        w = (w << np.uint64(bits)) | u[:, i]
    return w.astype(np.uint32).view(np.int32)


def full_range_floats(rng, n):
    """FP32 channel values from +-2^-10 to +-2^20 with exact small integers and the clamp limits
    (the generator of test_gpu_parity.test_parity_full_range_inputs)"""
    mag = np.exp2(rng.uniform(-10, 20, n)).astype(np.float32)
    small = rng.random(n) < 0.2
    mag[small] = rng.integers(0, 9, int(small.sum())).astype(np.float32)
    vals = np.where(rng.random(n) < 0.5, -mag, mag).astype(np.float32)
    vals[::97] = 7.0
    vals[1::97] = -8.0
    return vals


def _fp32(kind, n, rng):
    if kind == "zeros":
        return np.zeros(n, np.float32)
    if kind == "all_min":
        return np.full(n, -1e9, np.float32)
    if kind == "all_max":
        return np.full(n, 1e9, np.float32)
    if kind == "saturated":
        return np.where(rng.integers(0, 2, n) == 1, 1e9, -1e9).astype(np.float32)
    if kind == "ternary":
        return rng.integers(-1, 2, n).astype(np.float32)
    if kind == "sparse":
        v = np.zeros(n, np.float32)
        hit = rng.random(n) < 0.02
        v[hit] = rng.integers(-8, 8, int(hit.sum())).astype(np.float32)
        return v
    if kind == "random":
        return full_range_floats(rng, n)
    raise ValueError(kind)


def _hard(kind, n, rng):
    nbytes = (n + 31) // 32 * 4
    if kind == "zeros":
        b = np.zeros(nbytes, np.uint8)
    elif kind == "all_min":
        b = np.full(nbytes, 0xFF, np.uint8)
    elif kind == "all_max":
        b = np.full(nbytes, 0xAA, np.uint8)
    elif kind == "saturated":
        b = np.full(nbytes, 0x55, np.uint8)
    elif kind == "ternary":
        b = np.resize(np.array([0x1B, 0xE4, 0x39], np.uint8), nbytes)
    elif kind == "sparse":
        b = np.zeros(nbytes, np.uint8)
        hit = rng.random(nbytes) < 0.02
        b[hit] = rng.integers(0, 256, int(hit.sum()), dtype=np.uint8)
    elif kind == "random":
        b = rng.integers(0, 256, nbytes, dtype=np.uint8)
    else:
        raise ValueError(kind)
    return b.view(np.int32)


def pattern(opt, kind, n):
    rng = np.random.default_rng(SEED)
    ch = opt & 0xF
    if ch == vo.FP32:
        return _fp32(kind, n, rng)
    if ch == vo.HARD:
        return _hard(kind, n, rng)
    return _pack_soft(_soft_values(kind, n, _BITS[ch], rng), _BITS[ch])


def llr_pattern(opt, kind, n):
    """zeros; -1, 0, +1 divided by the scale; zeros with 2 % of the values an integer in [-8, 7] divided by the scale"""
    rng = np.random.default_rng(SEED)
    if kind == "zeros":
        v = np.zeros(n, np.float32)
    elif kind == "ternary":
        v = rng.integers(-1, 2, n).astype(np.float32)
    elif kind == "sparse":
        v = np.zeros(n, np.float32)
        hit = rng.random(n) < 0.02
        v[hit] = rng.integers(-8, 8, int(hit.sum())).astype(np.float32)
    else:
        raise ValueError(kind)
    return (v / np.float32(LLR_SCALE)).astype(np.float32)


def _frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def reference(opt, kind, nbits):
    """(oracle words, range ok) of pattern(opt, kind, 2 nbits)"""
    ref, ok = vo.decode(opt, pattern(opt, kind, 2 * nbits), input_num=2 * nbits, nthreads=16)
    return _frozen(ref), ok


@functools.lru_cache(maxsize=None)
def llr_reference(opt, kind, nbits):
    """(oracle words, range ok) of the oracle's pack of llr_pattern(opt, kind, 2 nbits)"""
    packed = vo.pack(opt, llr_pattern(opt, kind, 2 * nbits), LLR_SCALE)
    ref, ok = vo.decode(opt, packed, input_num=2 * nbits, nthreads=16)
    return _frozen(ref), ok
