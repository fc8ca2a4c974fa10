"""Frame test inputs (test helper): a numpy K = 7 (0171, 0133) encoder started in state 0, BPSK +-1 frames with
Gaussian noise, and the contract of a frame decode -- the oracle's one-chunk decode (nchunks = 1, O_B16 policy
0) of the SoftDecisionPacker packing of vitdec.pad_frame(frame values) -- with the oracle's words computed once
per (option, frame set) and read-only.  Random draws come from np.random.default_rng(seed), one generator per
call.  At SCALE these inputs saturate SOFT4, SOFT8 and FP32 at every value (no rounding or limit decides a word):
the values that do are in value_patterns.py."""
import functools

import numpy as np

import vd_oracle as vo

SIGMA = 0.3
SCALE = 40000.0
# the six options the definition was checked with on the CPU
OPTIONS6 = [vo.SOFT8 | vo.M_B16, vo.SOFT8 | vo.M_B32 | vo.O_B16, vo.HARD | vo.M_B32, vo.SOFT16 | vo.M_B32,
            vo.FP32 | vo.M_FP16, vo.SOFT4 | vo.M_FP16]


def encode(bits):
    """+-1 channel values (2 per bit, 0171 output first) of bits through the encoder started in state 0"""
    b = np.asarray(bits, dtype=np.uint8)
    out = np.zeros((b.size, 2), dtype=np.uint8)
    for col, poly in enumerate((0o171, 0o133)):
        for k in range(7):  # register bit 6 - k holds the input of k stages ago
            if (poly >> (6 - k)) & 1:
                out[k:, col] ^= b[:b.size - k]
    return np.where(out.reshape(-1) == 1, 1.0, -1.0).astype(np.float32)


def frame_bits(n, S, terminated, rng):
    """n frames of S information bits; terminated: the last min(6, S) are the tail zeros"""
    bits = rng.integers(0, 2, (n, S), dtype=np.uint8)
    if terminated:
        bits[:, max(S - 6, 0):] = 0
    return bits


@functools.lru_cache(maxsize=None)
def frames(n, S, terminated, seed=1, sigma=SIGMA):
    """(bits [n, S], values [n, 2 S]): noisy BPSK frames, read-only"""
    rng = np.random.default_rng(seed)
    bits = frame_bits(n, S, terminated, rng)
    vals = np.stack([encode(b) for b in bits]) + rng.normal(0.0, sigma, (n, 2 * S)).astype(np.float32)
    vals = vals.astype(np.float32)
    bits.setflags(write=False)
    vals.setflags(write=False)
    return bits, vals


def oracle_frame(vd, opt, values, terminated, scale=SCALE):
    """the words that define the decode of one frame: W 32-bit words, or 2 W 16-bit ones"""
    padded = vd.pad_frame(values, terminated, scale, opt)
    ref, ok = vo.decode(opt, vo.pack(opt, padded, scale), input_num=padded.size, nchunks=1, b16_policy=0, nthreads=1)
    assert ok
    W = (np.asarray(values).size // 2 + 31) // 32
    assert ref.size == (2 * W if (opt & 0xF00) == vo.O_B16 else W)
    return ref


_REFS = {}


def oracle_frames(vd, opt, n, S, terminated, seed=1, scale=SCALE):
    """oracle_frame of every frame of frames(n, S, terminated, seed): [n, words], computed once, read-only"""
    key = (opt, n, S, terminated, seed, scale)
    if key not in _REFS:
        vals = frames(n, S, terminated, seed)[1]
        ref = np.stack([oracle_frame(vd, opt, v, terminated, scale) for v in vals])
        ref.setflags(write=False)
        _REFS[key] = ref
    return _REFS[key]


def decoded_bits(opt, words, nbits):
    """the first nbits decoded bits of a frame's words, MSB first (as vd_count_errors reads them)"""
    w = np.asarray(words)
    width = 16 if (opt & 0xF00) == vo.O_B16 else 32
    shifts = np.arange(width - 1, -1, -1, dtype=np.uint32)
    return ((w.astype(np.uint32)[:, None] >> shifts) & 1).astype(np.uint8).reshape(-1)[:nbits]
