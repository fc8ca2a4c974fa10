"""Tail-biting frame test inputs (test helper): a numpy K = 7 (0171, 0133) tail-biting encoder (the register at the
first stage holds the frame's last six bits, cyclically for frames shorter than six), BPSK +-1 frames with Gaussian
noise drawn in the order of frames_common.frames, and the contract of a tail-biting frame decode -- the oracle's
one-chunk decode (nchunks = 1, O_B16 policy 0) of the SoftDecisionPacker packing of vitdec.wrap_frame(frame
values) -- with the oracle's words computed once per (option, frame set) and read-only."""
import functools

import numpy as np

import vd_oracle as vo
from frames_common import SCALE, SIGMA

# the lengths at which the wrap meets a group boundary (26 + S = 96, 192), the lead (S <= 26), a word boundary, or
# takes several turns; TB_SIZES_CPU adds the lengths the definition was checked with on the CPU only
TB_SIZES = [1, 2, 5, 25, 26, 27, 31, 32, 33, 69, 70, 71, 95, 96, 97, 165, 166, 167, 250, 1000]
TB_SIZES_CPU = [1, 2, 5, 6, 7, 25, 26, 27, 31, 32, 33, 69, 70, 71, 95, 96, 97, 165, 166, 167, 250, 1000]


def tb_encode(bits):
    """+-1 channel values (2 per bit, 0171 output first) of every row of bits [n, S] through the tail-biting encoder:
    output stage t is the parity of the bits t - k mod S over the taps k of each polynomial"""
    b = np.atleast_2d(np.asarray(bits, dtype=np.uint8))
    out = np.zeros(b.shape + (2,), dtype=np.uint8)
    for col, poly in enumerate((0o171, 0o133)):
        for k in range(7):  # register bit 6 - k holds the input of k stages ago
            if (poly >> (6 - k)) & 1:
                out[:, :, col] ^= np.roll(b, k, axis=1)
    return np.where(out.reshape(b.shape[0], -1) == 1, 1.0, -1.0).astype(np.float32)


@functools.lru_cache(maxsize=None)
def tb_frames(n, S, seed=1, sigma=SIGMA):
    """(bits [n, S], values [n, 2 S]): noisy BPSK tail-biting frames, read-only; bits first, then noise, from one
    default_rng(seed)"""
    rng = np.random.default_rng(seed)
    bits = rng.integers(0, 2, (n, S), dtype=np.uint8)
    vals = (tb_encode(bits) + rng.normal(0.0, sigma, (n, 2 * S)).astype(np.float32)).astype(np.float32)
    bits.setflags(write=False)
    vals.setflags(write=False)
    return bits, vals


def oracle_tb_frame(vd, opt, values, scale=SCALE):
    """the words that define the decode of one tail-biting frame: W 32-bit words, or 2 W 16-bit ones"""
    ext = vd.wrap_frame(values)
    ref, ok = vo.decode(opt, vo.pack(opt, ext, scale), input_num=ext.size, nchunks=1, b16_policy=0, nthreads=1)
    assert ok
    W = (np.asarray(values).size // 2 + 31) // 32
    assert ref.size == (2 * W if (opt & 0xF00) == vo.O_B16 else W)
    return ref


_REFS = {}


def oracle_tb_frames(vd, opt, n, S, seed=1, scale=SCALE, sigma=SIGMA):
    """oracle_tb_frame of every frame of tb_frames(n, S, seed, sigma): [n, words], computed once, read-only"""
    key = (opt, n, S, seed, scale, sigma)
    if key not in _REFS:
        vals = tb_frames(n, S, seed, sigma)[1]
        ref = np.stack([oracle_tb_frame(vd, opt, v, scale) for v in vals])
        ref.setflags(write=False)
        _REFS[key] = ref
    return _REFS[key]


def wrapped_bits(bits, nbits):
    """what the nbits decoded bits of a frame's words must be: information bit i mod S"""
    b = np.asarray(bits)
    return b[np.arange(nbits) % b.size]
