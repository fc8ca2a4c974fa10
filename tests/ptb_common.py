"""Punctured tail-biting frame test inputs (test helper): the noisy BPSK tail-biting frames of tb_common.py punctured
by vitdec.puncture, and the contract of their decode -- the oracle's one-chunk decode of vitdec.wrap_frame(
vitdec.depuncture(received values, pattern, 2 S)): the pattern's phase belongs to the frame stage, so the wrapped
copies of a stage carry the same erasures -- with the oracle's words computed once per (option, pattern, frame set)
and read-only."""
import numpy as np

from frames_common import SCALE
from tb_common import oracle_tb_frame, tb_frames

P23, P34 = (2, 0b01, 0b11), (3, 0b101, 0b011)
P78 = (7, 0b1010001, 0b0101111)
P16 = (16, 0xA5C3, 0x5A3D)
PNONE = (16, 0x8000, 0)  # keeps one value in 32: frames of up to 15 stages hold no value at all
SIGMA = 0.2  # (at 0.3 SOFT16 / M_B32 errs at rate 3/4: the code and the fixed window, not the decoder)

# the lengths at which the wrap meets a group boundary (26 + S = 96, 192), the lead (S <= 26), a word boundary, or
# takes several turns; not multiples of the periods 2, 3, 7, 16, shorter than a period, under 96
PTB_SIZES = [1, 2, 5, 7, 25, 26, 27, 31, 32, 33, 69, 70, 71, 95, 96, 97, 165, 166, 167, 250, 1000]
PTB_SIZES_CPU = [1, 2, 3, 5, 6, 7, 12, 24, 25, 26, 27, 31, 32, 33, 48, 69, 70, 71, 72, 95, 96, 97, 165, 166, 167, 168, 250,
                 1000]


def pid(p):
    return f"p{p[0]}-{p[1]:x}-{p[2]:x}"


def punctured(vd, vals, pattern):
    """the rows of vals punctured: [n, punctured_len(pattern, row length)]"""
    return np.stack([vd.puncture(v, pattern) for v in vals])


def oracle_ptb_frame(vd, opt, rx, pattern, S, scale=SCALE):
    """the words that define the decode of one punctured tail-biting frame of S stages from its received values"""
    return oracle_tb_frame(vd, opt, vd.depuncture(rx, pattern, 2 * S), scale)


_REFS = {}


def oracle_ptb_frames(vd, opt, pattern, n, S, seed, sigma=SIGMA):
    """oracle_ptb_frame of puncture(frame) for every frame of tb_frames(n, S, seed, sigma): [n, words], computed once,
    read-only"""
    key = (opt, pattern, n, S, seed, sigma)
    if key not in _REFS:
        vals = tb_frames(n, S, seed, sigma)[1]
        ref = np.stack([oracle_ptb_frame(vd, opt, vd.puncture(v, pattern), pattern, S) for v in vals])
        ref.setflags(write=False)
        _REFS[key] = ref
    return _REFS[key]
