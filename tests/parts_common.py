"""Frames in parts (test helper): the contract of a frame decode with a part length -- part j of a frame is the
oracle's one-chunk decode (nchunks = 1, O_B16 policy 0) of the SoftDecisionPacker packing of sub-stream j of
vitdec.frame_parts(the frame's padded or extended stream, part_bits), written at word j Wp of the frame's words --
for the four frame families, with the oracle's words computed once per (family, option, frame set, part length) and
read-only.  The frames are those of frames_common.frames and tb_common.tb_frames."""
import numpy as np

import vd_oracle as vo
from frames_common import SCALE, SIGMA, frames
from tb_common import tb_frames

# the noisy set on which a decode in parts differs from a whole-frame decode (tests/test_frame_parts.py asserts it)
NOISY_SIGMA, NOISY_S, NOISY_PART_BITS, NOISY_N, NOISY_SEED = 0.9, 1000, 96, 4, 1


def stream_of(vd, opt, kind, values, S, pattern=None, scale=SCALE):
    """the padded (kind 'term', 'open') or extended ('tb') stream of a frame of S stages; values: its 2 S floats, or
    with a pattern its received (kept) floats"""
    v = np.asarray(values, dtype=np.float32)
    if pattern is not None:
        v = vd.depuncture(v, pattern, 2 * S)
    return vd.wrap_frame(v) if kind == "tb" else vd.pad_frame(v, kind == "term", scale, opt)


def oracle_stream(opt, stream, scale=SCALE):
    ref, ok = vo.decode(opt, vo.pack(opt, stream, scale), input_num=stream.size, nchunks=1, b16_policy=0, nthreads=1)
    assert ok
    return ref


def oracle_parts(vd, opt, stream, part_bits, scale=SCALE):
    """the words that define the decode of one frame in parts of part_bits: W 32-bit words, or 2 W 16-bit ones"""
    o16 = (opt & 0xF00) == vo.O_B16
    out, at = [], 0
    for w0, w, sub in vd.frame_parts(stream, part_bits):
        assert w0 == at and sub.size == 2 * (64 + 32 * w)
        ref = oracle_stream(opt, sub, scale)
        assert ref.size == (2 * w if o16 else w)
        out.append(ref)
        at += w
    assert at == stream.size // 64 - 2
    return np.concatenate(out)


def family_frames(kind, n, S, seed, sigma=SIGMA):
    """(bits, values) of n frames of S stages of the family's kind ('term', 'open', 'tb')"""
    return tb_frames(n, S, seed, sigma) if kind == "tb" else frames(n, S, kind == "term", seed, sigma)


_REFS = {}


def oracle_parts_frames(vd, opt, kind, n, S, part_bits, seed, pattern=None, sigma=SIGMA):
    """oracle_parts of every frame of family_frames(kind, n, S, seed, sigma), punctured by pattern when one is given:
    [n, words], computed once, read-only"""
    key = (opt, kind, n, S, part_bits, seed, pattern, sigma)
    if key not in _REFS:
        vals = family_frames(kind, n, S, seed, sigma)[1]
        rows = []
        for v in vals:
            rx = vd.puncture(v, pattern) if pattern is not None else v
            rows.append(oracle_parts(vd, opt, stream_of(vd, opt, kind, rx, S, pattern), part_bits))
        ref = np.stack(rows)
        ref.setflags(write=False)
        _REFS[key] = ref
    return _REFS[key]
