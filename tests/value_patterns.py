"""Full-range, rounding-edge and special channel values (test helper): inputs on which the quantiser of a float or int8
entry point -- the rounding mode, the two saturation limits, the signed zeros, denormals and the x86 narrowing of
SoftDecisionPacker -- decides the decoded words, where the noisy +-1 codewords of frames_common.py and tb_common.py at
scale 40000 saturate SOFT4, SOFT8 and FP32 everywhere.

Float patterns are written in code units of the decoder's format (hi = 7 SOFT4, 127 SOFT8, 32767 SOFT16, 7 FP32, the
clamp) and divided by the scale in float32, so value * scale lands on the code again (exactly at the power-of-two
scales, after one more rounding at 0.37 and 40000):
  uniform       uniform in +-1.25 (hi + 1): both saturations, every intermediate code; fractional across FP32's clamp
  small         uniform in [-2.5, 2.5]: the rounding decides most branch metrics
  small_halves  k + 0.5, k an integer in [-3, 3): round-half-even ties around zero, -0.0 after rint
  halves        k + 0.5 over the whole code range, to two steps past each saturation
  edge          +-(hi + j + {0, 0.5}), j = -1 .. 2: at and on both sides of each saturation limit (FP32: 6.5 .. 8.5)
  satrand       +-4 (hi + 1) with random signs: no codeword, every code -hi-1 or +hi
  specials      test_gpu_llr.specials() sprinkled over a quarter of a `small` frame (FP32: non-finite ones +-1e30)
HARD decoders (the bit is value * scale > 0): zero_mix, draws from {-1, -0.0, +0.0, +1, +1e-40, -1e-40, NaN}, and
satrand, +-1.  Int8 inputs: every_byte (all 256 values shuffled and repeated, -128 and 127 next to each other at both
ends of a frame), small_bytes (integers in [-3, 3]) and sat_bytes (-128 or 127).
Every call draws from one np.random.default_rng(seed); returned arrays are read-only and computed once.

The quantiser mutants are wrong quantisers as numpy functions on stream * scale; a mutant's words are the oracle's
decode of vo.pack(opt, mutant(stream * scale), 1.0) (mutant_words).  GOOD is the right quantiser written the same way,
whose words equal the oracle's own: tests/test_value_patterns.py asserts both."""
import functools
import zlib

import numpy as np

import vd_oracle as vo
from test_gpu_llr import specials as llr_specials

HARD, SOFT4, SOFT8, SOFT16, FP32 = vo.HARD, vo.SOFT4, vo.SOFT8, vo.SOFT16, vo.FP32
HI = {SOFT4: 7, SOFT8: 127, SOFT16: 32767, FP32: 7}
# all valid channel x metric pairs
PAIRS = [HARD | vo.M_B32, HARD | vo.M_B16, HARD | vo.M_FP16, SOFT4 | vo.M_B32, SOFT4 | vo.M_B16, SOFT4 | vo.M_FP16,
         SOFT8 | vo.M_B32, SOFT8 | vo.M_B16, SOFT16 | vo.M_B32, FP32 | vo.M_B32, FP32 | vo.M_B16, FP32 | vo.M_FP16]
SOFT_PATTERNS = ["uniform", "small", "small_halves", "halves", "edge", "satrand", "specials"]
HARD_PATTERNS = ["zero_mix", "satrand"]
BYTE_PATTERNS = ["every_byte", "small_bytes", "sat_bytes"]
SCALES = [1.0, 0.37, 40000.0]
# exact products at extreme exponents (the pad -65536 / scale stays finite): for `small` and `edge` only
EXTREME_SCALES = [2.0 ** 100, 2.0 ** -100]
BYTE_SCALES = [1.0, 0.25, 0.37, 3.0]
P34, P56 = (3, 0b101, 0b011), (5, 0b10101, 0b01011)
N_FRAMES = 5  # a full workgroup of 4 waves and a partial one


def patterns(opt):
    """the float patterns of a decoder's format"""
    return HARD_PATTERNS if (opt & 0xF) == HARD else SOFT_PATTERNS


def scales(kind):
    """the scales a float pattern is run at"""
    return SCALES + (EXTREME_SCALES if kind in ("small", "edge") else [])


def _seed(*key):
    return zlib.crc32(repr(key).encode())


def _codes(ch, kind, n, rng):
    """n values of a float pattern in code units (float64)"""
    if ch == HARD:
        if kind == "zero_mix":
            return rng.choice(np.array([-1.0, -0.0, 0.0, 1.0, 1e-40, -1e-40, np.nan]), n)
        if kind == "satrand":
            return np.where(rng.integers(0, 2, n) == 1, 1.0, -1.0)
        raise ValueError(kind)
    hi = HI[ch]
    if kind == "uniform":
        return rng.uniform(-1.25 * (hi + 1), 1.25 * (hi + 1), n)
    if kind == "small":
        return rng.uniform(-2.5, 2.5, n)
    if kind == "small_halves":
        return rng.integers(-3, 3, n) + 0.5
    if kind == "halves":
        return rng.integers(-(hi + 3), hi + 3, n) + 0.5
    if kind == "edge":
        mags = np.arange(6.5, 8.75, 0.5) if ch == FP32 else np.arange(hi - 1.0, hi + 2.75, 0.5)
        return rng.choice(mags, n) * np.where(rng.integers(0, 2, n) == 1, 1.0, -1.0)
    if kind == "satrand":
        return np.where(rng.integers(0, 2, n) == 1, 4.0 * (hi + 1), -4.0 * (hi + 1))
    if kind == "specials":
        v = rng.uniform(-2.5, 2.5, n)
        _sprinkle(ch, v, max(n // 4, 1), rng)
        return v
    raise ValueError(kind)


def _sprinkle(ch, v, count, rng):
    """test_gpu_llr.specials(), shuffled and resized to count, at random places of v"""
    idx = rng.choice(v.size, count, replace=False)
    sp = np.resize(rng.permutation(llr_specials()), count).astype(np.float64)
    if ch == FP32:  # the FP32 branch metric of NaN is not defined by the reference: keep finite
        sp = np.where(np.isfinite(sp), sp, np.where(np.signbit(sp), -1e30, 1e30))
    v[idx] = sp


@functools.lru_cache(maxsize=None)
def frames(opt, kind, S, scale, n=N_FRAMES, seed=None):
    """n frames of S stages of a float pattern for a decoder of opt's format at scale: float32 [n, 2 S], the pattern's
    code values divided by the scale; read-only.  The same codes at every scale and metric type."""
    ch = opt & 0xF
    rng = np.random.default_rng(_seed(ch, kind, S, n) if seed is None else seed)
    with np.errstate(all="ignore"):
        v = (_codes(ch, kind, 2 * S * n, rng).astype(np.float32) / np.float32(scale)).astype(np.float32).reshape(n, 2 * S)
    v.setflags(write=False)
    return v


STREAM_PATTERNS = ["small", "small_halves", "uniform", "edge", "satrand"]


@functools.lru_cache(maxsize=None)
def stream(opt, nbits, scale, nspecials=500):
    """2 nbits values for the stream entry points: equal shares of small, small_halves, uniform, edge and satrand one
    after the other (HARD: zero_mix and satrand) with nspecials specials sprinkled over them; float32, read-only"""
    ch = opt & 0xF
    kinds = HARD_PATTERNS if ch == HARD else STREAM_PATTERNS
    rng = np.random.default_rng(_seed(ch, "stream", nbits))
    share = -(-2 * nbits // len(kinds))
    v = np.concatenate([_codes(ch, kind, share, rng) for kind in kinds])[:2 * nbits]
    _sprinkle(ch, v, nspecials, rng)
    with np.errstate(all="ignore"):
        v = (v.astype(np.float32) / np.float32(scale)).astype(np.float32)
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def byte_frames(kind, S, n=N_FRAMES, seed=None):
    """n frames of S stages of an int8 pattern: int8 [n, 2 S], read-only"""
    rng = np.random.default_rng(_seed("i8", kind, S, n) if seed is None else seed)
    m = 2 * S * n
    if kind == "every_byte":
        perms = [rng.permutation(256) - 128 for _ in range((m + 255) // 256)]
        q = np.concatenate(perms)[:m].astype(np.int8).reshape(n, 2 * S)
        q[:, 0], q[:, 1], q[:, -2], q[:, -1] = -128, 127, 127, -128
    elif kind == "small_bytes":
        q = rng.integers(-3, 4, m).astype(np.int8).reshape(n, 2 * S)
    elif kind == "sat_bytes":
        q = np.where(rng.integers(0, 2, m) == 1, 127, -128).astype(np.int8).reshape(n, 2 * S)
    else:
        raise ValueError(kind)
    q.setflags(write=False)
    return q


# ---- the quantisers as numpy functions on stream * scale: the right one, and the mutants
def _half_away(x):
    return np.copysign(np.floor(np.abs(x) + np.float32(0.5)), x)


def _sym_clip(hi):
    return lambda x: np.clip(np.rint(x), -hi, hi)


def _pm(bit):
    return np.where(bit, np.float32(1.0), np.float32(-1.0))


def _denorm_flush(x):
    return _pm(np.where(np.abs(x) < np.float32(2.0 ** -126), np.float32(0.0), x) > 0)


GOOD = {HARD: lambda x: _pm(x > 0), SOFT4: np.rint, SOFT8: np.rint, SOFT16: np.rint, FP32: lambda x: x}
MUTANTS = {
    HARD: {"ge0": lambda x: _pm(x >= 0), "nan_is_one": lambda x: _pm(np.isnan(x) | (x > 0)), "denorm_flush": _denorm_flush},
    SOFT4: {"trunc": np.trunc, "half_away": _half_away, "floor": np.floor, "sym_clip": _sym_clip(7)},
    SOFT8: {"trunc": np.trunc, "half_away": _half_away, "floor": np.floor, "sym_clip": _sym_clip(127)},
    SOFT16: {"trunc": np.trunc, "half_away": _half_away, "floor": np.floor, "sym_clip": _sym_clip(32767)},
    FP32: {"trunc_each": np.trunc, "rint_each": np.rint, "sym_clamp": lambda x: np.clip(x, -7, 7)},
}


def stream_words(opt, stream, scale):
    """(words, ok) of the oracle's one-chunk decode of a padded or extended stream, as the frame contracts decode it"""
    return vo.decode(opt, vo.pack(opt, stream, scale), input_num=stream.size, nchunks=1, b16_policy=0, nthreads=1)


def mutant_words(opt, stream, scale, quantiser):
    """the oracle's words of the stream quantised by `quantiser` (a function on stream * scale) instead of the packer"""
    with np.errstate(all="ignore"):
        x = np.asarray(stream, dtype=np.float32) * np.float32(scale)
        q = np.asarray(quantiser(x), dtype=np.float32)
    return stream_words(opt, q, 1.0)[0]
