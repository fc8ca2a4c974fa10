"""The value patterns of tests/value_patterns.py on the CPU, with the oracle alone: every pattern keeps the oracle's
metrics in the reference's exact range for every format, family, length and scale the GPU tests of
tests/test_gpu_frame_values.py use, and the patterns tell a wrong quantiser from the right one.

Why the patterns exist.  On the suite's earlier frame inputs -- frames_common.frames(64, S, True, seed=S)[:8], S = 97 and
250, terminated, at SCALE = 40000 (96 words a pair) -- every mutant of value_patterns.MUTANTS changes 0 words, for all
12 pairs: truncation, round half away from zero, floor and a symmetric clip for SOFT4, SOFT8 and SOFT16, truncating or
rounding each value and a symmetric clamp for FP32, `>= 0`, NaN-is-one and a denormal flush for HARD.  (A +-1 codeword
with sigma 0.3 times 40000 saturates SOFT4, SOFT8 and FP32 at every value, and a wrong rounding moves a SOFT16 code by
one unit in about 30,000.)  Swapping np.rint for np.trunc in the quantiser is invisible there; here it fails
test_the_right_quantiser_gives_the_oracles_words.

Words changed by each mutant, of the 192 oracle words per pattern (8 frames each of 97 and 250 stages, terminated and
tail-biting, scale 1.0; measured with the oracle on the CPU).  The best pattern per mutant and pair:

  pair           ge0 / trunc / trunc_each   nan_is_one / half_away / rint_each   denorm_flush / floor / sym_clamp   sym_clip
  HARD|M_B32     185 zero_mix               184 zero_mix                         184 zero_mix
  HARD|M_B16     185 zero_mix               184 zero_mix                         184 zero_mix
  HARD|M_FP16    184 zero_mix               184 zero_mix                         183 zero_mix
  SOFT4|M_B32    177 small                  168 small_halves                     182 small                          184 specials
  SOFT4|M_B16    177 small                  171 small_halves                     181 small                          184 specials
  SOFT4|M_FP16   176 small                  167 small_halves                     182 small                          184 specials
  SOFT8|M_B32    181 small                  165 small_halves                     179 small                          179 specials
  SOFT8|M_B16    180 small                  161 small_halves                     179 small                          180 specials
  SOFT16|M_B32   177 small                  166 small_halves                     179 small_halves                   169 specials
  FP32|M_B32     176 small                  160 small, specials                  100 satrand
  FP32|M_B16     177 small                  161 small                            101 satrand
  FP32|M_FP16    177 small                  162 specials                          93 satrand

Every pattern, for SOFT16|M_B32 (trunc, half_away, floor, sym_clip) and FP32|M_B32 (trunc_each, rint_each, sym_clamp):

  uniform        0,   0,   0,   0       77,  72,  43
  small        177,   0, 177,   0      176, 160,   0
  small_halves 144, 166, 179,   0      143, 147,   0
  halves         0,   0,   0,   0       69,  85,  43
  edge          26,  48,  21,  51       43,  44,  73
  satrand        0,   0,   0,  90        0,   0, 100
  specials     166,  89, 172, 169      168, 160,   0

sym_clip without the huge values of `specials` (which the x86 narrowing wraps and a clip does not): satrand changes 90
(SOFT16) to 109 (SOFT8|M_B16) words.  The smallest best count is 90 of 192; the test asks for a quarter, 48, which
leaves nearly a factor of two for another seed.  HARD `satrand` (+-1) changes nothing under any mutant, as it should."""
import numpy as np
import pytest

import value_patterns as vp
import vitdec as vd

SIZES = [5, 33, 70, 97, 250, 1000]  # (33: the fifth length of the GPU tests' mixed launches)
P23 = (2, 0b01, 0b11)  # (in the mixed launches' table)
PART_BITS = 96


def name(o):
    return f"0x{o:03x}"


def whole_streams(opt, values, S, scale):
    yield "terminated", vd.pad_frame(values, True, scale, opt)
    yield "tail-biting", vd.wrap_frame(values)
    if (opt & 0xF) == vp.HARD:
        return
    yield "open", vd.pad_frame(values, False, scale, opt)
    for p in (P23, vp.P34, vp.P56):
        dep = vd.depuncture(vd.puncture(values, p), p, 2 * S)
        yield f"terminated {p}", vd.pad_frame(dep, True, scale, opt)
        yield f"open {p}", vd.pad_frame(dep, False, scale, opt)
        yield f"tail-biting {p}", vd.wrap_frame(dep)


def family_streams(opt, values, S, scale):
    """(family, stream) of every stream the GPU tests decode the 2 S values as: the padded stream terminated and open,
    the extended stream, the same three of the depunctured values under 2/3, 3/4 and 5/6 (HARD: terminated and
    tail-biting only, the entry points' rule), and at 250 stages the sub-streams of each in parts of 96"""
    for fam, stream in whole_streams(opt, values, S, scale):
        yield fam, stream
        if S == 250:
            for w0, _, sub in vd.frame_parts(stream, PART_BITS):
                yield f"{fam} part at word {w0}", sub


@pytest.mark.parametrize("opt", vp.PAIRS, ids=name)
def test_every_pattern_stays_in_the_exact_metric_range(vo, opt):
    """all 12 pairs x every pattern of the format x S in {5, 33, 70, 97, 250, 1000} x every scale of the pattern (1.0,
    0.37, 40000; 2^100 and 2^-100 too for `small` and `edge`) x every stream family, the five frames the GPU tests
    decode: the oracle's one-chunk decode reports ok.  No pattern needed a reduced amplitude for any format."""
    bad = []
    for kind in vp.patterns(opt):
        for S in SIZES:
            for scale in vp.scales(kind):
                for f, v in enumerate(vp.frames(opt, kind, S, scale)):
                    for fam, stream in family_streams(opt, v, S, scale):
                        if not vp.stream_words(opt, stream, scale)[1]:
                            bad.append((kind, S, scale, f, fam))
    assert not bad, bad[:10]


@pytest.mark.parametrize("opt", [o for o in vp.PAIRS if (o & 0xF) in (vp.HARD, vp.SOFT4, vp.SOFT8)], ids=name)
def test_every_byte_pattern_stays_in_the_exact_metric_range(vo, opt):
    """the int8 patterns as (float)q at the four int8 scales, the same lengths and families"""
    bad = []
    for kind in vp.BYTE_PATTERNS:
        for S in SIZES:
            for scale in vp.BYTE_SCALES:
                for f, q in enumerate(vp.byte_frames(kind, S)):
                    for fam, stream in family_streams(opt, q.astype(np.float32), S, scale):
                        if not vp.stream_words(opt, stream, scale)[1]:
                            bad.append((kind, S, scale, f, fam))
    assert not bad, bad[:10]


@pytest.mark.parametrize("opt", vp.PAIRS, ids=name)
def test_the_stream_inputs_stay_in_the_exact_metric_range(vo, opt):
    """value_patterns.stream at 200,000 bits, scales 1.0 and 0.37, as run_llr decodes it and (not HARD) depunctured
    under 3/4 as run_punct does: the oracle's decode in the default chunks reports ok"""
    for scale in (1.0, 0.37):
        vals = vp.stream(opt, 200_000, scale)
        assert vals.dtype == np.float32 and vals.size == 400_000 and not vals.flags.writeable
        assert vo.decode(opt, vo.pack(opt, vals, scale), input_num=vals.size)[1], scale
        if (opt & 0xF) != vp.HARD:
            dep = vd.depuncture(vd.puncture(vals, vp.P34), vp.P34, vals.size)
            assert vo.decode(opt, vo.pack(opt, dep, scale), input_num=vals.size)[1], (scale, "3/4")


def mutant_streams(opt, kind):
    """the 32 streams of a pattern's 192 words: 8 frames each of 97 and 250 stages, terminated and tail-biting, scale 1.0"""
    for S in (97, 250):
        for v in vp.frames(opt, kind, S, 1.0, n=8):
            yield vd.pad_frame(v, True, 1.0, opt)
            yield vd.wrap_frame(v)


_REFS = {}


def oracle_words(opt, kind):
    """the oracle's own words of mutant_streams(opt, kind), one array, computed once and read-only"""
    if (opt, kind) not in _REFS:
        words = []
        for stream in mutant_streams(opt, kind):
            ref, ok = vp.stream_words(opt, stream, 1.0)
            assert ok
            words.append(ref)
        ref = np.concatenate(words)
        ref.setflags(write=False)
        assert ref.size == 192
        _REFS[opt, kind] = ref
    return _REFS[opt, kind]


def quantised_words(opt, kind, quantiser):
    return np.concatenate([vp.mutant_words(opt, stream, 1.0, quantiser) for stream in mutant_streams(opt, kind)])


@pytest.mark.parametrize("opt", vp.PAIRS, ids=name)
def test_the_right_quantiser_gives_the_oracles_words(vo, opt):
    """the mutants' machinery with the right quantiser in it (rint; FP32: the value itself; HARD: > 0) changes no word of
    any pattern -- so what a mutant changes is the mutant's doing"""
    for kind in vp.patterns(opt):
        got = quantised_words(opt, kind, vp.GOOD[opt & 0xF])
        assert np.array_equal(got, oracle_words(opt, kind)), (kind, int((got != oracle_words(opt, kind)).sum()))


@pytest.mark.parametrize("opt", vp.PAIRS, ids=name)
def test_every_mutant_changes_a_quarter_of_the_words_of_some_pattern(vo, opt):
    """a decoder that quantised like any mutant would fail the word-for-word tests on these patterns: each mutant of the
    format changes at least 48 of the 192 words of at least one pattern (measured: 90 to 185, the module docstring)"""
    for mutant, quantiser in vp.MUTANTS[opt & 0xF].items():
        changed = {kind: int((quantised_words(opt, kind, quantiser) != oracle_words(opt, kind)).sum())
                   for kind in vp.patterns(opt)}
        assert max(changed.values()) >= 192 // 4, (mutant, changed)


def test_patterns_are_float32_read_only_and_repeatable():
    for opt in (vp.HARD, vp.SOFT4, vp.SOFT8, vp.SOFT16, vp.FP32):
        for kind in vp.patterns(opt):
            v = vp.frames(opt, kind, 97, 0.37)
            assert v.dtype == np.float32 and v.shape == (5, 194) and not v.flags.writeable
            vp.frames.cache_clear()
            assert np.array_equal(vp.frames(opt, kind, 97, 0.37), v, equal_nan=True)
    for kind in vp.BYTE_PATTERNS:
        q = vp.byte_frames(kind, 250)
        assert q.dtype == np.int8 and q.shape == (5, 500) and not q.flags.writeable


@pytest.mark.parametrize("ch", [vp.SOFT4, vp.SOFT8, vp.SOFT16])
def test_patterns_reach_what_they_are_named_for(vo, ch):
    """in code units, as the oracle's packer quantises them at scales 1.0 and 0.37: `uniform` holds both saturation codes
    and (SOFT4, SOFT8) every code between, `satrand` nothing but the two, `small_halves` exact ties at scale 1.0, `edge`
    codes on both sides of both limits; `every_byte` all 256 bytes with -128 and 127 at both ends of every frame"""
    hi = vp.HI[ch]
    bits = {vp.SOFT4: 4, vp.SOFT8: 8, vp.SOFT16: 16}[ch]

    def codes(kind, scale):
        v = vp.frames(ch, kind, 250, scale).reshape(-1)
        w = vo.pack(ch, v, scale).view(np.uint32)
        per = 32 // bits
        c = (w[:, None] >> (np.arange(per - 1, -1, -1, dtype=np.uint32) * bits)) & ((1 << bits) - 1)
        c = c.reshape(-1)[:v.size].astype(np.int64)
        return np.where(c > hi, c - (1 << bits), c)

    for scale in (1.0, 0.37):
        uni = codes("uniform", scale)
        assert uni.min() == -hi - 1 and uni.max() == hi
        if ch != vp.SOFT16:
            assert np.unique(codes("uniform", scale)).size >= min(2 * hi + 2, 200)
        assert set(np.unique(codes("satrand", scale))) == {-hi - 1, hi}
        assert {-hi - 1, -hi, -hi + 1, hi - 1, hi} <= set(np.unique(codes("edge", scale)))
    x = vp.frames(ch, "small_halves", 250, 1.0)
    assert np.array_equal(np.abs(x - np.trunc(x)), np.full(x.shape, 0.5, np.float32))
    q = vp.byte_frames("every_byte", 250)
    assert np.unique(q).size == 256
    assert (q[:, 0] == -128).all() and (q[:, 1] == 127).all() and (q[:, -2] == 127).all() and (q[:, -1] == -128).all()
