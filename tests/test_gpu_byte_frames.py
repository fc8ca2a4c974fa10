"""GPU parity of int8 frame decodes (vd_run_byte_frames / vd_run_device_byte_frames; kernels vd_decode_tg<FRM+I8+...>,
the byte twins of the four frame families): every frame of a launch equals, word for word, the oracle's decode of the
frame (float)q by the family's own definition -- frames_common.oracle_frame (of vitdec.depuncture(...) for a punctured
frame), tb_common.oracle_tb_frame, ptb_common.oracle_ptb_frame, parts_common.oracle_parts -- and the float entry point
of the same family on the widened buffer, a second witness.  Inputs: noisy BPSK codewords quantised as
clip(rint(32 v), -128, 127), scale 1.0 (SOFT8, HARD) or 0.25 (SOFT4), unless a test says otherwise.  Every buffer a
device launch reads lies inside bytes of alternating 127 and -128, every output inside sentinel bytes 0xA5.  The byte
geometry alone: tests/test_byte_frames.py."""
import numpy as np
import pytest

from frames_common import SIGMA, frame_bits, frames, oracle_frame
from parts_common import oracle_parts, stream_of
from ptb_common import P16, P34, PNONE, oracle_ptb_frame
from tb_common import TB_SIZES, oracle_tb_frame, tb_frames
from vitdec import FP32, HARD, M_B16, M_B32, M_FP16, O_B16, SOFT4, SOFT8, SOFT16

OPEN, TERM, TB = 0, 1, 2
KIND_NAMES = {OPEN: "open", TERM: "term", TB: "tb"}
PLAIN = (1, 1, 1)
OPTIONS = [SOFT8 | M_B16, SOFT8 | M_B32 | O_B16, SOFT4 | M_FP16, HARD | M_B32]
# (kind, pattern): the four kernel families, both pad kinds of the two padded ones
FAMILIES = [(TERM, PLAIN), (OPEN, PLAIN), (TB, PLAIN), (TERM, P34), (OPEN, P34), (TB, P34), (OPEN, P16), (TB, P16)]
FOUR = [(TERM, PLAIN), (TB, PLAIN), (OPEN, P34), (TB, P34)]  # one of each family
SENTINEL = 0xA5


def name(o):
    return f"0x{o:03x}"


def scale_of(opt):
    return 0.25 if (opt & 0xF) == SOFT4 else 1.0


def allowed(opt, fam):
    """HARD decodes terminated and tail-biting frames under (1, 1, 1) only"""
    kind, pattern = fam
    return (opt & 0xF) != HARD or (kind != OPEN and pattern == PLAIN)


def fid(fam):
    return f"{KIND_NAMES[fam[0]]}-p{fam[1][0]}-{fam[1][1]:x}-{fam[1][2]:x}"


def quantise(v):
    return np.clip(np.rint(32.0 * np.asarray(v, dtype=np.float32)), -128, 127).astype(np.int8)


def short_frame(S, terminated, seed):
    """frames_common.frames(1, S, terminated, seed) for S < 7, which its encoder does not take: the encoder started
    in state 0, fewer stages than taps"""
    rng = np.random.default_rng(seed)
    bits = frame_bits(1, S, terminated, rng)[0]
    out = np.zeros((S, 2), dtype=np.uint8)
    for col, poly in enumerate((0o171, 0o133)):
        for k in range(S):
            if (poly >> (6 - k)) & 1:
                out[k:, col] ^= bits[:S - k]
    return (np.where(out.reshape(-1) == 1, 1.0, -1.0) + rng.normal(0.0, SIGMA, 2 * S)).astype(np.float32)


def codeword(kind, S, seed):
    """the 2 S int8 values of one noisy frame of the kind"""
    if kind == TB:
        return quantise(tb_frames(1, S, seed)[1][0])
    return quantise(frames(1, S, kind == TERM, seed)[1][0] if S >= 7 else short_frame(S, kind == TERM, seed))


def received(vd, q, pattern):
    """the kept bytes of a frame's 2 S values"""
    q = np.asarray(q, dtype=np.int8)
    return q if pattern == PLAIN else vd.puncture(q, pattern).astype(np.int8)


_REFS = {}


def oracle_byte_frame(vd, opt, rx, kind, pattern, S, scale):
    """the words that define the decode of one int8 frame of S stages from its kept bytes: the oracle on (float)q,
    computed once per frame"""
    rx = np.asarray(rx, dtype=np.int8)
    key = (opt, kind, pattern, S, scale, rx.tobytes())
    if key not in _REFS:
        v = rx.astype(np.float32)
        if kind == TB:
            ref = oracle_tb_frame(vd, opt, v, scale) if pattern == PLAIN else oracle_ptb_frame(vd, opt, v, pattern, S, scale)
        else:
            ref = oracle_frame(vd, opt, v if pattern == PLAIN else vd.depuncture(v, pattern, 2 * S), kind == TERM, scale)
        ref.setflags(write=False)
        _REFS[key] = ref
    return _REFS[key]


def poison(n):
    """n bytes of alternating 127 and -128: what no frame may read"""
    p = np.empty(n, dtype=np.int8)
    p[0::2] = 127
    p[1::2] = -128
    return p


def device_frames(vd, d, rxs, kind, pattern, max_bits, scale, lens=None, q_lead=16, q_stride=None):
    """run_device_byte_frames of the frames rxs (their kept bytes; frame f has lens[f] stages, max_bits when lens is
    None) at q_lead bytes into a buffer of poison, q_stride bytes apart (default: back to back, the bytes of a
    max_bits frame), into a buffer of sentinel bytes.  Returns (the bytes each frame wrote, whether every other output
    byte kept the sentinel)."""
    import torch
    n = len(rxs)
    need = vd.punctured_len(pattern, 2 * max_bits)
    q_stride = need if q_stride is None else q_stride
    host = poison(q_lead + (n - 1) * q_stride + need + 64)
    for f, rx in enumerate(rxs):
        assert rx.size <= need and rx.dtype == np.int8
        host[q_lead + f * q_stride: q_lead + f * q_stride + rx.size] = rx
    inp = torch.from_numpy(host).cuda()
    row = 4 * ((max_bits + 31) // 32)
    ostride = row + 8
    out = torch.full((8 + n * ostride + 16,), SENTINEL, dtype=torch.uint8, device="cuda")
    lens_d = None
    if lens is not None:
        lens_d = torch.from_numpy(np.asarray(lens, dtype=np.uint32).view(np.int32)).cuda()
    assert inp.data_ptr() % 256 == 0 and out.data_ptr() % 4 == 0
    d.run_device_byte_frames(inp.data_ptr() + q_lead, q_stride, out.data_ptr() + 8, ostride, max_bits, n, kind, pattern, scale,
                             frame_bits_ptr=lens_d.data_ptr() if lens_d is not None else 0,
                             stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    untouched = np.ones(got.size, dtype=bool)
    words = []
    for f in range(n):
        S = min(int(lens[f]), max_bits) if lens is not None else max_bits
        nb = 4 * ((S + 31) // 32)
        lo = 8 + f * ostride
        words.append(got[lo:lo + nb].copy())
        untouched[lo:lo + nb] = False
    return words, bool((got[untouched] == SENTINEL).all())


def check_launch(vd, d, opt, fam, sizes, max_bits, scale, seed0=0, part_bits=0, **layout):
    """one device launch of a codeword frame per size (0: an empty frame) against the oracle of each frame alone"""
    kind, pattern = fam
    rxs = [received(vd, codeword(kind, S, seed0 + S), pattern) if S else np.zeros(0, dtype=np.int8) for S in sizes]
    words, clean = device_frames(vd, d, rxs, kind, pattern, max_bits, scale, lens=sizes, **layout)
    for S, rx, w in zip(sizes, rxs, words):
        if not S:
            assert w.size == 0
            continue
        if part_bits:
            ref = oracle_parts(vd, opt, stream_of(vd, opt, KIND_NAMES[kind], rx.astype(np.float32), S,
                                                  None if pattern == PLAIN else pattern, scale), part_bits, scale)
        else:
            ref = oracle_byte_frame(vd, opt, rx, kind, pattern, S, scale)
        assert np.array_equal(w.view(ref.dtype), ref), (fid(fam), S, part_bits, np.flatnonzero(w.view(ref.dtype) != ref)[:5])
    assert clean, (fid(fam), "a byte outside the frames' words was written")


def float_twin(d, rx, kind, pattern, S, scale):
    """the float entry point of the family on the widened rows rx [n, L]"""
    v = rx.astype(np.float32)
    if pattern == PLAIN:
        return d.run_tb_frames(v, scale)[0] if kind == TB else d.run_frames(v, kind == TERM, scale)[0]
    if kind == TB:
        return d.run_punct_tb_frames(v, pattern, S, scale)[0]
    return d.run_punct_frames(v, pattern, S, kind == TERM, scale)[0]


# ---------------------------------------------------------------- 1. lengths
@pytest.mark.gpu
@pytest.mark.parametrize("opt", OPTIONS, ids=name)
def test_lengths_of_one_launch_between_poison_and_sentinels(gpu, vd, opt):
    """maxFrameBits = 1000 and a device lengths array of the 20 sizes of TB_SIZES plus 0 (21 frames, 6 workgroups), a
    launch per family at (1, 1, 1), 3/4 and the period-16 pattern, and one of frames of 1, 2, 5 and 0 stages under
    (16, 0x8000, 0), which hold no byte at all: every frame's words equal the oracle's, every other output byte keeps
    its sentinel"""
    sizes = list(TB_SIZES) + [0]
    assert len(sizes) == 21
    with vd.ViterbiCUDA(opt) as d:
        for fam in FAMILIES:
            if allowed(opt, fam):
                check_launch(vd, d, opt, fam, sizes, 1000, scale_of(opt))
        for kind in (TERM, OPEN, TB):
            if allowed(opt, (kind, PNONE)):
                assert vd.punctured_len(PNONE, 30) == 0
                check_launch(vd, d, opt, (kind, PNONE), [1, 2, 5, 0], 15, scale_of(opt), q_stride=3)


# ---------------------------------------------------------------- 2. values
def value_frames(S, rng):
    """four frames of 2 S int8 values: uniform over the full range with both ends present, tie-dense over {-1, 0, 1},
    constant -128, constant 127"""
    uni = rng.integers(-128, 128, 2 * S, dtype=np.int16).astype(np.int8)
    uni[3], uni[4], uni[2 * S - 1], uni[2 * S - 2] = -128, 127, 127, -128
    ties = rng.integers(-1, 2, 2 * S, dtype=np.int16).astype(np.int8)
    return np.stack([uni, ties, np.full(2 * S, -128, dtype=np.int8), np.full(2 * S, 127, dtype=np.int8)])


@pytest.mark.gpu
@pytest.mark.parametrize("scale", [1.0, 0.25, 4.0])
@pytest.mark.parametrize("opt", OPTIONS, ids=name)
def test_values_equal_the_oracle_and_the_float_entry_point(gpu, vd, opt, scale):
    """sign extension (-128 and 127 in both bytes of a pair), the byte order inside the 16-bit load (frames that are
    not symmetric in their two outputs), saturation (scale 4.0 on SOFT8, 1.0 on SOFT4) and ties"""
    with vd.ViterbiCUDA(opt) as d:
        for S in (97, 250):
            q = value_frames(S, np.random.default_rng(1000 * S + int(8 * scale)))
            for fam in FOUR:
                if not allowed(opt, fam):
                    continue
                kind, pattern = fam
                rx = np.stack([received(vd, r, pattern) for r in q])
                ref = np.stack([oracle_byte_frame(vd, opt, r, kind, pattern, S, scale) for r in rx])
                host, _ = d.run_byte_frames(rx, kind, pattern, S, scale)
                assert host.dtype == ref.dtype and np.array_equal(host, ref), (fid(fam), S, np.argwhere(host != ref)[:5])
                twin = float_twin(d, rx, kind, pattern, S, scale)
                assert np.array_equal(host, twin), (fid(fam), S, np.argwhere(host != twin)[:5])
                words, clean = device_frames(vd, d, list(rx), kind, pattern, S, scale)
                assert clean and all(np.array_equal(w.view(ref.dtype), r) for w, r in zip(words, ref)), (fid(fam), S)


# ---------------------------------------------------------------- 3. nothing outside the frame is read
@pytest.mark.gpu
@pytest.mark.parametrize("opt", OPTIONS, ids=name)
def test_nothing_outside_a_frame_is_read(gpu, vd, opt):
    """frames back to back (q_stride exactly the bytes of a maxFrameBits frame), each shorter than the maximum, the
    slack and the bytes before the first and after the last frame alternating 127 and -128: a read of them -- a virtual
    stage, a punctured value or a stage past the frame's end that the range check lets through, a wrap that leaves the
    frame -- puts an extreme value into the table and changes the words.  An open frame of one stage reads 2 bytes and
    decodes erasures from there on; each frame equals the oracle of that frame alone"""
    sizes = [1, 26, 70, 97, 166]
    with vd.ViterbiCUDA(opt) as d:
        for fam in FAMILIES:
            if allowed(opt, fam):
                check_launch(vd, d, opt, fam, sizes, 167, scale_of(opt), seed0=50)
                check_launch(vd, d, opt, fam, [1], 1, scale_of(opt), seed0=60)  # one frame of one stage, nothing after it


# ---------------------------------------------------------------- 4. alignment
@pytest.mark.gpu
@pytest.mark.parametrize("opt", OPTIONS, ids=name)
def test_alignment(gpu, vd, opt):
    """the punctured families at an odd address with an odd stride, the unpunctured ones at q_d + 2 with a stride that
    is 2 mod 4; an odd pointer or stride under (1, 1, 1) is VD_ERR_ARG"""
    sizes = [97, 33, 166, 5, 167]
    with vd.ViterbiCUDA(opt) as d:
        for fam in FAMILIES:
            if not allowed(opt, fam):
                continue
            if fam[1] == PLAIN:
                check_launch(vd, d, opt, fam, sizes, 167, scale_of(opt), seed0=70, q_lead=2, q_stride=2 * 167 + 4)
                assert (2 * 167 + 4) % 4 == 2
            else:
                odd = vd.punctured_len(fam[1], 2 * 167) + 2
                odd += 1 - odd % 2
                check_launch(vd, d, opt, fam, sizes, 167, scale_of(opt), seed0=70, q_lead=1, q_stride=odd)
        for kind in (TERM, TB):
            for kw in (dict(q_ptr=4097), dict(q_stride=335), dict(q_ptr=4099, q_stride=337)):
                a = dict(q_ptr=4096, q_stride=336, output_ptr=4096, output_stride=24, maxFrameBits=167, nframes=4, kind=kind,
                         pattern=PLAIN, scale=1.0)
                a.update(kw)
                with pytest.raises(vd.VitdecError, match="VD_ERR_ARG.*multiples of 2"):  # (checked before any pointer is used)
                    d.run_device_byte_frames(**a)


# ---------------------------------------------------------------- 5. parts
@pytest.mark.gpu
@pytest.mark.parametrize("part_bits", [96, 192])
@pytest.mark.parametrize("opt", OPTIONS, ids=name)
def test_frames_in_parts(gpu, vd, opt, part_bits):
    """set_frame_part_bits is honoured as by the float entry points: frames of 97, 300 and 1000 stages in one launch,
    all four families, each frame against oracle_parts of its padded or extended stream"""
    with vd.ViterbiCUDA(opt) as d:
        d.set_frame_part_bits(part_bits)
        for fam in FOUR + [(OPEN, PLAIN), (TERM, P34)]:
            if allowed(opt, fam):
                check_launch(vd, d, opt, fam, [97, 300, 1000], 1000, scale_of(opt), seed0=80, part_bits=part_bits)
        nm = d.kernel_for(1000, 3, 7)
        assert nm.startswith("vd_decode_tg<FRM+I8+") and f"{-(-32 // (part_bits // 32))} parts per frame" in nm, nm


# ---------------------------------------------------------------- 6. errors and names
@pytest.mark.gpu
def test_errors(gpu, vd):
    q = np.zeros((4, 500), dtype=np.int8)
    ok = dict(q_ptr=4096, q_stride=500, output_ptr=4096, output_stride=32, maxFrameBits=250, nframes=4, kind=TERM,
              pattern=PLAIN, scale=1.0)
    for opt in (SOFT16 | M_B32, FP32 | M_FP16, FP32 | M_B16 | O_B16):
        with vd.ViterbiCUDA(opt) as d:
            for kind in (OPEN, TERM, TB):
                with pytest.raises(vd.VitdecError, match="VD_ERR_OPTIONS.*SOFT16 or FP32"):
                    d.run_byte_frames(q, kind)
                with pytest.raises(vd.VitdecError, match="VD_ERR_OPTIONS.*SOFT16 or FP32"):
                    d.run_device_byte_frames(**dict(ok, kind=kind))  # (checked before any pointer is used)
    with vd.ViterbiCUDA(HARD | M_B32) as d:
        with pytest.raises(vd.VitdecError, match="VD_ERR_OPTIONS.*open frames on a HARD"):
            d.run_byte_frames(q, OPEN)
        for kind in (OPEN, TERM, TB):
            with pytest.raises(vd.VitdecError, match="VD_ERR_OPTIONS.*HARD"):
                d.run_byte_frames(q[:, :334], kind, P34, 250)
            with pytest.raises(vd.VitdecError, match="VD_ERR_OPTIONS.*HARD"):
                d.run_device_byte_frames(**dict(ok, kind=kind, pattern=(2, 3, 3)))  # keep-all, but not (1, 1, 1)
    with vd.ViterbiCUDA(SOFT8 | M_B16) as d:
        bad = [dict(kind=3), dict(kind=-1), dict(pattern=(0, 1, 1)), dict(pattern=(17, 1, 1)), dict(pattern=(3, 0b1000, 0b011)),
               dict(pattern=(3, 0, 0)), dict(q_stride=498), dict(q_stride=0), dict(output_stride=28), dict(output_stride=30),
               dict(pattern=P34, q_stride=333), dict(maxFrameBits=0), dict(maxFrameBits=(1 << 20) + 1, q_stride=4 << 20, output_stride=1 << 18),
               dict(nframes=0), dict(nframes=-1), dict(scale=0.0), dict(scale=-1.0), dict(scale=float("inf")), dict(scale=float("nan")),
               dict(scale=1e-40), dict(kind=TB, scale=0.0), dict(kind=TB, scale=float("inf")), dict(q_ptr=0), dict(output_ptr=0)]
        for kw in bad:
            with pytest.raises(vd.VitdecError, match="VD_ERR_ARG"):
                d.run_device_byte_frames(**dict(ok, **kw))
        with pytest.raises(vd.VitdecError, match="VD_ERR_ARG.*kind"):
            d.run_byte_frames(q, 3)
        with pytest.raises(vd.VitdecError, match="VD_ERR_ARG.*frames would overlap"):
            d.run_device_byte_frames(**dict(ok, q_stride=498))
        with pytest.raises(vd.VitdecError, match="maxFrameBits must be given"):
            d.run_byte_frames(q, TERM, P34)
        with pytest.raises(vd.VitdecError, match="rows of 333 values"):
            d.run_byte_frames(q[:, :333], TERM, P34, 250)
        d.set_frame_part_bits(96)
        with pytest.raises(vd.VitdecError, match="VD_ERR_ARG.*workgroups"):
            d.run_device_byte_frames(**dict(ok, maxFrameBits=1 << 20, q_stride=2 << 20, output_stride=1 << 17, nframes=0x7FFFFFFF))


@pytest.mark.gpu
def test_kernel_names(gpu, vd):
    """llr 7 .. 10: the float twin's name (llr 3 .. 6) with I8+ after FRM+, "-" where the call is refused"""
    for opt in OPTIONS + [SOFT4 | M_B32 | O_B16, HARD | M_FP16]:
        with vd.ViterbiCUDA(opt) as d:
            for part_bits in (0, 96):
                d.set_frame_part_bits(part_bits)
                for k in range(4):
                    for n in (1, 5, 10_000):
                        twin, byte = d.kernel_for(1000, n, 3 + k), d.kernel_for(1000, n, 7 + k)
                        assert byte == ("-" if twin == "-" else twin.replace("FRM+", "FRM+I8+", 1)), (name(opt), k, byte, twin)
                        assert (byte == "-") == ((opt & 0xF) == HARD and k in (1, 3))
                    assert d.kernel_for(0, 4, 7 + k) == "-" and d.kernel_for((1 << 20) + 1, 4, 7 + k) == "-"
    with vd.ViterbiCUDA(SOFT8 | M_B16) as d:
        assert d.kernel_for(1000, 4, 10).startswith("vd_decode_tg<FRM+I8+TB+PUN+SOFT8,B16,O32> one frame per wave, ")
        assert d.kernel_for(1000, 4, 7).startswith("vd_decode_tg<FRM+I8+SOFT8,B16,O32> one frame per wave, ")
        assert d.kernel_for(1000, 4, 3).startswith("vd_decode_tg<FRM+SOFT8,")  # the earlier names stay
    for opt in (SOFT16 | M_B32, FP32 | M_FP16, FP32 | M_B32 | O_B16):
        with vd.ViterbiCUDA(opt) as d:
            assert [d.kernel_for(1000, 4, llr) for llr in (7, 8, 9, 10)] == ["-"] * 4
            assert d.kernel_for(1000, 4, 3).startswith("vd_decode_tg<FRM+")


# ---------------------------------------------------------------- 7. host and device variants
@pytest.mark.gpu
@pytest.mark.parametrize("opt", OPTIONS, ids=name)
def test_host_and_device_variants_give_the_same_bytes(gpu, vd, opt):
    """run_byte_frames and run_device_byte_frames over the same rows, lengths and zeroed outputs: the same bytes, the
    ones no frame writes (short and empty frames) included"""
    import torch
    lens, max_bits = [250, 0, 97, 33, 1, 250, 166], 250
    with vd.ViterbiCUDA(opt) as d:
        for fam in FOUR:
            if not allowed(opt, fam):
                continue
            kind, pattern = fam
            L = vd.punctured_len(pattern, 2 * max_bits)
            rows = np.zeros((len(lens), L), dtype=np.int8)
            for f, S in enumerate(lens):
                rx = received(vd, codeword(kind, S, 90 + S), pattern) if S else np.zeros(0, dtype=np.int8)
                rows[f, :rx.size] = rx
            host, _ = d.run_byte_frames(rows, kind, pattern, max_bits, scale_of(opt), frame_bits=lens)
            inp = torch.from_numpy(rows.reshape(-1)).cuda()
            out = torch.zeros(host.nbytes, dtype=torch.uint8, device="cuda")
            lens_d = torch.from_numpy(np.asarray(lens, dtype=np.uint32).view(np.int32)).cuda()
            d.run_device_byte_frames(inp.data_ptr(), L, out.data_ptr(), host.nbytes // len(lens), max_bits, len(lens), kind,
                                     pattern, scale_of(opt), frame_bits_ptr=lens_d.data_ptr(),
                                     stream=torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            assert np.array_equal(out.cpu().numpy(), host.view(np.uint8).reshape(-1)), fid(fam)
            for f, S in enumerate(lens):
                nw = (S + 31) // 32 * (host.shape[1] // ((max_bits + 31) // 32))
                if S:
                    ref = oracle_byte_frame(vd, opt, rows[f, :vd.punctured_len(pattern, 2 * S)], kind, pattern, S, scale_of(opt))
                    assert np.array_equal(host[f, :nw], ref), (fid(fam), f)
                assert not host[f, nw:].any(), (fid(fam), f)


# ---------------------------------------------------------------- 8. LDS guard
@pytest.mark.gpu
@pytest.mark.parametrize("opt", OPTIONS, ids=name)
def test_lds_guard_words_stay_intact(gpu, vd, opt):
    with vd.ViterbiCUDA(opt) as d:
        d.set_guard_check(True)
        for fam in FOUR:
            if allowed(opt, fam):
                check_launch(vd, d, opt, fam, [1000] * 13, 1000, scale_of(opt), seed0=100)
        assert d.guard_violations() == 0
