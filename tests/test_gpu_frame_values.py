"""GPU parity of every float and int8 entry point on values for which the quantiser decides the words: the patterns of
tests/value_patterns.py -- full-range, rounding-edge, saturation-edge and special values, in code units of the
decoder's format, at scales 1.0, 0.37 (an inexact product), 40000 and for `small` and `edge` 2^100 and 2^-100 -- through
run_frames, run_punct_frames, run_tb_frames, run_punct_tb_frames, run_mixed_frames, frames in parts, run_byte_frames,
run_byte_mixed_frames, their device twins, and the stream entry points run_llr, run_punct and run_device_llr_batch.
tests/test_value_patterns.py shows on the CPU that a decoder which truncated, rounded half away from zero, floored,
saturated symmetrically, flushed a denormal or read a zero or NaN as 1 would fail here, and that none of that shows on
the noisy +-1 codewords at scale 40000 every other frame test decodes.

The method is the suite's: every frame of a launch equals, word for word, the oracle's decode of that frame alone by the
family's own definition -- frames_common.oracle_frame (of vitdec.depuncture(...) for a punctured frame),
tb_common.oracle_tb_frame, ptb_common.oracle_ptb_frame, parts_common.oracle_parts over vitdec.frame_parts,
test_gpu_mixed_frames.oracle_of -- each of which asserts that the oracle stayed in the reference's exact metric range.
Launches hold five frames (a full workgroup of four waves and a partial one) of 5 stages (shorter than the 26-stage
lead), 70 (26 + 70 = 96: the frame ends at the first group boundary), 97 (one stage past a group and past three
words) and 250 (a partial last word), the smallest lengths at which the load paths differ.  The oracle's words are
computed once per (family, option, pattern, length, scale).

Measured once on an MI355X with a scratch build of the library whose quantisers were wrong in four ways at once (SOFT4
and SOFT8: truncation instead of rint in TgInLlr::soft; SOFT16: saturation to [-32767, 32767]; FP32: a clamp to [-7, 7];
HARD: v >= 0): of the 362 cases of test_gpu_frames.py, test_gpu_tb_frames.py, test_gpu_punct_frames.py,
test_gpu_punct_tb_frames.py and test_gpu_byte_frames.py 323 passed -- every SOFT4 and SOFT8 case of the four float
families among them; the truncation showed only in the int8 tests at scale 0.25 -- while all 167 frame cases of this
file failed (sections 1 to 4).

Left out: the split packed launch with float input needs 13M bits a case (tests/test_gpu_ties.py and
tests/test_gpu_llr.py run it on their own inputs); NaN into FP32 decoders, whose branch metric the reference leaves
undefined (non-finite specials are +-1e30 there)."""
import numpy as np
import pytest

import value_patterns as vp
from frames_common import oracle_frame
from parts_common import oracle_parts, stream_of
from ptb_common import oracle_ptb_frame
from tb_common import oracle_tb_frame
from test_gpu_byte_frames import device_frames as device_byte_frames
from test_gpu_byte_frames import float_twin, oracle_byte_frame
from test_gpu_mixed_frames import device_launch as device_mixed_launch
from test_gpu_mixed_frames import oracle_of, zeros_of
from test_gpu_ties import LLR_OPTS, _differ, _to_device
from vitdec import FP32, HARD, M_B16, M_B32, M_FP16, O_B16, SOFT4, SOFT8, SOFT16

OPEN, TERM, TB = 0, 1, 2
FAMILY = {OPEN: "open", TERM: "term", TB: "tb"}
PLAIN, P23, P34, P56 = (1, 1, 1), (2, 0b01, 0b11), vp.P34, vp.P56
TABLE = [PLAIN, P23, P34, P56]
# the 12 channel x metric pairs, and 16-bit output words on one pair of each tagged core
OPTIONS = vp.PAIRS + [SOFT8 | M_B32 | O_B16, FP32 | M_FP16 | O_B16, SOFT4 | M_B16 | O_B16]
SOFT_OPTIONS = [o for o in OPTIONS if (o & 0xF) != HARD]
BYTE_OPTIONS = [o for o in OPTIONS if (o & 0xF) in (HARD, SOFT4, SOFT8)]
BYTE_SOFT_OPTIONS = [o for o in BYTE_OPTIONS if (o & 0xF) != HARD]
SIZES = [5, 70, 97, 250]
PART_BITS, PART_S = 96, 250  # three parts of 3, 3 and 2 words
PART_PAIRS = [SOFT8 | M_B16, SOFT4 | M_FP16, SOFT16 | M_B32, FP32 | M_B32, HARD | M_B16]
SENTINEL = 0xA5


def name(o):
    return f"0x{o:03x}"


def kinds_of(opt):
    """the frame kinds a decoder takes: no open frames on HARD"""
    return [TERM, TB] if (opt & 0xF) == HARD else [OPEN, TERM, TB]


def value_cases(opt):
    """(pattern, scale) of every float pattern of the format at every scale it is run at"""
    return [(vkind, scale) for vkind in vp.patterns(opt) for scale in vp.scales(vkind)]


def oracle_one(vd, opt, kind, rx, pattern, S, scale, part_bits=0):
    """the words that define one frame of S stages of the kind from its values (pattern None) or kept values"""
    if part_bits:
        return oracle_parts(vd, opt, stream_of(vd, opt, FAMILY[kind], rx, S, pattern, scale), part_bits, scale)
    if pattern is None:
        return oracle_tb_frame(vd, opt, rx, scale) if kind == TB else oracle_frame(vd, opt, rx, kind == TERM, scale)
    if kind == TB:
        return oracle_ptb_frame(vd, opt, rx, pattern, S, scale)
    return oracle_frame(vd, opt, vd.depuncture(rx, pattern, 2 * S), kind == TERM, scale)


_REFS = {}


def received(vd, opt, vkind, S, scale, pattern):
    """the five frames of a value pattern as the entry point takes them: [5, 2 S], or punctured [5, punctured_len]"""
    vals = vp.frames(opt, vkind, S, scale)
    return vals if pattern is None else np.stack([vd.puncture(v, pattern) for v in vals])


def reference(vd, opt, kind, pattern, vkind, S, scale, part_bits=0):
    """oracle_one of the five frames of a value pattern: [5, words], computed once, read-only"""
    key = (opt, kind, pattern, vkind, S, scale, part_bits)
    if key not in _REFS:
        ref = np.stack([oracle_one(vd, opt, kind, rx, pattern, S, scale, part_bits)
                        for rx in received(vd, opt, vkind, S, scale, pattern)])
        ref.setflags(write=False)
        _REFS[key] = ref
    return _REFS[key]


def same(got, ref, *tag):
    assert got.dtype == ref.dtype and got.shape == ref.shape, tag
    assert np.array_equal(got, ref), (tag, np.argwhere(got != ref)[:5].tolist())


def host_frames(d, kind, pattern, rows, S, scale):
    """the blocking host entry point of the family on rows [n, L] of frames of S stages"""
    if pattern is None:
        return d.run_tb_frames(rows, scale)[0] if kind == TB else d.run_frames(rows, kind == TERM, scale)[0]
    if kind == TB:
        return d.run_punct_tb_frames(rows, pattern, S, scale)[0]
    return d.run_punct_frames(rows, pattern, S, kind == TERM, scale)[0]


def uniform_family(vd, opt, kind, patterns, part_bits=0, sizes=SIZES):
    """every value pattern and scale of the format, every length, five frames a launch, against the oracle"""
    with vd.ViterbiCUDA(opt) as d:
        d.set_frame_part_bits(part_bits)
        for pattern in patterns:
            for S in sizes:
                for vkind, scale in value_cases(opt):
                    got = host_frames(d, kind, pattern, received(vd, opt, vkind, S, scale, pattern), S, scale)
                    same(got, reference(vd, opt, kind, pattern, vkind, S, scale, part_bits), FAMILY[kind], pattern, vkind, S, scale)


# ---------------------------------------------------------------- 1. the four float families
@pytest.mark.gpu
@pytest.mark.parametrize("case", [(o, k) for o in OPTIONS for k in (TERM, OPEN) if k in kinds_of(o)],
                         ids=lambda c: f"{name(c[0])}-{FAMILY[c[1]]}")
def test_frames(gpu, vd, case):
    """run_frames, terminated and open (the pad -65536 / scale and the +0.0 erasures next to the values)"""
    uniform_family(vd, case[0], case[1], [None])


@pytest.mark.gpu
@pytest.mark.parametrize("case", [(o, k) for o in SOFT_OPTIONS for k in (TERM, OPEN)], ids=lambda c: f"{name(c[0])}-{FAMILY[c[1]]}")
def test_punct_frames(gpu, vd, case):
    """run_punct_frames under 3/4 and 5/6: +0.0 at the punctured positions between the values"""
    uniform_family(vd, case[0], case[1], [P34, P56])


@pytest.mark.gpu
@pytest.mark.parametrize("opt", OPTIONS, ids=name)
def test_tb_frames(gpu, vd, opt):
    uniform_family(vd, opt, TB, [None])


@pytest.mark.gpu
@pytest.mark.parametrize("opt", SOFT_OPTIONS, ids=name)
def test_punct_tb_frames(gpu, vd, opt):
    uniform_family(vd, opt, TB, [P34, P56])


# ---------------------------------------------------------------- 2. mixed launches
LENS = [250, 5, 97, 70, 33]


def mixed_launch(vd, d, opt, kind, i8, lens, rates, vkinds, scale, part_bits=0):
    """one host launch of len(lens) frames back to back by mixed_layout, frame f of lens[f] stages under TABLE[rates[f]]
    holding frame f of value pattern vkinds[f]; every frame against the oracle of that frame alone.  Returns (kept
    values of every frame, offsets, total, the launch's words)."""
    rxs = []
    for f, (S, r, vkind) in enumerate(zip(lens, rates, vkinds)):
        if i8:
            rxs.append(vd.puncture(vp.byte_frames(vkind, S)[f].astype(np.float32), TABLE[r]).astype(np.int8))
        else:
            rxs.append(vd.puncture(vp.frames(opt, vkind, S, scale)[f], TABLE[r]))
    offs, total = vd.mixed_layout(lens, rates, TABLE)
    flat = np.concatenate(rxs)
    assert flat.size == total
    run = d.run_byte_mixed_frames if i8 else d.run_mixed_frames
    host, _ = run(flat, kind, max(lens), scale, frame_bits=lens, rates=rates, offsets=offs)
    per = 2 if (opt & 0xF00) == O_B16 else 1
    for f, rx in enumerate(rxs):
        nw = (lens[f] + 31) // 32 * per
        if part_bits:
            ref = oracle_one(vd, opt, kind, rx.astype(np.float32), TABLE[rates[f]], lens[f], scale, part_bits)
        else:
            ref = oracle_of(vd, opt, kind, rx, TABLE[rates[f]], lens[f], scale)
        same(host[f, :nw], ref, FAMILY[kind], f, lens[f], TABLE[rates[f]], vkinds[f], scale)
        assert not host[f, nw:].any(), (FAMILY[kind], f)
    if i8:  # the float entry point on the widened buffer
        twin, _ = d.run_mixed_frames(flat.astype(np.float32), kind, max(lens), scale, frame_bits=lens, rates=rates, offsets=offs)
        same(twin, host, FAMILY[kind], "float twin", vkinds, scale)
    return rxs, offs, total, host


def mixed_rounds(kinds, scales_of):
    """(vkinds of the five frames, scale): round i gives frame f pattern kinds[(i + f) % len(kinds)], so every frame
    place, length and rate meets every pattern at every scale all of a launch's patterns are run at"""
    for i in range(len(kinds)):
        vkinds = [kinds[(i + f) % len(kinds)] for f in range(len(LENS))]
        for scale in scales_of:
            yield i, vkinds, scale


@pytest.mark.gpu
@pytest.mark.parametrize("kind", [OPEN, TERM, TB], ids=FAMILY.get)
@pytest.mark.parametrize("opt", SOFT_OPTIONS, ids=name)
def test_mixed_frames(gpu, vd, opt, kind):
    """run_mixed_frames under the table [(1, 1, 1), 2/3, 3/4, 5/6] read at run time: five frames of different rates and
    lengths back to back, each another value pattern; `small` and `edge` alternating at 2^100 and 2^-100"""
    with vd.ViterbiCUDA(opt) as d:
        d.set_frame_patterns(TABLE)
        for i, vkinds, scale in mixed_rounds(vp.SOFT_PATTERNS, vp.SCALES):
            mixed_launch(vd, d, opt, kind, False, LENS, [(i + f) % 4 for f in range(5)], vkinds, scale)
        for i, vkinds, scale in mixed_rounds(["small", "edge"], vp.EXTREME_SCALES):
            mixed_launch(vd, d, opt, kind, False, LENS, [(i + f) % 4 for f in range(5)], vkinds, scale)


# ---------------------------------------------------------------- 3. frames in parts
@pytest.mark.gpu
@pytest.mark.parametrize("opt", PART_PAIRS, ids=name)
def test_frames_in_parts(gpu, vd, opt):
    """set_frame_part_bits(96) on frames of 250 stages: three parts, the 26 + 38 stages around each part boundary inside
    the values; terminated, tail-biting, punctured tail-biting and mixed terminated frames (HARD: the first two)
    against the oracle of vitdec.frame_parts"""
    uniform_family(vd, opt, TERM, [None], PART_BITS, [PART_S])
    uniform_family(vd, opt, TB, [None], PART_BITS, [PART_S])
    if (opt & 0xF) == HARD:
        return
    uniform_family(vd, opt, TB, [P34, P56], PART_BITS, [PART_S])
    with vd.ViterbiCUDA(opt) as d:
        d.set_frame_patterns(TABLE)
        d.set_frame_part_bits(PART_BITS)
        assert "3 parts per frame" in d.kernel_for(PART_S, 5, 11), d.kernel_for(PART_S, 5, 11)
        for i, vkinds, scale in mixed_rounds(vp.SOFT_PATTERNS, vp.SCALES):
            mixed_launch(vd, d, opt, TERM, False, [PART_S] * 5, [(i + f) % 4 for f in range(5)], vkinds, scale, PART_BITS)
        for i, vkinds, scale in mixed_rounds(["small", "edge"], vp.EXTREME_SCALES):
            mixed_launch(vd, d, opt, TERM, False, [PART_S] * 5, [(i + f) % 4 for f in range(5)], vkinds, scale, PART_BITS)


# ---------------------------------------------------------------- 4. int8 frames
@pytest.mark.gpu
@pytest.mark.parametrize("case", [(o, k) for o in BYTE_OPTIONS for k in kinds_of(o)], ids=lambda c: f"{name(c[0])}-{FAMILY[c[1]]}")
def test_byte_frames(gpu, vd, case):
    """run_byte_frames under (1, 1, 1) and 3/4 (HARD: (1, 1, 1)): the three byte patterns at the four int8 scales
    against the oracle on (float)q and the float entry point on the widened rows"""
    opt, kind = case
    with vd.ViterbiCUDA(opt) as d:
        for pattern in [PLAIN] if (opt & 0xF) == HARD else [PLAIN, P34]:
            for S in SIZES:
                for vkind in vp.BYTE_PATTERNS:
                    q = vp.byte_frames(vkind, S)
                    rx = q if pattern == PLAIN else np.stack([vd.puncture(r.astype(np.float32), pattern) for r in q]).astype(np.int8)
                    for scale in vp.BYTE_SCALES:
                        ref = np.stack([oracle_byte_frame(vd, opt, r, kind, pattern, S, scale) for r in rx])
                        host, _ = d.run_byte_frames(rx, kind, pattern, S, scale)
                        same(host, ref, FAMILY[kind], pattern, vkind, S, scale)
                        same(float_twin(d, rx, kind, pattern, S, scale), host, FAMILY[kind], pattern, vkind, S, scale, "float twin")


@pytest.mark.gpu
@pytest.mark.parametrize("kind", [OPEN, TERM, TB], ids=FAMILY.get)
@pytest.mark.parametrize("opt", BYTE_SOFT_OPTIONS, ids=name)
def test_byte_mixed_frames(gpu, vd, opt, kind):
    """run_byte_mixed_frames under the same table: against the oracle on (float)q and run_mixed_frames on the widened
    buffer"""
    with vd.ViterbiCUDA(opt) as d:
        d.set_frame_patterns(TABLE)
        for i, vkinds, scale in mixed_rounds(vp.BYTE_PATTERNS, vp.BYTE_SCALES):
            mixed_launch(vd, d, opt, kind, True, LENS, [(i + f) % 4 for f in range(5)], vkinds, scale)


# ---------------------------------------------------------------- 5. the device entry points
def device_rows(rows, max_bits, launch):
    """launch(in_ptr, in_stride, out_ptr, out_stride, stream) on the rows [n, L] copied to the device, the outputs 8
    bytes apart inside sentinel bytes.  Returns (the bytes of every frame's words [n, row], whether every other output
    byte kept the sentinel)."""
    import torch
    rows = np.array(rows)  # (a writable copy: the patterns are read-only)
    n = rows.shape[0]
    inp = torch.from_numpy(rows).cuda()
    row = 4 * ((max_bits + 31) // 32)
    ostride = row + 8
    out = torch.full((8 + n * ostride + 16,), SENTINEL, dtype=torch.uint8, device="cuda")
    launch(inp.data_ptr(), rows.shape[1] * rows.itemsize, out.data_ptr() + 8, ostride, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    body = got[8:8 + n * ostride].reshape(n, ostride)
    clean = bool((got[:8] == SENTINEL).all() and (got[8 + n * ostride:] == SENTINEL).all() and (body[:, row:] == SENTINEL).all())
    return np.ascontiguousarray(body[:, :row]), clean


DEVICE_FAMILIES = ["frames", "punct_frames", "tb_frames", "punct_tb_frames", "mixed_frames", "byte_frames", "byte_mixed_frames"]
DEVICE_CASES = [(o, fam) for o in (SOFT8 | M_B16, FP32 | M_FP16) for fam in DEVICE_FAMILIES
                if not (fam.startswith("byte") and (o & 0xF) == FP32)]


@pytest.mark.gpu
@pytest.mark.parametrize("case", DEVICE_CASES, ids=lambda c: f"{name(c[0])}-{c[1]}")
def test_device_entry_points(gpu, vd, case):
    """`uniform` (int8: `every_byte`) at scale 0.37 through the device entry point of every family: the words of the host
    entry point, and no byte outside the frames' words written into a buffer of 0xA5"""
    opt, fam = case
    scale = 0.37
    with vd.ViterbiCUDA(opt) as d:
        d.set_frame_patterns(TABLE)
        for S in SIZES:
            if fam in ("mixed_frames", "byte_mixed_frames"):
                i8 = fam == "byte_mixed_frames"
                vkinds = ["every_byte" if i8 else "uniform"] * 5
                lens, rates = LENS[1:] + [S], [1, 2, 3, 0, 2]
                for kind in (OPEN, TERM, TB):
                    rxs, offs, total, host = mixed_launch(vd, d, opt, kind, i8, lens, rates, vkinds, scale)
                    words, clean = device_mixed_launch(vd, d, i8, rxs, rates, lens, kind, max(lens), scale,
                                                       offsets=[int(o) for o in offs], lead=0,
                                                       fill=zeros_of(np.int8 if i8 else np.float32), total=total)
                    assert clean, (fam, FAMILY[kind], S)
                    per = 2 if (opt & 0xF00) == O_B16 else 1
                    for f, w in enumerate(words):
                        same(w.view(host.dtype), host[f, :(lens[f] + 31) // 32 * per], fam, FAMILY[kind], S, f)
            elif fam == "byte_frames":
                for kind in (OPEN, TERM, TB):
                    for pattern in (PLAIN, P34):
                        q = vp.byte_frames("every_byte", S)
                        rx = q if pattern == PLAIN else np.stack([vd.puncture(r.astype(np.float32), pattern) for r in q]).astype(np.int8)
                        host, _ = d.run_byte_frames(rx, kind, pattern, S, scale)
                        words, clean = device_byte_frames(vd, d, list(rx), kind, pattern, S, scale)
                        assert clean, (fam, FAMILY[kind], pattern, S)
                        for f, w in enumerate(words):
                            same(w.view(host.dtype), host[f], fam, FAMILY[kind], pattern, S, f)
            else:
                punct = fam.startswith("punct")
                for kind in ([TB] if fam.endswith("tb_frames") else [OPEN, TERM]):
                    for pattern in ([P34, P56] if punct else [None]):
                        rows = received(vd, opt, "uniform", S, scale, pattern)
                        host = host_frames(d, kind, pattern, rows, S, scale)
                        same(host, reference(vd, opt, kind, pattern, "uniform", S, scale), fam, FAMILY[kind], pattern, S)
                        if fam == "frames":
                            launch = lambda i, ist, o, ost, st: d.run_device_frames(i, ist, o, ost, S, 5, kind == TERM, scale, stream=st)
                        elif fam == "punct_frames":
                            launch = lambda i, ist, o, ost, st: d.run_device_punct_frames(i, ist, o, ost, S, 5, pattern, kind == TERM,
                                                                                          scale, stream=st)
                        elif fam == "tb_frames":
                            launch = lambda i, ist, o, ost, st: d.run_device_tb_frames(i, ist, o, ost, S, 5, scale, stream=st)
                        else:
                            launch = lambda i, ist, o, ost, st: d.run_device_punct_tb_frames(i, ist, o, ost, S, 5, pattern, scale, stream=st)
                        words, clean = device_rows(rows, S, launch)
                        assert clean, (fam, FAMILY[kind], pattern, S)
                        same(words.view(host.dtype), host, fam, FAMILY[kind], pattern, S, "device")


# ---------------------------------------------------------------- 6. the stream entry points
STREAM_BITS = 200_000
BATCH_BITS = 1_000_032


@pytest.mark.gpu
@pytest.mark.parametrize("opt", vp.PAIRS, ids=name)
def test_stream_llr(gpu, vd, vo, opt):
    """run_llr on 200,000 bits of small, small_halves, uniform, edge and satrand one after the other with specials
    sprinkled in (HARD: zero_mix and satrand), scales 1.0 and 0.37, against the oracle's pack + decode"""
    with vd.ViterbiCUDA(opt) as d:
        for scale in (1.0, 0.37):
            vals = vp.stream(opt, STREAM_BITS, scale)
            ref, ok = vo.decode(opt, vo.pack(opt, vals, scale), input_num=vals.size)
            assert ok
            out, _ = d.run_llr(vals, scale=scale)
            _differ(out, ref, f"{name(opt)} scale {scale}")


@pytest.mark.gpu
@pytest.mark.parametrize("opt", [o for o in vp.PAIRS if (o & 0xF) != HARD], ids=name)
def test_stream_punct(gpu, vd, vo, opt):
    """run_punct under 3/4 on the kept values of the same stream, against the oracle on the depunctured stream"""
    with vd.ViterbiCUDA(opt) as d:
        for scale in (1.0, 0.37):
            vals = vp.stream(opt, STREAM_BITS, scale)
            rx = vd.puncture(vals, P34)
            ref, ok = vo.decode(opt, vo.pack(opt, vd.depuncture(rx, P34, vals.size), scale), input_num=vals.size)
            assert ok
            out, _ = d.run_punct(rx, P34, vals.size, scale=scale)
            _differ(out, ref, f"{name(opt)} scale {scale}")


@pytest.mark.gpu
@pytest.mark.parametrize("opt", LLR_OPTS, ids=name)
def test_stream_llr_batched(gpu, vd, vo, opt):
    """one run_device_llr_batch launch of three batches of 1,000,032 bits -- small, uniform and satrand at scale 1.0
    (HARD: zero_mix, satrand and zero_mix from another seed) -- on vd_decode_pk's batched form with the fused packer"""
    import torch
    n, nb = 2 * BATCH_BITS, 3
    if (opt & 0xF) == HARD:
        batches = [vp.frames(opt, "zero_mix", BATCH_BITS, 1.0, 1)[0], vp.frames(opt, "satrand", BATCH_BITS, 1.0, 1)[0],
                   vp.frames(opt, "zero_mix", BATCH_BITS, 1.0, 1, 2)[0]]
    else:
        batches = [vp.frames(opt, vkind, BATCH_BITS, 1.0, 1)[0] for vkind in ("small", "uniform", "satrand")]
    vals, istride = _to_device(batches, 4 * n)
    nout = vd.lib().vd_output_size(opt, n)
    ostride = (nout + 255) // 256 * 256 + 256
    out = torch.full((nb * ostride,), SENTINEL, dtype=torch.uint8, device="cuda")
    with vd.ViterbiCUDA(opt) as d:
        assert d.kernel_for(n, nb, True).startswith("vd_decode_pk<LLR+") and " batched" in d.kernel_for(n, nb, True)
        d.run_device_llr_batch(vals.data_ptr(), istride, out.data_ptr(), ostride, n, nb, 1.0)
        torch.cuda.synchronize()
    for b, v in enumerate(batches):
        ref, ok = vo.decode(opt, vo.pack(opt, v, 1.0), input_num=n, nthreads=16)
        assert ok
        _differ(out[b * ostride:b * ostride + nout].cpu().numpy().view(ref.dtype), ref, f"batch {b}")
        assert bool((out[b * ostride + nout:(b + 1) * ostride] == SENTINEL).all())
