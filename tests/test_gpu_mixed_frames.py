"""GPU parity of mixed frame launches (vd_run_mixed_frames / vd_run_device_mixed_frames and their int8 twins; kernels
vd_decode_tg<FRM+MIX+...>): frames of several code rates, lengths and places in one launch.  Every frame of a launch
equals, word for word, the oracle's decode of that frame alone by its family's own definition -- frames_common.oracle_frame
of vitdec.depuncture(...) for open and terminated frames, ptb_common.oracle_ptb_frame for tail-biting ones -- and the
uniform entry point of its family run on the frames of its pattern, a second witness.  Float inputs: the noisy BPSK
frames of frames_common.py and tb_common.py (sigma 0.3, scale 40000); int8 inputs: the same frames quantised as
clip(rint(32 v), -128, 127), scale 1.0 (SOFT8) or 0.25 (SOFT4), as in tests/test_gpu_byte_frames.py.  The helpers alone:
tests/test_mixed_frames.py."""
import numpy as np
import pytest

from frames_common import SCALE, SIGMA, frame_bits, frames, oracle_frame
from ptb_common import oracle_ptb_frame
from tb_common import tb_frames
from vitdec import FP32, HARD, M_B16, M_B32, M_FP16, O_B16, SOFT4, SOFT8, SOFT16

OPEN, TERM, TB = 0, 1, 2
KINDS = {OPEN: "open", TERM: "term", TB: "tb"}
PLAIN = (1, 1, 1)
TABLE = [PLAIN, (2, 1, 3), (3, 5, 3), (7, 0x51, 0x2F), (16, 0xA5C3, 0x5A3D), (16, 0x8000, 0)]
SIZES = [1, 2, 15, 31, 32, 33, 69, 70, 71, 95, 96, 97, 250, 1000]
LAUNCHES = [1, 3, 5, 24]
# every non-HARD option: the 9 (format, metric) pairs x both output widths; the int8 twins: SOFT4 and SOFT8
PAIRS = [SOFT4 | M_B32, SOFT4 | M_B16, SOFT4 | M_FP16, SOFT8 | M_B32, SOFT8 | M_B16, SOFT16 | M_B32, FP32 | M_B32, FP32 | M_B16,
         FP32 | M_FP16]
FLOAT_OPTIONS = [p | o for p in PAIRS for o in (0, O_B16)]
BYTE_OPTIONS = [o for o in FLOAT_OPTIONS if (o & 0xF) in (SOFT4, SOFT8)]
SENTINEL = 0xA5


def name(o):
    return f"0x{o:03x}"


def byte_scale(opt):
    return 0.25 if (opt & 0xF) == SOFT4 else 1.0


def short_frame(S, terminated, seed):
    """frames_common.frames(1, S, terminated, seed) for S < 7, which its encoder does not take"""
    rng = np.random.default_rng(seed)
    bits = frame_bits(1, S, terminated, rng)[0]
    out = np.zeros((S, 2), dtype=np.uint8)
    for col, poly in enumerate((0o171, 0o133)):
        for k in range(S):
            if (poly >> (6 - k)) & 1:
                out[k:, col] ^= bits[:S - k]
    return (np.where(out.reshape(-1) == 1, 1.0, -1.0) + rng.normal(0.0, SIGMA, 2 * S)).astype(np.float32)


def codeword(kind, S, seed):
    """the 2 S float values of one noisy frame of the kind"""
    if kind == TB:
        return tb_frames(1, S, seed)[1][0]
    return frames(1, S, kind == TERM, seed)[1][0] if S >= 7 else short_frame(S, kind == TERM, seed)


def quantise(v):
    return np.clip(np.rint(32.0 * np.asarray(v, dtype=np.float32)), -128, 127).astype(np.int8)


def received(vd, kind, S, pattern, seed, i8):
    """the kept values of a frame: float32, or int8 (the quantised frame's)"""
    v = codeword(kind, S, seed)
    if i8:
        return vd.puncture(quantise(v).astype(np.float32), pattern).astype(np.int8)
    return vd.puncture(v, pattern)


_REFS = {}


def oracle_of(vd, opt, kind, rx, pattern, S, scale):
    """the words that define the decode of one frame of S stages from its kept values, computed once per frame"""
    key = (opt, kind, pattern, S, scale, rx.dtype.str, rx.tobytes())
    if key not in _REFS:
        v = rx.astype(np.float32)
        if kind == TB:
            ref = oracle_ptb_frame(vd, opt, v, pattern, S, scale)
        else:
            ref = oracle_frame(vd, opt, vd.depuncture(v, pattern, 2 * S), kind == TERM, scale)
        ref.setflags(write=False)
        _REFS[key] = ref
    return _REFS[key]


def uniform(vd, d, kind, rows, pattern, max_bits, lens, scale, i8):
    """the uniform entry point of the family on the frames of one pattern (rows [k, L]): [k, words]"""
    need = vd.punctured_len(pattern, 2 * max_bits)
    rows = np.ascontiguousarray(rows[:, :max(need, 1)])
    if i8:  # (1, 1, 1) selects the unpunctured byte family there: a stage's pair as one 16-bit load
        return d.run_byte_frames(rows, kind, pattern, max_bits, scale, frame_bits=lens)[0]
    if kind == TB:
        return d.run_punct_tb_frames(rows, pattern, max_bits, scale, frame_bits=lens)[0]
    return d.run_punct_frames(rows, pattern, max_bits, kind == TERM, scale, frame_bits=lens)[0]


def pairs_from(c0, n):
    """n (pattern index, length) pairs from position c0 of the walk that meets every pattern with every length in
    len(TABLE) * len(SIZES) steps, neighbours differing in both"""
    out = []
    for c in range(c0, c0 + n):
        p = c % len(TABLE)
        out.append((p, SIZES[(c // len(TABLE) + p) % len(SIZES)]))
    return out


def device_launch(vd, d, i8, rxs, rates, lens, kind, max_bits, scale, offsets=None, stride=None, lead=0, fill=None, total=None):
    """run_device_[byte_]mixed_frames of the frames rxs into a buffer of sentinel bytes.  Without offsets: frame f at
    lead + f * stride values of a buffer prefilled by fill(n); with offsets: at value index offsets[f] counted from
    `lead` values into a buffer of `total` + lead values.  Returns (the bytes each frame's words occupy, whether every
    other output byte kept the sentinel)."""
    import torch
    n = len(rxs)
    dt = np.int8 if i8 else np.float32
    if offsets is None:
        host = fill(lead + (n - 1) * stride + max(stride, 1) + 64)
        place = [lead + f * stride for f in range(n)]
    else:
        host = fill(lead + total + 64)
        place = [lead + int(o) if int(o) < total else None for o in offsets]
    assert host.dtype == dt
    for f, rx in enumerate(rxs):
        if rx.size:
            host[place[f]:place[f] + rx.size] = rx
    inp = torch.from_numpy(host).cuda()
    row = 4 * ((max_bits + 31) // 32)
    ostride = row + 8
    out = torch.full((8 + n * ostride + 16,), SENTINEL, dtype=torch.uint8, device="cuda")
    lens_d = torch.from_numpy(np.asarray(lens, dtype=np.uint32).view(np.int32)).cuda() if lens is not None else None
    rate_d = torch.from_numpy(np.asarray(rates, dtype=np.uint8)).cuda() if rates is not None else None
    off_d = torch.from_numpy(np.asarray(offsets, dtype=np.uint64).view(np.int64)).cuda() if offsets is not None else None
    assert inp.data_ptr() % 256 == 0 and out.data_ptr() % 4 == 0
    run = d.run_device_byte_mixed_frames if i8 else d.run_device_mixed_frames
    run(inp.data_ptr() + lead * host.itemsize, 0 if stride is None else stride * host.itemsize, out.data_ptr() + 8, ostride,
        max_bits, n, kind, scale, frame_bits_ptr=lens_d.data_ptr() if lens_d is not None else 0,
        rate_ptr=rate_d.data_ptr() if rate_d is not None else 0, offsets_ptr=off_d.data_ptr() if off_d is not None else 0,
        stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    untouched = np.ones(got.size, dtype=bool)
    words = []
    for f in range(n):
        S = min(int(lens[f]), max_bits) if lens is not None else max_bits
        if rates is not None and int(rates[f]) >= len(d.frame_patterns()):
            S = 0
        nb = 4 * ((S + 31) // 32)
        lo = 8 + f * ostride
        words.append(got[lo:lo + nb].copy())
        untouched[lo:lo + nb] = False
    return words, bool((got[untouched] == SENTINEL).all())


def zeros_of(dt):
    return lambda n: np.zeros(n, dtype=dt)


# ---------------------------------------------------------------- 1. parity
def parity_case(vd, opt, i8, oi):
    scale = byte_scale(opt) if i8 else SCALE
    dt = np.int8 if i8 else np.float32
    with vd.ViterbiCUDA(opt) as d:
        d.set_frame_patterns(TABLE)
        assert d.frame_patterns() == TABLE
        for kind in (OPEN, TERM, TB):
            c = 33 * kind + 7 * oi
            for n in LAUNCHES:
                pairs = pairs_from(c, n)
                c += n
                rates = [p for p, _ in pairs]
                lens = [S for _, S in pairs]
                # one frame: maxFrameBits is its length and no lengths array; else 1000 and the lengths on the device
                max_bits = lens[0] if n == 1 else 1000
                rxs = [received(vd, kind, S, TABLE[p], 100 * kind + f + S, i8) for f, (p, S) in enumerate(pairs)]
                refs = [oracle_of(vd, opt, kind, rx, TABLE[p], S, scale) for rx, (p, S) in zip(rxs, pairs)]
                L = max(vd.punctured_len(p, 2 * max_bits) for p in TABLE)
                rows = np.zeros((n, L), dtype=dt)
                for f, rx in enumerate(rxs):
                    rows[f, :rx.size] = rx
                tag = (KINDS[kind], n, pairs)
                # the blocking host variant: each frame's words, zeros behind a shorter frame's
                run = d.run_byte_mixed_frames if i8 else d.run_mixed_frames
                host, _ = run(rows, kind, max_bits, scale, frame_bits=None if n == 1 else lens, rates=rates)
                per = host.shape[1] // ((max_bits + 31) // 32)
                for f, ref in enumerate(refs):
                    nw = (lens[f] + 31) // 32 * per
                    assert host.dtype == ref.dtype and np.array_equal(host[f, :nw], ref), (tag, f, np.flatnonzero(host[f, :nw] != ref)[:5])
                    assert not host[f, nw:].any(), (tag, f)
                # the uniform entry point on the frames of each pattern
                for p in sorted(set(rates)):
                    idx = [f for f in range(n) if rates[f] == p]
                    twin = uniform(vd, d, kind, rows[idx], TABLE[p], max_bits, [lens[f] for f in idx], scale, i8)
                    assert np.array_equal(twin, host[idx]), (tag, "pattern", p, np.argwhere(twin != host[idx])[:5])
                # the device variant: the same bytes, nothing else written
                words, clean = device_launch(vd, d, i8, rxs, rates, None if n == 1 else lens, kind, max_bits, scale, stride=L, lead=0,
                                             fill=zeros_of(dt))
                assert clean, (tag, "a byte outside the frames' words was written")
                for f, ref in enumerate(refs):
                    assert np.array_equal(words[f].view(ref.dtype), ref), (tag, f)


@pytest.mark.gpu
@pytest.mark.parametrize("opt", FLOAT_OPTIONS, ids=name)
def test_float_frames_equal_the_oracle_and_the_uniform_entry_points(gpu, vd, opt):
    """launches of 1, 3, 5 and 24 frames of all three kinds under the six-pattern table, neighbouring frames at different
    patterns and lengths (a workgroup's four waves hold four patterns), every pattern meeting every length: each frame
    equals the oracle of its depunctured padded or extended stream and the uniform entry point run on the frames of its
    pattern; the host and device variants agree"""
    parity_case(vd, opt, False, FLOAT_OPTIONS.index(opt))


@pytest.mark.gpu
@pytest.mark.parametrize("opt", BYTE_OPTIONS, ids=name)
def test_byte_frames_equal_the_oracle_and_the_uniform_entry_points(gpu, vd, opt):
    """the same on int8 values; a (1, 1, 1) frame equals the unpunctured byte family's decode (16-bit loads there,
    single bytes here)"""
    parity_case(vd, opt, True, BYTE_OPTIONS.index(opt))


# ---------------------------------------------------------------- 2. ragged layout
def nan_fill(n):
    return np.full(n, np.nan, dtype=np.float32)


def poison_fill(n):
    p = np.empty(n, dtype=np.int8)
    p[0::2] = 127
    p[1::2] = -128
    return p


@pytest.mark.gpu
@pytest.mark.parametrize("i8", [False, True], ids=["float", "int8"])
@pytest.mark.parametrize("opt", [SOFT8 | M_B16, SOFT4 | M_FP16 | O_B16], ids=name)
def test_ragged_layout_reads_and_writes_exactly_the_frames(gpu, vd, opt, i8):
    """frames laid back to back by mixed_layout in reversed order (the last frame first in the buffer), two values of
    slack before each, two frames sharing one offset, on a base pointer that is 4- but not 8-byte aligned (int8: odd);
    lengths 0, 1, maxFrameBits and above it, one rate index equal to the table's length and one of 255, whose offsets
    point far outside the buffer.  Every value that belongs to no frame is NaN (int8: 127 and -128 alternating): a read
    of one changes the words.  Each frame equals the oracle of that frame alone; every output byte outside a decoded
    frame's words keeps its sentinel"""
    scale = byte_scale(opt) if i8 else SCALE
    max_bits = 250
    lens = [250, 0, 1, 300, 97, 33, 1000, 70, 250, 71, 96, 2]
    rates = [2, 1, 0, 3, len(TABLE), 4, 1, 255, 0, 5, 2, 1]
    n = len(lens)
    eff = [min(S, max_bits) for S in lens]
    with vd.ViterbiCUDA(opt) as d:
        d.set_frame_patterns(TABLE)
        for kind in (OPEN, TERM, TB):
            rxs = []
            for f in range(n):
                alive = rates[f] < len(TABLE) and eff[f] > 0
                rxs.append(received(vd, kind, eff[f], TABLE[rates[f]], 300 + f, i8) if alive else np.zeros(0, dtype=np.int8 if i8 else np.float32))
            # frame n (appended): frame 0's twin, same pattern, length and offset
            offs_r, total = vd.mixed_layout(eff[::-1], rates[::-1], TABLE)
            offsets = [int(offs_r[n - 1 - f]) + 2 * (n - f) for f in range(n)]
            total += 2 * n + 2
            for f in range(n):
                if rates[f] >= len(TABLE) or eff[f] == 0:
                    offsets[f] = (1 << 40) + f  # never read
            all_rx, all_rates, all_lens, all_offs = rxs + [rxs[0]], rates + [rates[0]], lens + [lens[0]], offsets + [offsets[0]]
            words, clean = device_launch(vd, d, i8, all_rx, all_rates, all_lens, kind, max_bits, scale, offsets=all_offs,
                                         lead=1, fill=poison_fill if i8 else nan_fill, total=total)
            assert clean, (KINDS[kind], "a byte outside the decoded frames' words was written")
            for f in range(n + 1):
                g = f % n
                if rates[g] >= len(TABLE) or eff[g] == 0:
                    assert words[f].size == 0
                    continue
                ref = oracle_of(vd, opt, kind, all_rx[f], TABLE[rates[g]], eff[g], scale)
                assert np.array_equal(words[f].view(ref.dtype), ref), (KINDS[kind], f, np.flatnonzero(words[f].view(ref.dtype) != ref)[:5])
            # the blocking host variant over the same flat buffer and offsets (in-range ones: it checks every frame's place)
            flat = (poison_fill if i8 else nan_fill)(total)
            for f in range(n):
                if all_rx[f].size:
                    flat[offsets[f]:offsets[f] + all_rx[f].size] = all_rx[f]
            host_offs = [o if o < total else 0 for o in all_offs]
            run = d.run_byte_mixed_frames if i8 else d.run_mixed_frames
            host, _ = run(flat, kind, max_bits, scale, frame_bits=all_lens, rates=all_rates, offsets=host_offs)
            per = host.shape[1] // ((max_bits + 31) // 32)
            for f in range(n + 1):
                dead = rates[f % n] >= len(TABLE) or eff[f % n] == 0
                nw = 0 if dead else (eff[f % n] + 31) // 32 * per
                assert np.array_equal(host[f, :nw], words[f].view(host.dtype)) and not host[f, nw:].any(), (KINDS[kind], f)
            with pytest.raises(vd.VitdecError, match="VD_ERR_ARG.*does not lie inside"):
                run(flat, kind, max_bits, scale, frame_bits=all_lens, rates=all_rates, offsets=[o + total for o in host_offs])


# ---------------------------------------------------------------- 3. parts
@pytest.mark.gpu
@pytest.mark.parametrize("part_bits", [96, 192])
@pytest.mark.parametrize("opt,i8", [(SOFT8 | M_B16, False), (SOFT16 | M_B32 | O_B16, False), (FP32 | M_FP16, False),
                                    (SOFT8 | M_B32, True), (SOFT4 | M_FP16 | O_B16, True)],
                         ids=["0x012", "0x103", "0x024", "0x002-i8", "0x121-i8"])
def test_frames_in_parts_equal_the_uniform_entry_points(gpu, vd, opt, i8, part_bits):
    """set_frame_part_bits is honoured: frames of 250 and 1000 stages at mixed rates, every part of a frame under the
    frame's pattern and offset, equal to the uniform entry points at the same part length"""
    scale = byte_scale(opt) if i8 else SCALE
    dt = np.int8 if i8 else np.float32
    lens = [250, 1000, 1000, 250, 1000, 250, 1000]
    rates = [0, 1, 2, 3, 4, 2, 0]
    n, max_bits = len(lens), 1000
    with vd.ViterbiCUDA(opt) as d:
        d.set_frame_patterns(TABLE)
        d.set_frame_part_bits(part_bits)
        for kind in (OPEN, TERM, TB):
            rxs = [received(vd, kind, S, TABLE[p], 500 + f, i8) for f, (p, S) in enumerate(zip(rates, lens))]
            offs, total = vd.mixed_layout(lens, rates, TABLE)
            flat = np.concatenate(rxs)
            assert flat.size == total and flat.dtype == dt
            run = d.run_byte_mixed_frames if i8 else d.run_mixed_frames
            host, _ = run(flat, kind, max_bits, scale, frame_bits=lens, rates=rates, offsets=offs)
            L = max(vd.punctured_len(p, 2 * max_bits) for p in TABLE)
            rows = np.zeros((n, L), dtype=dt)
            for f, rx in enumerate(rxs):
                rows[f, :rx.size] = rx
            for p in sorted(set(rates)):
                idx = [f for f in range(n) if rates[f] == p]
                twin = uniform(vd, d, kind, rows[idx], TABLE[p], max_bits, [lens[f] for f in idx], scale, i8)
                assert np.array_equal(twin, host[idx]), (KINDS[kind], part_bits, p, np.argwhere(twin != host[idx])[:5])
            words, clean = device_launch(vd, d, i8, rxs, rates, lens, kind, max_bits, scale, offsets=[int(o) for o in offs], lead=0,
                                         fill=zeros_of(dt), total=total)
            assert clean
            per = host.shape[1] // ((max_bits + 31) // 32)
            for f in range(n):
                assert np.array_equal(words[f].view(host.dtype), host[f, :(lens[f] + 31) // 32 * per]), (KINDS[kind], f)
        parts = -(-32 // (part_bits // 32))
        nm = d.kernel_for(1000, n, 13 if i8 else 11)
        assert nm.startswith("vd_decode_tg<FRM+I8+MIX+PUN+" if i8 else "vd_decode_tg<FRM+MIX+PUN+") and f"{parts} parts per frame" in nm, nm


# ---------------------------------------------------------------- 4. status codes, names, the table, the guard
@pytest.mark.gpu
def test_status_codes_and_the_table(gpu, vd):
    ok = dict(rx_ptr=4096, rx_stride=2000, output_ptr=4096, output_stride=32, maxFrameBits=250, nframes=4, kind=TERM, scale=1.0)
    bok = dict(ok, q_ptr=ok["rx_ptr"], q_stride=ok["rx_stride"])  # (the int8 twin's names)
    del bok["rx_ptr"], bok["rx_stride"]
    rows = np.zeros((4, 500), dtype=np.float32)
    with vd.ViterbiCUDA(HARD | M_B32) as d:
        d.set_frame_patterns(TABLE)
        for kind in (OPEN, TERM, TB):
            with pytest.raises(vd.VitdecError, match="VD_ERR_OPTIONS.*HARD"):
                d.run_device_mixed_frames(**dict(ok, kind=kind))  # (checked before any pointer is used)
            with pytest.raises(vd.VitdecError, match="VD_ERR_OPTIONS.*HARD"):
                d.run_device_byte_mixed_frames(**dict(bok, kind=kind))
        with pytest.raises(vd.VitdecError, match="VD_ERR_OPTIONS.*HARD"):
            d.run_mixed_frames(rows, TERM, 250, 1.0)
    for opt in (SOFT16 | M_B32, FP32 | M_FP16):
        with vd.ViterbiCUDA(opt) as d:
            d.set_frame_patterns(TABLE)
            with pytest.raises(vd.VitdecError, match="VD_ERR_OPTIONS.*SOFT16 or FP32"):
                d.run_device_byte_mixed_frames(**bok)
            with pytest.raises(vd.VitdecError, match="VD_ERR_OPTIONS.*SOFT16 or FP32"):
                d.run_byte_mixed_frames(rows.astype(np.int8), TERM, 250, 1.0)
    with vd.ViterbiCUDA(SOFT8 | M_B16) as d:
        assert d.frame_patterns() == []
        with pytest.raises(vd.VitdecError, match="VD_ERR_ARG.*pattern table is empty"):
            d.run_device_mixed_frames(**ok)
        with pytest.raises(vd.VitdecError, match="VD_ERR_ARG.*pattern table is empty"):
            d.run_device_byte_mixed_frames(**bok)
        for bad in ([(0, 1, 1)], [(17, 1, 1)], [PLAIN, (3, 0b1000, 0b011)], [PLAIN, (3, 0, 0)]):
            with pytest.raises(vd.VitdecError, match="VD_ERR_ARG.*invalid puncture pattern"):
                d.set_frame_patterns(bad)
        with pytest.raises(vd.VitdecError, match=r"VD_ERR_ARG.*n must be in \[0, 16\]"):
            d.set_frame_patterns([(3, 5, 3)] * 17)
        assert d.frame_patterns() == []  # a refused table changes nothing
        d.set_frame_patterns([(3, 5, 3)] * 16)
        assert d.frame_patterns() == [(3, 5, 3)] * 16
        d.set_frame_patterns([])
        assert d.frame_patterns() == []
        d.set_frame_patterns(TABLE)
        assert d.frame_patterns() == TABLE
        bad = [dict(rx_ptr=4098), dict(rx_ptr=4097), dict(rx_stride=1996), dict(rx_stride=1998), dict(rx_stride=0),
               dict(kind=3), dict(kind=-1), dict(output_stride=28), dict(output_stride=30), dict(maxFrameBits=0),
               dict(maxFrameBits=(1 << 20) + 1, rx_stride=8 << 20, output_stride=1 << 18), dict(nframes=0), dict(nframes=-1),
               dict(scale=0.0), dict(scale=float("inf")), dict(scale=float("nan")), dict(scale=1e-40), dict(kind=TB, scale=0.0),
               dict(rx_ptr=0), dict(output_ptr=0)]
        for kw in bad:
            with pytest.raises(vd.VitdecError, match="VD_ERR_ARG"):
                d.run_device_mixed_frames(**dict(ok, **kw))
        with pytest.raises(vd.VitdecError, match="VD_ERR_ARG.*rx_d must be 4-byte aligned"):
            d.run_device_mixed_frames(**dict(ok, rx_ptr=4098))
        with pytest.raises(vd.VitdecError, match="VD_ERR_ARG.*rx_d must be 4-byte aligned"):
            d.run_device_mixed_frames(**dict(ok, rx_ptr=4098, offsets_ptr=4096))
        with pytest.raises(vd.VitdecError, match="VD_ERR_ARG.*frames would overlap"):
            d.run_device_mixed_frames(**dict(ok, rx_stride=1996))  # (1, 1, 1) is in the table: 2000 bytes
        with pytest.raises(vd.VitdecError, match="VD_ERR_ARG.*frames would overlap"):
            d.run_device_byte_mixed_frames(**dict(bok, q_ptr=4097, q_stride=499))
        for kw in (dict(q_ptr=4097, q_stride=501), dict(q_ptr=4099, q_stride=500)):  # any address, any stride
            with pytest.raises(vd.VitdecError, match="VD_ERR_ARG.*output_stride"):
                d.run_device_byte_mixed_frames(**dict(bok, output_stride=30, **kw))
        d.set_frame_patterns(TABLE[2:3])
        with pytest.raises(vd.VitdecError, match="VD_ERR_ARG.*frames would overlap"):
            d.run_device_mixed_frames(**dict(ok, rx_stride=1332))  # 3/4: 334 floats
        d.set_frame_part_bits(96)
        with pytest.raises(vd.VitdecError, match="VD_ERR_ARG.*workgroups"):
            d.run_device_mixed_frames(**dict(ok, maxFrameBits=1 << 20, rx_stride=8 << 20, output_stride=1 << 17, nframes=0x7FFFFFFF))


@pytest.mark.gpu
def test_kernel_names(gpu, vd):
    """llr 11 .. 14: the punctured family's name (llr 4, 6, 8, 10) with MIX+ before PUN+ / TB+PUN+, "-" where the call is refused"""
    twins = {11: (4, "FRM+PUN+", "FRM+MIX+PUN+"), 12: (6, "FRM+TB+PUN+", "FRM+MIX+TB+PUN+"),
             13: (8, "FRM+I8+PUN+", "FRM+I8+MIX+PUN+"), 14: (10, "FRM+I8+TB+PUN+", "FRM+I8+MIX+TB+PUN+")}
    for opt in (SOFT8 | M_B16, SOFT4 | M_FP16 | O_B16, SOFT16 | M_B32, FP32 | M_B32 | O_B16, HARD | M_B32):
        with vd.ViterbiCUDA(opt) as d:
            for part_bits in (0, 96):
                d.set_frame_part_bits(part_bits)
                for llr, (t, a, b) in twins.items():
                    for n in (1, 5, 10_000):
                        twin, mixed = d.kernel_for(1000, n, t), d.kernel_for(1000, n, llr)
                        assert mixed == ("-" if twin == "-" else twin.replace(a, b, 1)), (name(opt), llr, mixed, twin)
                        assert (mixed == "-") == ((opt & 0xF) == HARD or (llr >= 13 and (opt & 0xF) > SOFT8))
                    assert d.kernel_for(0, 4, llr) == "-" and d.kernel_for((1 << 20) + 1, 4, llr) == "-"
    with vd.ViterbiCUDA(SOFT8 | M_B16) as d:
        assert d.kernel_for(1000, 4, 11).startswith("vd_decode_tg<FRM+MIX+PUN+SOFT8,B16,O32> one frame per wave, ")
        assert d.kernel_for(1000, 4, 12).startswith("vd_decode_tg<FRM+MIX+TB+PUN+SOFT8,B16,O32> one frame per wave, ")
        assert d.kernel_for(1000, 4, 13).startswith("vd_decode_tg<FRM+I8+MIX+PUN+SOFT8,B16,O32> one frame per wave, ")
        assert d.kernel_for(1000, 4, 14).startswith("vd_decode_tg<FRM+I8+MIX+TB+PUN+SOFT8,B16,O32> one frame per wave, ")
        assert d.kernel_for(1000, 4, 4).startswith("vd_decode_tg<FRM+PUN+SOFT8,")  # the earlier names stay


@pytest.mark.gpu
def test_default_pattern_table_at_run_time_and_the_lds_guard(gpu, vd):
    """rate_d NULL: every frame under pattern 0.  The kernel reads the table when it runs: the same call after
    set_frame_patterns decodes under the new pattern 0.  The LDS guard check reports 0 violations on mixed launches"""
    opt, S, n = SOFT8 | M_B16, 1000, 13
    with vd.ViterbiCUDA(opt) as d:
        d.set_guard_check(True)
        for table in ([TABLE[2], TABLE[1]], [TABLE[1], TABLE[2]]):
            d.set_frame_patterns(table)
            for kind in (TERM, TB):
                rxs = [received(vd, kind, S, table[0], 700 + f, False) for f in range(n)]
                L = max(vd.punctured_len(p, 2 * S) for p in table)  # the stride rule: the table's densest pattern
                rows = np.zeros((n, L), dtype=np.float32)
                rows[:, :rxs[0].size] = np.stack(rxs)
                host, _ = d.run_mixed_frames(rows, kind, S, SCALE)
                for f in range(n):
                    assert np.array_equal(host[f], oracle_of(vd, opt, kind, rxs[f], table[0], S, SCALE)), (table[0], KINDS[kind], f)
                words, clean = device_launch(vd, d, False, rxs, None, None, kind, S, SCALE, stride=L, fill=zeros_of(np.float32))
                assert clean and all(np.array_equal(w.view(host.dtype), h) for w, h in zip(words, host))
        d.set_frame_patterns(TABLE)
        rates = [f % 5 for f in range(n)]
        rxs = [received(vd, OPEN, S, TABLE[r], 800 + f, False) for f, r in enumerate(rates)]
        offs, total = vd.mixed_layout([S] * n, rates, TABLE)
        host, _ = d.run_mixed_frames(np.concatenate(rxs), OPEN, S, SCALE, rates=rates, offsets=offs)
        for f in range(n):
            assert np.array_equal(host[f], oracle_of(vd, opt, OPEN, rxs[f], TABLE[rates[f]], S, SCALE)), f
        assert d.guard_violations() == 0
