"""GPU parity of frame decodes in parts (vd_set_frame_part_bits; all eight frame entry points, kernels
vd_decode_tg<FRM+...>): with a part length, part j of every frame equals, word for word, the oracle's one-chunk decode
of sub-stream j of vitdec.frame_parts(the frame's padded or extended stream, part_bits), written at word j Wp of the
frame's words (parts_common.oracle_parts).  Inputs: the noisy BPSK frames of frames_common.py and tb_common.py, sigma
0.3 and scale 40000 unless a test says otherwise, and the sigma 0.9 set on which the oracle's part-wise words differ
from its whole-frame words (tests/test_frame_parts.py asserts that), so a launch that ignored the part length fails
here.  The geometry alone, and the definition on the CPU: tests/test_frame_parts.py."""
import ctypes

import numpy as np
import pytest

from frames_common import OPTIONS6, SCALE, decoded_bits, frames, oracle_frames
from parts_common import (NOISY_N, NOISY_PART_BITS, NOISY_S, NOISY_SEED, NOISY_SIGMA, family_frames, oracle_parts,
                          oracle_parts_frames, stream_of)
from ptb_common import pid, punctured
from tb_common import oracle_tb_frames
from vitdec import FP32, HARD, M_B16, M_B32, M_FP16, O_B16, SOFT4, SOFT8, SOFT16

PART_BITS = [96, 192]
# exactly one part, a last part of one word that is mostly virtual stages, uneven last parts
SIZES = [1, 95, 96, 97, 192, 193, 250, 1000]
# the wrap inside a later part's warm-up and traceback, and several turns
TB_SIZES = [1, 5, 70, 97, 100, 166, 250, 1000]
PATTERNS = [(2, 1, 3), (3, 5, 3), (16, 0x8000, 0)]
NFRAMES = 5


def name(o):
    return f"0x{o:03x}"


def kind_of(fam, terminated):
    return "tb" if fam in ("tb", "ptb") else "term" if terminated else "open"


def host_run(d, fam, data, S, pattern, terminated):
    if fam == "frm":
        return d.run_frames(data, terminated, SCALE)[0]
    if fam == "tb":
        return d.run_tb_frames(data, SCALE)[0]
    if fam == "pun":
        return d.run_punct_frames(data, pattern, S, terminated, SCALE)[0]
    return d.run_punct_tb_frames(data, pattern, S, SCALE)[0]


def device_call(d, fam, inp, istride, out, ostride, S, n, pattern, terminated, lens=0):
    import torch
    st = torch.cuda.current_stream().cuda_stream
    if fam == "frm":
        d.run_device_frames(inp, istride, out, ostride, S, n, terminated, SCALE, frame_bits_ptr=lens, stream=st)
    elif fam == "tb":
        d.run_device_tb_frames(inp, istride, out, ostride, S, n, SCALE, frame_bits_ptr=lens, stream=st)
    elif fam == "pun":
        d.run_device_punct_frames(inp, istride, out, ostride, S, n, pattern, terminated, SCALE, frame_bits_ptr=lens, stream=st)
    else:
        d.run_device_punct_tb_frames(inp, istride, out, ostride, S, n, pattern, SCALE, frame_bits_ptr=lens, stream=st)


def device_run(d, fam, data, S, pattern, terminated):
    """the device entry point of the family on the rows of data (n frames back to back) on the current stream"""
    import torch
    n, row = data.shape[0], 4 * ((S + 31) // 32)
    inp = torch.from_numpy(np.array(data)).cuda() if data.size else torch.zeros(4, device="cuda")
    out = torch.zeros(n * row // 4, dtype=torch.int32, device="cuda")
    device_call(d, fam, inp.data_ptr(), 4 * data.shape[1], out.data_ptr(), row, S, n, pattern, terminated)
    torch.cuda.synchronize()
    return out.cpu().numpy().view(d.decPack_t).reshape(n, -1)


def family_data(vd, fam, S, seed, pattern, terminated, n=NFRAMES, sigma=0.3):
    vals = family_frames(kind_of(fam, terminated), n, S, seed, sigma)[1]
    return punctured(vd, vals, pattern) if pattern is not None else vals


# OPTIONS6 (SOFT8 / M_B32 / O_B16 among them) and one more O_B16 option per family; HARD neither open nor punctured
PLAIN = [("frm", o, None, t) for o in OPTIONS6 + [FP32 | M_FP16 | O_B16] for t in (True, False) if t or (o & 0xF) != HARD]
TB = [("tb", o, None, True) for o in OPTIONS6 + [HARD | M_B16 | O_B16]]
SOFT = [o for o in OPTIONS6 if (o & 0xF) != HARD]
PUN = ([("pun", o, p, True) for p in PATTERNS for o in SOFT + [SOFT4 | M_B32 | O_B16]] +
       [("pun", o, PATTERNS[1], False) for o in SOFT + [SOFT4 | M_B32 | O_B16]])
PTB = [("ptb", o, p, True) for p in PATTERNS for o in SOFT + [SOFT16 | M_B32 | O_B16]]


def cid(c):
    fam, o, p, t = c
    return f"{fam}-{name(o)}" + (f"-{pid(p)}" if p else "") + ("" if fam in ("tb", "ptb") else "-terminated" if t else "-open")


@pytest.mark.gpu
@pytest.mark.parametrize("case", PLAIN + TB + PUN + PTB, ids=cid)
def test_parts_equal_the_oracle_of_frame_parts(gpu, vd, case):
    """1, 3 and 5 frames in parts of 96 and 192 stages, host and device entry points"""
    fam, opt, pattern, terminated = case
    kind = kind_of(fam, terminated)
    with vd.ViterbiCUDA(opt) as d:
        for pb in PART_BITS:
            d.set_frame_part_bits(pb)
            assert d.frame_part_bits() == pb
            for S in (TB_SIZES if kind == "tb" else SIZES):
                data = family_data(vd, fam, S, S, pattern, terminated)
                ref = oracle_parts_frames(vd, opt, kind, NFRAMES, S, pb, S, pattern)
                for n in (1, 3, 5):
                    host = host_run(d, fam, data[:n], S, pattern, terminated)
                    assert host.dtype == ref.dtype and np.array_equal(host, ref[:n]), (pb, S, n, np.argwhere(host != ref[:n])[:5])
                    dev = device_run(d, fam, data[:n], S, pattern, terminated)
                    assert np.array_equal(dev, host), (pb, S, n)


@pytest.mark.gpu
@pytest.mark.parametrize("opt", OPTIONS6, ids=name)
@pytest.mark.parametrize("fam", ["frm", "tb"])
def test_noisy_frames_decode_in_parts_not_whole(gpu, vd, fam, opt):
    """sigma 0.9, 1000 stages, parts of 96: the words are the oracle's part-wise words, which differ from the whole-frame
    words that the same buffers give with part length 0"""
    kind = kind_of(fam, True)
    data = family_data(vd, fam, NOISY_S, NOISY_SEED, None, True, NOISY_N, NOISY_SIGMA)
    ref = oracle_parts_frames(vd, opt, kind, NOISY_N, NOISY_S, NOISY_PART_BITS, NOISY_SEED, sigma=NOISY_SIGMA)
    with vd.ViterbiCUDA(opt) as d:
        whole = host_run(d, fam, data, NOISY_S, None, True)
        d.set_frame_part_bits(NOISY_PART_BITS)
        host = host_run(d, fam, data, NOISY_S, None, True)
        dev = device_run(d, fam, data, NOISY_S, None, True)
    assert np.array_equal(host, ref), np.argwhere(host != ref)[:5]
    assert np.array_equal(dev, ref)
    assert (whole != ref).any()


LENGTHS = [0, 1, 96, 97, 250, 1_000_000, 193, 0, 33, 249]
MAXBITS = 250
GUARDED = [("frm", SOFT8 | M_B16, None, True), ("frm", SOFT16 | M_B32, None, False), ("frm", HARD | M_B32 | O_B16, None, True),
           ("tb", FP32 | M_FP16 | O_B16, None, True), ("tb", HARD | M_B32, None, True), ("pun", SOFT8 | M_B32 | O_B16, (3, 5, 3), True),
           ("pun", SOFT4 | M_FP16, (16, 0x8000, 0), False), ("ptb", SOFT8 | M_B16, (2, 1, 3), True),
           ("ptb", SOFT16 | M_B32 | O_B16, (3, 5, 3), True)]


@pytest.mark.gpu
@pytest.mark.parametrize("pb", PART_BITS)
@pytest.mark.parametrize("case", GUARDED, ids=cid)
def test_variable_lengths_between_nan_guards_and_sentinels(gpu, vd, case, pb):
    """a device lengths array with 0, 1, 96, 97, maxFrameBits and larger values (clamped); frames at an odd stride with
    NaN in every float that belongs to no frame, the outputs inside a buffer of sentinel bytes: each frame equals the
    oracle of its parts on its own words, every other byte (the words of empty frames too) keeps the sentinel"""
    import torch
    fam, opt, pattern, terminated = case
    kind = kind_of(fam, terminated)
    n = len(LENGTHS)
    unit = 8 if pattern is None else 4  # the stride: an odd multiple of the family's alignment
    istride, ostride = (8 * (MAXBITS + 1) if pattern is None else 4 * (2 * MAXBITS + 3)), 4 * 8 + 8
    assert (istride // unit) % 2 == 1 and istride >= 8 * MAXBITS
    host_in = np.full(n * istride // 4 + 2, np.nan, dtype=np.float32)
    want = []
    for f, L in enumerate(LENGTHS):
        S = min(L, MAXBITS)
        want.append(None)
        if S:  # frame f: a frame of its own S stages
            v = family_frames(kind, n, S, 200 + S)[1][f]
            rx = vd.puncture(v, pattern) if pattern is not None else v
            host_in[2 + f * istride // 4: 2 + f * istride // 4 + rx.size] = rx
            want[f] = oracle_parts(vd, opt, stream_of(vd, opt, kind, rx, S, pattern), pb)
    inp = torch.from_numpy(host_in).cuda()
    lens = torch.from_numpy(np.array(LENGTHS, dtype=np.uint32).view(np.int32)).cuda()
    out = torch.full((n * ostride + 16,), 0xA5, dtype=torch.uint8, device="cuda")
    with vd.ViterbiCUDA(opt) as d:
        d.set_frame_part_bits(pb)
        device_call(d, fam, inp.data_ptr() + 8, istride, out.data_ptr() + 8, ostride, MAXBITS, n, pattern, terminated,
                    lens=lens.data_ptr())
        torch.cuda.synchronize()
    got = out.cpu().numpy()
    untouched = np.ones(got.size, dtype=bool)
    for f, L in enumerate(LENGTHS):
        S = min(L, MAXBITS)
        nb = 4 * ((S + 31) // 32)
        lo = 8 + f * ostride
        if S:
            assert np.array_equal(got[lo:lo + nb].view(want[f].dtype), want[f]), (f, L)
        untouched[lo:lo + nb] = False
    assert (got[untouched] == 0xA5).all()


@pytest.mark.gpu
@pytest.mark.parametrize("opt", [SOFT8 | M_B16, SOFT16 | M_B32 | O_B16], ids=name)
def test_one_part_and_part_length_zero_are_the_whole_frame_launch(gpu, vd, opt):
    """part_bits >= the frame length (one part) and part_bits = 0 give the words of the whole-frame launch of the same
    buffers, on the noisy set too, where parts would show"""
    S, n = NOISY_S, NOISY_N
    for fam, kind in (("frm", "term"), ("tb", "tb")):
        for sigma in (0.3, NOISY_SIGMA):
            data = family_frames(kind, n, S, NOISY_SEED, sigma)[1]
            with vd.ViterbiCUDA(opt) as d:
                whole = host_run(d, fam, data, S, None, True)
                if sigma == 0.3:
                    ref = oracle_frames(vd, opt, n, S, True, NOISY_SEED) if fam == "frm" else oracle_tb_frames(vd, opt, n, S, NOISY_SEED)
                    assert np.array_equal(whole, ref)
                for pb in (1056, 3072, 1048512, 0):
                    d.set_frame_part_bits(pb)
                    assert np.array_equal(host_run(d, fam, data, S, None, True), whole), (fam, sigma, pb)
                    assert np.array_equal(device_run(d, fam, data, S, None, True), whole), (fam, sigma, pb)


@pytest.mark.gpu
def test_errors(gpu, vd):
    with vd.ViterbiCUDA(SOFT8 | M_B16) as d:
        for pb in (1, 32, 48, 95, 97, 128, 1 << 20, 1048512 + 96, 1 << 32):
            with pytest.raises(vd.VitdecError, match="VD_ERR_ARG.*partBits"):
                d.set_frame_part_bits(pb)
            assert d.frame_part_bits() == 0
        for pb in (96, 1048512, 0, 192):
            d.set_frame_part_bits(pb)
            assert d.frame_part_bits() == pb
        # 2^20 frames of 2^20 stages in parts of 96 stages: 2731 workgroups a frame, more than 2^31 - 1 in all; through the
        # arguments alone (checked before any pointer is used)
        d.set_frame_part_bits(96)
        big = dict(maxFrameBits=1 << 20, nframes=1 << 20)
        with pytest.raises(vd.VitdecError, match="VD_ERR_ARG.*workgroups"):
            d.run_device_frames(16, 8 << 20, 16, 1 << 17, **big)
        with pytest.raises(vd.VitdecError, match="VD_ERR_ARG.*workgroups"):
            d.run_device_tb_frames(16, 8 << 20, 16, 1 << 17, **big)
        with pytest.raises(vd.VitdecError, match="VD_ERR_ARG.*workgroups"):
            d.run_device_punct_frames(16, 8 << 20, 16, 1 << 17, pattern=(3, 5, 3), **big)
        with pytest.raises(vd.VitdecError, match="VD_ERR_ARG.*workgroups"):
            d.run_device_punct_tb_frames(16, 8 << 20, 16, 1 << 17, pattern=(3, 5, 3), **big)
        rc = vd.lib().vd_run_frames(d._h, 16, 8 << 20, 16, 1 << 17, None, 1 << 20, 1 << 20, 1, SCALE, ctypes.byref(ctypes.c_float()))
        assert rc == -2 and b"workgroups" in vd.lib().vd_last_error()
        # 786336 such frames fit the grid (the check passes; the next one, the null lengths pointer aside, is the device's)
        with pytest.raises(vd.VitdecError, match="VD_ERR_ARG.*workgroups"):
            d.run_device_frames(16, 8 << 20, 16, 1 << 17, maxFrameBits=1 << 20, nframes=786337)
        d.set_frame_part_bits(0)
        with pytest.raises(vd.VitdecError, match="VD_ERR_ARG.*maxFrameBits"):
            d.run_device_frames(16, 8 << 21, 16, 1 << 18, maxFrameBits=(1 << 20) + 1, nframes=4)


@pytest.mark.gpu
@pytest.mark.parametrize("opt", [SOFT8 | M_B16, FP32 | M_FP16 | O_B16, SOFT16 | M_B32], ids=name)
def test_kernel_name_tells_the_parts(gpu, vd, opt):
    with vd.ViterbiCUDA(opt) as d:
        for llr in (3, 4, 5, 6):
            d.set_frame_part_bits(0)
            whole = d.kernel_for(1000, 5, llr)
            assert whole.startswith("vd_decode_tg<FRM+") and "parts" not in whole
            d.set_frame_part_bits(96)
            assert d.kernel_for(1000, 5, llr) == whole + ", 11 parts per frame: one part per wave"
            assert d.kernel_for(96, 5, llr) == whole
            d.set_frame_part_bits(192)
            assert d.kernel_for(1000, 7, llr) == whole + ", 6 parts per frame: one part per wave"
            d.set_frame_part_bits(1056)
            assert d.kernel_for(1000, 5, llr) == whole
            d.set_frame_part_bits(96)
            assert d.kernel_for(1 << 20, 1 << 20, llr) == "-"


@pytest.mark.gpu
@pytest.mark.parametrize("opt", [SOFT8 | M_B32, SOFT8 | M_B16, FP32 | M_FP16, SOFT16 | M_B32], ids=name)
def test_lds_guard_words_stay_intact(gpu, vd, opt):
    S = 1000
    with vd.ViterbiCUDA(opt) as d:
        d.set_guard_check(True)
        for pb in PART_BITS:
            d.set_frame_part_bits(pb)
            for fam, pattern in (("frm", None), ("tb", None), ("pun", (3, 5, 3)), ("ptb", (2, 1, 3))):
                data = family_data(vd, fam, S, S, pattern, True)
                out = host_run(d, fam, data, S, pattern, True)
                assert np.array_equal(out, oracle_parts_frames(vd, opt, kind_of(fam, True), NFRAMES, S, pb, S, pattern))
        assert d.guard_violations() == 0


@pytest.mark.gpu
def test_graph_capture_keeps_the_part_length_it_was_captured_with(gpu, vd):
    import torch
    opt, S, n, pb = SOFT8 | M_B16, NOISY_S, NOISY_N, NOISY_PART_BITS
    vals = family_frames("term", n, S, NOISY_SEED, NOISY_SIGMA)[1]
    ref = oracle_parts_frames(vd, opt, "term", n, S, pb, NOISY_SEED, sigma=NOISY_SIGMA)
    row = 4 * ((S + 31) // 32)
    with vd.ViterbiCUDA(opt) as d:
        d.set_frame_part_bits(pb)
        s = torch.cuda.Stream()
        inp = torch.from_numpy(np.array(vals)).cuda()
        out = torch.zeros(n * row // 4, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            d.run_device_frames(inp.data_ptr(), 8 * S, out.data_ptr(), row, S, n, True, SCALE,
                                stream=torch.cuda.current_stream().cuda_stream)
        d.set_frame_part_bits(0)  # read on the host at the call: the graph's launch keeps 96
        for _ in range(2):
            out.zero_()
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            assert np.array_equal(out.cpu().numpy().view(np.uint32).reshape(n, -1), ref)
        del g


@pytest.mark.gpu
def test_two_long_frames_in_parts_of_3072(gpu, vd):
    """2 terminated frames of 65,569 stages (2050 words: 21 parts of 96 words and one of 34) at sigma 0.3: the oracle's
    part-wise words, and 0 bit errors"""
    opt, S, n, pb = SOFT8 | M_B16, 65_569, 2, 3072
    bits, vals = frames(n, S, True, seed=65)
    with vd.ViterbiCUDA(opt) as d:
        d.set_frame_part_bits(pb)
        assert d.kernel_for(S, n, 3).endswith(", 22 parts per frame: one part per wave")
        out = host_run(d, "frm", vals, S, None, True)
        dev = device_run(d, "frm", vals, S, None, True)
    assert np.array_equal(dev, out)
    assert np.array_equal(out, oracle_parts_frames(vd, opt, "term", n, S, pb, 65))
    for b, w in zip(bits, out):
        assert int((decoded_bits(opt, w, S) != b).sum()) == 0
