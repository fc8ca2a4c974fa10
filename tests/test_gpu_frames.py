"""GPU parity of frame decodes (vd_run_frames / vd_run_device_frames; kernels vd_decode_tg<FRM+...>): every frame
of a launch equals, word for word, the oracle's one-chunk decode of vitdec.pad_frame(frame) -- 26 pad stages, the
frame, then pad stages (terminated) or erasures (open) -- so a frame decodes from its first bit to its last.
Inputs: BPSK +-1 frames from the numpy encoder of frames_common.py with Gaussian noise, sigma 0.3, scale 40000
unless a test says otherwise.  The geometry alone, and the definition on the CPU: tests/test_frames.py."""
import numpy as np
import pytest

import tie_patterns
from frames_common import SCALE, decoded_bits, frames, oracle_frame, oracle_frames
from test_gpu_parity import VALID, name
from vitdec import FP32, HARD, M_B16, M_B32, M_FP16, O_B16, SOFT4, SOFT8, SOFT16

SIZES = [1, 31, 32, 33, 95, 96, 97, 250, 1000]
# every valid non-DPX option terminated and open; HARD terminated only (an erasure has no hard code)
CASES = [(o, t) for o in VALID for t in (True, False) if t or (o & 0xF) != HARD]


def cid(c):
    return f"{name(c[0])}-{'terminated' if c[1] else 'open'}"


def device_frames(d, vals, S, terminated, scale=SCALE):
    """run_device_frames of the rows of vals (n frames of S stages, packed back to back) on the current stream"""
    import torch
    n = vals.shape[0]
    row = 4 * ((S + 31) // 32)
    inp = torch.from_numpy(np.array(vals)).cuda()
    out = torch.zeros(n * row // 4, dtype=torch.int32, device="cuda")
    d.run_device_frames(inp.data_ptr(), 8 * S, out.data_ptr(), row, S, n, terminated, scale,
                        stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return out.cpu().numpy().view(d.decPack_t).reshape(n, -1)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=cid)
def test_frames_equal_the_oracle_of_the_padded_stream(gpu, vd, case):
    """1, 3, 5 and 64 frames (3 and 5: a partial workgroup and a wave with nothing to do) of 1 .. 1000 stages"""
    opt, terminated = case
    with vd.ViterbiCUDA(opt) as d:
        for S in SIZES:
            vals = frames(64, S, terminated, seed=S)[1]
            ref = oracle_frames(vd, opt, 64, S, terminated, seed=S)
            for n in (1, 3, 5, 64):
                host, _ = d.run_frames(vals[:n], terminated, SCALE)
                assert host.dtype == ref.dtype and np.array_equal(host, ref[:n]), (S, n, np.argwhere(host != ref[:n])[:5])
                dev = device_frames(d, vals[:n], S, terminated)
                assert np.array_equal(dev, host), (S, n)


@pytest.mark.gpu
@pytest.mark.parametrize("terminated", [True, False], ids=["terminated", "open"])
@pytest.mark.parametrize("opt,amp", [(SOFT8 | M_B16, 100.0), (SOFT16 | M_B32, 20000.0)], ids=["s8-b16", "s16-b32"])
def test_values_in_code_units_at_scale_one(gpu, vd, opt, amp, terminated):
    """the pad must saturate at any scale: values already in the format's code units, scale 1"""
    with vd.ViterbiCUDA(opt) as d:
        for S in (33, 250):
            bits, unit = frames(5, S, terminated, seed=100 + S)
            vals = (unit * np.float32(amp)).astype(np.float32)
            ref = np.stack([oracle_frame(vd, opt, v, terminated, scale=1.0) for v in vals])
            host, _ = d.run_frames(vals, terminated, 1.0)
            assert np.array_equal(host, ref)
            assert np.array_equal(device_frames(d, vals, S, terminated, scale=1.0), ref)
            for b, w in zip(bits, host):
                assert np.array_equal(decoded_bits(opt, w, S), b)


LENGTHS = [0, 1, 250, 300, 33, 0, 1_000_000, 97, 32, 249]
MAXBITS = 250


@pytest.mark.gpu
@pytest.mark.parametrize("case", [(SOFT8 | M_B16, True), (SOFT8 | M_B16, False), (SOFT16 | M_B32, False),
                                  (FP32 | M_FP16 | O_B16, True), (HARD | M_B32, True), (SOFT4 | M_B32 | O_B16, False)], ids=cid)
def test_variable_lengths_between_nan_guards_and_sentinels(gpu, vd, case):
    """a device lengths array with 0, 1, maxFrameBits and values above it (clamped); the input stride an odd multiple
    of 8 with NaN in every float that belongs to no frame, the outputs inside a buffer of sentinel bytes: each frame
    equals the oracle on its own words, every other byte (the words of empty frames too) keeps the sentinel"""
    import torch
    opt, terminated = case
    n = len(LENGTHS)
    istride, ostride = 8 * (MAXBITS + 1), 4 * 8 + 8
    assert (istride // 8) % 2 == 1
    host_in = np.full(n * istride // 4 + 2, np.nan, dtype=np.float32)
    want = []
    for f, L in enumerate(LENGTHS):
        S = min(L, MAXBITS)
        if S:  # frame f: a frame of its own S stages (terminated: with its own tail zeros)
            v = frames(n, S, terminated, seed=200 + S)[1][f]
            host_in[2 + f * istride // 4: 2 + f * istride // 4 + 2 * S] = v
        want.append(oracle_frame(vd, opt, v, terminated) if S else None)
    inp = torch.from_numpy(host_in).cuda()
    lens = torch.from_numpy(np.array(LENGTHS, dtype=np.uint32).view(np.int32)).cuda()
    out = torch.full((n * ostride + 16,), 0xA5, dtype=torch.uint8, device="cuda")
    with vd.ViterbiCUDA(opt) as d:
        d.run_device_frames(inp.data_ptr() + 8, istride, out.data_ptr() + 8, ostride, MAXBITS, n, terminated, SCALE,
                            frame_bits_ptr=lens.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
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
@pytest.mark.parametrize("case", [(SOFT8 | M_B16, True), (SOFT8 | M_B32, False), (FP32 | M_B16, True), (SOFT16 | M_B32 | O_B16, False)],
                         ids=cid)
def test_nothing_outside_a_frame_is_read(gpu, vd, case):
    """fixed-length frames of 97 stages at a stride of 100: NaN before the first frame, between the frames and after
    the last one gives the same words as the frames alone"""
    import torch
    opt, terminated = case
    S, n, istride = 97, 5, 8 * 100
    vals = frames(n, S, terminated, seed=5)[1]
    ref = oracle_frames(vd, opt, n, S, terminated, seed=5)
    host_in = np.full(4 + n * istride // 4 + 64, np.nan, dtype=np.float32)
    for f in range(n):
        host_in[4 + f * istride // 4: 4 + f * istride // 4 + 2 * S] = vals[f]
    inp = torch.from_numpy(host_in).cuda()
    row = 4 * 4
    out = torch.zeros(n * row // 4, dtype=torch.int32, device="cuda")
    with vd.ViterbiCUDA(opt) as d:
        d.run_device_frames(inp.data_ptr() + 16, istride, out.data_ptr(), row, S, n, terminated, SCALE,
                            stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy().view(d.decPack_t).reshape(n, -1), ref)


@pytest.mark.gpu
@pytest.mark.parametrize("opt", [SOFT8 | M_B16, SOFT8 | M_B32, FP32 | M_FP16], ids=name)
@pytest.mark.parametrize("kind", tie_patterns.LLR_PATTERNS)
def test_tie_dense_open_frames(gpu, vd, opt, kind):
    """all-zero floats and the tie-dense patterns as open frames: most add-compare-selects are ties, so the words are
    the tie rule's; compared with the oracle word for word"""
    with vd.ViterbiCUDA(opt) as d:
        for S, n in ((97, 6), (250, 5)):
            vals = tie_patterns.llr_pattern(opt, kind, 2 * S * n).reshape(n, 2 * S)
            ref = np.stack([oracle_frame(vd, opt, v, False, scale=tie_patterns.LLR_SCALE) for v in vals])
            host, _ = d.run_frames(vals, False, tie_patterns.LLR_SCALE)
            assert np.array_equal(host, ref), (S, np.argwhere(host != ref)[:5])


@pytest.mark.gpu
@pytest.mark.parametrize("opt", [SOFT8 | M_B32, SOFT8 | M_B16, FP32 | M_FP16, SOFT16 | M_B32], ids=name)
def test_lds_guard_words_stay_intact(gpu, vd, opt):
    vals = frames(64, 1000, True, seed=1000)[1]
    with vd.ViterbiCUDA(opt) as d:
        d.set_guard_check(True)
        out, _ = d.run_frames(vals[:13], True, SCALE)
        assert d.guard_violations() == 0
    assert np.array_equal(out, oracle_frames(vd, opt, 64, 1000, True, seed=1000)[:13])


@pytest.mark.gpu
def test_graph_capture_on_a_side_stream(gpu, vd):
    import torch
    opt, S, n = SOFT8 | M_B16, 250, 64
    vals = frames(n, S, True, seed=S)[1]
    with vd.ViterbiCUDA(opt) as d:
        direct = device_frames(d, vals, S, True)
        s = torch.cuda.Stream()
        inp = torch.from_numpy(np.array(vals)).cuda()
        out = torch.zeros(n * 8, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            d.run_device_frames(inp.data_ptr(), 8 * S, out.data_ptr(), 32, S, n, True, SCALE,
                                stream=torch.cuda.current_stream().cuda_stream)
        for _ in range(2):
            out.zero_()
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            assert np.array_equal(out.cpu().numpy().view(np.uint32).reshape(n, -1), direct)
        del g


@pytest.mark.gpu
def test_errors(gpu, vd):
    vals = np.zeros((4, 2 * 250), dtype=np.float32)
    with vd.ViterbiCUDA(HARD | M_B32) as d:
        with pytest.raises(vd.VitdecError, match="VD_ERR_OPTIONS.*HARD"):
            d.run_frames(vals, terminated=False)
        with pytest.raises(vd.VitdecError, match="VD_ERR_OPTIONS.*HARD"):
            d.run_device_frames(16, 2000, 16, 32, 250, 4, False)  # (checked before any pointer is used)
    with vd.ViterbiCUDA(SOFT8 | M_B16) as d:
        bad = [dict(llr_stride=2004), dict(llr_stride=1992), dict(output_stride=30), dict(output_stride=28), dict(llr_ptr=20),
               dict(maxFrameBits=0), dict(maxFrameBits=(1 << 20) + 1, llr_stride=8 << 21, output_stride=1 << 18),
               dict(scale=0.0), dict(scale=-40000.0), dict(scale=float("inf")), dict(scale=float("nan")), dict(nframes=0),
               dict(nframes=-1)]
        for kw in bad:
            a = dict(llr_ptr=16, llr_stride=2000, output_ptr=16, output_stride=32, maxFrameBits=250, nframes=4, terminated=True,
                     scale=SCALE)
            a.update(kw)
            with pytest.raises(vd.VitdecError, match="VD_ERR_ARG"):
                d.run_device_frames(**a)
        for scale in (0.0, -1.0, float("inf")):
            with pytest.raises(vd.VitdecError, match="VD_ERR_ARG"):
                d.run_frames(vals, True, scale)


@pytest.mark.gpu
@pytest.mark.parametrize("opt", [SOFT8 | M_B16, HARD | M_FP16 | O_B16, SOFT16 | M_B32], ids=name)
def test_kernel_name(gpu, vd, opt):
    with vd.ViterbiCUDA(opt) as d:
        for n in (1, 5, 10_000):
            assert d.kernel_for(1000, n, 3).startswith("vd_decode_tg<FRM+"), d.kernel_for(1000, n, 3)
        assert d.kernel_for(0, 4, 3) == "-" and d.kernel_for((1 << 20) + 1, 4, 3) == "-"


@pytest.mark.gpu
def test_every_bit_of_256_frames_and_what_the_stream_decode_loses(gpu, vd):
    """256 terminated frames of 1000 stages decode with 0 errors over all 256,000 bits; the same values as one
    concatenated stream through run_llr (a valid codeword: every frame ends in state 0) give the stream's bits
    26 .. 255,961 only -- its first 26 and last 38 bits are never decoded"""
    opt, n, S = SOFT8 | M_B16, 256, 1000
    bits, vals = frames(n, S, True, seed=2560)
    with vd.ViterbiCUDA(opt) as d:
        out, _ = d.run_frames(vals, True, SCALE)
        stream, _ = d.run_llr(vals.reshape(-1), scale=SCALE)
    got = np.stack([decoded_bits(opt, w, S) for w in out])
    assert int((got != bits).sum()) == 0
    assert stream.size * 32 == n * S - 64
    sbits = decoded_bits(opt, stream, stream.size * 32)
    assert np.array_equal(sbits, bits.reshape(-1)[26:n * S - 38])
