"""GPU parity of tail-biting frame decodes (vd_run_tb_frames / vd_run_device_tb_frames; kernels
vd_decode_tg<FRM+TB+...>): every frame of a launch equals, word for word, the oracle's one-chunk decode of
vitdec.wrap_frame(frame) -- stage p of the extended stream is frame stage (p - 26) mod S -- so a tail-biting frame
decodes from its first bit to its last in one pass.  Inputs: BPSK +-1 frames from the numpy tail-biting encoder of
tb_common.py with Gaussian noise, sigma 0.3, scale 40000 unless a test says otherwise.  The geometry alone, and the
definition on the CPU: tests/test_tb_frames.py."""
import numpy as np
import pytest

import tie_patterns
from frames_common import SCALE, decoded_bits, frames, oracle_frames
from tb_common import TB_SIZES, oracle_tb_frame, oracle_tb_frames, tb_frames, wrapped_bits
from test_gpu_parity import VALID, name
from vitdec import DPX, FP32, HARD, M_B16, M_B32, M_FP16, O_B16, SOFT4, SOFT8, SOFT16

MANY = (33, 97, 250)  # 64 frames at these lengths


def device_tb_frames(d, vals, S, scale=SCALE):
    """run_device_tb_frames of the rows of vals (n frames of S stages, packed back to back) on the current stream"""
    import torch
    n = vals.shape[0]
    row = 4 * ((S + 31) // 32)
    inp = torch.from_numpy(np.array(vals)).cuda()
    out = torch.zeros(n * row // 4, dtype=torch.int32, device="cuda")
    d.run_device_tb_frames(inp.data_ptr(), 8 * S, out.data_ptr(), row, S, n, scale,
                           stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return out.cpu().numpy().view(d.decPack_t).reshape(n, -1)


@pytest.mark.gpu
@pytest.mark.parametrize("opt", VALID, ids=name)
def test_tb_frames_equal_the_oracle_of_the_extended_stream(gpu, vd, opt):
    """1, 3 and 5 frames (3 and 5: a partial workgroup and a wave with nothing to do) at every length, 64 at three"""
    with vd.ViterbiCUDA(opt) as d:
        for S in TB_SIZES:
            most = 64 if S in MANY else 5
            vals = tb_frames(most, S, seed=S)[1]
            ref = oracle_tb_frames(vd, opt, most, S, seed=S)
            for n in (1, 3, 5) + ((64,) if S in MANY else ()):
                host, _ = d.run_tb_frames(vals[:n], SCALE)
                assert host.dtype == ref.dtype and np.array_equal(host, ref[:n]), (S, n, np.argwhere(host != ref[:n])[:5])
                dev = device_tb_frames(d, vals[:n], S)
                assert np.array_equal(dev, ref[:n]), (S, n, np.argwhere(dev != ref[:n])[:5])


@pytest.mark.gpu
@pytest.mark.parametrize("opt,amp", [(SOFT8 | M_B16, 100.0), (SOFT16 | M_B32, 20000.0)], ids=["s8-b16", "s16-b32"])
def test_values_in_code_units_at_scale_one(gpu, vd, opt, amp):
    """values already in the format's code units, scale 1"""
    with vd.ViterbiCUDA(opt) as d:
        for S in (5, 33, 250):
            bits, unit = tb_frames(5, S, seed=100 + S)
            vals = (unit * np.float32(amp)).astype(np.float32)
            ref = np.stack([oracle_tb_frame(vd, opt, v, scale=1.0) for v in vals])
            host, _ = d.run_tb_frames(vals, 1.0)
            assert np.array_equal(host, ref)
            assert np.array_equal(device_tb_frames(d, vals, S, scale=1.0), ref)
            if S >= 7:  # (shorter frames than the constraint length may err: the code, not the decoder)
                for b, w in zip(bits, host):
                    assert np.array_equal(decoded_bits(opt, w, S), b)


LENGTHS = [0, 1, 250, 300, 33, 0, 1_000_000, 97, 32, 249, 5, 70]
MAXBITS = 250


@pytest.mark.gpu
@pytest.mark.parametrize("opt", [SOFT8 | M_B16, SOFT8 | M_B32, SOFT16 | M_B32, FP32 | M_FP16 | O_B16, HARD | M_B32,
                                 SOFT4 | M_B32 | O_B16], ids=name)
def test_variable_lengths_between_nan_guards_and_sentinels(gpu, vd, opt):
    """a device lengths array with 0, 1, maxFrameBits and values above it (clamped); the input stride an odd multiple
    of 8 with NaN in every float that belongs to no frame, the outputs inside a buffer of sentinel bytes.  The wrap's
    characteristic failure is a read of the neighbouring frame or of the floats between the frames: a NaN read into
    the table changes the words, so each frame equal to the oracle on its own values proves that nothing outside
    its 2 S_f floats was read; every byte outside the frames' words (those of empty frames too) keeps the sentinel"""
    import torch
    n = len(LENGTHS)
    istride, ostride = 8 * (MAXBITS + 1), 4 * 8 + 8
    assert (istride // 8) % 2 == 1
    host_in = np.full(n * istride // 4 + 4, np.nan, dtype=np.float32)
    want = []
    for f, L in enumerate(LENGTHS):
        S = min(L, MAXBITS)
        if S:  # frame f: a tail-biting frame of its own S stages
            v = tb_frames(n, S, seed=200 + S)[1][f]
            host_in[2 + f * istride // 4: 2 + f * istride // 4 + 2 * S] = v
        want.append(oracle_tb_frame(vd, opt, v) if S else None)
    inp = torch.from_numpy(host_in).cuda()
    lens = torch.from_numpy(np.array(LENGTHS, dtype=np.uint32).view(np.int32)).cuda()
    out = torch.full((n * ostride + 16,), 0xA5, dtype=torch.uint8, device="cuda")
    with vd.ViterbiCUDA(opt) as d:
        d.run_device_tb_frames(inp.data_ptr() + 8, istride, out.data_ptr() + 8, ostride, MAXBITS, n, SCALE,
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
def test_host_lengths_array_keeps_unwritten_words(gpu, vd):
    """run_tb_frames with frame_bits: shorter frames decode their own stages, the words past them stay 0"""
    opt, S, n = SOFT8 | M_B16, 97, 6
    vals = np.array(tb_frames(n, S, seed=S)[1])
    lens = np.array([97, 0, 33, 97, 500, 1], dtype=np.uint32)
    feed = np.full_like(vals, np.nan)
    want = np.zeros((n, 4), dtype=np.uint32)
    for f, L in enumerate(lens):
        s = min(int(L), S)
        if s:
            v = tb_frames(n, s, seed=300 + s)[1][f]
            feed[f, :2 * s] = v
            want[f, :(s + 31) // 32] = oracle_tb_frame(vd, opt, v)
    with vd.ViterbiCUDA(opt) as d:
        out, _ = d.run_tb_frames(feed, SCALE, frame_bits=lens)
    assert np.array_equal(out, want)


@pytest.mark.gpu
@pytest.mark.parametrize("opt", [SOFT8 | M_B16, SOFT8 | M_B32, FP32 | M_FP16, SOFT16 | M_B32, HARD | M_B16], ids=name)
@pytest.mark.parametrize("kind", tie_patterns.LLR_PATTERNS)
def test_tie_dense_frames(gpu, vd, opt, kind):
    """all-zero floats and the tie-dense patterns as tail-biting frames: most add-compare-selects are ties, so the
    words are the tie rule's; compared with the oracle word for word"""
    with vd.ViterbiCUDA(opt) as d:
        for S, n in ((5, 7), (97, 6), (250, 5)):
            vals = tie_patterns.llr_pattern(opt, kind, 2 * S * n).reshape(n, 2 * S)
            ref = np.stack([oracle_tb_frame(vd, opt, v, scale=tie_patterns.LLR_SCALE) for v in vals])
            host, _ = d.run_tb_frames(vals, tie_patterns.LLR_SCALE)
            assert np.array_equal(host, ref), (S, np.argwhere(host != ref)[:5])


@pytest.mark.gpu
@pytest.mark.parametrize("opt", [SOFT8 | M_B32, SOFT8 | M_B16, FP32 | M_FP16, SOFT16 | M_B32, HARD | M_B32], ids=name)
def test_lds_guard_words_stay_intact(gpu, vd, opt):
    vals = tb_frames(13, 1000, seed=1000)[1]
    with vd.ViterbiCUDA(opt) as d:
        d.set_guard_check(True)
        out, _ = d.run_tb_frames(vals, SCALE)
        assert d.guard_violations() == 0
    assert np.array_equal(out, oracle_tb_frames(vd, opt, 13, 1000, seed=1000))


@pytest.mark.gpu
def test_graph_capture_on_a_single_stream(gpu, vd):
    import torch
    opt, S, n = SOFT8 | M_B16, 250, 64
    vals = tb_frames(n, S, seed=S)[1]
    with vd.ViterbiCUDA(opt) as d:
        direct = device_tb_frames(d, vals, S)
        assert np.array_equal(direct, oracle_tb_frames(vd, opt, n, S, seed=S))
        s = torch.cuda.Stream()
        inp = torch.from_numpy(np.array(vals)).cuda()
        out = torch.zeros(n * 8, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):  # one kernel node: no parallel branches
            d.run_device_tb_frames(inp.data_ptr(), 8 * S, out.data_ptr(), 32, S, n, SCALE,
                                   stream=torch.cuda.current_stream().cuda_stream)
        out.zero_()
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy().view(np.uint32).reshape(n, -1), direct)
        del g


@pytest.mark.gpu
def test_errors(gpu, vd):
    vals = np.zeros((4, 2 * 250), dtype=np.float32)
    with vd.ViterbiCUDA(SOFT8 | M_B16) as d:
        # (the pointers are never used: the checks come first)
        bad = [dict(llr_stride=2004), dict(llr_stride=1992), dict(output_stride=30), dict(output_stride=28), dict(llr_ptr=20),
               dict(maxFrameBits=0), dict(maxFrameBits=(1 << 20) + 1, llr_stride=8 << 21, output_stride=1 << 18),
               dict(scale=0.0), dict(scale=-40000.0), dict(scale=float("inf")), dict(scale=float("nan")), dict(nframes=0),
               dict(nframes=-1), dict(llr_ptr=0), dict(output_ptr=0)]
        for kw in bad:
            a = dict(llr_ptr=16, llr_stride=2000, output_ptr=16, output_stride=32, maxFrameBits=250, nframes=4, scale=SCALE)
            a.update(kw)
            with pytest.raises(vd.VitdecError, match="VD_ERR_ARG"):
                d.run_device_tb_frames(**a)
        for scale in (0.0, -1.0, float("inf"), float("nan")):
            with pytest.raises(vd.VitdecError, match="VD_ERR_ARG"):
                d.run_tb_frames(vals, scale)
    with vd.ViterbiCUDA(HARD | M_B32) as d:  # every format decodes: HARD gets the same VD_ERR_ARG, no VD_ERR_OPTIONS
        with pytest.raises(vd.VitdecError, match="VD_ERR_ARG"):
            d.run_device_tb_frames(16, 1992, 16, 32, 250, 4)


@pytest.mark.gpu
@pytest.mark.parametrize("opt", [SOFT8 | M_B16, HARD | M_B32 | O_B16], ids=name)
def test_dpx_option_decodes_as_reg(gpu, vd, opt):
    vals = tb_frames(5, 97, seed=97)[1]
    with vd.ViterbiCUDA(opt | DPX) as d:
        out, _ = d.run_tb_frames(vals, SCALE)
    assert np.array_equal(out, oracle_tb_frames(vd, opt, 5, 97, seed=97))


@pytest.mark.gpu
@pytest.mark.parametrize("opt", [SOFT8 | M_B16, HARD | M_FP16 | O_B16, SOFT16 | M_B32], ids=name)
def test_kernel_name(gpu, vd, opt):
    with vd.ViterbiCUDA(opt) as d:
        for n in (1, 5, 10_000):
            assert d.kernel_for(1000, n, 5).startswith("vd_decode_tg<FRM+TB+"), d.kernel_for(1000, n, 5)
        assert d.kernel_for(0, 4, 5) == "-" and d.kernel_for((1 << 20) + 1, 4, 5) == "-"
        assert d.kernel_for(1000, 4, 3).startswith("vd_decode_tg<FRM+" + ("SOFT" if opt & 0xF else "HARD"))


@pytest.mark.gpu
@pytest.mark.parametrize("opt", [SOFT8 | M_B16, SOFT16 | M_B32], ids=name)
def test_frame_launches_on_the_same_decoder_are_unchanged(gpu, vd, opt):
    """run_frames before and after a tail-biting launch on one decoder object: the same words (shared state)"""
    S, n = 250, 5
    term = frames(n, S, True, seed=S)[1]
    tb = tb_frames(n, S, seed=S)[1]
    with vd.ViterbiCUDA(opt) as d:
        before, _ = d.run_frames(term, True, SCALE)
        mid, _ = d.run_tb_frames(tb, SCALE)
        after, _ = d.run_frames(term, True, SCALE)
        again, _ = d.run_tb_frames(tb, SCALE)
    assert np.array_equal(before, oracle_frames(vd, opt, n, S, True, seed=S)) and np.array_equal(after, before)
    assert np.array_equal(mid, oracle_tb_frames(vd, opt, n, S, seed=S)) and np.array_equal(again, mid)


@pytest.mark.gpu
@pytest.mark.parametrize("opt", [SOFT8 | M_B16, HARD | M_B32], ids=name)
def test_every_bit_of_256_frames(gpu, vd, opt):
    """256 tail-biting frames of 1000 stages at sigma 0.3 decode with 0 errors over all 256,000 bits, and the 24
    bits past each frame decode the wrap"""
    n, S = 256, 1000
    bits, vals = tb_frames(n, S, seed=2560, sigma=0.3)
    with vd.ViterbiCUDA(opt) as d:
        out, _ = d.run_tb_frames(vals, SCALE)
    got = np.stack([decoded_bits(opt, w, 1024) for w in out])
    assert int((got[:, :S] != bits).sum()) == 0
    assert np.array_equal(got, np.stack([wrapped_bits(b, 1024) for b in bits]))
