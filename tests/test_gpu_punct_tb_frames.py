"""GPU parity of punctured tail-biting frame decodes (vd_run_punct_tb_frames / vd_run_device_punct_tb_frames; kernels
vd_decode_tg<FRM+TB+PUN+...>): every frame of a launch equals, word for word, the oracle's one-chunk decode of
vitdec.wrap_frame(vitdec.depuncture(its received values)) -- the tail-biting decode of the depunctured frame, the
pattern's phase that of the frame stage, restarting at every wrap.  Inputs: the noisy BPSK tail-biting frames of
tb_common.py (sigma 0.2), punctured by vitdec.puncture, scale 40000 unless a test says otherwise.  The index
arithmetic alone, and the definition on the CPU: tests/test_punct_tb_frames.py."""
import numpy as np
import pytest

import tie_patterns
from frames_common import SCALE, decoded_bits, frames
from ptb_common import P16, P23, P34, P78, PNONE, PTB_SIZES, SIGMA, oracle_ptb_frame, oracle_ptb_frames, pid, punctured
from tb_common import oracle_tb_frame, oracle_tb_frames, tb_frames, wrapped_bits
from test_gpu_parity import VALID, name
from test_gpu_punct_frames import oracle_punct_frames
from vitdec import DPX, FP32, HARD, M_B16, M_B32, M_FP16, O_B16, SOFT8, SOFT16

NON_HARD = [o for o in VALID if (o & 0xF) != HARD]
MANY = (33, 97, 250)  # 64 frames at these lengths
LONG_PERIODS = (SOFT8 | M_B16, SOFT16 | M_B32)  # the options that also take the period-7 and period-16 patterns


def device_ptb_frames(d, rx, S, pattern, scale=SCALE):
    """run_device_punct_tb_frames of the rows of rx (n frames of S stages, packed back to back) on the current stream"""
    import torch
    n, L = rx.shape
    row = 4 * ((S + 31) // 32)
    inp = torch.from_numpy(np.ascontiguousarray(rx).reshape(-1)).cuda() if rx.size else torch.zeros(4, device="cuda")
    out = torch.zeros(n * row // 4, dtype=torch.int32, device="cuda")
    d.run_device_punct_tb_frames(inp.data_ptr(), 4 * L, out.data_ptr(), row, S, n, pattern, scale,
                                 stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return out.cpu().numpy().view(d.decPack_t).reshape(n, -1)


@pytest.mark.gpu
@pytest.mark.parametrize("opt", NON_HARD, ids=name)
def test_punctured_tb_frames_equal_the_oracle_of_the_depunctured_extended_stream(gpu, vd, opt):
    """1, 3 and 5 frames (3 and 5: a partial workgroup and a wave with nothing to do) at every length, 64 at three,
    at 2/3 and 3/4; SOFT8 / M_B16 and SOFT16 / M_B32 also at 7/8 and a period-16 pattern.  The lengths include ones
    that are no multiple of the period, shorter than it and under 96: the phase restart, the several-turn wrap and
    the two-pair select"""
    with vd.ViterbiCUDA(opt) as d:
        for pattern in (P23, P34) + ((P78, P16) if opt in LONG_PERIODS else ()):
            for S in PTB_SIZES:
                most = 64 if S in MANY else 5
                vals = tb_frames(most, S, seed=S, sigma=SIGMA)[1]
                ref = oracle_ptb_frames(vd, opt, pattern, most, S, seed=S)
                rx = punctured(vd, vals, pattern)
                assert rx.shape[1] == vd.punctured_len(pattern, 2 * S)
                for n in (1, 3, 5) + ((64,) if S in MANY else ()):
                    host, _ = d.run_punct_tb_frames(rx[:n], pattern, S, SCALE)
                    assert host.dtype == ref.dtype and np.array_equal(host, ref[:n]), \
                        (pattern, S, n, np.argwhere(host != ref[:n])[:5])
                    dev = device_ptb_frames(d, rx[:n], S, pattern)
                    assert np.array_equal(dev, ref[:n]), (pattern, S, n, np.argwhere(dev != ref[:n])[:5])


@pytest.mark.gpu
@pytest.mark.parametrize("opt", NON_HARD, ids=name)
def test_unpunctured_pattern_equals_run_tb_frames_of_the_same_buffer(gpu, vd, opt):
    with vd.ViterbiCUDA(opt) as d:
        for S in (5, 33, 97, 250):
            vals = tb_frames(5, S, seed=S, sigma=SIGMA)[1]
            want, _ = d.run_tb_frames(vals, SCALE)
            got, _ = d.run_punct_tb_frames(vals, (1, 1, 1), S, SCALE)
            assert np.array_equal(got, want), (S, np.argwhere(got != want)[:5])
            assert np.array_equal(device_ptb_frames(d, np.array(vals), S, (1, 1, 1)), want)


LENGTHS = [0, 1, 250, 300, 33, 0, 1_000_000, 97, 32, 249, 5, 70]
MAXBITS = 250


@pytest.mark.gpu
@pytest.mark.parametrize("pattern", [P34, P16], ids=pid)
@pytest.mark.parametrize("opt", [SOFT8 | M_B16, SOFT16 | M_B32, FP32 | M_FP16 | O_B16], ids=name)
def test_variable_lengths_between_nan_guards_and_sentinels(gpu, vd, opt, pattern):
    """a device lengths array (in stages) with 0, 1, maxFrameBits and values above it (clamped); the base pointer 4-
    but not 8-byte aligned, the stride an odd number of floats and larger than needed, NaN in every float that
    belongs to no frame -- the float right after each frame's punctured_len(2 S_f) included -- and the outputs
    inside sentinel bytes.  The wrap's characteristic failure is a read of the neighbouring frame or of the floats
    between the frames: a NaN read into the table changes the words, so each frame equal to the oracle on its own
    values proves that nothing outside its received floats was read; every other byte (the words of empty frames
    too) keeps the sentinel"""
    import torch
    n = len(LENGTHS)
    fstride = vd.punctured_len(pattern, 2 * MAXBITS) + 3
    fstride += 1 - fstride % 2  # odd: the stride is no multiple of 8 bytes
    ostride = 4 * 8 + 8
    host_in = np.full(1 + n * fstride + 8, np.nan, dtype=np.float32)
    want = []
    for f, L in enumerate(LENGTHS):
        S = min(L, MAXBITS)
        if S:  # frame f: a tail-biting frame of its own S stages, the phase at 0
            rx = vd.puncture(tb_frames(n, S, seed=300 + S, sigma=SIGMA)[1][f], pattern)
            assert rx.size == vd.punctured_len(pattern, 2 * S) < fstride
            host_in[1 + f * fstride: 1 + f * fstride + rx.size] = rx
            want.append(oracle_ptb_frame(vd, opt, rx, pattern, S))
        else:
            want.append(None)
    inp = torch.from_numpy(host_in).cuda()
    assert inp.data_ptr() % 8 == 0 and (4 * fstride) % 8 == 4
    lens = torch.from_numpy(np.array(LENGTHS, dtype=np.uint32).view(np.int32)).cuda()
    out = torch.full((n * ostride + 16,), 0xA5, dtype=torch.uint8, device="cuda")
    with vd.ViterbiCUDA(opt) as d:
        d.run_device_punct_tb_frames(inp.data_ptr() + 4, 4 * fstride, out.data_ptr() + 8, ostride, MAXBITS, n, pattern, SCALE,
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
@pytest.mark.parametrize("opt", [SOFT8 | M_B16, SOFT16 | M_B32, FP32 | M_B32 | O_B16], ids=name)
def test_frames_without_a_kept_value(gpu, vd, opt):
    """(16, 0x8000, 0) keeps the first output of every 16th stage only: frames of 1, 5 and 15 stages hold no value and
    decode, in a buffer of NaN, as the all-zero tail-biting frame; frames of 16 and 17 stages read exactly one
    float (the NaN after it stays unread)"""
    with vd.ViterbiCUDA(opt) as d:
        for S, kept in ((1, 0), (5, 0), (15, 0), (16, 1), (17, 1)):
            n = 5
            vals = tb_frames(n, S, seed=400 + S, sigma=SIGMA)[1]
            rx = punctured(vd, vals, PNONE)
            assert rx.shape == (n, kept) and vd.punctured_len(PNONE, 2 * S) == kept
            ref = np.stack([oracle_ptb_frame(vd, opt, r, PNONE, S) for r in rx])
            if kept == 0:
                zero = oracle_tb_frame(vd, opt, np.zeros(2 * S, dtype=np.float32))
                assert all(np.array_equal(r, zero) for r in ref)
            buf = np.full((n, 3), np.nan, dtype=np.float32)
            buf[:, :kept] = rx
            host, _ = d.run_punct_tb_frames(buf, PNONE, S, SCALE)
            assert np.array_equal(host, ref), (S, host, ref)
            assert np.array_equal(device_ptb_frames(d, buf, S, PNONE), ref), S
            if kept == 0:  # rows of no float at all
                host, _ = d.run_punct_tb_frames(rx, PNONE, S, SCALE)
                assert np.array_equal(host, ref), S


@pytest.mark.gpu
@pytest.mark.parametrize("opt", [SOFT8 | M_B16, SOFT8 | M_B32, FP32 | M_FP16, SOFT16 | M_B32], ids=name)
@pytest.mark.parametrize("kind", tie_patterns.LLR_PATTERNS)
def test_tie_dense_frames(gpu, vd, opt, kind):
    """all-zero floats and the tie-dense patterns as tail-biting frames punctured at 3/4: most add-compare-selects are
    ties, so the words are the tie rule's; compared with the oracle word for word"""
    with vd.ViterbiCUDA(opt) as d:
        for S, n in ((5, 7), (97, 6), (250, 5)):
            vals = tie_patterns.llr_pattern(opt, kind, 2 * S * n).reshape(n, 2 * S)
            rx = punctured(vd, vals, P34)
            ref = np.stack([oracle_ptb_frame(vd, opt, r, P34, S, scale=tie_patterns.LLR_SCALE) for r in rx])
            host, _ = d.run_punct_tb_frames(rx, P34, S, tie_patterns.LLR_SCALE)
            assert np.array_equal(host, ref), (S, np.argwhere(host != ref)[:5])


@pytest.mark.gpu
@pytest.mark.parametrize("opt", [SOFT8 | M_B32, SOFT8 | M_B16, FP32 | M_FP16, SOFT16 | M_B32], ids=name)
def test_lds_guard_words_stay_intact(gpu, vd, opt):
    vals = tb_frames(13, 1000, seed=1000, sigma=SIGMA)[1]
    with vd.ViterbiCUDA(opt) as d:
        d.set_guard_check(True)
        for pattern in (P34, P16):
            out, _ = d.run_punct_tb_frames(punctured(vd, vals, pattern), pattern, 1000, SCALE)
            assert np.array_equal(out, oracle_ptb_frames(vd, opt, pattern, 13, 1000, seed=1000))
        assert d.guard_violations() == 0


@pytest.mark.gpu
def test_graph_capture_on_a_single_stream(gpu, vd):
    import torch
    opt, S, n = SOFT8 | M_B16, 250, 64
    rx = punctured(vd, tb_frames(n, S, seed=S, sigma=SIGMA)[1], P34)
    L = rx.shape[1]
    with vd.ViterbiCUDA(opt) as d:
        direct = device_ptb_frames(d, rx, S, P34)
        assert np.array_equal(direct, oracle_ptb_frames(vd, opt, P34, n, S, seed=S))
        s = torch.cuda.Stream()
        inp = torch.from_numpy(rx.reshape(-1)).cuda()
        out = torch.zeros(n * 8, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):  # one kernel node: no parallel branches
            d.run_device_punct_tb_frames(inp.data_ptr(), 4 * L, out.data_ptr(), 32, S, n, P34, SCALE,
                                         stream=torch.cuda.current_stream().cuda_stream)
        out.zero_()
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy().view(np.uint32).reshape(n, -1), direct)
        del g


def loaded_hip():
    """the HIP runtime this process runs on (torch's own copy, loaded before libvitdec.so: tests/conftest.py)"""
    import ctypes
    with open("/proc/self/maps") as f:
        paths = sorted({ln.split()[-1] for ln in f if "libamdhip64.so" in ln})
    assert len(paths) == 1, paths
    return ctypes.CDLL(paths[0])


@pytest.mark.gpu
def test_a_captured_launch_is_one_kernel_node(gpu, vd):
    """the device entry point captured on a stream (the runtime's own capture calls, so that the graph can be asked):
    the graph holds exactly one node, a kernel node -- no copy, no memset, no second launch"""
    import ctypes
    import torch
    opt, S, n = SOFT8 | M_B16, 250, 64
    rx = punctured(vd, tb_frames(n, S, seed=S, sigma=SIGMA)[1], P34)
    hip = loaded_hip()
    vp, sz = ctypes.c_void_p, ctypes.c_size_t
    hip.hipStreamBeginCapture.argtypes = [vp, ctypes.c_int]
    hip.hipStreamEndCapture.argtypes = [vp, ctypes.POINTER(vp)]
    hip.hipGraphGetNodes.argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(sz)]
    hip.hipGraphNodeGetType.argtypes = [vp, ctypes.POINTER(ctypes.c_int)]
    hip.hipGraphDestroy.argtypes = [vp]
    with vd.ViterbiCUDA(opt) as d:
        s = torch.cuda.Stream()
        inp = torch.from_numpy(rx.reshape(-1)).cuda()
        out = torch.zeros(n * 8, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        graph, count, kind = vp(), sz(0), ctypes.c_int(-1)
        assert hip.hipStreamBeginCapture(s.cuda_stream, 2) == 0  # hipStreamCaptureModeRelaxed
        try:
            d.run_device_punct_tb_frames(inp.data_ptr(), 4 * rx.shape[1], out.data_ptr(), 32, S, n, P34, SCALE, stream=s.cuda_stream)
        finally:
            ended = hip.hipStreamEndCapture(s.cuda_stream, ctypes.byref(graph))
        assert ended == 0 and graph.value
        try:
            assert hip.hipGraphGetNodes(graph, None, ctypes.byref(count)) == 0
            assert count.value == 1, count.value
            node = vp()
            assert hip.hipGraphGetNodes(graph, ctypes.byref(node), ctypes.byref(count)) == 0 and count.value == 1
            assert hip.hipGraphNodeGetType(node, ctypes.byref(kind)) == 0
            assert kind.value == 0, kind.value  # hipGraphNodeTypeKernel
        finally:
            assert hip.hipGraphDestroy(graph) == 0
        torch.cuda.synchronize()
        assert int(out.abs().sum()) == 0  # captured, not run


@pytest.mark.gpu
@pytest.mark.parametrize("opt", [SOFT8 | M_B16, SOFT16 | M_B32 | O_B16], ids=name)  # (M_FP16 has no DPX mode)
def test_dpx_option_decodes_as_reg(gpu, vd, opt):
    vals = tb_frames(5, 97, seed=97, sigma=SIGMA)[1]
    with vd.ViterbiCUDA(opt | DPX) as d:
        out, _ = d.run_punct_tb_frames(punctured(vd, vals, P34), P34, 97, SCALE)
    assert np.array_equal(out, oracle_ptb_frames(vd, opt, P34, 5, 97, seed=97))


@pytest.mark.gpu
@pytest.mark.parametrize("opt", [SOFT8 | M_B16, FP32 | M_FP16 | O_B16, SOFT16 | M_B32], ids=name)
def test_kernel_name(gpu, vd, opt):
    with vd.ViterbiCUDA(opt) as d:
        for n in (1, 5, 10_000):
            nm = d.kernel_for(1000, n, 6)
            assert nm.startswith("vd_decode_tg<FRM+TB+PUN+") and "one frame per wave" in nm, nm
        assert d.kernel_for(0, 4, 6) == "-" and d.kernel_for((1 << 20) + 1, 4, 6) == "-"
        # the earlier frame launches' names are unchanged
        assert d.kernel_for(1000, 4, 3).startswith("vd_decode_tg<FRM+" + ("SOFT" if (opt & 0xF) != FP32 else "FP32"))
        assert d.kernel_for(1000, 4, 4).startswith("vd_decode_tg<FRM+PUN+")
        assert d.kernel_for(1000, 4, 5).startswith("vd_decode_tg<FRM+TB+" + ("SOFT" if (opt & 0xF) != FP32 else "FP32"))
    with vd.ViterbiCUDA(SOFT8 | M_B16) as d:
        assert d.kernel_for(1000, 4, 6).startswith("vd_decode_tg<FRM+TB+PUN+SOFT8,B16,O32> one frame per wave, ")
    with vd.ViterbiCUDA(HARD | M_B32) as d:
        assert d.kernel_for(1000, 4, 6) == "-"
        assert d.kernel_for(1000, 4, 5).startswith("vd_decode_tg<FRM+TB+HARD,") and d.kernel_for(1000, 4, 4) == "-"


@pytest.mark.gpu
@pytest.mark.parametrize("opt", [SOFT8 | M_B16, SOFT16 | M_B32], ids=name)
def test_frame_launches_on_the_same_decoder_are_unchanged(gpu, vd, opt):
    """run_tb_frames and run_punct_frames before and after a punctured tail-biting launch on one decoder object: the
    same words (shared state)"""
    S, n = 250, 5
    tb = tb_frames(n, S, seed=S)[1]
    term = frames(n, S, True, seed=S)[1]
    prx = punctured(vd, term, P34)
    ptb = punctured(vd, tb_frames(n, S, seed=S, sigma=SIGMA)[1], P34)
    with vd.ViterbiCUDA(opt) as d:
        tb0, _ = d.run_tb_frames(tb, SCALE)
        pf0, _ = d.run_punct_frames(prx, P34, S, True, SCALE)
        mid, _ = d.run_punct_tb_frames(ptb, P34, S, SCALE)
        tb1, _ = d.run_tb_frames(tb, SCALE)
        pf1, _ = d.run_punct_frames(prx, P34, S, True, SCALE)
        again, _ = d.run_punct_tb_frames(ptb, P34, S, SCALE)
    assert np.array_equal(tb0, oracle_tb_frames(vd, opt, n, S, seed=S)) and np.array_equal(tb1, tb0)
    assert np.array_equal(pf0, oracle_punct_frames(vd, opt, P34, n, S, True, seed=S)) and np.array_equal(pf1, pf0)
    assert np.array_equal(mid, oracle_ptb_frames(vd, opt, P34, n, S, seed=S)) and np.array_equal(again, mid)


@pytest.mark.gpu
def test_errors(gpu, vd):
    rx = np.zeros((4, 334), dtype=np.float32)  # 3/4 of 250 stages: 334 floats
    assert vd.punctured_len(P34, 500) == 334
    with vd.ViterbiCUDA(HARD | M_B32) as d:
        with pytest.raises(vd.VitdecError, match="VD_ERR_OPTIONS.*HARD"):
            d.run_punct_tb_frames(rx, P34, 250)
        with pytest.raises(vd.VitdecError, match="VD_ERR_OPTIONS.*HARD"):
            d.run_device_punct_tb_frames(16, 1336, 16, 32, 250, 4, P34)  # (checked before any pointer is used)
    with vd.ViterbiCUDA(SOFT8 | M_B16) as d:
        bad = [dict(pattern=(0, 1, 1)), dict(pattern=(17, 1, 1)), dict(pattern=(3, 0b1000, 0b011)), dict(pattern=(3, 0b101, 0b1011)),
               dict(pattern=(3, 0, 0)), dict(rx_ptr=18), dict(rx_stride=1338), dict(rx_stride=1332), dict(output_stride=30),
               dict(output_stride=28), dict(maxFrameBits=0), dict(maxFrameBits=(1 << 20) + 1, rx_stride=8 << 21, output_stride=1 << 18),
               dict(nframes=0), dict(nframes=-1), dict(scale=0.0), dict(scale=-40000.0), dict(scale=float("inf")),
               dict(scale=float("nan")), dict(rx_ptr=0), dict(output_ptr=0)]
        for kw in bad:
            a = dict(rx_ptr=16, rx_stride=1336, output_ptr=16, output_stride=32, maxFrameBits=250, nframes=4, pattern=P34,
                     scale=SCALE)
            a.update(kw)
            with pytest.raises(vd.VitdecError, match="VD_ERR_ARG"):
                d.run_device_punct_tb_frames(**a)
        for scale in (0.0, -1.0, float("inf"), float("nan")):
            with pytest.raises(vd.VitdecError, match="VD_ERR_ARG"):
                d.run_punct_tb_frames(rx, P34, 250, scale)
        with pytest.raises(vd.VitdecError, match="VD_ERR_ARG"):
            d.run_punct_tb_frames(rx, (17, 1, 1), 250)
        with pytest.raises(vd.VitdecError, match="received values"):
            d.run_punct_tb_frames(rx[:, :333], P34, 250)


@pytest.mark.gpu
def test_long_and_far_frames(gpu, vd):
    """one frame of 2^20 stages and five of 4099 at rate 3/4 equal the oracle (the frame beyond a 4 GiB rx_stride
    offset: test_strides_past_4_gib below)"""
    opt = SOFT8 | M_B16
    with vd.ViterbiCUDA(opt) as d:
        S = 1 << 20
        rx = punctured(vd, tb_frames(1, S, seed=20, sigma=SIGMA)[1], P34)
        out, _ = d.run_punct_tb_frames(rx, P34, S, SCALE)
        assert np.array_equal(out, oracle_ptb_frames(vd, opt, P34, 1, S, seed=20))
        assert np.array_equal(device_ptb_frames(d, rx, S, P34), out)
        S = 4099
        rx = punctured(vd, tb_frames(5, S, seed=S, sigma=SIGMA)[1], P34)
        out, _ = d.run_punct_tb_frames(rx, P34, S, SCALE)
        assert np.array_equal(out, oracle_ptb_frames(vd, opt, P34, 5, S, seed=S))
        assert np.array_equal(device_ptb_frames(d, rx, S, P34), out)


@pytest.mark.gpu
def test_strides_past_4_gib(gpu, vd):
    """2 frames of 250 stages at rate 3/4 (334 floats) 2^32 + 4 * 335 bytes apart -- no multiple of 8 --, their
    outputs 2^32 + 40 bytes apart, in uninitialised buffers (8.6 GiB, as tests/test_gpu_frames_limits.py allocates
    for the other families); at the 32-bit alias of frame 1's input offset (4 * 335 bytes in) lies a third valid
    frame, at the alias of its output offset sentinel bytes.  Frame 1's resource is built from its own base,
    rx_d + rx_stride, over its 1336 received bytes: it equals the oracle of its own values and the alias keeps the
    sentinel, where an offset truncated to 32 bits reads and writes inside the same allocations and shows as wrong
    words"""
    import torch
    opt, S, nb = SOFT8 | M_B16, 250, 32
    istride, ostride = (1 << 32) + 4 * 335, (1 << 32) + 40
    rows = punctured(vd, tb_frames(3, S, seed=4000 + S, sigma=SIGMA)[1], P34)
    assert istride % 8 == 4 and ostride % 4 == 0 and 4 * rows.shape[1] == 1336 <= 4 * 335
    refs = oracle_ptb_frames(vd, opt, P34, 3, S, seed=4000 + S)
    assert not np.array_equal(refs[1], refs[2]) and not np.array_equal(refs[1], refs[0])
    inp = torch.empty(istride + 4 * 335, dtype=torch.uint8, device="cuda")
    out = torch.empty(ostride + 64, dtype=torch.uint8, device="cuda")
    assert inp.data_ptr() % 4 == 0 and out.data_ptr() % 4 == 0
    for at, r in ((0, rows[0]), (istride, rows[1]), (istride - (1 << 32), rows[2])):
        inp[at: at + 4 * r.size] = torch.from_numpy(np.array(r).view(np.uint8))
    out[:128] = 0xA5
    out[ostride - 64:] = 0xA5
    with vd.ViterbiCUDA(opt) as d:
        d.run_device_punct_tb_frames(inp.data_ptr(), istride, out.data_ptr(), ostride, S, 2, P34, SCALE,
                                     stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
    low, high = out[:128].cpu().numpy(), out[ostride - 64:].cpu().numpy()
    del inp, out
    torch.cuda.empty_cache()  # (8.6 GiB back to the device, not kept in the allocator's pool for the rest of the session)
    assert np.array_equal(high[64:64 + nb].view(refs.dtype), refs[1]), "frame 1"
    assert np.array_equal(low[:nb].view(refs.dtype), refs[0]), "frame 0"
    assert (low[nb:] == 0xA5).all(), "the 32-bit alias of frame 1's output offset (bytes 40 .. 72) was written"
    assert (high[:64] == 0xA5).all() and (high[64 + nb:] == 0xA5).all()


@pytest.mark.gpu
@pytest.mark.parametrize("opt", [SOFT8 | M_B16, SOFT16 | M_B32], ids=name)
@pytest.mark.parametrize("pattern", [P34, P23], ids=pid)
def test_every_bit_of_256_frames(gpu, vd, opt, pattern):
    """256 punctured tail-biting frames of 1000 stages at sigma 0.2 (seed 2560) decode with 0 errors over all 256,000
    bits, and the 24 bits past each frame decode the wrap"""
    n, S = 256, 1000
    bits, vals = tb_frames(n, S, seed=2560, sigma=0.2)
    with vd.ViterbiCUDA(opt) as d:
        out, _ = d.run_punct_tb_frames(punctured(vd, vals, pattern), pattern, S, SCALE)
    got = np.stack([decoded_bits(opt, w, 1024) for w in out])
    assert int((got[:, :S] != bits).sum()) == 0
    assert np.array_equal(got, np.stack([wrapped_bits(b, 1024) for b in bits]))
