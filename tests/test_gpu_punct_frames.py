"""GPU parity of punctured frame decodes (vd_run_punct_frames / vd_run_device_punct_frames; kernels
vd_decode_tg<FRM+PUN+...>): every frame of a launch equals, word for word, the oracle's one-chunk decode of
vitdec.pad_frame(vitdec.depuncture(its received values)) -- the frame decode of the depunctured frame, the pattern's
phase restarting at the frame's first stage.  Inputs: the noisy BPSK frames of frames_common.py (sigma 0.3 unless a
test says otherwise), punctured by vitdec.puncture, scale 40000.  The index arithmetic alone, and the definition
on the CPU: tests/test_punct_frames.py."""
import numpy as np
import pytest

import tie_patterns
from frames_common import SCALE, decoded_bits, frames, oracle_frame
from test_gpu_parity import VALID, name
from vitdec import FP32, HARD, M_B16, M_B32, M_FP16, O_B16, SOFT8, SOFT16

P23, P34 = (2, 0b01, 0b11), (3, 0b101, 0b011)
P78 = (7, 0b1010001, 0b0101111)
P16 = (16, 0xA5C3, 0x5A3D)
PNONE = (16, 0x8000, 0)  # keeps one value in 32: frames of up to 15 stages hold no value at all
NON_HARD = [o for o in VALID if (o & 0xF) != HARD]
SIZES = [1, 2, 31, 32, 33, 69, 70, 71, 95, 96, 97, 250, 1000]  # 70: the frame stage at which the second group starts
CASES = [(o, t) for o in NON_HARD for t in (True, False)]


def cid(c):
    return f"{name(c[0])}-{'terminated' if c[1] else 'open'}"


def pid(p):
    return f"p{p[0]}-{p[1]:x}-{p[2]:x}"


def punctured(vd, vals, pattern):
    """the rows of vals punctured: [n, punctured_len(pattern, row length)]"""
    return np.stack([vd.puncture(v, pattern) for v in vals])


_REFS = {}


def oracle_punct_frames(vd, opt, pattern, n, S, terminated, seed, sigma=0.3):
    """the oracle's words of pad_frame(depuncture(puncture(frame))) for every frame of frames(n, S, terminated, seed,
    sigma): [n, words], computed once per (option, pattern, frame set), read-only"""
    key = (opt, pattern, n, S, terminated, seed, sigma)
    if key not in _REFS:
        vals = frames(n, S, terminated, seed, sigma)[1]
        ref = np.stack([oracle_frame(vd, opt, vd.depuncture(vd.puncture(v, pattern), pattern, 2 * S), terminated) for v in vals])
        ref.setflags(write=False)
        _REFS[key] = ref
    return _REFS[key]


def device_punct_frames(d, rx, S, pattern, terminated, scale=SCALE):
    """run_device_punct_frames of the rows of rx (n frames of S stages, packed back to back) on the current stream"""
    import torch
    n, L = rx.shape
    row = 4 * ((S + 31) // 32)
    inp = torch.from_numpy(np.ascontiguousarray(rx).reshape(-1)).cuda() if rx.size else torch.zeros(4, device="cuda")
    out = torch.zeros(n * row // 4, dtype=torch.int32, device="cuda")
    d.run_device_punct_frames(inp.data_ptr(), 4 * L, out.data_ptr(), row, S, n, pattern, terminated, scale,
                              stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return out.cpu().numpy().view(d.decPack_t).reshape(n, -1)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=cid)
def test_punctured_frames_equal_the_oracle_of_the_depunctured_padded_stream(gpu, vd, case):
    """1, 3 and 5 frames (a partial workgroup and a wave with nothing to do) of 1 .. 1000 stages at 2/3, 3/4, 7/8 and
    a period-16 pattern; 64 frames at 3/4"""
    opt, terminated = case
    with vd.ViterbiCUDA(opt) as d:
        for pattern in (P23, P34, P78, P16):
            for S in SIZES:
                many = pattern == P34 and S in (33, 250)
                nmax = 64 if many else 5
                vals = frames(nmax, S, terminated, seed=S)[1]
                ref = oracle_punct_frames(vd, opt, pattern, nmax, S, terminated, seed=S)
                rx = punctured(vd, vals, pattern)
                assert rx.shape[1] == vd.punctured_len(pattern, 2 * S)
                for n in (1, 3, 5, 64) if many else (1, 3, 5):
                    host, _ = d.run_punct_frames(rx[:n], pattern, S, terminated, SCALE)
                    assert host.dtype == ref.dtype and np.array_equal(host, ref[:n]), \
                        (pattern, S, n, np.argwhere(host != ref[:n])[:5])
                    dev = device_punct_frames(d, rx[:n], S, pattern, terminated)
                    assert np.array_equal(dev, host), (pattern, S, n)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=cid)
def test_unpunctured_pattern_equals_run_frames_of_the_same_buffer(gpu, vd, case):
    opt, terminated = case
    with vd.ViterbiCUDA(opt) as d:
        for S in (33, 250):
            vals = frames(5, S, terminated, seed=S)[1]
            want, _ = d.run_frames(vals, terminated, SCALE)
            got, _ = d.run_punct_frames(vals, (1, 1, 1), S, terminated, SCALE)
            assert np.array_equal(got, want), (S, np.argwhere(got != want)[:5])
            assert np.array_equal(device_punct_frames(d, np.array(vals), S, (1, 1, 1), terminated), want)


LENGTHS = [0, 1, 250, 300, 33, 0, 1_000_000, 97, 32, 249]
MAXBITS = 250


@pytest.mark.gpu
@pytest.mark.parametrize("pattern", [P34, P16], ids=pid)
@pytest.mark.parametrize("case", [(SOFT8 | M_B16, True), (SOFT16 | M_B32, False), (FP32 | M_FP16 | O_B16, True)], ids=cid)
def test_variable_lengths_between_nan_guards_and_sentinels(gpu, vd, case, pattern):
    """a device lengths array (in stages) with 0, 1, maxFrameBits and values above it (clamped); the base pointer 4-
    but not 8-byte aligned, the stride an odd number of floats, NaN in every float that belongs to no frame -- the
    float right after each frame's punctured_len(2 S_f) included -- and the outputs inside sentinel bytes: each frame
    equals the oracle on its own words, every other byte (the words of empty frames too) keeps the sentinel"""
    import torch
    opt, terminated = case
    n = len(LENGTHS)
    fstride = vd.punctured_len(pattern, 2 * MAXBITS) + 1
    fstride += 1 - fstride % 2  # odd
    ostride = 4 * 8 + 8
    host_in = np.full(1 + n * fstride + 8, np.nan, dtype=np.float32)
    want = []
    for f, L in enumerate(LENGTHS):
        S = min(L, MAXBITS)
        if S:  # frame f: a frame of its own S stages (terminated: with its own tail zeros), the phase at 0
            rx = vd.puncture(frames(n, S, terminated, seed=300 + S)[1][f], pattern)
            assert rx.size == vd.punctured_len(pattern, 2 * S) < fstride
            host_in[1 + f * fstride: 1 + f * fstride + rx.size] = rx
            want.append(oracle_frame(vd, opt, vd.depuncture(rx, pattern, 2 * S), terminated))
        else:
            want.append(None)
    inp = torch.from_numpy(host_in).cuda()
    assert inp.data_ptr() % 8 == 0
    lens = torch.from_numpy(np.array(LENGTHS, dtype=np.uint32).view(np.int32)).cuda()
    out = torch.full((n * ostride + 16,), 0xA5, dtype=torch.uint8, device="cuda")
    with vd.ViterbiCUDA(opt) as d:
        d.run_device_punct_frames(inp.data_ptr() + 4, 4 * fstride, out.data_ptr() + 8, ostride, MAXBITS, n, pattern, terminated,
                                  SCALE, frame_bits_ptr=lens.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
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
@pytest.mark.parametrize("case", [(SOFT8 | M_B16, True), (SOFT8 | M_B16, False), (SOFT16 | M_B32, False), (FP32 | M_B32 | O_B16, True)],
                         ids=cid)
def test_frames_without_a_kept_value(gpu, vd, case):
    """(16, 0x8000, 0) keeps the first output of every 16th stage only: frames of 1, 15, 16, 17 and 40 stages hold 0,
    0, 1, 1 and 2 values.  Everything else in the buffer is NaN; the frames decode as erasures between the pads"""
    opt, terminated = case
    with vd.ViterbiCUDA(opt) as d:
        for S, kept in ((1, 0), (15, 0), (16, 1), (17, 1), (40, 2)):
            n = 5
            vals = frames(n, S, terminated, seed=400 + S)[1]
            rx = punctured(vd, vals, PNONE)
            assert rx.shape == (n, kept) and vd.punctured_len(PNONE, 2 * S) == kept
            ref = np.stack([oracle_frame(vd, opt, vd.depuncture(r, PNONE, 2 * S), terminated) for r in rx])
            buf = np.full((n, 3), np.nan, dtype=np.float32)
            buf[:, :kept] = rx
            host, _ = d.run_punct_frames(buf, PNONE, S, terminated, SCALE)
            assert np.array_equal(host, ref), (S, host, ref)
            assert np.array_equal(device_punct_frames(d, buf, S, PNONE, terminated), ref), S
            if kept == 0:  # rows of no float at all
                host, _ = d.run_punct_frames(rx, PNONE, S, terminated, SCALE)
                assert np.array_equal(host, ref), S


@pytest.mark.gpu
@pytest.mark.parametrize("opt", [SOFT8 | M_B16, SOFT8 | M_B32, FP32 | M_FP16], ids=name)
@pytest.mark.parametrize("kind", tie_patterns.LLR_PATTERNS)
def test_tie_dense_open_frames(gpu, vd, opt, kind):
    """all-zero floats and the tie-dense patterns as open frames at 3/4: most add-compare-selects are ties, so the
    words are the tie rule's; compared with the oracle word for word"""
    with vd.ViterbiCUDA(opt) as d:
        for S, n in ((97, 6), (250, 5)):
            vals = tie_patterns.llr_pattern(opt, kind, 2 * S * n).reshape(n, 2 * S)
            rx = punctured(vd, vals, P34)
            ref = np.stack([oracle_frame(vd, opt, vd.depuncture(r, P34, 2 * S), False, scale=tie_patterns.LLR_SCALE) for r in rx])
            host, _ = d.run_punct_frames(rx, P34, S, False, tie_patterns.LLR_SCALE)
            assert np.array_equal(host, ref), (S, np.argwhere(host != ref)[:5])


@pytest.mark.gpu
@pytest.mark.parametrize("opt", [SOFT8 | M_B32, SOFT8 | M_B16, FP32 | M_FP16, SOFT16 | M_B32], ids=name)
def test_lds_guard_words_stay_intact(gpu, vd, opt):
    vals = frames(5, 1000, True, seed=1000)[1]
    with vd.ViterbiCUDA(opt) as d:
        d.set_guard_check(True)
        for pattern in (P34, P16):
            out, _ = d.run_punct_frames(punctured(vd, vals, pattern), pattern, 1000, True, SCALE)
            assert np.array_equal(out, oracle_punct_frames(vd, opt, pattern, 5, 1000, True, seed=1000))
        assert d.guard_violations() == 0


@pytest.mark.gpu
def test_graph_capture_on_a_side_stream(gpu, vd):
    """one captured launch, replayed twice over changed input"""
    import torch
    opt, S, n = SOFT8 | M_B16, 250, 5
    rxs = [punctured(vd, frames(n, S, True, seed=sd)[1], P34) for sd in (S, S + 1)]
    refs = [oracle_punct_frames(vd, opt, P34, n, S, True, seed=sd) for sd in (S, S + 1)]
    assert not np.array_equal(refs[0], refs[1])
    L = rxs[0].shape[1]
    with vd.ViterbiCUDA(opt) as d:
        s = torch.cuda.Stream()
        inp = torch.zeros(n * L, dtype=torch.float32, device="cuda")
        out = torch.zeros(n * 8, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            d.run_device_punct_frames(inp.data_ptr(), 4 * L, out.data_ptr(), 32, S, n, P34, True, SCALE,
                                      stream=torch.cuda.current_stream().cuda_stream)
        for rx, ref in zip(rxs, refs):
            inp.copy_(torch.from_numpy(rx.reshape(-1)))
            out.zero_()
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            assert np.array_equal(out.cpu().numpy().view(np.uint32).reshape(n, -1), ref)
        del g


@pytest.mark.gpu
def test_errors(gpu, vd):
    rx = np.zeros((4, 334), dtype=np.float32)  # 3/4 of 250 stages: 334 floats
    assert vd.punctured_len(P34, 500) == 334
    with vd.ViterbiCUDA(HARD | M_B32) as d:
        for terminated in (True, False):
            with pytest.raises(vd.VitdecError, match="VD_ERR_OPTIONS.*HARD"):
                d.run_punct_frames(rx, P34, 250, terminated)
            with pytest.raises(vd.VitdecError, match="VD_ERR_OPTIONS.*HARD"):
                d.run_device_punct_frames(16, 1336, 16, 32, 250, 4, P34, terminated)  # (checked before any pointer is used)
    with vd.ViterbiCUDA(SOFT8 | M_B16) as d:
        bad = [dict(pattern=(0, 1, 1)), dict(pattern=(17, 1, 1)), dict(pattern=(3, 0b1000, 0b011)), dict(pattern=(3, 0b101, 0b1011)),
               dict(pattern=(3, 0, 0)), dict(rx_ptr=18), dict(rx_stride=1338), dict(rx_stride=1332), dict(output_stride=30),
               dict(output_stride=28), dict(maxFrameBits=0), dict(maxFrameBits=(1 << 20) + 1, rx_stride=8 << 21, output_stride=1 << 18),
               dict(nframes=0), dict(nframes=-1), dict(scale=0.0), dict(scale=float("inf")), dict(scale=float("nan"))]
        for kw in bad:
            a = dict(rx_ptr=16, rx_stride=1336, output_ptr=16, output_stride=32, maxFrameBits=250, nframes=4, pattern=P34,
                     terminated=True, scale=SCALE)
            a.update(kw)
            with pytest.raises(vd.VitdecError, match="VD_ERR_ARG"):
                d.run_device_punct_frames(**a)
        for scale in (0.0, float("inf"), float("nan")):
            with pytest.raises(vd.VitdecError, match="VD_ERR_ARG"):
                d.run_punct_frames(rx, P34, 250, True, scale)
        with pytest.raises(vd.VitdecError, match="VD_ERR_ARG"):
            d.run_punct_frames(rx, (17, 1, 1), 250)
        with pytest.raises(vd.VitdecError, match="received values"):
            d.run_punct_frames(rx[:, :333], P34, 250)


@pytest.mark.gpu
@pytest.mark.parametrize("opt", [SOFT8 | M_B16, FP32 | M_FP16 | O_B16, SOFT16 | M_B32], ids=name)
def test_kernel_name(gpu, vd, opt):
    with vd.ViterbiCUDA(opt) as d:
        for n in (1, 5, 10_000):
            nm = d.kernel_for(1000, n, 4)
            assert nm.startswith("vd_decode_tg<FRM+PUN+") and "one frame per wave" in nm, nm
        assert d.kernel_for(0, 4, 4) == "-" and d.kernel_for((1 << 20) + 1, 4, 4) == "-"
    with vd.ViterbiCUDA(SOFT8 | M_B16) as d:
        assert d.kernel_for(1000, 4, 4).startswith("vd_decode_tg<FRM+PUN+SOFT8,B16,O32> one frame per wave, ")
    with vd.ViterbiCUDA(HARD | M_B32) as d:
        assert d.kernel_for(1000, 4, 4) == "-"


@pytest.mark.gpu
@pytest.mark.parametrize("opt", [SOFT8 | M_B16, SOFT16 | M_B32], ids=name)
@pytest.mark.parametrize("pattern", [P34, P23], ids=pid)
def test_every_bit_of_256_terminated_and_256_open_frames(gpu, vd, opt, pattern):
    """256 frames of 1000 stages at sigma 0.2: 0 errors over all 256,000 bits, terminated and open"""
    n, S = 256, 1000
    with vd.ViterbiCUDA(opt) as d:
        for terminated in (True, False):
            bits, vals = frames(n, S, terminated, seed=7, sigma=0.2)
            out, _ = d.run_punct_frames(punctured(vd, vals, pattern), pattern, S, terminated, SCALE)
            got = np.stack([decoded_bits(opt, w, S) for w in out])
            assert int((got != bits).sum()) == 0
