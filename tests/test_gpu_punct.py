"""GPU parity of punctured decodes (vd_run_punct / vd_run_device_punct / vd_run_device_punct_batch; kernels
vd_decode_tg<PUN+...>): a punctured decode equals, word for word, the rate-1/2 decode of the depunctured
stream -- the received value at the kept positions, +0.0f at the punctured ones -- both by the oracle
(pack + decode) and by vd_run_llr on the same decoder.  Inputs at snr 1.2, so that ties and wrong paths occur.
The index arithmetic alone: tests/test_punct.py."""
import functools

import numpy as np
import pytest

from vitdec import FP32, HARD, M_B16, M_B32, M_FP16, O_B16, SOFT4, SOFT8, SOFT16
from test_gpu_llr import channel_values, channel_values_fast
from test_gpu_parity import VALID, name

P23, P34 = (2, 0b01, 0b11), (3, 0b101, 0b011)
P56, P78 = (5, 0b10101, 0b01011), (7, 0b1010001, 0b0101111)  # the DVB-S masks
P16 = (16, 0x8001, 0x7FFE)
NON_HARD = [o for o in VALID if (o & 0xF) != HARD]
SCALE = 40000.0


def pid(p):
    return f"p{p[0]}-{p[1]:x}-{p[2]:x}"


@functools.lru_cache(maxsize=None)
def values_400k():
    v = channel_values(2 * 200_000, 1.2, 31)
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def depunctured_400k(pattern):
    """(received values, depunctured stream) of values_400k under pattern"""
    import vitdec
    rx = vitdec.puncture(values_400k(), pattern)
    dep = vitdec.depuncture(rx, pattern, values_400k().size)
    rx.setflags(write=False)
    dep.setflags(write=False)
    return rx, dep


def oracle_words(vo, opt, dep, **kw):
    ref, ok = vo.decode(opt, vo.pack(opt, dep, SCALE), input_num=dep.size, **kw)
    assert ok
    return ref


def differing(out, ref):
    bad = np.flatnonzero(out != ref)
    return f"{bad.size} words differ, first at {bad[:5]}" if bad.size else ""


@pytest.mark.gpu
@pytest.mark.parametrize("opt", NON_HARD, ids=name)
@pytest.mark.parametrize("pattern", [P23, P34, P56, P78, P16], ids=pid)
def test_punctured_decode_equals_oracle_and_llr(gpu, vd, vo, opt, pattern):
    """2 * 200,000 values: 6,248 words over 6,400 chunks (ragged and empty chunks, chunk starts at every residue
    of each period)"""
    rx, dep = depunctured_400k(pattern)
    assert rx.size == vd.punctured_len(pattern, dep.size)
    ref = oracle_words(vo, opt, dep)
    with vd.ViterbiCUDA(opt) as d:
        assert "vd_decode_tg<PUN+" in d.kernel_for(dep.size, 1, 2)
        out, _ = d.run_punct(rx, pattern, dep.size, scale=SCALE)
        llr, _ = d.run_llr(dep, scale=SCALE)
    assert not differing(out, ref)
    assert not differing(llr, ref)


@pytest.mark.gpu
@pytest.mark.parametrize("opt", [SOFT4 | M_B16, SOFT8 | M_B16, SOFT16 | M_B32, FP32 | M_FP16], ids=name)
def test_unpunctured_pattern_equals_llr_on_the_same_buffer(gpu, vd, opt):
    vals = values_400k()
    with vd.ViterbiCUDA(opt) as d:
        assert vd.punctured_len((1, 1, 1), vals.size) == vals.size
        out, _ = d.run_punct(vals, (1, 1, 1), vals.size, scale=SCALE)
        llr, _ = d.run_llr(vals, scale=SCALE)
    assert not differing(out, llr)


@pytest.mark.gpu
@pytest.mark.parametrize("opt", [SOFT8 | M_B16, FP32 | M_FP16], ids=name)
@pytest.mark.parametrize("pattern", [(3, 0b000, 0b010), (2, 0b11, 0b00)], ids=pid)
def test_sparse_patterns(gpu, vd, vo, opt, pattern):
    """whole stages erased and one value per period; the second output erased throughout"""
    rx, dep = depunctured_400k(pattern)
    ref = oracle_words(vo, opt, dep)
    with vd.ViterbiCUDA(opt) as d:
        out, _ = d.run_punct(rx, pattern, dep.size, scale=SCALE)
    assert not differing(out, ref)


def device_punct(vd, d, rx, n, pattern, tail=64, lead=1):
    """run_device_punct on a buffer of exactly rx.size floats placed `lead` floats into an allocation (4-byte
    alignment only) and followed by `tail` NaN floats"""
    import torch
    buf = torch.full((lead + rx.size + tail,), float("nan"), dtype=torch.float32, device="cuda")
    buf[lead:lead + rx.size] = torch.from_numpy(np.array(rx)).cuda()
    out = torch.zeros(d.getOutputSize(n) // 4 + 1, dtype=torch.int32, device="cuda")
    d.run_device_punct(buf.data_ptr() + 4 * lead, out.data_ptr(), n, pattern, scale=SCALE,
                       stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return out.cpu().numpy()[:d.getOutputSize(n) // 4].view(d.decPack_t)


@pytest.mark.gpu
@pytest.mark.parametrize("opt", [SOFT8 | M_B16, SOFT16 | M_B32, FP32 | M_B32 | O_B16], ids=name)
@pytest.mark.parametrize("n", [128, 130, 192, 198, 2 * 4096 + 6])
def test_short_and_odd_sizes_with_a_nan_guard(gpu, vd, vo, opt, n):
    """the last period cut mid-way; the buffer holds exactly punctured_len floats and NaNs follow it: a read past
    the received data would reach the metrics.  128 and 130 values decode to no output word (vd_message_len is
    0): the punctured entry points reject them as vd_run_llr does"""
    vals = values_400k()[:n]
    rx = vd.puncture(vals, P34)
    assert rx.size == vd.punctured_len(P34, n)
    dep = vd.depuncture(rx, P34, n)
    if vd.lib().vd_message_len(opt, n) == 0:
        assert n < 192
        with vd.ViterbiCUDA(opt) as d:
            for call in (lambda: d.run_llr(dep, scale=SCALE), lambda: d.run_punct(rx, P34, n, scale=SCALE),
                         lambda: d.run_device_punct(16, 16, n, P34)):
                with pytest.raises(vd.VitdecError, match="VD_ERR_ARG.*inputNum too small"):
                    call()
        return
    ref = oracle_words(vo, opt, dep)
    with vd.ViterbiCUDA(opt) as d:
        got = device_punct(vd, d, rx, n, P34)
        host, _ = d.run_punct(rx, P34, n, scale=SCALE)
    assert np.array_equal(got, ref) and np.array_equal(host, ref)


@pytest.mark.gpu
@pytest.mark.parametrize("opt", [SOFT8 | M_B16, SOFT16 | M_B32, FP32 | M_FP16, SOFT4 | M_B16 | O_B16], ids=name)
def test_punctured_batch(gpu, vd, vo, opt):
    """3 punctured batches in one launch at an rx_stride that is no multiple of 16: each equals the oracle of its
    own depunctured stream; the bytes between the outputs stay untouched"""
    import torch
    n, nb = 2 * 150_000, 3
    vals = [channel_values_fast(n, 1.2, 41 + b) for b in range(nb)]
    rxs = [vd.puncture(v, P34) for v in vals]
    refs = [oracle_words(vo, opt, vd.depuncture(rx, P34, n)) for rx in rxs]
    plen = vd.punctured_len(P34, n)
    istride = 4 * (plen + 3)
    assert istride % 16 != 0 and istride % 4 == 0
    nout = vd.lib().vd_output_size(opt, n)
    ostride = (nout + 255) // 256 * 256 + 256
    inp = torch.full((nb * istride // 4,), float("nan"), dtype=torch.float32, device="cuda")
    for b in range(nb):
        inp[b * istride // 4: b * istride // 4 + plen] = torch.from_numpy(rxs[b]).cuda()
    out = torch.full((nb * ostride,), 0xA5, dtype=torch.uint8, device="cuda")
    with vd.ViterbiCUDA(opt) as d:
        assert "vd_decode_tg<PUN+" in d.kernel_for(n, nb, 2) and "one chunk per wave" in d.kernel_for(n, nb, 2)
        d.run_device_punct_batch(inp.data_ptr(), istride, out.data_ptr(), ostride, n, nb, P34, SCALE,
                                 torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
    for b in range(nb):
        got = out[b * ostride: b * ostride + nout].cpu().numpy().view(refs[b].dtype)
        np.testing.assert_array_equal(got, refs[b])
        assert bool((out[b * ostride + nout: (b + 1) * ostride] == 0xA5).all())


@pytest.mark.gpu
@pytest.mark.parametrize("opt,pattern", [(SOFT8 | M_B16, P34), (SOFT16 | M_B32, P23)], ids=["s8-b16-3/4", "s16-b32-2/3"])
def test_punctured_segment_launch(gpu, vd, vo, opt, pattern):
    """16M bits in one launch: 78 words per chunk, so the punctured decode takes vd_decode_tg's segment launch
    (speculative segment starts inside chunks, re-decodes from boundary blocks at every residue of the period)"""
    n = 2 * 16_000_000
    rx = vd.puncture(channel_values_fast(n, 1.2, 13), pattern)
    dep = vd.depuncture(rx, pattern, n)
    ref = oracle_words(vo, opt, dep, nthreads=16)
    caps, before = vd.split_cap_exits(), vd.split_redecodes()
    with vd.ViterbiCUDA(opt) as d:
        kn = d.kernel_for(n, 1, 2)
        assert "vd_decode_tg<PUN+" in kn and "segment launch" in kn, kn
        out, _ = d.run_punct(rx, pattern, n, scale=SCALE)
    # (codewords at snr 1.2: few re-decodes or none; tests/test_gpu_seg_count.py pins the count on noise)
    print(f"{kn}: {vd.split_redecodes() - before} segments re-decoded")
    assert not differing(out, ref)
    assert vd.split_cap_exits() == caps == 0


@pytest.mark.gpu
def test_device_path_and_graph_capture(gpu, vd):
    import torch
    opt, n = SOFT8 | M_B16, 2 * 200_000
    rx, dep = depunctured_400k(P34)
    with vd.ViterbiCUDA(opt) as d:
        host, _ = d.run_punct(rx, P34, n, scale=SCALE)
        s = torch.cuda.Stream()
        buf = torch.from_numpy(np.array(rx)).cuda()
        out = torch.zeros(d.getOutputSize(n) // 4, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            d.run_device_punct(buf.data_ptr(), out.data_ptr(), n, P34, scale=SCALE, stream=s.cuda_stream)
        s.synchronize()
        assert np.array_equal(out.cpu().numpy().view(np.uint32), host)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            d.run_device_punct(buf.data_ptr(), out.data_ptr(), n, P34, scale=SCALE,
                               stream=torch.cuda.current_stream().cuda_stream)
        for _ in range(2):
            out.zero_()
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            assert np.array_equal(out.cpu().numpy().view(np.uint32), host)
        del g


@pytest.mark.gpu
def test_errors(gpu, vd):
    rx = np.zeros(2 * 200_000, dtype=np.float32)
    with vd.ViterbiCUDA(HARD | M_B32) as d:
        with pytest.raises(vd.VitdecError, match="VD_ERR_OPTIONS.*HARD"):
            d.run_punct(rx, P34, rx.size)
        assert d.kernel_for(rx.size, 1, 2) == "-"
    with vd.ViterbiCUDA(SOFT8 | M_B16) as d:
        for bad in [(0, 1, 1), (17, 1, 1), (3, 0b1000, 0b001), (3, 0b001, 0b1000), (3, 0, 0)]:
            assert vd.punctured_len(bad, rx.size) == 0
            with pytest.raises(vd.VitdecError, match="VD_ERR_ARG"):
                d.run_punct(rx, bad, rx.size)
            with pytest.raises(vd.VitdecError, match="VD_ERR_ARG"):
                d.run_device_punct(16, 16, rx.size, bad)  # (the pattern is checked before any pointer is used)
        with pytest.raises(vd.VitdecError, match="VD_ERR_ARG"):
            d.run_device_punct(18, 16, rx.size, P34)  # rx_d not 4-byte aligned
        with pytest.raises(vd.VitdecError, match="VD_ERR_ARG"):
            d.run_device_punct_batch(16, 6, 16, 1 << 20, rx.size, 2, P34)  # rx_stride not a multiple of 4
        with pytest.raises(vd.VitdecError, match="VD_ERR_ARG"):
            d.run_punct(rx, P34, 126)  # inputNum too small


@pytest.mark.gpu
@pytest.mark.parametrize("opt", [SOFT8 | M_B16, SOFT16 | M_B32, FP32 | M_B32], ids=name)
@pytest.mark.parametrize("rate", ["2/3", "3/4"])
def test_named_rates_decode_without_errors(gpu, vd, vo, opt, rate):
    """snr 5 (sigma 0.1), the input the named patterns were chosen on: no bit errors at rates 2/3 and 3/4"""
    bits, vals = vo.channel(200_000, 5.0, 1, 2)
    pattern = vd.PUNCTURE[rate]
    with vd.ViterbiCUDA(opt) as d:
        out, _ = d.run_punct(vd.puncture(vals, pattern), pattern, vals.size, scale=SCALE)
    assert vd.count_errors(opt, bits, out) == 0
