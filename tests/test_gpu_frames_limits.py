"""Frame launches (vd_decode_tg<FRM+...>, <FRM+PUN+...>, <FRM+TB+...>) at the lengths, counts and strides
include/vd_capi.h allows, word for word against the oracle through the existing definitions (vitdec.pad_frame,
depuncture, wrap_frame; tests/limits_common.py describes a launch once for the three families):
  1. frames of up to 2^20 stages: the load offsets' reduced-width arithmetic (24-bit products, the 32-bit and 16-bit
     reciprocals of the wrap, the clamp of frame_offset, pfrm_base up to 2^23) and the O_B16 stores past word 31;
  3. 20,003 frames in a launch: the waves that run with the fairness controller off, workgroups that follow a
     retired one on the same CU, a frame index past 2^13; 6400, 6401 and 6404 frames, where the controller switches;
  4. strides past 2^32: batch * inStride and batch * outStride beyond 32 bits;
  5. the three families at once on three streams of one decoder;
  6. NaN, infinities, -0.0, round-to-even halves and denormals through the pad select and the wrapped loads.
(2. is the CPU part, tests/test_frames_limits.py.)  Inputs: the noisy BPSK frames of frames_common.py / tb_common.py,
sigma 0.3, scale 40000 unless a test says otherwise.  No tolerance anywhere: the contract is bit-exact."""
import functools

import numpy as np
import pytest

import limits_common as lc
from frames_common import SCALE, decoded_bits
from tb_common import wrapped_bits
from test_gpu_llr import specials
from vitdec import FP32, HARD, M_B16, M_B32, M_FP16, SOFT4, SOFT8, SOFT16

SENTINEL = 0xA5


def cur_stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


# ---------------------------------------------------------------- 1. long frames, up to the limit
def check_long_words(vd, c, got, refs):
    """got: the output buffer as bytes.  Every frame equals the oracle on its own words, every other byte (the words
    of the empty frame too) keeps the sentinel; the terminated and the tail-biting frames of 4096 stages and more
    decode every bit (the oracle's own words do: tests/test_frames_limits.py)"""
    n, off, ostride = len(lc.LONG_LENGTHS), lc.LONG_OUT_OFFSET, lc.LONG_OUT_STRIDE
    want = lc.expected_bytes(got.size, off, ostride, refs, SENTINEL)
    assert np.array_equal(got, want), lc.first_difference(got, want, off, ostride, n)
    if c.fam == "pun" or c.term is False:
        return
    for f, (S, fr) in enumerate(zip(lc.LONG_LENGTHS, lc.long_frames(lc.long_kind(c)))):
        if S < lc.LONG_CHECKED:
            continue
        w = got[off + f * ostride: off + f * ostride + lc.frame_nbytes(S)].view(refs[f].dtype)
        if c.fam == "tb":
            nb = 32 * ((S + 31) // 32)
            bits, src = decoded_bits(c.opt, w, nb), wrapped_bits(fr[0], nb)
        else:
            bits, src = decoded_bits(c.opt, w, S), fr[0]
        assert np.array_equal(bits, src), (f, S, int((bits != src).sum()))


@pytest.mark.gpu
@pytest.mark.parametrize("case", lc.CASES, ids=lc.cid)
def test_long_frames_device(gpu, vd, case):
    """one launch of the eight frames of LONG_LENGTHS, maxFrameBits 2^20, a device lengths array, the input rows 8 << 20
    bytes apart (punctured: the bytes of 2^20 stages) with NaN in every float that belongs to no frame, the outputs
    inside sentinel bytes"""
    import torch
    n = len(lc.LONG_LENGTHS)
    istride, ostride = lc.long_in_stride(vd, case), lc.LONG_OUT_STRIDE
    rows, refs = lc.long_rows(vd, case), lc.long_refs(vd, case)
    inp = torch.full((n * istride // 4,), float("nan"), dtype=torch.float32, device="cuda")
    for f, r in enumerate(rows):
        if r is not None:
            assert 4 * r.size == lc.row_bytes(vd, case, lc.LONG_LENGTHS[f]) <= istride
            inp[f * istride // 4: f * istride // 4 + r.size] = torch.from_numpy(np.array(r))
    lens = torch.from_numpy(np.array(lc.LONG_LENGTHS, dtype=np.int32)).cuda()
    out = torch.full((n * ostride + 16,), SENTINEL, dtype=torch.uint8, device="cuda")
    with vd.ViterbiCUDA(case.opt) as d:
        lc.launch_device(d, case, inp.data_ptr(), istride, out.data_ptr() + lc.LONG_OUT_OFFSET, ostride, lc.LONG_MAX, n,
                         lens_ptr=lens.data_ptr(), stream=cur_stream())
        torch.cuda.synchronize()
    check_long_words(vd, case, out.cpu().numpy(), refs)


@pytest.mark.gpu
@pytest.mark.parametrize("case", lc.S8_CASES, ids=lc.cid)
def test_long_frames_blocking(gpu, vd, case):
    """the same launch through the blocking host entry point, over host buffers of the same layout; prints kernel_ms"""
    n = len(lc.LONG_LENGTHS)
    istride, ostride = lc.long_in_stride(vd, case), lc.LONG_OUT_STRIDE
    rows, refs = lc.long_rows(vd, case), lc.long_refs(vd, case)
    host_in = np.full(n * istride // 4, np.nan, dtype=np.float32)
    for f, r in enumerate(rows):
        if r is not None:
            host_in[f * istride // 4: f * istride // 4 + r.size] = r
    lens = np.array(lc.LONG_LENGTHS, dtype=np.uint32)
    out = np.full(n * ostride + 16, SENTINEL, dtype=np.uint8)
    with vd.ViterbiCUDA(case.opt) as d:
        ms = lc.launch_host(vd, d, case, host_in, istride, out, lc.LONG_OUT_OFFSET, ostride, lens, lc.LONG_MAX, n)
    print(f"kernel_ms {lc.cid(case)} long frames: {ms:.3f}")
    check_long_words(vd, case, out, refs)


# ---------------------------------------------------------------- 3. many frames
MANY = 20_003  # odd: a partial last workgroup; 13,603 frames with the controller off; more than twice the 8192 resident waves
TILE = 61      # prime: a frame index mangled by any power of two decodes another frame's values
MANY_BITS = 97
# the lengths of the 61 tiled frames of the variable-length launch: the word and group edges, values above
# maxFrameBits (clamped), the rest drawn once
LEN61 = np.concatenate([np.array([0, 1, 32, 33, 96, 97, 98, 130, 1_000_000, 0xFFFFFFFF], dtype=np.uint32),
                        np.random.default_rng(TILE).integers(0, 130, TILE - 10).astype(np.uint32)])
assert LEN61.size == TILE


@functools.lru_cache(maxsize=None)
def tiled(vd, c, S, seed):
    """(rows [61, floats], oracle words [61, words]) of 61 distinct frames of S stages of the case's kind"""
    vals = lc.small_frames(c, TILE, S, seed)[1]
    rows = np.stack([lc.row_of(vd, c, v) for v in vals])
    ref = np.stack([lc.oracle_row(vd, c, r, S) for r in rows])
    rows.setflags(write=False)
    ref.setflags(write=False)
    return rows, ref


def assert_tiled(got, ref, n):
    """row f of got equals row f % 61 of ref"""
    want = ref[np.arange(n) % TILE]
    assert got.shape == want.shape and got.dtype == want.dtype
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError(f"{np.unique(bad[:, 0]).size} of {n} frames differ, first (frame, word): {bad[:6].tolist()}")


def run_tiled_device(vd, d, c, S, n, seed):
    import torch
    rows, ref = tiled(vd, c, S, seed)
    assert rows.shape[1] * 4 == lc.row_bytes(vd, c, S)
    inp = torch.from_numpy(rows[np.arange(n) % TILE].reshape(-1)).cuda()
    nb = lc.frame_nbytes(S)
    out = torch.zeros(n * nb, dtype=torch.uint8, device="cuda")
    lc.launch_device(d, c, inp.data_ptr(), 4 * rows.shape[1], out.data_ptr(), nb, S, n, stream=cur_stream())
    torch.cuda.synchronize()
    assert_tiled(out.cpu().numpy().view(ref.dtype).reshape(n, -1), ref, n)


@pytest.mark.gpu
@pytest.mark.parametrize("case", lc.CASES, ids=lc.cid)
def test_many_frames_fixed_length(gpu, vd, case):
    """20,003 contiguous frames of 97 stages, tiled from 61: all rows against the oracle of the 61"""
    with vd.ViterbiCUDA(case.opt) as d:
        run_tiled_device(vd, d, case, MANY_BITS, MANY, seed=MANY_BITS)


@pytest.mark.gpu
@pytest.mark.parametrize("case", lc.CASES, ids=lc.cid)
def test_many_frames_variable_lengths(gpu, vd, case):
    """20,003 frames with a device lengths array tiled from LEN61, maxFrameBits 97: frame f is a frame of its own
    min(LEN61[f % 61], 97) stages with NaN in the rest of its row, the outputs inside sentinel bytes: each frame
    equals the oracle on its own words, every other byte (the words of empty frames too) keeps the sentinel"""
    import torch
    n, rowf = MANY, lc.row_bytes(vd, case, MANY_BITS) // 4
    ostride = lc.frame_nbytes(MANY_BITS) + 8
    rows = np.full((TILE, rowf), np.nan, dtype=np.float32)
    refs = []
    for i, L in enumerate(LEN61):
        S = min(int(L), MANY_BITS)
        if S == 0:
            refs.append(None)
            continue
        r = lc.row_of(vd, case, lc.small_frames(case, TILE, S, 300 + S)[1][i])
        rows[i, :r.size] = r
        refs.append(lc.oracle_row(vd, case, r, S))
    idx = np.arange(n) % TILE
    inp = torch.from_numpy(rows[idx].reshape(-1)).cuda()
    lens = torch.from_numpy(LEN61[idx].view(np.int32)).cuda()
    out = torch.full((n * ostride + 16,), SENTINEL, dtype=torch.uint8, device="cuda")
    with vd.ViterbiCUDA(case.opt) as d:
        lc.launch_device(d, case, inp.data_ptr(), 4 * rowf, out.data_ptr() + 8, ostride, MANY_BITS, n, lens_ptr=lens.data_ptr(),
                         stream=cur_stream())
        torch.cuda.synchronize()
    got = out.cpu().numpy()
    want61 = lc.expected_bytes(TILE * ostride, 0, ostride, refs, SENTINEL).reshape(TILE, ostride)
    assert (got[:8] == SENTINEL).all() and (got[8 + n * ostride:] == SENTINEL).all()
    assert_tiled(got[8:8 + n * ostride].reshape(n, ostride), want61, n)


@pytest.mark.gpu
@pytest.mark.parametrize("case", lc.S8_CASES, ids=lc.cid)
def test_many_frames_blocking(gpu, vd, case):
    """the 20,003 frames through the blocking host entry point"""
    rows, ref = tiled(vd, case, MANY_BITS, MANY_BITS)
    feed = rows[np.arange(MANY) % TILE]
    with vd.ViterbiCUDA(case.opt) as d:
        if case.fam == "tb":
            out, ms = d.run_tb_frames(feed, SCALE)
        elif case.fam == "pun":
            out, ms = d.run_punct_frames(feed, case.pat, MANY_BITS, case.term, SCALE)
        else:
            out, ms = d.run_frames(feed, case.term, SCALE)
    print(f"kernel_ms {lc.cid(case)} {MANY} frames of {MANY_BITS}: {ms:.3f}")
    assert_tiled(out, ref, MANY)


@pytest.mark.gpu
@pytest.mark.parametrize("case", [lc.Case("frm", SOFT8 | M_B16, True, None), lc.Case("pun", SOFT16 | M_B32, False, lc.P34),
                                  lc.Case("tb", HARD | M_B32, None, None)], ids=lc.cid)
@pytest.mark.parametrize("n", [6400, 6401, 6404])
def test_frame_counts_where_the_controller_switches(gpu, vd, case, n):
    """6400 frames: the controller runs in every wave; 6401: off for frame 0 only; 6404: off for the first workgroup"""
    with vd.ViterbiCUDA(case.opt) as d:
        run_tiled_device(vd, d, case, 33, n, seed=33)


# ---------------------------------------------------------------- 4. offsets past 4 GiB
@pytest.mark.gpu
@pytest.mark.parametrize("case", lc.S8_CASES, ids=lc.cid)
def test_strides_past_4_gib(gpu, vd, case):
    """2 frames of 250 stages 2^32 + 8 * 251 bytes apart, their outputs 2^32 + 40 bytes apart, in uninitialised
    buffers; at the 32-bit alias of frame 1's input offset (8 * 251 bytes in) lies a third valid frame, at the alias of
    its output offset sentinel bytes.  Frame 1 equals the oracle of its own values and the alias keeps the sentinel:
    an offset truncated to 32 bits reads and writes inside the same allocations and shows as wrong words"""
    import torch
    S, nb = 250, lc.frame_nbytes(250)
    istride, ostride = (1 << 32) + 8 * 251, (1 << 32) + 40
    assert istride % 8 == 0 and ostride % 4 == 0 and lc.row_bytes(vd, case, S) <= 8 * 251
    vals = lc.small_frames(case, 3, S, 4000 + S)[1]
    rows = [lc.row_of(vd, case, v) for v in vals]
    refs = [lc.oracle_row(vd, case, r, S) for r in rows]
    assert not np.array_equal(refs[1], refs[2]) and not np.array_equal(refs[1], refs[0])
    inp = torch.empty(istride + 8 * 251, dtype=torch.uint8, device="cuda")
    out = torch.empty(ostride + 64, dtype=torch.uint8, device="cuda")
    assert inp.data_ptr() % 8 == 0 and out.data_ptr() % 4 == 0
    for at, r in ((0, rows[0]), (istride, rows[1]), (istride - (1 << 32), rows[2])):
        inp[at: at + 4 * r.size] = torch.from_numpy(np.array(r).view(np.uint8))
    out[:128] = SENTINEL
    out[ostride - 64:] = SENTINEL
    with vd.ViterbiCUDA(case.opt) as d:
        lc.launch_device(d, case, inp.data_ptr(), istride, out.data_ptr(), ostride, S, 2, stream=cur_stream())
        torch.cuda.synchronize()
    low, high = out[:128].cpu().numpy(), out[ostride - 64:].cpu().numpy()
    del inp, out
    torch.cuda.empty_cache()  # (8.6 GiB back to the device, not kept in the allocator's pool for the rest of the session)
    assert np.array_equal(high[64:64 + nb].view(refs[1].dtype), refs[1]), "frame 1"
    assert np.array_equal(low[:nb].view(refs[0].dtype), refs[0]), "frame 0"
    assert (low[nb:] == SENTINEL).all(), "the 32-bit alias of frame 1's output offset (bytes 40 .. 72) was written"
    assert (high[:64] == SENTINEL).all() and (high[64 + nb:] == SENTINEL).all()


# ---------------------------------------------------------------- 5. three families at once on one decoder
@pytest.mark.gpu
@pytest.mark.parametrize("guard", [False, True], ids=["plain", "guard-check"])
def test_three_families_on_three_streams_of_one_decoder(gpu, vd, guard):
    """one SOFT8 | M_B16 decoder, three non-blocking streams, one family each: eight launches of 2000 frames of 1000
    stages (tiled from 61) per stream into separate outputs, issued interleaved, one synchronise at the end.  Every
    output equals the family's single launch, which equals the oracle of the 61 frames"""
    import torch
    S, n, reps = 1000, 2000, 8
    nb = lc.frame_nbytes(S)
    inputs, singles = [], []
    with vd.ViterbiCUDA(lc.S8) as d:
        if guard:
            d.set_guard_check(True)
        for c in lc.S8_CASES:
            rows, ref = tiled(vd, c, S, S)
            inp = torch.from_numpy(rows[np.arange(n) % TILE].reshape(-1)).cuda()
            one = torch.zeros(n * nb, dtype=torch.uint8, device="cuda")
            lc.launch_device(d, c, inp.data_ptr(), 4 * rows.shape[1], one.data_ptr(), nb, S, n, stream=cur_stream())
            torch.cuda.synchronize()
            single = one.cpu().numpy()
            assert_tiled(single.view(ref.dtype).reshape(n, -1), ref, n)
            inputs.append((inp, 4 * rows.shape[1]))
            singles.append(single)
        outs = [[torch.zeros(n * nb, dtype=torch.uint8, device="cuda") for _ in range(reps)] for _ in lc.S8_CASES]
        streams = [torch.cuda.Stream() for _ in lc.S8_CASES]
        torch.cuda.synchronize()
        for k in range(reps):
            for i, c in enumerate(lc.S8_CASES):
                lc.launch_device(d, c, inputs[i][0].data_ptr(), inputs[i][1], outs[i][k].data_ptr(), nb, S, n,
                                 stream=streams[i].cuda_stream)
        torch.cuda.synchronize()
        if guard:
            assert d.guard_violations() == 0
    for i, c in enumerate(lc.S8_CASES):
        for k in range(reps):
            got = outs[i][k].cpu().numpy()
            bad = np.flatnonzero(got != singles[i])
            assert bad.size == 0, f"{lc.cid(c)} launch {k}: {bad.size} bytes differ, first in frame {int(bad[0]) // nb}"


# ---------------------------------------------------------------- 6. odd values inside frames
EDGE_OPTS = [HARD | M_B32, SOFT4 | M_B16, SOFT8 | M_B16, SOFT16 | M_B32, FP32 | M_FP16]
EDGE_CASES = [lc.Case("frm", o, t, None) for o in EDGE_OPTS for t in (True, False) if t or (o & 0xF) != HARD] + \
             [lc.Case("pun", o, t, lc.P34) for o in EDGE_OPTS if (o & 0xF) != HARD for t in (True, False)] + \
             [lc.Case("tb", o, None, None) for o in EDGE_OPTS]


def edge_rows(vd, c, S, seed):
    """5 frames of S stages as the launch reads them, 60 floats of each overwritten with test_gpu_llr.specials(): the
    frame's first and last stage always, for tail-biting frames floats of the stages the wrap reads twice (the last 26,
    which the lead repeats, and the first ones, which follow the frame again), the rest drawn"""
    rng = np.random.default_rng(seed)
    rows = np.stack([lc.row_of(vd, c, v) for v in lc.small_frames(c, 5, S, seed)[1]])
    L = rows.shape[1]
    sp = specials()
    if (c.opt & 0xF) == FP32:  # the FP32 branch metric of NaN and infinities is not defined by the reference: keep finite
        sp = np.where(np.isfinite(sp), sp, np.float32(1e30)).astype(np.float32)
    for f in range(rows.shape[0]):
        fixed = np.array([0, 1, L - 2, L - 1] + ([2 * (S - 26), 2 * (S - 25) + 1, 2 * (S - 2), 4, 7, 2 * 20 + 1] if c.fam == "tb" else []))
        fixed = np.unique(fixed)
        rest = np.setdiff1d(np.arange(L), fixed)
        idx = np.concatenate([fixed, rng.choice(rest, 60 - fixed.size, replace=False)])
        rows[f, idx] = np.roll(np.resize(sp, idx.size), f)  # (the first and last floats take another value in every frame)
    return rows


@pytest.mark.gpu
@pytest.mark.parametrize("scale", [SCALE, 1.0], ids=["scale40000", "scale1"])
@pytest.mark.parametrize("case", EDGE_CASES, ids=lc.cid)
def test_odd_values_inside_frames(gpu, vd, case, scale):
    """NaN, +-inf, -0.0, the round-to-even halves, saturating values and denormals inside frames of 250 and 97 stages:
    word parity with the oracle of the same floats, blocking and device entry points"""
    import torch
    with vd.ViterbiCUDA(case.opt) as d:
        for S in (250, 97):
            rows = edge_rows(vd, case, S, seed=600 + S)
            ref = np.stack([lc.oracle_row(vd, case, r, S, scale) for r in rows])
            if case.fam == "tb":
                host, _ = d.run_tb_frames(rows, scale)
            elif case.fam == "pun":
                host, _ = d.run_punct_frames(rows, case.pat, S, case.term, scale)
            else:
                host, _ = d.run_frames(rows, case.term, scale)
            assert host.dtype == ref.dtype and np.array_equal(host, ref), (S, np.argwhere(host != ref)[:5].tolist())
            n, nb = rows.shape[0], lc.frame_nbytes(S)
            inp = torch.from_numpy(rows.reshape(-1).copy()).cuda()
            out = torch.zeros(n * nb, dtype=torch.uint8, device="cuda")
            lc.launch_device(d, case, inp.data_ptr(), 4 * rows.shape[1], out.data_ptr(), nb, S, n, scale, stream=cur_stream())
            torch.cuda.synchronize()
            assert np.array_equal(out.cpu().numpy().view(ref.dtype).reshape(n, -1), ref), S
