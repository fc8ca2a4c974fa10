"""The re-decode predictor of tests/split_predict.py (CPU only): its passes per chunk equal the host model's
(tools/split_model.py split_passes, an independent numpy walk of the same pass loop), and on the HARD input of
tests/test_gpu_split_count.py it gives the numbers worked out beforehand with a numpy prototype."""
import numpy as np
import pytest
import torch

import split_predict as sp

NBITS = 13_107_264  # 64 words per chunk: the smallest split launch


def seed5_bytes(nin):
    """the input of test_gpu_pk.test_packed_split_random_input_redecodes, cut to nin bytes"""
    g = torch.Generator(device="cpu").manual_seed(5)
    return torch.randint(0, 256, (nin + 256,), dtype=torch.uint8, generator=g)[:nin].numpy()


def test_pk_cut_is_the_models():
    sm = sp.split_model()
    assert sp.K_WARM == sm.K_WARM
    for W in (64, 65, 78, 79, 157, 300):
        for P in (2, 8):
            assert [sp.pk_cut(p, P, W) for p in range(P + 2)] == [sm.pk_cut(p, P, W) for p in range(P + 2)]
    assert sp.default_tail(256) == 256 and sp.default_tail(304) == 320 and sp.default_tail(64) == 0


@pytest.mark.parametrize("words,o16,seed", [(64, False, 3), (70, False, 2), (131, True, 23)])
def test_passes_equal_the_split_model(vo, words, o16, seed):
    """SOFT8, uniformly random bytes, 24 chunks of which the last 8 are tail chunks (P = 8); a ragged partition
    (chunks of `words` and `words` + 1 words) and 16-bit output words (W = (words + 1) / 2) too.  The seeds are
    the first whose tail chunks hold a cascade of three passes and a wave with both halves re-decoding."""
    sm = sp.split_model()
    nchunks, tail = 24, 8
    bpp = 16 if o16 else 32
    opt = vo.SOFT8 | vo.M_B16 | (vo.O_B16 if o16 else 0)
    nbits = bpp * (words * nchunks + (5 if words != 64 else 0)) + 64
    packed = np.random.default_rng(seed).integers(-128, 128, 2 * nbits).astype(np.int8).view(np.int32)
    pred = sp.predict(vo, opt, packed, 2 * nbits, tail, nchunks=nchunks, nthreads=4)
    want = [sm.split_passes(sp.model_chunk(opt, packed, nbits, nchunks, c), 8 if c >= nchunks - tail else 2)[0]
            for c in range(nchunks)]
    assert pred.passes.tolist() == want
    assert max(want[:nchunks - tail]) == 2 and max(want[nchunks - tail:]) >= 3 and pred.both_halves >= 1
    assert pred.total == pred.whole_fail + pred.tail_redecodes >= sum(w - 1 for w in want)
    assert pred.whole_fail == sum(w - 1 for w in want[:nchunks - tail])
    assert pred.tail_hist == {k: want[nchunks - tail:].count(k) for k in sorted(set(want[nchunks - tail:]))}
    # without tail workgroups every chunk is a two-part chunk
    flat = sp.predict(vo, opt, packed, 2 * nbits, 0, nchunks=nchunks, nthreads=4)
    assert flat.passes.tolist() == [sm.split_passes(sp.model_chunk(opt, packed, nbits, nchunks, c), 2)[0]
                                    for c in range(nchunks)]
    assert flat.total == flat.whole_fail == int((flat.passes == 2).sum()) and flat.tail_hist == {}


def test_hard_seed5_expectations(vo):
    """HARD, 13,107,264 bits, torch seed-5 random bytes, 256 tail chunks.  637 / 182 / 819, the histogram and the
    7 wave-passes are the numpy prototype's numbers.  For the launch without tail workgroups that prototype said
    664; the predictor says 668: the 637 of the first 6,144 chunks and 31 in the last 256, where the prototype had
    27.  A numpy recursion that shares no code with the predictor (below: the last 256 chunks as two-part chunks,
    branch metrics read from the bits by numpy) finds the same 31 chunks."""
    opt = vo.HARD | vo.M_B32
    n = 2 * NBITS
    packed = seed5_bytes(vo.input_size(opt, n)).view(np.int32)
    pred = sp.predict(vo, opt, packed, n, 256)
    assert pred.whole_fail == 637
    assert pred.tail_redecodes == 182
    assert pred.total == 819
    assert pred.tail_hist == {1: 123, 2: 128, 3: 5}
    assert pred.both_halves == 7
    assert np.bincount(pred.passes[:6144]).tolist() == [0, 6144 - 637, 637]
    flat = sp.predict(vo, opt, packed, n, 0)
    assert flat.total == 668 and flat.whole_fail == 668 and flat.tail_redecodes == 0 and flat.both_halves == 0
    assert (flat.passes[:6144] == pred.passes[:6144]).all()

    sm = sp.split_model()
    bm = sp.numpy_branch_metrics(opt, packed, NBITS)
    first = 32 * 64 * np.arange(6144, 6400)  # 64 words per chunk

    def run(start, nblk):  # the last 256 chunks at once, from equal metrics
        pm = np.zeros((start.size, 64), np.int64)
        for t in range(32 * nblk):
            pm = (pm[:, sm.PREV] + bm[start + t][:, sm.LAB]).max(axis=2)
        return pm - pm[:, :1]
    cut = sp.pk_cut(1, 2, 64)
    fails = (run(first, cut) != run(first + 32 * (cut - sp.K_WARM), sp.K_WARM)).any(axis=1)
    assert int(fails.sum()) == 31
    assert (fails == (flat.passes[6144:] == 2)).all()
