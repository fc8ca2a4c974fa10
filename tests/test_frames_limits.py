"""The long frames of tests/test_gpu_frames_limits.py on the CPU: the oracle's own words of exactly those frames
(limits_common.long_frames: lengths up to 2^20 stages, sigma 0.3, scale 40000, seeds LONG_SEED + f) decode every bit
of the terminated and the tail-biting frames of 4096 stages and more with no error, in all six options.  The GPU
tests assert the same of the kernels' words, which they also compare with these words one by one; this file keeps
that assertion from ever blaming a kernel for the code's own limit at a seed.  (Punctured frames are left out: at
3/4 and sigma 0.3 the fixed window leaves a few bit errors in 2^20 stages, the documented window limit.)"""
import numpy as np
import pytest

import limits_common as lc
from frames_common import OPTIONS6, decoded_bits
from tb_common import wrapped_bits


def test_case_lists():
    """every format, metric core and output width in each family; HARD only where the API takes it; each pattern with
    SOFT8 | M_B16"""
    frm = [c for c in lc.CASES if c.fam == "frm"]
    pun = [c for c in lc.CASES if c.fam == "pun"]
    tb = [c for c in lc.CASES if c.fam == "tb"]
    assert len(frm) == 11 and len(pun) == 14 and len(tb) == 6 and len(set(lc.CASES)) == 31
    assert {c.opt for c in frm if c.term} == set(OPTIONS6) == {c.opt for c in tb}
    assert all((c.opt & 0xF) != lc.HARD for c in frm if not c.term) and all((c.opt & 0xF) != lc.HARD for c in pun)
    assert {c.pat for c in pun if c.opt == lc.S8} == {lc.P34, lc.P78, lc.P16}
    assert lc.LONG_LENGTHS == [1 << 20, (1 << 20) - 31, 65536 + 33, 65535, 4097, 97, 0, 1] and lc.LONG_MAX == 1 << 20
    assert [c.fam for c in lc.S8_CASES] == ["frm", "pun", "tb"] and all(c.opt == lc.S8 for c in lc.S8_CASES)


def test_long_frames_are_drawn_once_and_differ():
    for kind in ("terminated", "open", "tb"):
        fr = lc.long_frames(kind)
        assert fr is lc.long_frames(kind) and [0 if f is None else f[0].size for f in fr] == lc.LONG_LENGTHS
        assert all(f is None or (f[1].dtype == np.float32 and f[1].size == 2 * f[0].size) for f in fr)
        assert not np.array_equal(fr[0][0][:4096], fr[1][0][:4096])  # (a seed per frame: no frame is a prefix of another)
    term = lc.long_frames("terminated")
    assert all(f is None or not f[0][-6:].any() for f in term)


@pytest.mark.parametrize("case", [c for c in lc.CASES if c.fam == "tb" or (c.fam == "frm" and c.term)], ids=lc.cid)
def test_the_oracle_decodes_every_bit_of_the_long_frames(vd, vo, case):
    refs = lc.long_refs(vd, case)
    for S, fr, w in zip(lc.LONG_LENGTHS, lc.long_frames(lc.long_kind(case)), refs):
        if S < lc.LONG_CHECKED:
            continue
        if case.fam == "tb":
            nb = 32 * ((S + 31) // 32)
            got, want = decoded_bits(case.opt, w, nb), wrapped_bits(fr[0], nb)
        else:
            got, want = decoded_bits(case.opt, w, S), fr[0]
        assert np.array_equal(got, want), (S, int((got != want).sum()), np.flatnonzero(got != want)[:5])
