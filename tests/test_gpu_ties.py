"""Tie-dense and degenerate inputs through every launch form, word for word against the oracle.

On channel noise or uniformly random words few add-compare-selects tie (the oracle's M_B32 and M_B16 words
differ in 49 of 31,249 on random SOFT8 bytes), so parity on such inputs hardly checks the tie rules -- which is
what the tagged formats implement in a roundabout way (+-2^j tags in the history field, the +tag area of M_B32's
phase 0, the complemented upper half of the SOFT8 ring, the tracebacks' fix-ups).  The patterns of
tests/tie_patterns.py make ties the rule: on all-zero soft input every decision is a tie and the cores' words
differ everywhere.  Forms: vd_decode_tg (single batch of 1,000,032 bits: chunks of 4 and 5 words), vd_decode_pk
batched (three batches, each another pattern; 5,649 chunks of 5 words, so one wave holds chunks of different
length), vd_decode_pk split (13,107,264 bits: 64 words per chunk, the smallest split launch; with and without
tail workgroups, and vd_decode_tg's segment launch), and the fused-LLR twins of the last two.
Every pattern keeps the metrics in the reference's exact range (the oracle reports ok) for every format, SOFT16
included, at both sizes; every test asserts it.
"""
import numpy as np
import pytest
import torch

import tie_patterns as tp
from test_gpu_parity import VALID, name
from test_gpu_pk import _decode_batched, _single
from vitdec import FP32, HARD, M_B16, M_B32, M_FP16, O_B16, SOFT4, SOFT8

NBITS = 1_000_032
NSPLIT = 13_107_264
PK_PAIRS = [ch | me for ch in (HARD, SOFT4, FP32) for me in (M_B32, M_B16, M_FP16)] + [SOFT8 | M_B32, SOFT8 | M_B16]
PK_OPTS = PK_PAIRS + [HARD | M_B32 | O_B16, SOFT4 | M_FP16 | O_B16, SOFT8 | M_B32 | O_B16, SOFT8 | M_B16 | O_B16,
                      FP32 | M_B16 | O_B16]
LLR_OPTS = [HARD | M_B32, SOFT4 | M_B16, SOFT8 | M_B32, SOFT8 | M_B16, FP32 | M_FP16]
# three batches per launch, rotating through the seven patterns: every pattern is decoded
GROUPS = [[tp.PATTERNS[(3 * g + b) % 7] for b in range(3)] for g in range(3)]
CORES = {HARD: (M_B32, M_B16, M_FP16), SOFT4: (M_B32, M_B16, M_FP16), SOFT8: (M_B32, M_B16), FP32: (M_B32, M_B16, M_FP16)}


def _differ(got, ref, what):
    bad = np.flatnonzero(got != ref)
    assert bad.size == 0, f"{what}: {bad.size} of {ref.size} words differ, first {bad[:5]}: " \
                          f"{[hex(int(x)) for x in got[bad[:3]]]} for {[hex(int(x)) for x in ref[bad[:3]]]}"


@pytest.mark.parametrize("ch", list(CORES), ids=lambda c: name(c).split("-")[0])
def test_patterns_tell_the_tie_rules_apart(vo, ch):
    """Not vacuous: for every pair of metric cores of a format some pattern's oracle words differ in at least 1,000
    of 31,249 words (SOFT4 / SOFT8 / FP32: all of them on `zeros`; HARD M_B32 against M_B16 only on `random`), so
    a kernel that applied another core's tie rule would fail the parity tests below."""
    cores = CORES[ch]
    todo = {(a, b) for i, a in enumerate(cores) for b in cores[i + 1:]}
    for kind in ("zeros", "random", "saturated", "sparse", "ternary", "all_min", "all_max"):
        for a, b in sorted(todo):
            if int((tp.reference(ch | a, kind, NBITS)[0] != tp.reference(ch | b, kind, NBITS)[0]).sum()) >= 1000:
                todo.discard((a, b))
        if not todo:
            break
    assert not todo, f"no pattern separates the cores {sorted(todo)}"
    if ch != HARD:
        words = {me: tp.reference(ch | me, "zeros", NBITS)[0] for me in cores}
        # (M_B32's rule goes by the stage's phase in the chunk, stage mod 6, so a word's place in its chunk shows)
        assert {int(w) for w in np.unique(words[M_B32])} == {0xF83F83F8, 0xF0BF0BF0, 0xF23F23F2}
        assert (words[M_B16] == 0xF03F03F0).all()
        assert M_FP16 not in words or (words[M_FP16] == 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", tp.PATTERNS)
@pytest.mark.parametrize("opt", VALID, ids=name)
def test_ties_single_batch_tagged_kernel(gpu, vo, opt, kind):
    """vd_decode_tg, one chunk per wave, chunks of 4 and 5 words: every valid option on every pattern"""
    n = 2 * NBITS
    ref, ok = tp.reference(opt, kind, NBITS)
    assert ok, "the oracle left the reference's exact metric range"
    with gpu.ViterbiCUDA(opt) as d:
        assert d.kernel_for(n, 1).startswith("vd_decode_tg<")
        out, _ = d.run(tp.pattern(opt, kind, n), inputNum=n)
    _differ(out, ref, f"{name(opt)} {kind}")


def _to_device(arrays, nin):
    """the batches' bytes at a 256-byte stride in one device buffer"""
    stride = (nin + 255) // 256 * 256
    host = torch.zeros(len(arrays) * stride, dtype=torch.uint8)
    for b, a in enumerate(arrays):
        host[b * stride:b * stride + nin] = torch.from_numpy(a.view(np.uint8)[:nin].copy())
    return host.to("cuda"), stride


@pytest.mark.gpu
@pytest.mark.parametrize("group", range(3), ids=lambda g: "+".join(GROUPS[g]))
@pytest.mark.parametrize("opt", PK_OPTS, ids=name)
def test_ties_batched_packed_kernel(gpu, vo, opt, group):
    """vd_decode_pk batched: three batches, each another pattern, equal to the oracle and to vd_decode_tg
    (VD_NO_PK=1); nothing written between the batches' outputs (_decode_batched checks it)"""
    n, nb = 2 * NBITS, 3
    kinds = GROUPS[group]
    nin = gpu.lib().vd_input_size(opt, n)
    packed, stride = _to_device([tp.pattern(opt, k, n) for k in kinds], nin)
    with gpu.ViterbiCUDA(opt) as d:
        assert d.kernel_for(n, nb).startswith("vd_decode_pk<") and " batched" in d.kernel_for(n, nb)
    pk, ostride, nout = _decode_batched(gpu, opt, packed, stride, n, nb, no_pk=False)
    tg, _, _ = _decode_batched(gpu, opt, packed, stride, n, nb, no_pk=True)
    for b, kind in enumerate(kinds):
        ref, ok = tp.reference(opt, kind, NBITS)
        assert ok
        _differ(pk[b * ostride:b * ostride + nout].cpu().numpy().view(ref.dtype), ref, f"batch {b} ({kind})")
        assert torch.equal(pk[b * ostride:b * ostride + nout], tg[b * ostride:b * ostride + nout]), kind


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["zeros", "ternary", "sparse", "saturated"])
@pytest.mark.parametrize("opt", PK_OPTS, ids=name)
def test_ties_split_packed_kernel(gpu, vo, opt, kind):
    """vd_decode_pk split (the default launch and VD_PK_TAIL=0) and vd_decode_tg's segment launch
    (VD_PK_SPLIT=0): equal to each other and to the oracle; no wave reaches the pass cap"""
    n = 2 * NSPLIT
    host = tp.pattern(opt, kind, n)
    nin = gpu.lib().vd_input_size(opt, n)
    packed, _ = _to_device([host], nin)
    with gpu.ViterbiCUDA(opt) as d:
        assert d.kernel_for(n, 1).startswith("vd_decode_pk<") and " split" in d.kernel_for(n, 1)
    caps = gpu.split_cap_exits()
    pk = _single(gpu, opt, packed, nin, n, {})
    notail = _single(gpu, opt, packed, nin, n, {"VD_PK_TAIL": "0"})
    tg = _single(gpu, opt, packed, nin, n, {"VD_PK_SPLIT": "0"})
    assert gpu.split_cap_exits() == caps == 0
    ref, ok = vo.decode(opt, host, input_num=n, nthreads=16)
    assert ok
    _differ(pk.cpu().numpy().view(ref.dtype), ref, f"{name(opt)} {kind}")
    assert torch.equal(pk, notail) and torch.equal(pk, tg)


@pytest.mark.gpu
@pytest.mark.parametrize("opt", LLR_OPTS, ids=name)
def test_ties_fused_llr_batched(gpu, vo, opt):
    """vd_decode_pk batched with the packer fused into the table build: the three float patterns as the three
    batches of one launch, equal to the oracle's pack + decode"""
    n, nb = 2 * NBITS, 3
    vals, istride = _to_device([tp.llr_pattern(opt, k, n) for k in tp.LLR_PATTERNS], 4 * n)
    nout = gpu.lib().vd_output_size(opt, n)
    ostride = (nout + 255) // 256 * 256 + 256
    out = torch.full((nb * ostride,), 0x5A, dtype=torch.uint8, device="cuda")
    with gpu.ViterbiCUDA(opt) as d:
        assert d.kernel_for(n, nb, True).startswith("vd_decode_pk<LLR+") and " batched" in d.kernel_for(n, nb, True)
        d.run_device_llr_batch(vals.data_ptr(), istride, out.data_ptr(), ostride, n, nb, tp.LLR_SCALE)
        torch.cuda.synchronize()
    for b, kind in enumerate(tp.LLR_PATTERNS):
        ref, ok = tp.llr_reference(opt, kind, NBITS)
        assert ok
        _differ(out[b * ostride:b * ostride + nout].cpu().numpy().view(ref.dtype), ref, f"batch {b} ({kind})")
        assert bool((out[b * ostride + nout:(b + 1) * ostride] == 0x5A).all())


@pytest.mark.gpu
@pytest.mark.parametrize("kind", tp.LLR_PATTERNS)
@pytest.mark.parametrize("opt", LLR_OPTS, ids=name)
def test_ties_fused_llr_split(gpu, vo, opt, kind):
    """vd_decode_pk split with the packer fused: equal to the oracle's pack + decode, no pass-cap exit"""
    n = 2 * NSPLIT
    host = tp.llr_pattern(opt, kind, n)
    vals = torch.from_numpy(host).to("cuda")
    nout = gpu.lib().vd_output_size(opt, n)
    out = torch.full((nout + 256,), 0x5A, dtype=torch.uint8, device="cuda")
    caps = gpu.split_cap_exits()
    with gpu.ViterbiCUDA(opt) as d:
        assert d.kernel_for(n, 1, True).startswith("vd_decode_pk<LLR+") and " split" in d.kernel_for(n, 1, True)
        d.run_device_llr(vals.data_ptr(), out.data_ptr(), n, tp.LLR_SCALE)
        torch.cuda.synchronize()
    assert gpu.split_cap_exits() == caps == 0
    assert bool((out[nout:] == 0x5A).all())
    ref, ok = vo.decode(opt, vo.pack(opt, host, tp.LLR_SCALE), input_num=n, nthreads=16)
    assert ok
    _differ(out[:nout].cpu().numpy().view(ref.dtype), ref, f"{name(opt)} {kind}")
