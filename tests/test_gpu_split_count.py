"""vd_split_redecodes equals its CPU prediction, exactly, for split launches of vd_decode_pk.

The split launch's pass loop (vd_kernel_pk.h "Split" and "Early stop": replay or checkpoints, both halves of a wave
re-decoding in one pass, cascades of three passes in tail workgroups, kmax truncation) decodes the right words
even if it re-decodes every part or compares the wrong halves; only the counter shows it.  The count is a
function of the input alone: tests/split_predict.py walks the same loop on the oracle's metric vectors.  Every
case here is one launch of 13,107,264 bits (64 words per chunk: the smallest split launch, the shortest tail
parts, the most cascades) with `==` on the counter, vd_split_cap_exits staying 0 and the words equal to the oracle's.

Predicted (and, on an MI355X with 256 CUs, counted) re-decodes; "tail" = 256 tail chunks (6400 mod 4 * 256), their
passes histogram {passes: chunks}, "both" = tail wave-passes with both halves re-decoding, seed 5 everywhere:

  input                                   option             default = whole + tail   tail histogram         both  VD_PK_TAIL=0
  torch.randint bytes, manual_seed(5)     HARD|M_B32            819 =  637 + 182      {1:123, 2:128, 3:5}       7      668
  same                                    SOFT4|M_B16          1218 =  959 + 259      {1: 86, 2:169, 3:1}      14      988
  same                                    SOFT8|M_B16          1806 = 1438 + 368      {1: 57, 2:194, 3:5}      31     1487
  same                                    SOFT8|M_B32|O_B16    1806 = 1438 + 368      {1: 57, 2:194, 3:5}      31     1487
  full-range floats, default_rng(5)       FP32|M_FP16          1261 =  971 + 290      {1: 73, 2:179, 3:4}      18     1009
  normal floats * 2e-3, default_rng(5),   SOFT8|M_B16          1835 = 1392 + 443      {1: 40, 2:210, 3:6}      38     1442
    fused LLR launch (scale 40000)
  simulated channel, SNR 15, seeds 91/92  HARD|M_B32, SOFT8|M_B16   0                 {1:256}                   0        0

Seed 5 was the first tried for every format and already has a tail chunk with three passes.  The SNR-15 cases are
the ones that catch a spurious re-decode: the prediction is 0 and the counter must not move.
"""
import contextlib
import functools
import os

import numpy as np
import pytest
import torch

import split_predict as sp
import tie_patterns as tp
import vd_oracle
from vitdec import FP32, HARD, M_B16, M_B32, M_FP16, O_B16, SOFT4, SOFT8

NBITS = 13_107_264
N = 2 * NBITS
SEED = 5
LLR_SCALE = 40000.0


def random_bytes(opt, n, seed=SEED):
    """the input of test_gpu_pk.test_packed_split_random_input_redecodes, cut to the input size"""
    nin = vd_oracle.input_size(opt, n)
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randint(0, 256, (nin + 256,), dtype=torch.uint8, generator=g)[:nin].numpy().view(np.int32)


def _floats(opt, n):
    return tp.full_range_floats(np.random.default_rng(SEED), n)


def _llr(opt, n):
    return (np.random.default_rng(SEED).standard_normal(n) * 2e-3).astype(np.float32)


def _snr15(opt, n):
    return vd_oracle.simulate(opt, n // 2, 15.0, 91, 92)[1]


# id: (option, input, fused LLR launch, expects re-decodes)
CASES = {"random-h-b32": (HARD | M_B32, random_bytes, False, True),
         "random-s4-b16": (SOFT4 | M_B16, random_bytes, False, True),
         "random-s8-b16": (SOFT8 | M_B16, random_bytes, False, True),
         "random-s8-b32-o16": (SOFT8 | M_B32 | O_B16, random_bytes, False, True),
         "random-f-f16": (FP32 | M_FP16, _floats, False, True),
         "llr-s8-b16": (SOFT8 | M_B16, _llr, True, True),
         "snr15-h-b32": (HARD | M_B32, _snr15, False, False),
         "snr15-s8-b16": (SOFT8 | M_B16, _snr15, False, False)}


@functools.lru_cache(maxsize=1)
def _case(case):
    """(host input, packed words, oracle words) of a case, shared by its two launches"""
    opt, make, llr, _ = CASES[case]
    host = make(opt, N)
    packed = vd_oracle.pack(opt, host, LLR_SCALE) if llr else host
    ref, ok = vd_oracle.decode(opt, packed, input_num=N, nthreads=16)
    assert ok
    for a in (host, packed, ref):
        a.setflags(write=False)
    return host, packed, ref


@contextlib.contextmanager
def _env(env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.mark.gpu
@pytest.mark.parametrize("tails", ["default", "notail"])
@pytest.mark.parametrize("case", list(CASES))
def test_split_redecode_count_equals_prediction(gpu, vo, case, tails):
    opt, _, llr, redecodes = CASES[case]
    host, packed, ref = _case(case)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    tail = sp.default_tail(cus) if tails == "default" else 0
    pred = sp.predict(vo, opt, packed, N, tail)
    print(f"{case} {tails}: {cus} CUs, {tail} tail chunks; predicted {pred.total} = {pred.whole_fail} whole-chunk waves + "
          f"{pred.tail_redecodes} in tail workgroups, tail passes {pred.tail_hist}, both halves {pred.both_halves}")
    # not vacuous (on the prediction, never on the kernel's counter)
    if redecodes:
        assert pred.whole_fail >= 100
        if tail:
            assert max(pred.tail_hist) >= 3, "no tail chunk with a cascade of three passes"
            assert pred.both_halves >= 1, "no tail wave-pass with both halves re-decoding"
    else:
        assert pred.total == 0

    dev = torch.tensor(host.view(np.uint8)).to("cuda")  # (a copy: the shared input stays read-only)
    nout = gpu.lib().vd_output_size(opt, N)
    out = torch.full((nout + 256,), 0x5A, dtype=torch.uint8, device="cuda")
    with _env({} if tails == "default" else {"VD_PK_TAIL": "0"}), gpu.ViterbiCUDA(opt) as d:
        kernel = d.kernel_for(N, 1, llr)
        assert kernel.startswith("vd_decode_pk<LLR+" if llr else "vd_decode_pk<") and " split" in kernel
        before, caps = gpu.split_redecodes(), gpu.split_cap_exits()
        if llr:
            d.run_device_llr(dev.data_ptr(), out.data_ptr(), N, LLR_SCALE)
        else:
            d.run_device(dev.data_ptr(), out.data_ptr(), N)
        torch.cuda.synchronize()
        counted = gpu.split_redecodes() - before
    print(f"{case} {tails}: counted {counted}")
    assert gpu.split_cap_exits() == caps == 0
    assert bool((out[nout:] == 0x5A).all())
    got = out[:nout].cpu().numpy().view(ref.dtype)
    bad = np.flatnonzero(got != ref)
    assert bad.size == 0, f"{bad.size} of {ref.size} words differ, first {bad[:5]}"
    assert counted == pred.total, f"counted {counted} re-decodes, predicted {pred.total}"
