"""vd_split_redecodes equals its CPU prediction, exactly, for segment launches of vd_decode_tg.

The segment launch's pass loop (vd_kernel_tg.h "segment launches": speculative segment starts inside chunks,
checked against the left neighbour's end vector, re-decoded from the boundary block) decodes the right words even
if it compares the wrong vectors, re-decodes every segment or takes its start vector from the wrong neighbour;
only the counter shows it.  The count is a function of the input and the segment table alone:
tests/seg_predict.py walks the same loop on the oracle's metric vectors.  Every case is one launch of 13,107,264
bits (64 words per chunk: the smallest segment launch; the one O_B16 case has chunks of 130 and 129 16-bit words)
at each of the three tables (VD_SPLIT=pieces / thirds / sevenths; VD_PK_SPLIT=0 where the option has a packed
kernel), with `==` on the counter, vd_split_cap_exits staying 0, the words equal to the oracle's, the bytes after
the output untouched and no LDS guard word overwritten.  Punctured launches re-decode from boundary blocks at
every residue of their period (3, 5, 7), with the buffer one float into its allocation and NaNs behind it.

Predicted re-decodes (tests/test_seg_predict.py pins them; 1024 SIMDs) as pieces / thirds / sevenths, seed 5
everywhere, scale 40000 for float input:

  input                                      option, entry point                 predicted = counted    3 passes
  uniformly random 32-bit words              SOFT16|M_B32, packed                 324 / 2095 /  918        0
  same, nbits = 64 + 16 (6400 * 129 + 3201)  SOFT16|M_B32|O_B16, packed           323 / 2146 /  868        0
  torch.randint bytes, manual_seed(5)        HARD|M_B32, packed, VD_PK_SPLIT=0    148 /  953 /  381        0
  same                                       SOFT8|M_B16, packed, VD_PK_SPLIT=0   273 / 2039 /  909        0
  full-range floats                          FP32|M_FP16, packed, VD_PK_SPLIT=0   234 / 1507 /  652        0
  normal floats * 2e-3                       SOFT16|M_B32, fused LLR              291 / 2112 /  886        0
  same, punctured 3/4 (3, 101, 011)          SOFT8|M_B16, punctured               632 / 4396 / 1877        2
  same, 5/6 (5, 10101, 01011)                SOFT8|M_B16, punctured               722 / 5026 / 2156       12
  same, 7/8 (7, 1010001, 0101111)            SOFT8|M_B16, punctured               790 / 5154 / 2212       33
  same, 7/8                                  SOFT16|M_B32, punctured              790 / 5154 / 2212       33
  same, 2/3 (2, 01, 11)                      FP32|M_B32|O_B16, punctured          486 / 3421 / 1546        1
  channel values, SNR 15, seeds 91/92,       SOFT8|M_B16, SOFT16|M_B32,             0 /    0 /    0        0
    punctured 3/4 and 7/8                      FP32|M_B32|O_B16, punctured
  simulated channel, SNR 15, seeds 91/92     SOFT16|M_B32, packed                   0 /    0 /    0        0

Counted on an MI355X with 256 CUs (1024 SIMDs: 1792 / 2048 / 1792 workgroups, of which 256 / 1792 / 768 hold three
speculative segments each): every launch counted exactly its prediction.  The predictions of the first row and of
the SOFT8 punctured rows are those of the numpy prototype the cases were chosen with; seed 5 was the first tried.
Under 7/8 almost every speculative start fails (5154 of 5376 in thirds) and the few that converge do so in SOFT8
and SOFT16 alike: the values, about +-80 after scaling, are clamped at +-127 in SOFT8 only, which moves no count.

"3 passes" = piece workgroups (of 256) that run two re-decode passes (a re-decoded piece's new end vector
differing from the one its right neighbour restarted from); thirds and sevenths never need a second.  The SNR-15
cases are the ones that catch a spurious re-decode: the prediction is 0 and the counter must not move.
"""
import contextlib
import functools
import os

import numpy as np
import pytest
import torch

import seg_predict as sg
import tie_patterns as tp
import vd_oracle
import vitdec
from vitdec import FP32, HARD, M_B16, M_B32, M_FP16, O_B16, SOFT8, SOFT16

NBITS = 13_107_264
NBITS_O16 = 64 + 16 * (6400 * 129 + 3201)  # chunks of 130 and 129 16-bit words
SEED = 5
SCALE = 40000.0
P23, P34 = (2, 0b01, 0b11), (3, 0b101, 0b011)
P56, P78 = (5, 0b10101, 0b01011), (7, 0b1010001, 0b0101111)
PACKED, LLR, PUN = 0, 1, 2  # the entry point: run_device, run_device_llr, run_device_punct


def _words16(opt, n):
    nin = vd_oracle.input_size(opt, n)
    return np.random.default_rng(SEED).integers(0, 2**32, nin // 4, dtype=np.uint64).astype(np.uint32).view(np.int32)


def _bytes(opt, n):
    """the input of test_gpu_split_count.random_bytes"""
    nin = vd_oracle.input_size(opt, n)
    g = torch.Generator(device="cpu").manual_seed(SEED)
    return torch.randint(0, 256, (nin + 256,), dtype=torch.uint8, generator=g)[:nin].numpy().view(np.int32)


def _floats(opt, n):
    return tp.full_range_floats(np.random.default_rng(SEED), n)


def _normals(opt, n):
    return (np.random.default_rng(SEED).standard_normal(n) * 2e-3).astype(np.float32)


def _snr15_values(opt, n):
    return vd_oracle.channel(n // 2, 15.0, 91, 92)[1]


def _snr15_packed(opt, n):
    return vd_oracle.simulate(opt, n // 2, 15.0, 91, 92)[1]


# id: (option, bits, input, entry point, puncturing pattern, expects re-decodes)
CASES = {"rand-s16-b32": (SOFT16 | M_B32, NBITS, _words16, PACKED, None, True),
         "rand-s16-b32-o16": (SOFT16 | M_B32 | O_B16, NBITS_O16, _words16, PACKED, None, True),
         "bytes-h-b32": (HARD | M_B32, NBITS, _bytes, PACKED, None, True),
         "bytes-s8-b16": (SOFT8 | M_B16, NBITS, _bytes, PACKED, None, True),
         "floats-f-f16": (FP32 | M_FP16, NBITS, _floats, PACKED, None, True),
         "llr-s16-b32": (SOFT16 | M_B32, NBITS, _normals, LLR, None, True),
         "p34-s8-b16": (SOFT8 | M_B16, NBITS, _normals, PUN, P34, True),
         "p56-s8-b16": (SOFT8 | M_B16, NBITS, _normals, PUN, P56, True),
         "p78-s8-b16": (SOFT8 | M_B16, NBITS, _normals, PUN, P78, True),
         "p78-s16-b32": (SOFT16 | M_B32, NBITS, _normals, PUN, P78, True),
         "p23-f-b32-o16": (FP32 | M_B32 | O_B16, NBITS, _normals, PUN, P23, True),
         "snr15-p34-s8-b16": (SOFT8 | M_B16, NBITS, _snr15_values, PUN, P34, False),
         "snr15-p34-s16-b32": (SOFT16 | M_B32, NBITS, _snr15_values, PUN, P34, False),
         "snr15-p34-f-b32-o16": (FP32 | M_B32 | O_B16, NBITS, _snr15_values, PUN, P34, False),
         "snr15-p78-s8-b16": (SOFT8 | M_B16, NBITS, _snr15_values, PUN, P78, False),
         "snr15-p78-s16-b32": (SOFT16 | M_B32, NBITS, _snr15_values, PUN, P78, False),
         "snr15-p78-f-b32-o16": (FP32 | M_B32 | O_B16, NBITS, _snr15_values, PUN, P78, False),
         "snr15-s16-b32": (SOFT16 | M_B32, NBITS, _snr15_packed, PACKED, None, False)}
MODES = ["pieces", "thirds", "sevenths"]


@functools.lru_cache(maxsize=1)
def case_input(case):
    """(device input, packed words) of a case: what the launch reads and what the oracle and the predictor read"""
    opt, nbits, make, entry, pattern, _ = CASES[case]
    n = 2 * nbits
    host = make(opt, n)
    if entry == PUN:
        host = vitdec.puncture(host, pattern)
        packed = vd_oracle.pack(opt, vitdec.depuncture(host, pattern, n), SCALE)
    else:
        packed = vd_oracle.pack(opt, host, SCALE) if entry == LLR else host
    for a in (host, packed):
        a.setflags(write=False)
    return host, packed


@functools.lru_cache(maxsize=1)
def _oracle_words(case):
    opt, nbits = CASES[case][:2]
    ref, ok = vd_oracle.decode(opt, case_input(case)[1], input_num=2 * nbits, nthreads=16)
    assert ok
    ref.setflags(write=False)
    return ref


def check_not_vacuous(case, mode, pred):
    """properties of the chosen inputs, asserted on the prediction, never on the kernel's counter"""
    _, _, _, entry, _, redecodes = CASES[case]
    if not redecodes:
        assert pred.total == 0
        return
    assert pred.total >= 100
    # a kernel that re-decoded every speculative segment after pass 0, or only those whose own comparison failed,
    # counts otherwise
    assert len(pred.mismatch0) + pred.chained < 3 * pred.spec_wgs and pred.chained >= 50
    if entry == PUN and mode == "pieces":
        assert max(pred.hist) >= 3, "no piece workgroup with three passes (a cascade of two re-decode passes)"


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
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", list(CASES))
def test_segment_redecode_count_equals_prediction(gpu, vo, case, mode):
    opt, nbits, _, entry, pattern, _ = CASES[case]
    n = 2 * nbits
    host, packed = case_input(case)
    ref = _oracle_words(case)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    table = sg.launch_table(4 * cus, sg.MODES[mode])
    assert table, f"no segment table for {cus} CUs"
    pred = sg.predict(vo, opt, packed, n, table)
    print(f"{case} {mode}: {cus} CUs, {len(table) - 1} workgroups, {pred.spec_wgs} with a speculative segment; "
          f"predicted {pred.total} (chained {pred.chained}), passes {pred.hist}")
    check_not_vacuous(case, mode, pred)

    # the input one float (4 bytes) into its allocation and followed by NaNs where the entry point takes 4-byte
    # aligned floats (punctured); 16-byte aligned otherwise
    lead = 1 if entry == PUN else 0
    raw = np.ascontiguousarray(host).view(np.uint8)
    buf = torch.full((4 * lead + raw.size + 256,), 0xFF, dtype=torch.uint8, device="cuda")  # 0xFFFFFFFF: a NaN
    buf[4 * lead:4 * lead + raw.size] = torch.tensor(raw).to("cuda")
    nout = gpu.lib().vd_output_size(opt, n)
    out = torch.full((nout + 256,), 0x5A, dtype=torch.uint8, device="cuda")
    env = {"VD_SPLIT": mode}
    if entry != PUN and (opt & 0xF) != SOFT16:
        env["VD_PK_SPLIT"] = "0"
    with _env(env), gpu.ViterbiCUDA(opt) as d:
        kernel = d.kernel_for(n, 1, entry)
        assert kernel.startswith(("vd_decode_tg<", "vd_decode_tg<LLR+", "vd_decode_tg<PUN+")[entry]), kernel
        assert (entry != PACKED or "+" not in kernel.split(">")[0]) and "segment launch" in kernel, kernel
        d.set_guard_check(True)
        before, caps = gpu.split_redecodes(), gpu.split_cap_exits()
        if entry == PUN:
            d.run_device_punct(buf.data_ptr() + 4 * lead, out.data_ptr(), n, pattern, scale=SCALE)
        elif entry == LLR:
            d.run_device_llr(buf.data_ptr(), out.data_ptr(), n, SCALE)
        else:
            d.run_device(buf.data_ptr(), out.data_ptr(), n)
        torch.cuda.synchronize()
        counted = gpu.split_redecodes() - before
        guards = d.guard_violations()
    print(f"{case} {mode}: counted {counted}")
    assert gpu.split_cap_exits() == caps == 0
    assert guards == 0, f"{guards} LDS guard words overwritten"
    assert bool((out[nout:] == 0x5A).all())
    got = out[:nout].cpu().numpy().view(ref.dtype)
    bad = np.flatnonzero(got != ref)
    assert bad.size == 0, f"{bad.size} of {ref.size} words differ, first {bad[:5]}"
    assert counted == pred.total, f"counted {counted} re-decodes, predicted {pred.total}"
