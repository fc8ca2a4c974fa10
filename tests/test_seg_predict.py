"""The re-decode predictor of tests/seg_predict.py (CPU only): its restatement of the segment-launch geometry
equals, line for line, the dump of the kernel's own functions (tests/cxx/seg_runs_dump.cpp, built with hipcc for
the host); the workgroups it finds failing at their first boundary are the ones an independent numpy recursion
finds; and on the inputs of tests/test_gpu_seg_count.py it gives the numbers pinned below for a device of 1024
SIMDs (256 CUs), with the properties that keep the GPU test from being vacuous."""
import os
import subprocess

import numpy as np
import pytest

import seg_predict as sg
import split_predict as sp
import test_gpu_seg_count as gc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
NSIMD = 1024

# packNum, 16-bit output words: the sizes of tests/test_gpu_seg_count.py, then 16M and 32M bits
SIZES = [((gc.NBITS - 64) // 32, False), ((gc.NBITS - 64) // 16, True), ((gc.NBITS_O16 - 64) // 16, True),
         (499_998, False), (999_996, True), (999_998, False), (1_999_996, True)]


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    exe = tmp_path_factory.mktemp("seg") / "seg_runs_dump"
    src = os.path.join(ROOT, "tests", "cxx", "seg_runs_dump.cpp")
    csrc = os.path.join(ROOT, "gpu-accelerated-viterbi-decoder_amd", "csrc")
    r = subprocess.run([HIPCC, "-x", "hip", "--offload-arch=gfx950", "-O1", "-std=c++17", "-w", "-I", csrc, src,
                        "-o", str(exe)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]

    def run(nsimd, mode, pack, o16):
        r = subprocess.run([str(exe), str(nsimd), str(mode), str(pack), "16" if o16 else "32"], capture_output=True,
                           text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
        return r.stdout.splitlines()
    return run


@pytest.mark.parametrize("mode", list(sg.MODES))
def test_geometry_equals_the_kernels_functions(dump, mode):
    m = sg.MODES[mode]
    for pack, o16 in SIZES:
        want = dump(NSIMD, m, pack, o16)
        got = sg.dump_lines(NSIMD, m, pack, o16)
        assert len(want) > 6400 // 4, "the dump is empty"
        assert len(got) == len(want)
        diff = [(a, b) for a, b in zip(got, want) if a != b]
        assert not diff, f"pack {pack}, o16 {o16}: {len(diff)} lines differ, first {diff[0]}"
    # the 13M-bit launches have the speculative starts the GPU test counts on (64 words: pieces of 16)
    runs = [ln.split() for ln in sg.dump_lines(NSIMD, m, SIZES[0][0], False) if ln.startswith("run")]
    spec = [r for r in runs if int(r[8]) >= 0]
    assert len(spec) == {"pieces": 3 * 256, "thirds": 3 * 1792, "sevenths": 3 * 768}[mode]
    assert all(int(r[8]) == sg.WARM and int(r[7]) == sg.WARM - 1 and int(r[5]) % 3 == 0 for r in spec)


def test_absent_tables_are_empty_on_both_sides(dump):
    """304 CUs: pieces has no table (6400 mod 1216 chunks do not fill a quarter of the SIMDs), thirds neither;
    100 SIMDs: none of the three.  The launch then takes pieces, or no segment table at all."""
    for nsimd, mode in [(1216, sg.PIECES), (1216, sg.THIRDS), (100, sg.PIECES), (100, sg.THIRDS), (100, sg.SEVENTHS)]:
        assert dump(nsimd, mode, SIZES[0][0], False) == [] == sg.dump_lines(nsimd, mode, SIZES[0][0], False)
    assert sg.launch_table(NSIMD, sg.SEVENTHS) == sg.seg_table(NSIMD, sg.SEVENTHS) != []
    assert sg.launch_table(100, sg.SEVENTHS) == []


@pytest.mark.parametrize("case", ["bytes-h-b32", "bytes-s8-b16"])
def test_first_boundary_failures_equal_a_numpy_recursion(vo, case):
    """pieces, 13,107,264 bits of torch seed-5 random bytes: chunks 6144 .. 6399 are one workgroup each, 64 words
    in pieces of 16, the first boundary at word 14 (16 - 17 % 3).  Segment 1's start vector is the one after
    blocks 9 .. 14 from equal metrics, segment 0's end vector the one after blocks 0 .. 14.  The recursion below
    reads the branch metrics with numpy (split_predict.numpy_branch_metrics) and shares no code with the
    predictor or with the oracle's block_vectors."""
    opt, nbits = gc.CASES[case][:2]
    _, packed = gc.case_input(case)
    table = sg.seg_table(NSIMD, sg.PIECES)
    assert len(table) - 1 == 1536 + 256 and table[1536] == 6144
    pred = sg.predict(vo, opt, packed, 2 * nbits, table)
    assert pred.spec_wgs == 256 and all(g >= 1536 for g, _ in pred.mismatch0)
    a = sg.seg_bound([64], 1)[1]
    assert a == 14

    sm = sp.split_model()
    bm = sp.numpy_branch_metrics(opt, packed, nbits)
    first = 32 * 64 * np.arange(6144, 6400)

    def run(start, nblk):  # the last 256 chunks at once, from equal metrics
        pm = np.zeros((start.size, 64), np.int64)
        for t in range(32 * nblk):
            pm = (pm[:, sm.PREV] + bm[start + t][:, sm.LAB]).max(axis=2)
        return pm - pm[:, :1]
    fails = (run(first, a + 1) != run(first + 32 * (a + 1 - sg.WARM), sg.WARM)).any(axis=1)
    want = {1536 + int(c) for c in np.flatnonzero(fails)}
    assert {g for g, q in pred.mismatch0 if q == 1} == want
    assert len(want) >= 20
    # a workgroup whose first boundary fails re-decodes its three speculative segments in the first pass
    assert all(pred.passes[g] >= 2 for g in want)


# case: (total, passes histogram over the workgroups with a speculative segment, those workgroups, chained) at
# pieces, thirds, sevenths, as the committed predictor gives them for 1024 SIMDs
EXPECTED = {
    "rand-s16-b32": [(324, {1: 111, 2: 145}, 256, 141), (2095, {1: 818, 2: 974}, 1792, 862), (918, {1: 352, 2: 416}, 768, 398)],
    "rand-s16-b32-o16": [(323, {1: 116, 2: 140}, 256, 139), (2146, {1: 810, 2: 982}, 1792, 885), (868, {1: 369, 2: 399}, 768, 358)],
    "bytes-h-b32": [(148, {1: 186, 2: 70}, 256, 73), (953, {1: 1334, 2: 458}, 1792, 444), (381, {1: 576, 2: 192}, 768, 169)],
    "bytes-s8-b16": [(273, {1: 125, 2: 131}, 256, 113), (2039, {1: 846, 2: 946}, 1792, 836), (909, {1: 344, 2: 424}, 768, 361)],
    "floats-f-f16": [(234, {1: 156, 2: 100}, 256, 112), (1507, {1: 1090, 2: 702}, 1792, 677), (652, {1: 463, 2: 305}, 768, 288)],
    "llr-s16-b32": [(291, {1: 123, 2: 133}, 256, 115), (2112, {1: 815, 2: 977}, 1792, 880), (886, {1: 367, 2: 401}, 768, 361)],
    "p34-s8-b16": [(632, {1: 12, 2: 242, 3: 2}, 256, 131), (4396, {1: 80, 2: 1712}, 1792, 982), (1877, {1: 33, 2: 735}, 768, 429)],
    "p56-s8-b16": [(722, {2: 244, 3: 12}, 256, 82), (5026, {1: 4, 2: 1788}, 1792, 541), (2156, {1: 6, 2: 762}, 768, 238)],
    "p78-s8-b16": [(790, {2: 223, 3: 33}, 256, 67), (5154, {1: 3, 2: 1789}, 1792, 356), (2212, {1: 1, 2: 767}, 768, 147)],
    "p78-s16-b32": [(790, {2: 223, 3: 33}, 256, 67), (5154, {1: 3, 2: 1789}, 1792, 356), (2212, {1: 1, 2: 767}, 768, 147)],
    "p23-f-b32-o16": [(486, {1: 51, 2: 204, 3: 1}, 256, 151), (3421, {1: 326, 2: 1466}, 1792, 1108), (1546, {1: 115, 2: 653}, 768, 493)],
}
ZERO = [(0, {1: 256}, 256, 0), (0, {1: 1792}, 1792, 0), (0, {1: 768}, 768, 0)]


@pytest.mark.parametrize("case", list(gc.CASES))
def test_pinned_predictions(vo, case):
    opt, nbits, _, _, _, redecodes = gc.CASES[case]
    assert redecodes == (case in EXPECTED)
    _, packed = gc.case_input(case)
    for mode, want in zip(gc.MODES, EXPECTED.get(case, ZERO)):
        pred = sg.predict(vo, opt, packed, 2 * nbits, sg.seg_table(NSIMD, sg.MODES[mode]))
        assert (pred.total, pred.hist, pred.spec_wgs, pred.chained) == want, mode
        assert pred.total == len(pred.mismatch0) + pred.chained or max(pred.hist) > 2, mode
        gc.check_not_vacuous(case, mode, pred)
        if mode != "pieces":
            # segments of 3/4 chunk: every left end vector comes from a run that starts at a chunk start, so a
            # re-decode never changes one and no workgroup needs a second re-decode pass
            assert max(pred.hist) <= 2, mode
