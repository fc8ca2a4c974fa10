"""Tail-biting frames on the CPU: the wrapped load geometry, argument checks and plan (csrc/vd_frames.h, vd_plan.h;
checked by tests/cxx/tb_frames_check.cpp against an enumeration of the extended stream, built stand-alone with the
host sanitizers), and the definition itself: vitdec.wrap_frame through the unchanged oracle (one chunk) decodes
every bit of a tail-biting frame with no error, and the bits past the frame decode the wrap.  The decodes on the
GPU: tests/test_gpu_tb_frames.py."""
import os
import subprocess

import numpy as np
import pytest

from frames_common import OPTIONS6, decoded_bits, encode
from tb_common import TB_SIZES_CPU, oracle_tb_frame, tb_encode, tb_frames, wrapped_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"


def name(o):
    return f"0x{o:03x}"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_wrapped_offsets_arguments_and_plan_against_enumeration(tmp_path):
    exe = tmp_path / "tb_frames_check"
    src = os.path.join(ROOT, "tests", "cxx", "tb_frames_check.cpp")
    csrc = os.path.join(ROOT, "gpu-accelerated-viterbi-decoder_amd", "csrc")
    r = subprocess.run([HIPCC, "-x", "hip", "--offload-arch=gfx950", "-O1", "-std=c++17", "-w", "-Xarch_host",
                        "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all", "-I", csrc, src,
                        "-o", str(exe)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.stdout[-2000:], r.stderr[-2000:])


def test_wrap_frame_layout(vd):
    for S in (1, 2, 5, 25, 26, 27, 33, 97, 250):
        v = np.arange(1, 2 * S + 1, dtype=np.float32)
        e = vd.wrap_frame(v)
        P = 64 + 32 * ((S + 31) // 32)
        assert e.dtype == np.float32 and e.size == 2 * P
        for p in range(P):  # stage p = frame stage (p - 26) mod S, by stepping from stage 26 = frame stage 0
            t = (p - 26) % S
            assert 0 <= t < S and e[2 * p] == 2 * t + 1 and e[2 * p + 1] == 2 * t + 2, (S, p)
        assert np.array_equal(e[52:52 + 2 * min(S, P - 26)], v[:2 * min(S, P - 26)])
    one = vd.wrap_frame(np.array([3.0, -4.0], dtype=np.float32))  # S = 1: every stage is the frame's one stage
    assert one.size == 2 * 96 and (one[0::2] == 3.0).all() and (one[1::2] == -4.0).all()
    short = vd.wrap_frame(np.arange(10, dtype=np.float32))  # S = 5 < 26: the lead takes several turns backwards
    assert np.array_equal(short[:2], [8.0, 9.0]) and np.array_equal(short[50:54], [8.0, 9.0, 0.0, 1.0])
    for bad in (np.zeros(0, np.float32), np.zeros(3, np.float32)):
        with pytest.raises(vd.VitdecError, match="wrap_frame"):
            vd.wrap_frame(bad)


def test_tail_biting_encoder_is_the_frame_encoder_after_six_zeros():
    rng = np.random.default_rng(3)
    for S in (7, 33, 250):
        bits = rng.integers(0, 2, S, dtype=np.uint8)
        bits[max(S - 6, 0):] = 0  # the register at the first stage holds six zeros: the encoder started in state 0
        assert np.array_equal(tb_encode(bits)[0], encode(bits))
    # and it is cyclic: rotating the bits rotates the stages
    bits = rng.integers(0, 2, 40, dtype=np.uint8)
    assert np.array_equal(tb_encode(np.roll(bits, 9))[0], np.roll(tb_encode(bits)[0], 18))
    # shorter than the register: the bits wrap several times
    assert np.array_equal(tb_encode(np.array([1], np.uint8))[0], [1.0, 1.0])  # five taps, five taps: parity 1, 1


@pytest.mark.parametrize("opt", OPTIONS6, ids=name)
@pytest.mark.parametrize("S", TB_SIZES_CPU)
def test_wrapped_frames_decode_every_bit_through_the_oracle(vd, vo, S, opt):
    """8 noisy tail-biting frames (sigma 0.3, seed S) per length: 0 errors in bits [0, S) of each, and the bits of
    the last word past S equal the wrapped bits (frame bit i mod S)"""
    bits, vals = tb_frames(8, S, seed=S, sigma=0.3)
    for b, v in zip(bits, vals):
        ref = oracle_tb_frame(vd, opt, v)
        nb = 32 * ((S + 31) // 32)
        got = decoded_bits(opt, ref, nb)
        assert np.array_equal(got[:S], b), (S, np.flatnonzero(got[:S] != b))
        assert np.array_equal(got, wrapped_bits(b, nb)), (S, np.flatnonzero(got != wrapped_bits(b, nb)))


def test_binding_declares_the_tail_biting_entry_points(vd):
    for n in ("vd_run_device_tb_frames", "vd_run_tb_frames"):
        assert n in vd.EXPORTS and getattr(vd.lib(), n).argtypes
    for meth in ("run_tb_frames", "run_device_tb_frames"):
        assert callable(getattr(vd.ViterbiCUDA, meth))
    assert callable(vd.wrap_frame)
