"""int8 frames on the CPU: the byte geometry of the four frame families, frame_args_error message by message for the int8 families, the
52 kernels of the byte twins' tables and their names (csrc/vd_frames.h "int8 frames", vd_plan.h; checked by
tests/cxx/byte_frames_check.cpp against a plain enumeration, built stand-alone with the host sanitizers), and the
binding's declarations.  The decodes on the GPU: tests/test_gpu_byte_frames.py."""
import os
import subprocess

import pytest

from ptb_common import P16, P23, P34, P78, PNONE, PTB_SIZES_CPU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
PATTERNS = [(1, 1, 1), P23, P34, P78, P16, PNONE]
PART_BITS = [0, 96, 192]


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_byte_offsets_arguments_tables_and_names_against_enumeration(tmp_path):
    exe = tmp_path / "byte_frames_check"
    src = os.path.join(ROOT, "tests", "cxx", "byte_frames_check.cpp")
    csrc = os.path.join(ROOT, "gpu-accelerated-viterbi-decoder_amd", "csrc")
    r = subprocess.run([HIPCC, "-x", "hip", "--offload-arch=gfx950", "-O1", "-std=c++17", "-w", "-Xarch_host",
                        "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all", "-I", csrc, src,
                        "-o", str(exe)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    args = ["sizes=" + ",".join(str(s) for s in PTB_SIZES_CPU), "parts=" + ",".join(str(b) for b in PART_BITS)]
    args += [f"pat={p[0]},{p[1]},{p[2]}" for p in PATTERNS]
    r = subprocess.run([str(exe)] + args, capture_output=True, text=True, timeout=300)
    want = f"ok {len(PTB_SIZES_CPU)} sizes {len(PART_BITS)} parts {len(PATTERNS)} patterns"
    assert r.returncode == 0 and r.stdout.strip() == want, (r.stdout[-2000:], r.stderr[-2000:])


def test_binding_declares_the_byte_frame_entry_points(vd):
    for n in ("vd_run_device_byte_frames", "vd_run_byte_frames"):
        assert n in vd.EXPORTS and len(getattr(vd.lib(), n).argtypes) == 14
    for meth in ("run_byte_frames", "run_device_byte_frames"):
        assert callable(getattr(vd.ViterbiCUDA, meth))
    assert (vd.FRAMES_OPEN, vd.FRAMES_TERMINATED, vd.FRAMES_TAILBITING) == (0, 1, 2)


def test_header_defines_the_kinds_and_names_no_digit():
    """the three kinds as the binding exports them, and entry-point names that tests/test_capi.py's scan can see"""
    import re
    src = open(os.path.join(ROOT, "include", "vd_capi.h")).read()
    for name, value in (("VD_FRAMES_OPEN", 0), ("VD_FRAMES_TERMINATED", 1), ("VD_FRAMES_TAILBITING", 2)):
        assert re.search(rf"#define\s+{name}\s+{value}\b", src), name
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert {"vd_run_device_byte_frames", "vd_run_byte_frames"} <= set(re.findall(r"\b(vd_[a-z_]+)\s*\(", code))
