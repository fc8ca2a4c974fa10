"""The workgroup-wide traceback of vd_decode_pk's batched launches (vd_kernel_pk.h "Batched", vd_pk_wg.h): the
four waves of a workgroup decode in lockstep over the workgroup's longest chunk and one wave, taken in turn,
traces the words of all four rings between two workgroup barriers.  Batched launches of 2 and 3 batches must
equal the oracle and vd_decode_tg (VD_NO_PK=1) word for word, with the LDS guard check on (0 violations) and
the bytes around and between the outputs untouched, at the smallest shapes where the assignment of words to
lanes and the shared block count can go wrong (nbits = 64 + 32 pack, 6400 chunks):
  pack 5            one workgroup with work (five 1-word chunks, three empty), 799 empty ones;
  pack 4685         workgroups that mix 1-word chunks, a wave with an empty half and empty waves;
  pack 6400*5 + 3   chunks of 6 and 5 words in one workgroup (TBS = 5: a last pass on, before and after a
  pack 6400*6+4681  regular one), of 7 and 6 (TBS = 6), the boundary inside a workgroup: its waves differ in
                    length; all values of the workgroup index & 3 stagger;
  pack 6400*12 + 1  13- and 12-word chunks: more than two regular passes, every wave traces in its turn.
With O_B16 the same nbits give twice the words, 16 bits each, and chunks with an odd 16-bit tail word.
Inputs: simulate_device at 0.5 dB and one uniformly random buffer per format.  tests/test_pk_wg_blocks.py
checks the schedule behind these shapes on the CPU."""
import os

import numpy as np
import pytest
import torch

from vitdec import FP32, HARD, M_B16, M_B32, M_FP16, O_B16, SOFT4, SOFT8
from test_gpu_parity import name

OPTS = [HARD | M_B32, SOFT8 | M_B16, SOFT8 | M_B32, SOFT4 | M_B16, FP32 | M_FP16, HARD | M_B32 | O_B16, SOFT8 | M_B16 | O_B16]
PACKS = [5, 4685, 6400 * 5 + 3, 6400 * 6 + 4681, 6400 * 12 + 1]
NB = 3
GUARD, PAT = 4096, 0x5C


def _inputs(gpu, opt, nbits, kind):
    """NB batches of input on the device, 256-byte strides: (buffer, stride, bytes per batch)"""
    n = 2 * nbits
    nin = gpu.lib().vd_input_size(opt, n)
    stride = (nin + 255) // 256 * 256
    if kind == "sim":
        packed = torch.zeros(NB * stride, dtype=torch.uint8, device="cuda")
        bits = torch.empty(nbits, dtype=torch.uint8, device="cuda")
        for b in range(NB):
            gpu.simulate_device(opt, nbits, 0.5, 171 + 2 * b, 172 + 2 * b, bits.data_ptr(), packed.data_ptr() + b * stride)
        torch.cuda.synchronize()
        return packed, stride, nin
    g = torch.Generator(device="cpu").manual_seed(29)
    if (opt & 0xF) == FP32:  # finite floats
        host = ((torch.rand(NB * stride // 4, generator=g) - 0.5) * 16.0).view(torch.uint8)
    else:
        host = torch.randint(0, 256, (NB * stride,), dtype=torch.uint8, generator=g)
    return host.to("cuda"), stride, nin


def _decode(gpu, opt, packed, stride, n, nb, no_pk):
    """one batched launch of nb batches into a guarded buffer with the LDS guard check on: the output bytes"""
    nout = gpu.lib().vd_output_size(opt, n)
    ostride = (nout + 255) // 256 * 256 + 256
    buf = torch.full((GUARD + nb * ostride + GUARD,), PAT, dtype=torch.uint8, device="cuda")
    out = buf[GUARD:GUARD + nb * ostride]
    old = os.environ.get("VD_NO_PK")
    os.environ["VD_NO_PK"] = "1" if no_pk else "0"
    try:
        with gpu.ViterbiCUDA(opt) as dec:
            want = "vd_decode_tg<" if no_pk else "vd_decode_pk<"
            assert dec.kernel_for(n, nb).startswith(want) and (no_pk or " batched" in dec.kernel_for(n, nb))
            dec.set_guard_check(True)
            dec.run_device_batch(packed.data_ptr(), stride, out.data_ptr(), ostride, n, nb,
                                 torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            bad = dec.guard_violations()
    finally:
        if old is None:
            del os.environ["VD_NO_PK"]
        else:
            os.environ["VD_NO_PK"] = old
    assert bad == 0, f"{bad} LDS guard words overwritten"
    assert bool((buf[:GUARD] == PAT).all()) and bool((buf[-GUARD:] == PAT).all()), "bytes around the outputs written"
    for b in range(nb):
        assert bool((out[b * ostride + nout:(b + 1) * ostride] == PAT).all()), f"bytes after batch {b}'s output written"
    return [out[b * ostride:b * ostride + nout].cpu().numpy() for b in range(nb)]


@pytest.mark.gpu
@pytest.mark.parametrize("opt", OPTS, ids=name)
@pytest.mark.parametrize("pack", PACKS)
def test_workgroup_traceback_equals_oracle_and_fp32_kernel(gpu, vo, opt, pack):
    nbits = 64 + 32 * pack
    n = 2 * nbits
    for kind in ("sim", "random"):
        packed, stride, nin = _inputs(gpu, opt, nbits, kind)
        refs = []  # the oracle's words per batch, computed once for both launches
        for b in range(NB):
            p = packed[b * stride:b * stride + nin].cpu().numpy().view(np.int32)
            refs.append(vo.decode(opt, p, input_num=n, nthreads=16)[0])
        for nb in (2, NB):
            pk = _decode(gpu, opt, packed, stride, n, nb, no_pk=False)
            tg = _decode(gpu, opt, packed, stride, n, nb, no_pk=True)
            for b in range(nb):
                got = pk[b].view(refs[b].dtype)
                assert got.size == refs[b].size == pack * (2 if opt & O_B16 else 1)
                bad = np.flatnonzero(got != refs[b])
                assert bad.size == 0, (f"{kind}, {nb} batches, batch {b}: {bad.size} of {got.size} words differ "
                                       f"(pack {pack}, rem {pack % 6400}), first {bad[:5]}")
                assert np.array_equal(pk[b], tg[b]), f"{kind}, {nb} batches, batch {b}: differs from vd_decode_tg"
