"""Cost of the punctured decode path: kernel time of one 32M-bit SOFT8/M_B16 batch through run_device_punct at
rate 3/4 and at the unpunctured pattern (1, 1, 1), next to run_device_llr of the same mother-size batch on
the same kernel family (vd_decode_tg, VD_NO_PK=1).  Median of 20 launches after 5 warm-up launches, each
timed with its own event pair; the input is the reference harness's channel source at snr 5 (a codeword:
noise-only input would time the segment launch's re-decodes instead).

    python tools/punct_cost.py                        # this tree's library: punctured launches and the LLR launch
    VITDEC_LIB=<path>/libvitdec.so python tools/punct_cost.py --llr-only     # another build's LLR launch

Prints one JSON line.  DESIGN.md "Punctured streams" records the figures."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gpu-accelerated-viterbi-decoder_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bits", type=int, default=32_000_000)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--llr-only", action="store_true")
    a = ap.parse_args()
    os.environ["VD_NO_PK"] = "1"  # the LLR launch on vd_decode_tg, the family the punctured kernels belong to
    import torch
    import vitdec as vd

    n = 2 * a.bits
    opt = vd.SOFT8 | vd.M_B16
    stream = torch.cuda.current_stream().cuda_stream
    bits = torch.zeros(a.bits, dtype=torch.uint8, device="cuda")
    vals = torch.zeros(n, dtype=torch.float32, device="cuda")
    vd.channel_device(a.bits, 5.0, 1, 2, bits.data_ptr(), vals.data_ptr(), stream)
    out = torch.zeros(vd.lib().vd_output_size(opt, n) // 4, dtype=torch.int32, device="cuda")

    def timed(launch):
        for _ in range(5):
            launch()
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.launches):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            launch()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}

    res = {"bits": a.bits, "option": "SOFT8/M_B16", "launches": a.launches, "lib": vd.LIB_PATH}
    with vd.ViterbiCUDA(opt) as d:
        res["llr_kernel"] = d.kernel_for(n, 1, 1)
        res["llr"] = timed(lambda: d.run_device_llr(vals.data_ptr(), out.data_ptr(), n, stream=stream))
        ref = out.clone()
        if not a.llr_only:
            res["punct_kernel"] = d.kernel_for(n, 1, 2)
            for label, pattern in (("punct_1/2", vd.PUNCTURE["1/2"]), ("punct_3/4", vd.PUNCTURE["3/4"])):
                period, k0, k1 = pattern
                r = torch.arange(a.bits, device="cuda") % period
                kept = torch.stack([(k0 >> r) & 1, (k1 >> r) & 1], dim=1).reshape(-1).bool()
                rx = vals[kept].contiguous()
                assert rx.numel() == vd.punctured_len(pattern, n)
                del r, kept
                res[label] = timed(lambda: d.run_device_punct(rx.data_ptr(), out.data_ptr(), n, pattern, stream=stream))
                res[label]["rx_floats"] = rx.numel()
                if label == "punct_1/2":  # the same stream: the same words
                    res[label]["equals_llr"] = bool(torch.equal(out, ref))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
