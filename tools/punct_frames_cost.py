"""Cost of the punctured frame decode path: kernel time of 8192 terminated frames of 4096 stages (every SIMD full)
through run_device_punct_frames (vd_decode_tg<FRM+PUN+...>, one frame per wave) at (1, 1, 1) and at rate 3/4, next
to what a caller without it runs: run_device_frames (vd_decode_tg<FRM+...>) over the same frames depunctured to 2 S
floats -- the caller's expansion pass not counted.  SOFT8/M_B16 and SOFT16/M_B32.  Median of 20 launches after 5
warm-up launches, each timed with its own event pair, the two launches of a case taking turns; the input is the
reference harness's channel source at snr 5 (the frames ignore that the encoder did not restart, only the time is
read).

    python tools/punct_frames_cost.py                       # this tree's library: both launches
    VITDEC_LIB=<path>/libvitdec.so python tools/punct_frames_cost.py --frames-only   # another build's frame launch

Prints one JSON line.  DESIGN.md "Punctured frames" records the figures."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gpu-accelerated-viterbi-decoder_amd"))

PATTERNS = {"1/2": (1, 1, 1), "3/4": (3, 0b101, 0b011)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=8192)
    ap.add_argument("--stages", type=int, default=4096)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--frames-only", action="store_true")
    a = ap.parse_args()
    import numpy as np
    import torch
    import vitdec as vd

    total = a.frames * a.stages
    stream = torch.cuda.current_stream().cuda_stream
    bits = torch.zeros(total, dtype=torch.uint8, device="cuda")
    vals = torch.zeros(2 * total, dtype=torch.float32, device="cuda")
    vd.channel_device(total, 5.0, 1, 2, bits.data_ptr(), vals.data_ptr(), stream)
    del bits
    vals = vals.view(a.frames, 2 * a.stages)

    def timed(launches):
        """the launches taking turns, so that a drift of the clocks meets all of them alike"""
        for launch in launches:
            for _ in range(5):
                launch()
        torch.cuda.synchronize()
        ms = [[] for _ in launches]
        for _ in range(a.launches):
            for k, launch in enumerate(launches):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                launch()
                e1.record()
                e1.synchronize()
                ms[k].append(e0.elapsed_time(e1))
        return [{"median_ms": round(statistics.median(m), 4), "min_ms": round(min(m), 4), "max_ms": round(max(m), 4),
                 "ns_per_kstage": round(statistics.median(m) * 1e6 / (total / 1000), 4)} for m in ms]

    res = {"frames": a.frames, "stages": a.stages, "launches": a.launches, "lib": vd.LIB_PATH}
    for rate, pattern in PATTERNS.items():
        # the received rows (the kept values of every frame, the phase at 0) and the depunctured rows
        kept = torch.from_numpy(np.ascontiguousarray(vd._kept(pattern, 2 * a.stages))).cuda()
        rx = vals[:, kept].contiguous()
        dep = torch.zeros_like(vals)
        dep[:, kept] = rx
        L = rx.shape[1]
        for label, opt in (("SOFT8/M_B16", vd.SOFT8 | vd.M_B16), ("SOFT16/M_B32", vd.SOFT16 | vd.M_B32)):
            r = {"received_floats_per_frame": L}
            with vd.ViterbiCUDA(opt) as d:
                row = vd.frame_output_size(opt, a.stages)
                fout = torch.zeros(a.frames * row // 4, dtype=torch.int32, device="cuda")
                pout = torch.zeros_like(fout)
                r["frames_kernel"] = d.kernel_for(a.stages, a.frames, 3)
                launches = [lambda: d.run_device_frames(dep.data_ptr(), 8 * a.stages, fout.data_ptr(), row, a.stages, a.frames,
                                                        True, stream=stream)]
                if not a.frames_only:
                    r["punct_frames_kernel"] = d.kernel_for(a.stages, a.frames, 4)
                    launches.append(lambda: d.run_device_punct_frames(rx.data_ptr(), 4 * L, pout.data_ptr(), row, a.stages,
                                                                      a.frames, pattern, True, stream=stream))
                t = timed(launches)
                r["frames_of_depunctured"] = t[0]
                if not a.frames_only:
                    r["punct_frames"] = t[1]
                    r["same_words"] = bool(torch.equal(pout, fout))
                    r["ratio"] = round(t[1]["median_ms"] / t[0]["median_ms"], 4)
            res[f"{label} {rate}"] = r
        del rx, dep
    print(json.dumps(res))


if __name__ == "__main__":
    main()
