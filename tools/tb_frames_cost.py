"""Cost of the tail-biting frame decode path: kernel time of 8192 frames of 4096 stages (every SIMD full) through
run_device_tb_frames (vd_decode_tg<FRM+TB+...>, one frame per wave), next to the frame launch it is made from:
run_device_frames (vd_decode_tg<FRM+...>, terminated) over the same buffer.  SOFT8/M_B16 and SOFT16/M_B32.  Median of
20 launches after 5 warm-up launches, each timed with its own event pair, the two launches of a case taking turns;
the input is the reference harness's channel source at snr 5 (the frames ignore that the encoder neither restarted
nor bit its tail, only the time is read).

    python tools/tb_frames_cost.py                       # this tree's library: both launches
    VITDEC_LIB=<path>/libvitdec.so python tools/tb_frames_cost.py --frames-only   # another build's frame launch

Prints one JSON line.  DESIGN.md "Tail-biting frames" records the figures."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gpu-accelerated-viterbi-decoder_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=8192)
    ap.add_argument("--stages", type=int, default=4096)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--frames-only", action="store_true")
    a = ap.parse_args()
    import torch
    import vitdec as vd

    total = a.frames * a.stages
    stream = torch.cuda.current_stream().cuda_stream
    bits = torch.zeros(total, dtype=torch.uint8, device="cuda")
    vals = torch.zeros(2 * total, dtype=torch.float32, device="cuda")
    vd.channel_device(total, 5.0, 1, 2, bits.data_ptr(), vals.data_ptr(), stream)
    del bits

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
    for label, opt in (("SOFT8/M_B16", vd.SOFT8 | vd.M_B16), ("SOFT16/M_B32", vd.SOFT16 | vd.M_B32)):
        r = {}
        with vd.ViterbiCUDA(opt) as d:
            row = vd.frame_output_size(opt, a.stages)
            fout = torch.zeros(a.frames * row // 4, dtype=torch.int32, device="cuda")
            tout = torch.zeros_like(fout)
            r["frames_kernel"] = d.kernel_for(a.stages, a.frames, 3)
            launches = [lambda: d.run_device_frames(vals.data_ptr(), 8 * a.stages, fout.data_ptr(), row, a.stages, a.frames,
                                                    True, stream=stream)]
            if not a.frames_only:
                r["tb_frames_kernel"] = d.kernel_for(a.stages, a.frames, 5)
                launches.append(lambda: d.run_device_tb_frames(vals.data_ptr(), 8 * a.stages, tout.data_ptr(), row, a.stages,
                                                               a.frames, stream=stream))
            t = timed(launches)
            r["frames"] = t[0]
            if not a.frames_only:
                r["tb_frames"] = t[1]
                # (a sanity figure, not a check: once the survivors have merged past a frame's start the two launches
                # decide alike until the stages after its end come into the traceback, so the interior words agree)
                fw, tw = fout.view(a.frames, -1), tout.view(a.frames, -1)
                r["same_interior_words"] = bool(torch.equal(fw[:, 4:-4], tw[:, 4:-4]))
                r["ratio"] = round(t[1]["median_ms"] / t[0]["median_ms"], 4)
        res[label] = r
    print(json.dumps(res))


if __name__ == "__main__":
    main()
