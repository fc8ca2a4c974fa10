"""Cost of the int8 frame launch next to the float frame launch: kernel time of 4096 terminated frames of 8192 stages,
SOFT8/M_B16, scale 1.0, at rate 1/2 (pattern (1, 1, 1): vd_decode_tg<FRM+I8+...> against vd_decode_tg<FRM+...>) and at
rate 3/4 (vd_decode_tg<FRM+I8+PUN+...> against vd_decode_tg<FRM+PUN+...>).  Three timings per rate:
  (a) float:        the float frame launch on the widened buffer (float)q;
  (b) byte:         the byte launch on the int8 buffer q;
  (c) widen+float:  a torch .to(float32) of q followed by (a), what a caller holding int8 values does without (b).
Median of 20 launches after 5 warm-up launches, each timed with its own event pair.  The input is the reference
harness's channel source at snr 5 quantised as clip(rint(32 v), -128, 127) (the frames ignore that the encoder did not
restart; the words of (a) and (b) are compared, the time is what is read).  The launches read 8 (a) and 2 (b) bytes a
stage at rate 1/2.

    python tools/byte_frames_cost.py

Prints one JSON line.  DESIGN.md 16 records the figures."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gpu-accelerated-viterbi-decoder_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=4096)
    ap.add_argument("--stages", type=int, default=8192)
    ap.add_argument("--launches", type=int, default=20)
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
    q_all = torch.clamp(torch.round(32.0 * vals), -128, 127).to(torch.int8).view(a.frames, 2 * a.stages)
    del vals

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

    opt = vd.SOFT8 | vd.M_B16
    res = {"frames": a.frames, "stages": a.stages, "launches": a.launches, "option": "SOFT8/M_B16", "scale": 1.0,
           "lib": vd.LIB_PATH}
    row = vd.frame_output_size(opt, a.stages)
    with vd.ViterbiCUDA(opt) as d:
        for label, pattern in (("1/2", (1, 1, 1)), ("3/4", vd.PUNCTURE["3/4"])):
            plain = pattern == (1, 1, 1)
            if plain:
                q = q_all
            else:  # the kept bytes of every frame, the pattern's phase at 0 at its first stage
                kept = torch.from_numpy(vd._kept(pattern, 2 * a.stages)).cuda()
                q = q_all[:, kept].contiguous()
            L = q.shape[1]
            assert L == vd.punctured_len(pattern, 2 * a.stages)
            wide = q.to(torch.float32)
            out_f = torch.zeros(a.frames * row // 4, dtype=torch.int32, device="cuda")
            out_b = torch.zeros_like(out_f)

            def float_launch(buf=wide):
                if plain:
                    d.run_device_frames(buf.data_ptr(), 4 * L, out_f.data_ptr(), row, a.stages, a.frames, True, 1.0, stream=stream)
                else:
                    d.run_device_punct_frames(buf.data_ptr(), 4 * L, out_f.data_ptr(), row, a.stages, a.frames, pattern, True, 1.0,
                                              stream=stream)

            def byte_launch():
                d.run_device_byte_frames(q.data_ptr(), L, out_b.data_ptr(), row, a.stages, a.frames, vd.FRAMES_TERMINATED, pattern,
                                         1.0, stream=stream)

            def widen_float_launch():
                float_launch(q.to(torch.float32))

            r = {"float_kernel": d.kernel_for(a.stages, a.frames, 3 if plain else 4),
                 "byte_kernel": d.kernel_for(a.stages, a.frames, 7 if plain else 8),
                 "input_bytes_per_frame": {"float": 4 * L, "byte": L}}
            r["float"] = timed(float_launch)
            r["byte"] = timed(byte_launch)
            r["widen+float"] = timed(widen_float_launch)
            torch.cuda.synchronize()
            r["words_equal"] = bool(torch.equal(out_f, out_b))
            for k in ("float", "byte", "widen+float"):
                r[k]["ns_per_kstage"] = round(r[k]["median_ms"] * 1e6 / (total / 1000), 4)
            r["byte_minus_float_ms"] = round(r["byte"]["median_ms"] - r["float"]["median_ms"], 4)
            r["float_spread_ms"] = round(r["float"]["max_ms"] - r["float"]["min_ms"], 4)
            res[label] = r
            del wide, out_f, out_b
    print(json.dumps(res))


if __name__ == "__main__":
    main()
