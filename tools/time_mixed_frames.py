"""Cost of the mixed frame launch next to the uniform frame launches: kernel time of 4096 terminated frames of 8192
stages, SOFT8/M_B16, float (scale 40000) and int8 (scale 1.0) values.  Three things per value type:
  (a) uniform:  the rate-3/4 launch of the existing entry point (vd_run_device_punct_frames / vd_run_device_byte_frames);
  (b) mixed, every frame at 3/4, on the same buffer (table 1/2, 2/3, 3/4; a rate index and an offset per frame): what
      the per-wave record, rate index and offset cost;
  (c) a third of the frames each at 1/2, 2/3 and 3/4: one mixed launch over the frames laid back to back
      (vitdec.mixed_layout) against three uniform launches of the thirds, back to back on one stream (the rate-1/2 third on
      the unpunctured entry point), timed as one.
Median of 20 launches after 5 warm-up launches, each timed with its own event pair, with its min and max; the whole
series twice (--runs).  The input is the reference harness's channel source at snr 5 (the frames ignore that the
encoder did not restart; the words of the launches compared are checked equal, the time is what is read).
--mixed-first times (b) before (a), to tell the order in a series from the kernels.

    python tools/time_mixed_frames.py

Prints one JSON line.  DESIGN.md 17 records the figures."""
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
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--mixed-first", action="store_true", help="time (b) before (a): the order of the two in a series")
    a = ap.parse_args()
    import numpy as np
    import torch
    import vitdec as vd

    n, S = a.frames, a.stages
    stream = torch.cuda.current_stream().cuda_stream
    bits = torch.zeros(n * S, dtype=torch.uint8, device="cuda")
    vals = torch.zeros(2 * n * S, dtype=torch.float32, device="cuda")
    vd.channel_device(n * S, 5.0, 1, 2, bits.data_ptr(), vals.data_ptr(), stream)
    del bits
    vals = vals.view(n, 2 * S)
    table = [vd.PUNCTURE["1/2"], vd.PUNCTURE["2/3"], vd.PUNCTURE["3/4"]]
    kept = [torch.from_numpy(vd._kept(p, 2 * S)).cuda() for p in table]
    lens = [vd.punctured_len(p, 2 * S) for p in table]

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
    row = vd.frame_output_size(opt, S)
    res = {"frames": n, "stages": S, "launches": a.launches, "option": "SOFT8/M_B16", "lib": vd.LIB_PATH, "mixed_first": a.mixed_first,
           "runs": []}
    third = n // 3
    counts = [third, third, n - 2 * third]
    first = [0, third, 2 * third]
    rates_c = np.repeat(np.arange(3, dtype=np.uint8), counts)
    offs_c, total_c = vd.mixed_layout([S] * n, rates_c, table)
    with vd.ViterbiCUDA(opt) as d:
        d.set_frame_patterns(table)
        for run in range(a.runs):
            out_run = {}
            for i8 in (False, True):
                scale = 1.0 if i8 else 40000.0
                src = torch.clamp(torch.round(32.0 * vals), -128, 127).to(torch.int8) if i8 else vals
                vb = 1 if i8 else 4
                # (a), (b): every frame at 3/4, rows back to back
                rx34 = src[:, kept[2]].contiguous()
                L = lens[2]
                offs_b = torch.arange(n, dtype=torch.int64, device="cuda") * L
                rate_b = torch.full((n,), 2, dtype=torch.uint8, device="cuda")
                out_a = torch.zeros(n * row // 4, dtype=torch.int32, device="cuda")
                out_b = torch.zeros_like(out_a)
                out_c = torch.zeros_like(out_a)
                out_u = torch.zeros_like(out_a)
                # (c): the thirds, each its own buffer for the uniform launches, and all frames back to back for the mixed one
                parts = [src[first[k]:first[k] + counts[k]][:, kept[k]].contiguous() for k in range(3)]
                flat = torch.cat([p.reshape(-1) for p in parts])
                assert flat.numel() == total_c
                offs_d = torch.from_numpy(offs_c.view(np.int64)).cuda()
                rate_d = torch.from_numpy(rates_c).cuda()

                def uniform_launch(buf, stride, out_ptr, frames, pattern):
                    if i8:
                        d.run_device_byte_frames(buf.data_ptr(), stride, out_ptr, row, S, frames, vd.FRAMES_TERMINATED, pattern, scale,
                                                 stream=stream)
                    elif pattern == (1, 1, 1):
                        d.run_device_frames(buf.data_ptr(), stride, out_ptr, row, S, frames, True, scale, stream=stream)
                    else:
                        d.run_device_punct_frames(buf.data_ptr(), stride, out_ptr, row, S, frames, pattern, True, scale, stream=stream)

                def mixed_launch(buf, out, rate, offs):
                    run_mixed = d.run_device_byte_mixed_frames if i8 else d.run_device_mixed_frames
                    run_mixed(buf.data_ptr(), 0, out.data_ptr(), row, S, n, vd.FRAMES_TERMINATED, scale, rate_ptr=rate.data_ptr(),
                              offsets_ptr=offs.data_ptr(), stream=stream)

                def launch_a():
                    uniform_launch(rx34, vb * L, out_a.data_ptr(), n, table[2])

                def launch_b():
                    mixed_launch(rx34, out_b, rate_b, offs_b)

                def launch_c_mixed():
                    mixed_launch(flat, out_c, rate_d, offs_d)

                def launch_c_uniform():
                    for k in range(3):
                        uniform_launch(parts[k], vb * lens[k], out_u.data_ptr() + first[k] * row, counts[k], table[k])

                r = {"uniform_kernel": d.kernel_for(S, n, 8 if i8 else 4), "mixed_kernel": d.kernel_for(S, n, 13 if i8 else 11)}
                if a.mixed_first:
                    r["b_mixed_all_3_4"] = timed(launch_b)
                    r["a_uniform_3_4"] = timed(launch_a)
                else:
                    r["a_uniform_3_4"] = timed(launch_a)
                    r["b_mixed_all_3_4"] = timed(launch_b)
                r["c_mixed_thirds"] = timed(launch_c_mixed)
                r["c_three_uniform"] = timed(launch_c_uniform)
                torch.cuda.synchronize()
                r["words_equal"] = bool(torch.equal(out_a, out_b)) and bool(torch.equal(out_c, out_u))
                r["b_minus_a_ms"] = round(r["b_mixed_all_3_4"]["median_ms"] - r["a_uniform_3_4"]["median_ms"], 4)
                r["b_inside_a_range"] = r["a_uniform_3_4"]["min_ms"] <= r["b_mixed_all_3_4"]["median_ms"] <= r["a_uniform_3_4"]["max_ms"]
                r["c_mixed_over_three"] = round(r["c_mixed_thirds"]["median_ms"] / r["c_three_uniform"]["median_ms"], 4)
                out_run["int8" if i8 else "float"] = r
                del rx34, parts, flat, out_a, out_b, out_c, out_u, src
            res["runs"].append(out_run)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
