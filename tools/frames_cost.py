"""Cost of the frame decode path: kernel time of 4096 terminated frames of 8192 stages through run_device_frames
(vd_decode_tg<FRM+...>, one frame per wave), next to run_device_llr_batch over the same number of stages on the
same kernel family (VD_NO_PK=1: vd_decode_tg<LLR+...>, one chunk per wave): 5 batches of 6,710,912 stages, so a
wave's chunk is about a frame long.  SOFT8/M_B16 and SOFT16/M_B32.  Median of 20 launches after 5 warm-up launches,
each timed with its own event pair; the input is the reference harness's channel source at snr 5 (codewords for
both paths; the frames ignore that the encoder did not restart, only the time is read).

    python tools/frames_cost.py                        # this tree's library: the frame launch and the LLR batch launch
    VITDEC_LIB=<path>/libvitdec.so python tools/frames_cost.py --llr-only     # another build's LLR batch launch

Prints one JSON line.  DESIGN.md "Frames" records the figures."""
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
    ap.add_argument("--batches", type=int, default=5)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--llr-only", action="store_true")
    a = ap.parse_args()
    os.environ["VD_NO_PK"] = "1"  # the LLR batches on vd_decode_tg, the family the frame kernels belong to
    import torch
    import vitdec as vd

    total = a.frames * a.stages                      # stages either path decodes
    # stages per batch, 6,710,912: a few more than a fifth of the total, so the batches' windows overlap a little
    # (inputs are only read); stride in floats, a multiple of 16 bytes
    per_batch = -(-total // (a.batches * 128)) * 128
    stride = (2 * total - 2 * per_batch) // (a.batches - 1) // 4 * 4 if a.batches > 1 else 0
    stream = torch.cuda.current_stream().cuda_stream
    bits = torch.zeros(total, dtype=torch.uint8, device="cuda")
    vals = torch.zeros(2 * total, dtype=torch.float32, device="cuda")
    vd.channel_device(total, 5.0, 1, 2, bits.data_ptr(), vals.data_ptr(), stream)
    del bits

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

    res = {"frames": a.frames, "stages": a.stages, "batches": a.batches, "stages_per_batch": per_batch,
           "launches": a.launches, "lib": vd.LIB_PATH}
    for label, opt in (("SOFT8/M_B16", vd.SOFT8 | vd.M_B16), ("SOFT16/M_B32", vd.SOFT16 | vd.M_B32)):
        r = {}
        with vd.ViterbiCUDA(opt) as d:
            n = 2 * per_batch
            ob = vd.lib().vd_output_size(opt, n)
            out = torch.zeros(a.batches * ob // 4 + 4, dtype=torch.int32, device="cuda")
            r["llr_kernel"] = d.kernel_for(n, a.batches, 1)
            r["llr_batch"] = timed(lambda: d.run_device_llr_batch(vals.data_ptr(), 4 * stride, out.data_ptr(), ob, n, a.batches,
                                                                  stream=stream))
            r["llr_batch"]["ns_per_kstage"] = round(r["llr_batch"]["median_ms"] * 1e6 / (a.batches * per_batch / 1000), 4)
            if not a.llr_only:
                row = vd.frame_output_size(opt, a.stages)
                fout = torch.zeros(a.frames * row // 4, dtype=torch.int32, device="cuda")
                r["frames_kernel"] = d.kernel_for(a.stages, a.frames, 3)
                r["frames"] = timed(lambda: d.run_device_frames(vals.data_ptr(), 8 * a.stages, fout.data_ptr(), row, a.stages,
                                                                a.frames, True, stream=stream))
                r["frames"]["ns_per_kstage"] = round(r["frames"]["median_ms"] * 1e6 / (total / 1000), 4)
        res[label] = r
    print(json.dumps(res))


if __name__ == "__main__":
    main()
