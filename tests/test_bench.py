"""bench.py's contract (host logic on CPU, the JSON line on the GPU).

CPU: the roofline helpers read the committed round profiles (profiles/<PMC_ROUND>/pmc_summary.json,
ablate_batched.log and valu_model.json) the way the bench line quotes them.  GPU: a short bench run prints one JSON line with the keys
the driver and the judge read (metric, value, roofline with its binding VALU view, config)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_algorithmic_bytes_match_survey():
    # HARD 0.375 B, SOFT8 2.125 B per decoded bit at 32M bits (31,999,936 decoded bits)
    n = 2 * bench.N_BITS
    assert bench.algorithmic_bytes(0x00, n) == 11_999_992
    assert bench.algorithmic_bytes(0x12, n) == 67_999_992


def test_mix_ceiling_from_committed_ablation():
    # the packed kernels (vd_decode_pk) have their ACS-only ablation (tools/vd_pkab): (ACS-only, full) ms on one box
    for name in ("hard_b32", "soft8_b16", "fp32_f16"):
        ab = bench.acs_only_ms(name)
        assert ab is not None and 0.04 < ab[0] < ab[1] < 0.2, (name, ab)
    assert bench.acs_only_ms("soft16_b32") is None


def test_valu_view_from_committed_pmc():
    pmc = bench.load_pmc()
    assert {"hard_b32", "soft8_b16"} <= set(pmc)
    for name in ("hard_b32", "soft8_b16"):
        p = pmc[name]
        # HBM bytes per launch within 1.2x of the algorithmic bytes
        alg = bench.algorithmic_bytes(0x00 if name == "hard_b32" else 0x12, 2 * bench.N_BITS)
        assert alg <= p["traffic_bytes"] <= 1.2 * alg, (name, p["traffic_bytes"], alg)
        v = bench.valu_view(p, 0.11 if name == "hard_b32" else 0.13, 32_409_536, name, 31_999_936)
        for k in ("insts_per_chunk_stage", "issue_pct", "cycles_per_inst_per_simd", "pmc_run_clock_ghz",
                  "issue_pct_live", "cycle_model_pct", "cycle_model_pct_live", "cycle_model", "mix_ceiling"):
            assert k in v, (name, k)
        assert "busy_pct" not in v  # the gfx94x SIMD-16 formula does not read as a percentage on gfx950
        # per chunk-stage on vd_decode_pk (two chunks per wave): ~2.3 VALU instructions for HARD, ~3 for SOFT8
        lo, hi = (2.5, 3.6) if name == "soft8_b16" else (1.8, 2.8)
        assert lo < v["insts_per_chunk_stage"] < hi, v["insts_per_chunk_stage"]
        # the ISA-derived mix agrees with the counted instructions within 10 %
        assert abs(v["cycle_model"]["valu_insts_per_chunk_stage_isa"] / v["insts_per_chunk_stage"] - 1) < 0.1, v
        assert 1.5 < v["pmc_run_clock_ghz"] < 2.6
        # the per-opcode cycle model (ubench-priced ISA mix): the binding resource, above the 2-cycle issue view,
        # and a fraction of the cycles available (a model above 100 % would contradict the timing)
        assert v["issue_pct"] < v["cycle_model_pct"] <= 100.0 and v["cycle_model_pct_live"] <= 100.0, v
        mc = v["mix_ceiling"]
        assert 0.4 < mc["frac"] < 1 and abs(mc["acs_only_ms"] - mc["frac"] * (0.11 if name == "hard_b32" else 0.13)) < 1e-3


@pytest.mark.gpu
def test_bench_prints_one_json_line_with_the_contract_keys():
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1", "--warm-s", "0.05",
           "--full", "--no-cpu-baseline", "--no-llr", "--no-pcie", "--no-channel", "--no-other"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=240, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 3 and d["unit"] == "Gb/s" and d["value"] > 0
    ro = d["roofline"]
    assert ro["bound"] == "valu" and ro["unit"] == "GB/s" and 0 < ro["frac"] < 1
    assert ro["kernel"].startswith("soft8_b16")
    assert {"hard_b32", "soft8_b16"} == set(ro["per_kernel"])
    assert ro["int_op_roofline"]["ops_per_bit"] == 256
    # both batches decoded correctly at the bench SNR (the harness chain is near noiseless there)
    assert all(b < 1e-5 for b in d["config"]["ber"].values())
    # N = 1 runs the same collectives as N > 1 (a 1-rank RCCL group): the final gather reached rank 0 intact
    fg = d["config"]["final_gather"]
    assert fg["world"] == 1 and fg["checksums_match"] is True, fg


def _bench_line(*args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], capture_output=True, text=True,
                       timeout=240, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_times_the_steps_and_nothing_else():
    """Without --full the line holds the headline figure and its roofline, and none of the blocks that take runs
    or host decodes of their own after the timed region."""
    d = _bench_line("--gpus", "1", "--steps", "2", "--warmup", "1", "--warm-s", "0.05")
    assert d["steps"] == 2 and d["value"] > 0 and d["ms_per_step"] > 0 and d["unit"] == "Gb/s"
    assert d["higher_is_better"] is True and d["dtype"].startswith("exact integers")
    assert d["config"]["launch"]["batches_per_launch"] == 2 and d["roofline"]["bound"] == "valu"
    for k in ("cpu_baseline", "checksums"):
        assert k not in d, k
    for k in ("ber", "parity", "final_gather", "other_configs", "single_launch", "llr_input", "pcie_inclusive",
              "channel_source"):
        assert k not in d["config"], k


@pytest.mark.gpu
def test_dump_outputs_writes_the_last_steps_words(tmp_path):
    """--dump-outputs: one float64 array per workload holding the decoded words of the last timed step.  At
    --steps 1 that is batch 0, whose words the parity block checks against the oracle and whose xor is the
    line's checksum."""
    import numpy as np
    d = _bench_line("--steps", "1", "--warmup", "1", "--warm-s", "0.05", "--full", "--no-cpu-baseline", "--no-llr",
                    "--no-pcie", "--no-channel", "--no-other", "--dump-outputs", str(tmp_path / "out"))
    assert d["config"]["parity"]["all_match"] is True, d["config"]["parity"]
    assert sorted(os.listdir(tmp_path / "out")) == ["hard_b32.npy", "soft8_b16.npy"]
    for i, name in enumerate(("hard_b32", "soft8_b16")):
        a = np.load(tmp_path / "out" / (name + ".npy"))
        assert a.dtype == np.float64 and a.shape == (d["config"]["parity"]["paths"][name + "[batch 0]"]["words"],)
        w = a.astype(np.uint32)
        assert np.array_equal(w.astype(np.float64), a)
        assert int(np.bitwise_xor.reduce(w)) == int(d["checksums"][0][i], 16)


@pytest.mark.gpu
def test_bench_under_torchrun_one_rank():
    """`torch.distributed.run --nproc-per-node 1 bench.py --gpus 1`: the launcher's environment, RCCL group
    with device_id, barrier, max over ranks, checksum gather and the gather to rank 0 on cuda tensors."""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=1", "--master-addr",
           "127.0.0.1", "--master-port", str(bench.free_port()), os.path.join(ROOT, "bench.py"), "--gpus", "1",
           "--steps", "4", "--warmup", "1", "--warm-s", "0.05", "--full", "--no-cpu-baseline", "--no-llr", "--no-pcie",
           "--no-channel", "--no-other"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=240, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["n_gpus"] == 1 and d["value"] > 0
    assert d["config"]["final_gather"]["checksums_match"] is True, d["config"]["final_gather"]
