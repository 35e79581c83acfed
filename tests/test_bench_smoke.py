"""-m gpu: bench.py end to end on a tiny configuration -- the JSON contract the driver parses, both sharding modes, the
in-library RCCL leg, and a two-rank rehearsal (gloo: both ranks share the one GPU of the box)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--tris", "20000", "--width", "320", "--height", "184", "--spp", "2", "--depth", "8", "--steps", "2", "--warmup", "1",
         "--cpu-seconds", "0.5", "--tex-size", "32"]


def _run(cmd, **kw):
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=900, **kw)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.strip()]
    assert len(lines) == 1 and lines[0].startswith("{"), f"stdout must be exactly ONE JSON line, got {len(lines)}: {[l[:60] for l in lines]}"
    return json.loads(lines[0])


@pytest.mark.gpu
def test_bench_json_contract(built):
    r = _run([sys.executable, os.path.join(ROOT, "bench.py"), "--full"] + SMALL)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype",
              "data", "config", "roofline", "cpu_baseline"):
        assert k in r, k
    assert r["unit"] == "Mray/s" and r["n_gpus"] == 1 and r["steps"] == 2 and r["vs_baseline"] is None and r["dtype"] == "f32"
    assert r["data"] == "synthetic" and "workload" in r["config"] and "model" not in r["config"] and r["config"]["mode"] == "tiles"
    rf = r["roofline"]
    assert rf["bound"] == "hbm" and rf["unit"] == "GB/s" and rf["peak"] == 8000.0 and abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-3
    assert rf["traffic"] is None and rf["traffic_note"].startswith("null")   # PMC traffic is only quoted for the configuration AND source it was measured on
    assert "ALGORITHMIC" in rf["basis"] and rf["device_bytes_per_launch"] > 0 and len(rf["kernel_source_sha"]) == 16
    cb = r["cpu_baseline"]
    assert cb["kind"] == "port" and cb["cores"] >= 1 and cb["value"] > 0 and "sample" in cb
    assert cb["per_thread_mray_s"] > 0 and cb["slowest_block_over_mean_block"] >= 1.0
    assert "scene.rs:44-85" in cb["memory_placement"] and cb["numa_spread_run"]["value"] > 0
    assert rf["unique_line_bytes"] > 0 and rf["unique_lines"]["triangle_attributes"] > 0 and "memside_frac_measured" in rf
    assert r["parity"]["culled_equals_reference_traversal"] is True and r["parity"]["oracle_bit_exact_on_sample"] is True
    assert "glibc" in r["parity"]["against"]
    assert r["render_multi"]["equals_bench_frame"] is True and r["render_multi"]["n_devices"] == 1 and r["render_multi"]["collective_ms"] > 0
    assert r["value"] > 0 and r["ms_per_step"] > 0
    ss = r["scene_setup"]
    assert ss["entry"] == "mipt_scene_create_from_triangles" and ss["device_bvh_build_ms"] > 0 and ss["device_layout_ms"] > 0 and ss["total_ms"] <= ss["call_s"] * 1e3 + 1
    assert "RGBA8 epilogue" in r["config"]["workload"]


@pytest.mark.gpu
def test_bench_samples_mode(built):
    r = _run([sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--mode", "samples"] + SMALL)
    assert r["config"]["mode"] == "samples" and "per-sample seeds" in r["config"]["workload"]
    assert r["parity"]["oracle_bit_exact_on_sample"] is True and r["render_multi"]["equals_bench_frame"] is True


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["tiles", "samples"])
def test_bench_two_ranks_rehearsal(built, mode):
    """The N > 1 code path with world_size 2 (collectives over gloo, both ranks on the one GPU): gathered / reduced frame vs
    the single-GPU frame, and the other mode's rate in the same line."""
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    r = _run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
              "--master-port", "29611" if mode == "tiles" else "29612", os.path.join(ROOT, "bench.py"), "--gpus", "2", "--dist-backend", "gloo",
              "--full", "--mode", mode] + SMALL, env=env)
    assert r["n_gpus"] == 2 and r["config"]["mode"] == mode and r["other_mode"]["mode"] != mode and r["other_mode"]["value"] > 0
    if mode == "tiles":
        assert r["parity"]["gathered_frame_equals_single_gpu_frame"] is True
    else:
        assert r["parity"]["reduced_frame_max_rel_diff_vs_single_gpu"] < 1e-5


MID = ["--tris", "300000", "--width", "960", "--height", "540", "--spp", "4", "--depth", "16", "--steps", "6", "--warmup", "2",
       "--no-cpu-baseline", "--tex-size", "64"]


@pytest.mark.gpu
def test_bench_single_process_entry(built):
    """`bench.py --gpus 1 --single-process`: the one-process launch model (mipt_multi_create + one mipt_render_multi_device call per
    frame -- what `python bench.py --gpus 8` uses when started without torch.distributed.run) with a one-rank communicator.
    Same frame as the plain N = 1 line; the rate within 25 % of it at this size (a 5 ms frame on a shared box: the host thread hand-off,
    gather and de-interleave are ~0.3 ms and two separate processes see different clocks; at the bench size of 75 ms the two lines
    agree to 0.01 %: profiles/r3_bench_default_run.json vs r3_bench_single_process.json, 2 640.8 vs 2 640.6 Mray/s)."""
    plain = _run([sys.executable, os.path.join(ROOT, "bench.py"), "--full"] + MID)
    one = _run([sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--gpus", "1", "--single-process"] + MID)
    assert one["n_gpus"] == 1 and one["config"]["launch"] == "single-process" and plain["config"]["launch"] == "single-gpu"
    assert one["config"]["frame_crc32"] == plain["config"]["frame_crc32"]
    assert one["config"]["rays_per_frame"] == plain["config"]["rays_per_frame"]
    assert one["parity"]["gathered_frame_equals_single_gpu_frame"] is True
    sp = one["single_process"]
    assert len(sp["device_kernel_ms"]) == 1 and sp["collective_ms"] > 0 and sp["call_wall_ms"] >= sp["device_kernel_ms"][0]
    assert "ncclGather" in one["config"]["sharding"]
    assert abs(one["value"] / plain["value"] - 1.0) < 0.25, (one["value"], plain["value"])
    for k in ("achieved", "frac", "kernel_ms", "algorithmic_bytes_per_launch"):
        assert one["roofline"][k] > 0


@pytest.mark.gpu
def test_bench_more_gpus_than_visible_fails_with_a_message(built, rrt):
    n = rrt.load().mipt_device_count()
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(n + 1)] + SMALL, capture_output=True, text=True, timeout=600)
    assert out.returncode != 0 and out.stdout.strip() == ""
    assert f"--gpus {n + 1} but only {n} HIP device(s) visible" in out.stderr and "Traceback" not in out.stderr


def test_bench_rejects_a_world_size_that_is_not_gpus():
    """CPU: WORLD_SIZE / --gpus mismatch is an error before anything touches a GPU (it was silently accepted)."""
    env = dict(os.environ, RANK="0", WORLD_SIZE="2", LOCAL_RANK="0")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "4"], capture_output=True, text=True, timeout=600, env=env)
    assert out.returncode != 0 and "WORLD_SIZE=2" in out.stderr and "Traceback" not in out.stderr and out.stdout.strip() == ""


@pytest.mark.gpu
def test_bench_plain_run_and_dump_outputs(built, tmp_path):
    """A plain run times exactly --steps steps and carries no --full leg; --dump-outputs writes the last timed frame (its bytes are
    the frame_crc32 of the line) and the same arguments give the same outputs, whatever --steps is."""
    import zlib

    import numpy as np
    i, j = SMALL.index("--steps"), SMALL.index("--warmup")
    assert (j, SMALL[i + 1], SMALL[j + 1]) == (i + 2, "2", "1")
    small = SMALL[:i] + SMALL[j + 2:]
    runs = []
    for steps in (2, 3):
        out = tmp_path / f"s{steps}"
        r = _run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1",
                  "--dump-outputs", str(out)] + small)
        assert r["steps"] == steps and r["warmup"] == 1 and r["ms_per_step"] > 0 and r["value"] > 0
        assert r["unit"] == "Mray/s" and r["higher_is_better"] is True and r["dtype"] == "f32"
        for k in ("parity", "cpu_baseline", "render_multi", "reference_traversal", "other_mode"):
            assert k not in r, k
        hdr, rgba = np.load(out / "hdr.npy"), np.load(out / "rgba8.npy")
        assert sorted(os.listdir(out)) == ["hdr.npy", "rgba8.npy"]
        assert hdr.dtype == np.float32 and hdr.shape == (184, 320, 3) and rgba.dtype == np.float32 and rgba.shape == (184, 320, 4)
        assert f"{zlib.crc32(hdr.tobytes()) & 0xFFFFFFFF:08x}" == r["config"]["frame_crc32"]
        assert np.array_equal(rgba, np.round(rgba)) and rgba.min() >= 0 and rgba.max() <= 255 and np.all(rgba[..., 3] == 255)
        runs.append((hdr, rgba))
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])


def test_bench_dump_outputs_caps_the_size(built, tmp_path, monkeypatch):
    """CPU: above the cap, --dump-outputs writes the same seeded pixel sample of both arrays plus its indices, all float32 /
    float64, below the cap together; below it, the whole frame."""
    import numpy as np

    import bench
    rng = np.random.default_rng(1)
    hdr = rng.random((48, 64, 3), dtype=np.float32)
    rgba = rng.integers(0, 256, (48, 64, 4), dtype=np.uint8)
    bench.dump_outputs(str(tmp_path / "whole"), hdr, rgba)
    assert sorted(os.listdir(tmp_path / "whole")) == ["hdr.npy", "rgba8.npy"]
    assert np.array_equal(np.load(tmp_path / "whole" / "hdr.npy"), hdr)
    assert np.array_equal(np.load(tmp_path / "whole" / "rgba8.npy"), rgba.astype(np.float32))
    monkeypatch.setattr(bench, "DUMP_BYTES", 60_000)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), hdr, rgba)
        files = sorted(os.listdir(tmp_path / d))
        assert files == ["hdr.npy", "pixel_index.npy", "rgba8.npy"]
        assert sum(os.path.getsize(tmp_path / d / f) for f in files) <= 60_000
    got = {f: np.load(tmp_path / "a" / f) for f in files}
    assert all(np.array_equal(got[f], np.load(tmp_path / "b" / f)) for f in files)
    idx = got["pixel_index.npy"]
    assert idx.dtype == np.float64 and got["hdr.npy"].dtype == np.float32 and got["rgba8.npy"].dtype == np.float32
    assert len(idx) > 1000 and np.all(np.diff(idx) > 0) and idx[-1] < 48 * 64
    ii = idx.astype(np.int64)
    assert np.array_equal(got["hdr.npy"], hdr.reshape(-1, 3)[ii]) and np.array_equal(got["rgba8.npy"], rgba.reshape(-1, 4)[ii].astype(np.float32))


def test_bench_rejects_a_step_count_below_one():
    """CPU: --steps sets the number of timed steps, so 0 is an error before anything touches a GPU."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True, timeout=600)
    assert out.returncode != 0 and "--steps must be >= 1" in out.stderr and "Traceback" not in out.stderr and out.stdout.strip() == ""
