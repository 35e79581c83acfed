"""Renderer::denoise_variance of the C++ host mirror (include/mipt_host.hpp) over the C ABI: its argument handling without a device,
and on the GPU its results against the model of tests/tools/variance_model.py, exchanged through files."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import variance_model as VM  # noqa: E402


def _build(tmp_path):
    exe = str(tmp_path / "test_host_variance")
    lib_dir = os.path.join(ROOT, "rust_ray_tracing_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_host_variance.cpp"),
                           "-o", exe, "-L", lib_dir, "-l:libmipt.so", f"-Wl,-rpath,{lib_dir}", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_cpp_denoise_variance_checks_arguments_without_a_device(built, tmp_path):
    out = subprocess.run([_build(tmp_path), "cpu"], capture_output=True, text=True)
    assert out.returncode == 0 and "cpu ok" in out.stdout, out.stdout + out.stderr


@pytest.mark.gpu
def test_cpp_denoise_variance_matches_the_model(rrt, orc, tmp_path):
    w, h, v = 65, 9, 2
    rng = np.random.default_rng(78)
    hdr = (rng.random((v, h, w, 3)) ** 2 * 4.0).astype(np.float32)
    normal = rng.normal(0, 0.6, (v, h, w, 3)).astype(np.float32)
    depth = (2.0 + rng.random((v, h, w)) * 0.4).astype(np.float32)
    depth[rng.random((v, h, w)) < 0.2] = np.float32(1e30)
    albedo = rng.random((v, h, w, 3)).astype(np.float32)
    albedo[0, 3, 3] = 0.0
    variance = (rng.random((v, h, w)) ** 3).astype(np.float32)
    length = rng.integers(1, 9, (v, h, w)).astype(np.float32)               # both sides of short_history = 4
    (tmp_path / "in.bin").write_bytes(hdr.tobytes() + normal.tobytes() + depth.tobytes() + albedo.tobytes() + variance.tobytes() + length.tobytes())
    out = subprocess.run([_build(tmp_path), "gpu", str(tmp_path / "in.bin"), str(tmp_path / "out.bin"), str(w), str(h), str(v)], capture_output=True, text=True)
    assert out.returncode == 0 and "gpu ok" in out.stdout, out.stdout + out.stderr
    got = np.frombuffer((tmp_path / "out.bin").read_bytes(), dtype=np.float32)
    n = v * h * w
    frames = [got[: 3 * n], got[4 * n: 7 * n], got[7 * n: 10 * n], got[10 * n: 13 * n]]
    frames = [f.reshape(v, h, w, 3) for f in frames]
    vout = got[3 * n: 4 * n].reshape(v, h, w)
    assert got.size == 13 * n
    full = VM.denoise_variance(orc, hdr, variance, length, normal, depth, albedo)
    assert VM.same_bits(frames[0], full[0]) and VM.same_bits(vout, full[1]) and VM.same_bits(frames[3], full[0])
    assert VM.same_bits(frames[1], VM.denoise_variance(orc, hdr, None, None, normal, depth, albedo)[0])
    assert VM.same_bits(frames[2], VM.denoise_variance(orc, hdr, variance, length, depth=depth, iterations=3, sigma_depth=0.25, sigma_luminance=4.0,
                                                       short_history=0.0)[0])
    assert not VM.same_bits(frames[0], frames[1]) and not VM.same_bits(frames[0], hdr)
