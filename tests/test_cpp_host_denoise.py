"""Renderer::denoise of the C++ host mirror (include/mipt_host.hpp) over the C ABI: its argument handling without a device, and on the
GPU its results against the model of tests/tools/denoise_model.py, exchanged through files."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import denoise_model as D  # noqa: E402


def _build(tmp_path):
    exe = str(tmp_path / "test_host_denoise")
    lib_dir = os.path.join(ROOT, "rust_ray_tracing_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_host_denoise.cpp"),
                           "-o", exe, "-L", lib_dir, "-l:libmipt.so", f"-Wl,-rpath,{lib_dir}", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_cpp_denoise_checks_arguments_without_a_device(built, tmp_path):
    out = subprocess.run([_build(tmp_path), "cpu"], capture_output=True, text=True)
    assert out.returncode == 0 and "cpu ok" in out.stdout, out.stdout + out.stderr


@pytest.mark.gpu
def test_cpp_denoise_matches_the_model(rrt, orc, tmp_path):
    w, h, v = 65, 9, 2
    rng = np.random.default_rng(77)
    hdr = (rng.random((v, h, w, 3)) ** 2 * 4.0).astype(np.float32)
    normal = rng.normal(0, 0.6, (v, h, w, 3)).astype(np.float32)
    depth = (2.0 + rng.random((v, h, w)) * 0.4).astype(np.float32)
    depth[rng.random((v, h, w)) < 0.2] = np.float32(1e30)
    albedo = rng.random((v, h, w, 3)).astype(np.float32)
    albedo[0, 3, 3] = 0.0
    (tmp_path / "in.bin").write_bytes(hdr.tobytes() + normal.tobytes() + depth.tobytes() + albedo.tobytes())
    out = subprocess.run([_build(tmp_path), "gpu", str(tmp_path / "in.bin"), str(tmp_path / "out.bin"), str(w), str(h), str(v)], capture_output=True, text=True)
    assert out.returncode == 0 and "gpu ok" in out.stdout, out.stdout + out.stderr
    got = np.frombuffer((tmp_path / "out.bin").read_bytes(), dtype=np.float32).reshape(4, v, h, w, 3)
    full = D.denoise(orc, hdr, normal, depth, albedo)
    assert D.same_bits(got[0], full) and D.same_bits(got[3], full)
    assert D.same_bits(got[1], D.denoise(orc, hdr, depth=depth, iterations=3, sigma_depth=0.25))
    assert D.same_bits(got[2], D.denoise(orc, hdr))
    assert not D.same_bits(got[0], got[2]) and not D.same_bits(got[2], hdr)
