"""Renderer::render_adaptive and Renderer::sample_map of the C++ host mirror (include/mipt_host.hpp) over the C ABI: their argument
handling without a device, and on the GPU sample_map's results against the model of tests/tools/sample_map_model.py, exchanged
through files."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import sample_map_model as SM  # noqa: E402


def _build(tmp_path):
    exe = str(tmp_path / "test_host_adaptive")
    lib_dir = os.path.join(ROOT, "rust_ray_tracing_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_host_adaptive.cpp"),
                           "-o", exe, "-L", lib_dir, "-l:libmipt.so", f"-Wl,-rpath,{lib_dir}", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_cpp_adaptive_checks_arguments_without_a_device(built, tmp_path):
    out = subprocess.run([_build(tmp_path), "cpu"], capture_output=True, text=True)
    assert out.returncode == 0 and "cpu ok" in out.stdout, out.stdout + out.stderr


@pytest.mark.gpu
def test_cpp_sample_map_matches_the_model(rrt, tmp_path):
    w, h, v = 65, 9, 2                                                     # one lane past a wave, several blocks
    rng = np.random.default_rng(83)
    variance = (rng.random((v, h, w)) ** 4).astype(np.float32)
    hdr = (rng.random((v, h, w, 3)) ** 2 * 3.0).astype(np.float32)
    albedo = rng.random((v, h, w, 3)).astype(np.float32)
    variance[0, 0, :3] = [np.nan, np.inf, -1.0]
    albedo[1, 2, 3] = 0.0
    (tmp_path / "in.bin").write_bytes(variance.tobytes() + hdr.tobytes() + albedo.tobytes())
    out = subprocess.run([_build(tmp_path), "gpu", str(tmp_path / "in.bin"), str(tmp_path / "out.bin"), str(w), str(h), str(v)],
                         capture_output=True, text=True)
    assert out.returncode == 0 and "gpu ok" in out.stdout, out.stdout + out.stderr
    got = np.frombuffer((tmp_path / "out.bin").read_bytes(), dtype=np.uint32).reshape(3, v, h, w)
    assert np.array_equal(got[0], SM.sample_map(variance, hdr, albedo, 1, 8, 2.0))
    assert np.array_equal(got[1], SM.sample_map(variance, hdr, None, 0, 16, 1.5))
    assert np.array_equal(got[2], SM.sample_map(variance, None, None, 0, 16, 1.5))
    assert not np.array_equal(got[0], got[1]) and not np.array_equal(got[1], got[2])
