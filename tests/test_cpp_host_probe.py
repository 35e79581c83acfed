"""The probe methods of the C++ host mirror (include/mipt_host.hpp): bake_probes_on, Scene::bake_probes, mipt::probe_grid and
mipt::probe_irradiance over the C ABI -- argument handling without a device, and on the GPU the wrappers against the C entries
(compared inside the program) and against the models of tests/tools/probe_model.py, exchanged through a file."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import probe_model as PM  # noqa: E402


def _build(tmp_path):
    exe = str(tmp_path / "test_host_probe")
    lib_dir = os.path.join(ROOT, "rust_ray_tracing_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_host_probe.cpp"),
                           "-o", exe, "-L", lib_dir, "-l:libmipt.so", f"-Wl,-rpath,{lib_dir}", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_cpp_probe_methods_check_arguments_without_a_device(built, tmp_path):
    out = subprocess.run([_build(tmp_path), "cpu"], capture_output=True, text=True)
    assert out.returncode == 0 and "cpu ok" in out.stdout, out.stdout + out.stderr


@pytest.mark.gpu
def test_cpp_probe_methods_match_the_c_entries_and_the_models(rrt, orc, tmp_path):
    from rust_ray_tracing_amd import synth
    obj = synth.write_cornell_obj(str(tmp_path))
    sc = rrt.Scene.load(obj)                                     # the same loader and BVH::build the C++ mirror calls
    grid = ((-0.5, -0.5, -0.5), (1.0, 1.0, 1.0), (2, 2, 2))
    n_probes, n = 8, 10
    out = subprocess.run([_build(tmp_path), "gpu", obj, str(tmp_path / "out.bin")], capture_output=True, text=True)
    assert out.returncode == 0 and "gpu ok" in out.stdout, out.stdout + out.stderr
    raw = (tmp_path / "out.bin").read_bytes()
    assert len(raw) == n_probes * 16 + n_probes * 108 + 4 * n * 12
    probes = np.frombuffer(raw[: n_probes * 16], dtype=PM.PROBE)
    assert PM.same_bits(probes["position"], PM.grid_positions(*grid)) and np.array_equal(probes["seed"], np.arange(8))
    sh = np.frombuffer(raw[n_probes * 16: n_probes * 124], dtype=np.float32).reshape(n_probes, 9, 3)
    want = PM.Bake(orc, sc).run(probes, 4, 4)                    # the program's options: 4 samples, depth 4, stride = the probe count
    assert want["hit"].any() and not want["hit"].all()
    assert PM.same_bits(sh, want["mean"]), "the coefficients differ from the model"
    position, normal, irradiance, masked = np.frombuffer(raw[n_probes * 124:], dtype=np.float32).reshape(4, n, 3)
    valid = np.ones(8, dtype=np.uint8)
    valid[[0, 3, 6]] = 0
    assert PM.same_bits(irradiance, PM.lookup(sh, grid, position, normal)), "the irradiance differs from the model"
    assert PM.same_bits(masked, PM.lookup(sh, grid, position, normal, valid, clamp=True)), "the irradiance with a valid plane differs from the model"
