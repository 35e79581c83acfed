"""The radiance-query methods of the C++ host mirror (include/mipt_host.hpp): query_radiance_on, Scene::query_radiance and
Renderer::query_radiance over the C ABI -- argument handling without a device, and on the GPU the results against the model of
tests/tools/radiance_model.py, exchanged through files."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import radiance_model as R  # noqa: E402


def _build(tmp_path):
    exe = str(tmp_path / "test_host_radiance")
    lib_dir = os.path.join(ROOT, "rust_ray_tracing_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_host_radiance.cpp"),
                           "-o", exe, "-L", lib_dir, "-l:libmipt.so", f"-Wl,-rpath,{lib_dir}", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_cpp_radiance_methods_check_arguments_without_a_device(built, tmp_path):
    out = subprocess.run([_build(tmp_path), "cpu"], capture_output=True, text=True)
    assert out.returncode == 0 and "cpu ok" in out.stdout, out.stdout + out.stderr


@pytest.mark.gpu
def test_cpp_radiance_methods_match_the_model(rrt, orc, tmp_path):
    from rust_ray_tracing_amd import synth
    obj = synth.write_cornell_obj(str(tmp_path))
    sc = rrt.Scene.load(obj)                                     # the same loader and BVH::build the C++ mirror calls
    m = R.Model(orc, sc)
    rays = R.make_rays(sc.tris, 200, seed=20)
    want = m.trace(rays, 3, 6)                                   # the program's options: 3 samples, depth 6, reference traversal
    R.conditions(want, m.first_hits(rays))
    (tmp_path / "rays.bin").write_bytes(rays.tobytes())
    out = subprocess.run([_build(tmp_path), "gpu", obj, str(tmp_path / "rays.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True)
    assert out.returncode == 0 and "gpu ok" in out.stdout, out.stdout + out.stderr
    got = np.frombuffer((tmp_path / "out.bin").read_bytes(), dtype=np.float32).reshape(2, len(rays), 3)
    assert R.same_bits(got[0], want["mean"]), "Scene::query_radiance differs from the model"
    assert R.same_bits(got[1], want["sum"]), "Renderer::query_radiance (MIPT_FLAG_SUM) differs from the model"
