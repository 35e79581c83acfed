"""The baking methods of the C++ host mirror (include/mipt_host.hpp): bake_texels_on, bake_gather_on, Scene::bake_texels and
Scene::bake_gather over the C ABI -- argument handling without a device, and on the GPU the wrappers against the C entries (compared
inside the program) and against the models of tests/tools/bake_model.py, exchanged through a file."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import bake_model as B  # noqa: E402


def _build(tmp_path):
    exe = str(tmp_path / "test_host_bake")
    lib_dir = os.path.join(ROOT, "rust_ray_tracing_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_host_bake.cpp"),
                           "-o", exe, "-L", lib_dir, "-l:libmipt.so", f"-Wl,-rpath,{lib_dir}", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_cpp_bake_methods_check_arguments_without_a_device(built, tmp_path):
    out = subprocess.run([_build(tmp_path), "cpu"], capture_output=True, text=True)
    assert out.returncode == 0 and "cpu ok" in out.stdout, out.stdout + out.stderr


@pytest.mark.gpu
def test_cpp_bake_methods_match_the_c_entries_and_the_model(rrt, orc, tmp_path):
    from rust_ray_tracing_amd import synth
    obj = synth.write_cornell_obj(str(tmp_path))
    sc = rrt.Scene.load(obj)                                     # the same loader and BVH::build the C++ mirror calls: tree order = caller's
    w = h = 24
    want_pts, winfo = B.texels(sc.tris, w, h)
    assert winfo["covered"] > 0
    want = B.Gather(orc, sc, sc.tris).run(want_pts, 3, 4)         # the program's options: 3 samples, depth 4, stride = the texel count
    assert not np.any(np.isnan(want["mean"]))
    out = subprocess.run([_build(tmp_path), "gpu", obj, str(tmp_path / "out.bin")], capture_output=True, text=True)
    assert out.returncode == 0 and "gpu ok" in out.stdout, out.stdout + out.stderr
    raw = (tmp_path / "out.bin").read_bytes()
    n = w * h
    assert len(raw) == n * 16 + n * 12
    assert B.same_bits(np.frombuffer(raw[: n * 16], dtype=B.POINT), want_pts), "Scene::bake_texels differs from the model"
    assert B.same_bits(np.frombuffer(raw[n * 16:], dtype=np.float32).reshape(n, 3), want["mean"]), "Scene::bake_gather differs from the model"
