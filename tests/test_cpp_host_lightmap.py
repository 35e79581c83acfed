"""The lightmap methods of the C++ host mirror (include/mipt_host.hpp): bake_surface_on, Scene::bake_surface, mipt::lightmap_filter and
mipt::lightmap_dilate over the C ABI -- argument handling without a device, and on the GPU the wrappers against the C entries
(compared inside the program) and against the models of tests/tools/lightmap_model.py, exchanged through a file."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import bake_model as B  # noqa: E402
import lightmap_model as M  # noqa: E402


def _build(tmp_path):
    exe = str(tmp_path / "test_host_lightmap")
    lib_dir = os.path.join(ROOT, "rust_ray_tracing_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_host_lightmap.cpp"),
                           "-o", exe, "-L", lib_dir, "-l:libmipt.so", f"-Wl,-rpath,{lib_dir}", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_cpp_lightmap_methods_check_arguments_without_a_device(built, tmp_path):
    out = subprocess.run([_build(tmp_path), "cpu"], capture_output=True, text=True)
    assert out.returncode == 0 and "cpu ok" in out.stdout, out.stdout + out.stderr


@pytest.mark.gpu
def test_cpp_lightmap_methods_match_the_c_entries_and_the_models(rrt, orc, tmp_path):
    from rust_ray_tracing_amd import synth
    obj = synth.write_cornell_obj(str(tmp_path))
    sc = rrt.Scene.load(obj)                                     # the same loader and BVH::build the C++ mirror calls: tree order = caller's
    w = h = 24
    n = w * h
    pts, winfo = B.texels(sc.tris, w, h)
    assert winfo["covered"] > 0
    cov = (pts["prim"] != B.NONE).reshape(h, w)
    mean = B.Gather(orc, sc, sc.tris).run(pts, 2, 4)["mean"]     # the program's options: 2 samples, depth 4, stride = the texel count
    pos, nrm = M.surface_all(sc.tris, pts, unit=True)
    filtered = M.filter(orc, mean.reshape(h, w, 3), cov, position=pos, normal=nrm, iterations=2, sigma_color=2.0, sigma_normal=0.5, sigma_plane=0.1,
                        sigma_distance=0.5)
    dilated, level = M.dilate(filtered, cov, 2)
    out = subprocess.run([_build(tmp_path), "gpu", obj, str(tmp_path / "out.bin")], capture_output=True, text=True)
    assert out.returncode == 0 and "gpu ok" in out.stdout, out.stdout + out.stderr
    raw = (tmp_path / "out.bin").read_bytes()
    assert len(raw) == n * 16 + 5 * n * 12 + n * 4
    assert B.same_bits(np.frombuffer(raw[: n * 16], dtype=B.POINT), pts)
    planes = np.frombuffer(raw[n * 16: n * 16 + 5 * n * 12], dtype=np.float32).reshape(5, n, 3)
    for name, got, want in zip(("radiance", "position", "normal", "filtered", "dilated"), planes, (mean, pos, nrm, filtered, dilated)):
        assert M.same_bits(got, np.asarray(want).reshape(n, 3)), f"{name} differs from the model"
    assert np.array_equal(np.frombuffer(raw[n * 16 + 5 * n * 12:], dtype=np.uint32), level.reshape(-1))
