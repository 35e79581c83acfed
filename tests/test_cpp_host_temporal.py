"""Renderer::temporal of the C++ host mirror (include/mipt_host.hpp) over the C ABI: its argument handling without a device, and on
the GPU its results against the model of tests/tools/temporal_model.py, exchanged through files."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import temporal_model as T  # noqa: E402
import temporal_world as WD  # noqa: E402


def _model(cams, planes, history, albedo=True):
    return T.step(planes["hdr"], planes["position"], planes["normal"], planes["depth"], planes["material"], cams, history,
                  planes["albedo"] if albedo else None, **T.DEFAULTS)


def _build(tmp_path):
    exe = str(tmp_path / "test_host_temporal")
    lib_dir = os.path.join(ROOT, "rust_ray_tracing_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_host_temporal.cpp"),
                           "-o", exe, "-L", lib_dir, "-l:libmipt.so", f"-Wl,-rpath,{lib_dir}", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_cpp_temporal_checks_arguments_without_a_device(built, tmp_path):
    out = subprocess.run([_build(tmp_path), "cpu"], capture_output=True, text=True)
    assert out.returncode == 0 and "cpu ok" in out.stdout, out.stdout + out.stderr


@pytest.mark.gpu
def test_cpp_temporal_matches_the_model(rrt, tmp_path):
    size, v = (65, 9), 2
    w, h = size
    n = v * h * w
    cams, first = WD.frame(size, v, WD.SAME, seed=20)
    _, second = WD.frame(size, v, WD.SAME, seed=21)                           # the same cameras, other radiance
    order = ("hdr", "position", "normal", "depth", "material", "albedo")
    (tmp_path / "in.bin").write_bytes(cams.tobytes() + b"".join(p[k].tobytes() for p in (first, second) for k in order))
    out = subprocess.run([_build(tmp_path), "gpu", str(tmp_path / "in.bin"), str(tmp_path / "out.bin"), str(w), str(h), str(v)], capture_output=True, text=True)
    assert out.returncode == 0 and "gpu ok" in out.stdout, out.stdout + out.stderr
    hw = T.history_words(v, h, w)
    got = np.frombuffer((tmp_path / "out.bin").read_bytes(), dtype=np.uint32).reshape(4, n * 3 + hw + 2 * n)
    m0 = _model(cams, first, None)
    m1 = _model(cams, second, m0["history"])
    m2 = _model(cams, second, m0["history"], albedo=False)
    assert (m1["cls"] >= T.REUSED4).sum() > 0.5 * n and not T.same_bits(m1["out"], m2["out"])
    for i, want in enumerate((m0, m1, m2, m1)):
        call = dict(out=got[i, : n * 3].view(np.float32).reshape(v, h, w, 3), history=got[i, n * 3: n * 3 + hw],
                    length=got[i, n * 3 + hw: n * 4 + hw].view(np.float32).reshape(v, h, w), variance=got[i, n * 4 + hw:].view(np.float32).reshape(v, h, w))
        assert T.same_bits(call["out"], want["out"]) and T.same_bits(call["length"], want["length"]) and T.same_bits(call["variance"], want["variance"]), i
        assert T.same_history(call["history"], want["history"], v, h, w), i
