"""Renderer::upsample of the C++ host mirror (include/mipt_host.hpp) over the C ABI: its argument handling without a device, and on
the GPU its results against the model of tests/tools/upsample_model.py, exchanged through files."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import upsample_model as UM  # noqa: E402


def _build(tmp_path):
    exe = str(tmp_path / "test_host_upsample")
    lib_dir = os.path.join(ROOT, "rust_ray_tracing_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_host_upsample.cpp"),
                           "-o", exe, "-L", lib_dir, "-l:libmipt.so", f"-Wl,-rpath,{lib_dir}", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_cpp_upsample_checks_arguments_without_a_device(built, tmp_path):
    out = subprocess.run([_build(tmp_path), "cpu"], capture_output=True, text=True)
    assert out.returncode == 0 and "cpu ok" in out.stdout, out.stdout + out.stderr


@pytest.mark.gpu
def test_cpp_upsample_matches_the_model(rrt, orc, tmp_path):
    w, h, v, k = 13, 3, 2, 5                                                # 65x15 at full resolution: one lane past the tile row
    W, H = w * k, h * k
    rng = np.random.default_rng(79)
    rep = lambda a: np.repeat(np.repeat(a, k, axis=1), k, axis=2)  # noqa: E731
    lo_hdr = (rng.random((v, h, w, 3)) ** 2 * 4.0).astype(np.float32)
    lo = dict(normal=rng.normal(0, 0.6, (v, h, w, 3)).astype(np.float32), depth=(2.0 + rng.random((v, h, w)) * 0.4).astype(np.float32),
              albedo=rng.random((v, h, w, 3)).astype(np.float32), material=rng.integers(0, 2, (v, h, w)).astype(np.uint32))
    hi = dict(normal=(rep(lo["normal"]) + rng.normal(0, 0.1, (v, H, W, 3))).astype(np.float32),
              depth=(rep(lo["depth"]) + rng.normal(0, 0.1, (v, H, W))).astype(np.float32),
              albedo=rng.random((v, H, W, 3)).astype(np.float32), material=rep(lo["material"]).copy())
    lo["depth"][rng.random((v, h, w)) < 0.2] = np.float32(1e30)
    hi["depth"][rng.random((v, H, W)) < 0.2] = np.float32(1e30)
    hi["material"][rng.random((v, H, W)) < 0.1] = 9
    lo["albedo"][0, 1, 3] = 0.0
    order = ("normal", "depth", "albedo", "material")
    (tmp_path / "in.bin").write_bytes(lo_hdr.tobytes() + b"".join(lo[g].tobytes() for g in order) + b"".join(hi[g].tobytes() for g in order))
    out = subprocess.run([_build(tmp_path), "gpu", str(tmp_path / "in.bin"), str(tmp_path / "out.bin"), str(W), str(H), str(v), str(k)],
                         capture_output=True, text=True)
    assert out.returncode == 0 and "gpu ok" in out.stdout, out.stdout + out.stderr
    got = np.frombuffer((tmp_path / "out.bin").read_bytes(), dtype=np.float32)
    n = v * H * W
    assert got.size == 10 * n
    frames = [f.reshape(v, H, W, 3) for f in (got[: 3 * n], got[4 * n: 7 * n], got[7 * n: 10 * n])]
    weight = got[3 * n: 4 * n].reshape(v, H, W)
    full = UM.upsample(orc, lo_hdr, k, lo, hi)
    assert UM.same_bits(frames[0], full[0]) and UM.same_bits(weight, full[1]) and (weight == 0).any()
    assert UM.same_bits(frames[1], UM.upsample(orc, lo_hdr, k)[0])
    sub = ("depth", "material")
    assert UM.same_bits(frames[2], UM.upsample(orc, lo_hdr, k, {g: lo[g] for g in sub}, {g: hi[g] for g in sub}, sigma_depth=0.25)[0])
    assert not UM.same_bits(frames[0], frames[1]) and not UM.same_bits(frames[1], frames[2])
