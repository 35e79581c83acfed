"""The count-aware Renderer::temporal overload and SampleMapSettings::rounds of the C++ host mirror (include/mipt_host.hpp) over the C
ABI: their argument handling without a device, and on the GPU their results against the models of tests/tools/temporal_counts_model.py
and tests/tools/sample_map_fill_model.py, exchanged through files."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import sample_map_fill_model as FM  # noqa: E402
import sample_map_model as SM  # noqa: E402
import temporal_counts_model as TC  # noqa: E402
import temporal_model as T  # noqa: E402
import temporal_world as WD  # noqa: E402


def _build(tmp_path):
    exe = str(tmp_path / "test_host_weighted")
    lib_dir = os.path.join(ROOT, "rust_ray_tracing_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_host_weighted.cpp"),
                           "-o", exe, "-L", lib_dir, "-l:libmipt.so", f"-Wl,-rpath,{lib_dir}", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_cpp_weighted_checks_arguments_without_a_device(built, tmp_path):
    out = subprocess.run([_build(tmp_path), "cpu"], capture_output=True, text=True)
    assert out.returncode == 0 and "cpu ok" in out.stdout, out.stdout + out.stderr


@pytest.mark.gpu
def test_cpp_weighted_matches_the_models(rrt, tmp_path):
    size, v = (65, 9), 2
    w, h = size
    n = v * h * w
    cams, first = WD.frame(size, v, WD.SAME, seed=20)
    _, second = WD.frame(size, v, WD.SAME, seed=21)                           # the same cameras, other radiance
    rng = np.random.default_rng(9)
    counts = [rng.choice(np.array([0, 1, 2, 3, 5, 9], dtype=np.uint32), size=(v, h, w)).astype(np.uint32) for _ in range(2)]
    variance = (rng.random((v, h, w)) ** 6 * 1e-2).astype(np.float32)
    variance[:, ::4, ::7] = 4.0                                               # saturate in round 1
    order = ("hdr", "position", "normal", "depth", "material", "albedo")
    (tmp_path / "in.bin").write_bytes(cams.tobytes() + b"".join(b"".join(p[k].tobytes() for k in order) + c.tobytes()
                                                               for p, c in ((first, counts[0]), (second, counts[1]))) + variance.tobytes())
    out = subprocess.run([_build(tmp_path), "gpu", str(tmp_path / "in.bin"), str(tmp_path / "out.bin"), str(w), str(h), str(v)], capture_output=True, text=True)
    assert out.returncode == 0 and "gpu ok" in out.stdout, out.stdout + out.stderr
    hw = T.history_words(v, h, w)
    call_words = n * 3 + hw + 2 * n
    got = np.frombuffer((tmp_path / "out.bin").read_bytes(), dtype=np.uint32)
    assert got.size == 2 * call_words + 3 * n

    def model(p, c, history):
        return TC.step(p["hdr"], p["position"], p["normal"], p["depth"], p["material"], cams, c, 5, history, p["albedo"], **T.DEFAULTS)

    m0 = model(first, counts[0], None)
    m1 = model(second, counts[1], m0["history"])
    assert (m1["reuse"] & (m1["n"] == 0)).sum() > 20 and (m1["reuse"] & (m1["n"] > 0)).sum() > 0.3 * n
    for i, want in enumerate((m0, m1)):
        c = got[i * call_words: (i + 1) * call_words]
        call = dict(out=c[: n * 3].view(np.float32).reshape(v, h, w, 3), history=c[n * 3: n * 3 + hw],
                    length=c[n * 3 + hw: n * 4 + hw].view(np.float32).reshape(v, h, w), variance=c[n * 4 + hw:].view(np.float32).reshape(v, h, w))
        assert T.same_bits(call["out"], want["out"]) and T.same_bits(call["length"], want["length"]) and T.same_bits(call["variance"], want["variance"]), i
        assert T.same_history(call["history"], want["history"], v, h, w), i
    maps = got[2 * call_words:].reshape(3, v, h, w)
    plain = SM.sample_map(variance, None, None, 1, 8, 2.0)
    assert np.array_equal(maps[0], plain) and np.array_equal(maps[1], plain)
    assert np.array_equal(maps[2], FM.fill(variance, None, None, 1, 8, 2.0, 4)) and not np.array_equal(maps[2], plain)
