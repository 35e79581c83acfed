"""CPU: the entries that make adaptive sampling pay (mipt_temporal_counts, mipt_temporal_counts_device,
mipt_sample_map_fill_workspace_bytes, mipt_sample_map_fill, mipt_sample_map_fill_device) are declared, exported and bound, the new
struct has the size the header states, and every argument check they add runs before anything touches a device and names its field."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("mipt_temporal_counts", "mipt_temporal_counts_device", "mipt_sample_map_fill_workspace_bytes", "mipt_sample_map_fill",
           "mipt_sample_map_fill_device")


def test_symbols_declared_exported_and_bound(rrt):
    from rust_ray_tracing_amd import _lib as L
    header = open(os.path.join(ROOT, "include", "mipt.h")).read()
    declared = set(re.findall(r"\b(mipt_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)))
    out = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    lib = rrt.load()
    for s in ENTRIES:
        assert s in declared and s in exported and s in L.EXPORTS, s
        assert getattr(lib, s).argtypes is not None, s
    assert len(lib.mipt_temporal_counts.argtypes) == 6 and len(lib.mipt_temporal_counts_device.argtypes) == 6
    assert len(lib.mipt_sample_map_fill.argtypes) == 3 and len(lib.mipt_sample_map_fill_device.argtypes) == 4
    assert lib.mipt_sample_map_fill_workspace_bytes.restype is C.c_uint64 and len(lib.mipt_sample_map_fill_workspace_bytes.argtypes) == 4
    assert lib.mipt_abi_version() == 4
    assert re.search(r"\}\s*MiptSampleMapFillOptions;\s*/\* 64 B", header)
    # both contracts are in the header
    for phrase in ("len_q > 0", "al = nf / ln", "is NOT READ", "Histories interchange", "E_k = A < E ? E - A : 0", "room = span - e_{k-1}"):
        assert phrase in header, phrase


def test_struct_sizes_and_workspace_bytes(rrt):
    from rust_ray_tracing_amd import _lib as L
    lib = rrt.load()
    assert C.sizeof(L.MiptSampleMapFillOptions) == 64 and L.MiptSampleMapFillOptions.rounds.offset == 28
    for name in ("width", "height", "n_views", "flags", "min_samples", "max_samples", "budget"):   # the plain options' fields, where they were
        assert getattr(L.MiptSampleMapFillOptions, name).offset == getattr(L.MiptSampleMapOptions, name).offset, name
    assert L.MiptSampleMapFillOptions.reserved.offset == 32 and L.MiptSampleMapFillOptions.reserved.size == 32
    ws = lib.mipt_sample_map_fill_workspace_bytes
    assert [ws(1, 1, 1, r) for r in range(1, 9)] == [32 * r for r in range(1, 9)]
    assert ws(1920, 1080, 4, 4) == 128
    assert ws(8, 8, 1, 0) == 0 and ws(8, 8, 1, 9) == 0 and ws(8, 8, 1, 0xFFFFFFFF) == 0
    assert ws(0, 8, 1, 2) == 0 and ws(8, 0, 1, 2) == 0 and ws(8, 8, 0, 2) == 0
    assert ws(65536, 65536, 1, 2) == 0 and ws(40000, 40000, 3, 2) == 0


# ---- mipt_sample_map_fill* ---------------------------------------------------------------------------------------------------------
def _map_args(L, n=64):
    opt = L.MiptSampleMapFillOptions()
    opt.width, opt.height, opt.n_views, opt.min_samples, opt.max_samples, opt.budget, opt.rounds = 8, 8, 1, 1, 8, 2.0, 3
    keep = dict(variance=np.zeros(n, dtype=np.float32), hdr=np.zeros(n * 3, dtype=np.float32), albedo=np.zeros(n * 3, dtype=np.float32),
                counts=np.zeros(n, dtype=np.uint32))
    bufs = L.MiptSampleMapBuffers()
    for k, a in keep.items():
        setattr(bufs, k, a.ctypes.data)
    return opt, bufs, keep


def _set(obj, **kw):
    for k, v in kw.items():
        setattr(obj, k, v)


@pytest.mark.parametrize("which", ENTRIES[3:])
def test_sample_map_fill_argument_errors_without_a_device(rrt, which):
    from rust_ray_tracing_amd import _lib as L
    lib = rrt.load()
    work = np.zeros(48, dtype=np.uint64)
    base = (work.ctypes.data + 15) & ~15

    def call(opt, bufs, workspace="default"):
        o = C.byref(opt) if opt is not None else None
        b = C.byref(bufs) if bufs is not None else None
        if which == "mipt_sample_map_fill":
            return lib.mipt_sample_map_fill(o, b, 0)
        return lib.mipt_sample_map_fill_device(o, b, C.c_void_p(base) if workspace == "default" else workspace, None)

    def case(msg, edit=None, opt_none=False, bufs_none=False, **kw):
        opt, bufs, keep = _map_args(L)
        if edit:
            edit(opt, bufs, keep)
        assert call(None if opt_none else opt, None if bufs_none else bufs, **kw) == L.ERR_INVALID_ARG, msg
        err = lib.mipt_last_error().decode()
        assert msg in err and err.startswith(which + ":"), (msg, err)

    case("rounds 0: must be 1 ... 8", lambda o, b, k: _set(o, rounds=0))
    case("rounds 9: must be 1 ... 8", lambda o, b, k: _set(o, rounds=9))
    # and everything the plain map refuses, under this entry's name
    case("null opt", opt_none=True)
    case("null buffers", bufs_none=True)
    case("null variance", lambda o, b, k: _set(b, variance=None))
    case("null counts", lambda o, b, k: _set(b, counts=None))
    case("null hdr: albedo is given only with hdr", lambda o, b, k: _set(b, hdr=None))
    case("width and height", lambda o, b, k: _set(o, width=0))
    case("n_views == 0", lambda o, b, k: _set(o, n_views=0))
    case("below 2^32", lambda o, b, k: _set(o, width=65536, height=65536))
    case("flags 0x1", lambda o, b, k: _set(o, flags=1))
    for i in (0, 7):
        case("reserved option fields", lambda o, b, k, i=i: o.reserved.__setitem__(i, 1))
    case("reserved buffer pointers", lambda o, b, k: b.reserved.__setitem__(3, 16))
    case("max_samples 65536", lambda o, b, k: _set(o, max_samples=65536))
    case("min_samples 9", lambda o, b, k: _set(o, min_samples=9))
    case("budget", lambda o, b, k: _set(o, budget=8.5))
    case("budget", lambda o, b, k: _set(o, budget=float("nan")))
    def shifted_counts(o, b, k):
        # one array of this case's own holds both planes: variance in its first 64 words, counts 8 words behind it -- inside the array
        k["both"] = np.zeros(64 + 8, dtype=np.float32)
        _set(b, variance=k["both"].ctypes.data, counts=k["both"].ctypes.data + 32)
    case("counts overlaps variance", shifted_counts)
    if which == "mipt_sample_map_fill_device":
        case("null workspace", workspace=None)
        case("workspace must be 16-byte aligned", workspace=C.c_void_p(base + 8))
        case("counts must be 4-byte aligned", lambda o, b, k: _set(b, counts=k["counts"].ctypes.data + 1))
        # the workspace is 32 B per round: a counts plane 64 B behind its start overlaps it at rounds = 3, not at rounds = 2
        for rounds, msg in ((3, "counts overlaps the workspace"), (2, "is not device memory")):
            opt, bufs, keep = _map_args(L)
            opt.rounds = rounds
            bufs.counts = base + 64
            assert call(opt, bufs) == L.ERR_INVALID_ARG and msg in lib.mipt_last_error().decode(), (rounds, lib.mipt_last_error())
        case("is not device memory")                            # well-formed, but host pointers


# ---- mipt_temporal_counts* ----------------------------------------------------------------------------------------------------------
W, H, V = 8, 4, 2
N = V * W * H


def _temporal_args(L):
    o = L.MiptTemporalOptions()
    o.width, o.height, o.n_views = W, H, V
    o.alpha_min, o.max_history, o.normal_tol, o.depth_tol = 0.0, 32.0, 0.1, 0.1
    hw = 16 * V + 12 * N
    keep = dict(hdr=np.zeros(N * 3, dtype=np.float32), position=np.zeros(N * 3, dtype=np.float32), normal=np.zeros(N * 3, dtype=np.float32),
                depth=np.zeros(N, dtype=np.float32), material=np.zeros(N, dtype=np.uint32), albedo=np.zeros(N * 3, dtype=np.float32),
                history_in=np.zeros(hw + 4, dtype=np.uint32), history_out=np.zeros(hw + 4, dtype=np.uint32), out=np.zeros(N * 3, dtype=np.float32),
                length=np.zeros(N, dtype=np.float32), variance=np.zeros(N, dtype=np.float32), counts=np.ones(N + 4, dtype=np.uint32))
    b = L.MiptTemporalBuffers()
    for k, a in keep.items():
        if k != "counts":
            setattr(b, k, (a.ctypes.data + 15) & ~15 if k.startswith("history") else a.ctypes.data)
    cams = np.zeros(V, dtype=L.CAMERA)
    for c in cams:
        c["look_at"] = np.eye(4, dtype=np.float32)
    return o, b, keep, cams


@pytest.mark.parametrize("which", ENTRIES[:2])
def test_temporal_counts_argument_errors_without_a_device(rrt, which):
    from rust_ray_tracing_amd import _lib as L
    lib = rrt.load()

    def call(o, b, cams, counts, cap):
        f = getattr(lib, which)
        return f(C.byref(o) if o is not None else None, L.ptr(cams) if cams is not None else None, C.byref(b) if b is not None else None,
                 counts, cap, 0 if which == "mipt_temporal_counts" else None)

    def case(msg, edit=None, counts="default", cap=5, o_none=False, b_none=False, c_none=False):
        o, b, keep, cams = _temporal_args(L)
        if edit:
            edit(o, b, keep)
        cp = C.c_void_p(keep["counts"].ctypes.data) if counts == "default" else (counts(keep) if callable(counts) else counts)
        assert call(None if o_none else o, None if b_none else b, None if c_none else cams, cp, cap) == L.ERR_INVALID_ARG, msg
        err = lib.mipt_last_error().decode()
        assert msg in err and err.startswith(which + ":"), (msg, err)

    case("null counts", counts=None)
    case("samples_cap 0: must be 1 ... 65535", cap=0)
    case("samples_cap 65536: must be 1 ... 65535", cap=65536)
    # what mipt_temporal refuses is refused here too, under this entry's name
    case("null opt", o_none=True)
    case("null cameras", c_none=True)
    case("null buffers", b_none=True)
    case("null hdr", lambda o, b, k: _set(b, hdr=None))
    case("null history_out", lambda o, b, k: _set(b, history_out=None))
    case("width and height", lambda o, b, k: _set(o, width=0))
    case("flags 0x1", lambda o, b, k: _set(o, flags=1))
    case("reserved option fields", lambda o, b, k: o.reserved.__setitem__(0, 1))
    case("reserved buffer pointers", lambda o, b, k: b.reserved.__setitem__(0, 16))
    case("max_history", lambda o, b, k: _set(o, max_history=0.5))
    case("alpha_min", lambda o, b, k: _set(o, alpha_min=1.5))
    case("out overlaps albedo", lambda o, b, k: _set(b, out=k["albedo"].ctypes.data))
    if which == "mipt_temporal_counts_device":
        case("counts must be 4-byte aligned", counts=lambda k: C.c_void_p(k["counts"].ctypes.data + 2))
        case("counts overlaps hdr", counts=lambda k: C.c_void_p(k["hdr"].ctypes.data + 8))
        case("counts overlaps depth", counts=lambda k: C.c_void_p(k["depth"].ctypes.data))
        # The count plane is N words.  Starting in the last word of the N-word variance array it ran N - 1 words past the array's end,
        # over whatever the allocator had put there: when that was another plane of the call, an earlier name of the table was
        # reported ("counts overlaps length").  Both planes now lie in one array of 2 N words that the case owns.
        def shared_variance(o, b, k):
            k["both"] = np.zeros(2 * N, dtype=np.float32)
            _set(b, variance=k["both"].ctypes.data)
        case("counts overlaps variance", shared_variance, counts=lambda k: C.c_void_p(k["both"].ctypes.data + 4 * N - 4))
        case("counts overlaps history_in", counts=lambda k: C.c_void_p(((k["history_in"].ctypes.data + 15) & ~15) + 64))
        def roomy_history_out(o, b, k):                         # the same: N words of room behind the history's last word
            k["history_out"] = np.zeros(16 * V + 12 * N + 4 + N, dtype=np.uint32)
            _set(b, history_out=(k["history_out"].ctypes.data + 15) & ~15)
        case("counts overlaps history_out", roomy_history_out,
             counts=lambda k: C.c_void_p(((k["history_out"].ctypes.data + 15) & ~15) + 4 * (16 * V + 12 * N) - 4))
        case("is not device memory")                            # well-formed, but host pointers


def test_renderer_mirrors_check_their_arguments(rrt):
    r = rrt.Renderer(rrt.RendererOptions(samples=4, max_ray_depth=1, output_image_dimensions=(W, H), output_image_path="/dev/null"))
    hdr = np.zeros((V, H, W, 3), dtype=np.float32)
    feats = dict(position=hdr, normal=hdr, depth=np.zeros((V, H, W), dtype=np.float32), material=np.zeros((V, H, W), dtype=np.uint32))
    cams = [rrt.Camera(position=(0.0, 0.0, 0.0), pitch=0.0, yaw=0.0) for _ in range(V)]
    for c in cams:
        c.update_view()
    with pytest.raises(ValueError, match="samples_cap"):
        r.temporal(hdr, feats, cams, samples_cap=3)
    with pytest.raises(ValueError, match="counts: expected uint32"):
        r.temporal(hdr, feats, cams, counts=np.ones((V, H, W), dtype=np.int32))
    with pytest.raises(ValueError, match="counts: expected shape"):
        r.temporal(hdr, feats, cams, counts=np.ones((V, H, W + 1), dtype=np.uint32))
    with pytest.raises(RuntimeError, match="samples_cap 0"):
        r.temporal(hdr, feats, cams, counts=np.ones((V, H, W), dtype=np.uint32), samples_cap=0)
    with pytest.raises(RuntimeError, match="rounds 9"):
        r.sample_map(np.zeros((V, H, W), dtype=np.float32), rounds=9)
