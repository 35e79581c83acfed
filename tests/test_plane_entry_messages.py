"""CPU: the whole text of mipt_last_error(), and the order in which the checks fire, for the fourteen image-space entries of
include/mipt.h -- mipt_denoise, mipt_denoise_variance, mipt_upsample, mipt_temporal, mipt_temporal_counts, mipt_sample_map,
mipt_sample_map_fill and their _device forms.  The model tests beside this one feed one fault at a time and look for a substring;
here every refusal is held to its status code and its full message, and inputs with two faults fix which of the two is reported.

Every case is refused before anything is launched: the planes are zero-filled host arrays of W x H x V = 8 x 4 x 2 pixels, which the
device entries turn away as "not device memory" at the latest, and the host entries are only ever given a fault or a device ordinal
that does not exist.  At the end no plane has been written."""
import ctypes as C

import numpy as np
import pytest

W, H, V, SCALE = 8, 4, 2, 2
N = W * H * V
N_LO = N // (SCALE * SCALE)
HIST = 64 * V + 48 * N
PAD = 64                                                            # bytes behind every plane, so that a shifted pointer stays inside
NO_DEVICE = 1 << 20                                                 # a device ordinal no machine has
# hipSetDevice's text for NO_DEVICE: without any device, and with devices but not this one
HIP_TEXTS = ("no ROCm-capable device is detected", "invalid device ordinal")

_arrays = []                                                        # every plane handed to the library, for the last test


def _block(n_bytes, pad=PAD):
    """n_bytes + pad zero bytes, 16-byte aligned"""
    raw = np.zeros(n_bytes + pad + 16, dtype=np.uint8)
    off = -raw.ctypes.data % 16
    a = raw[off: off + n_bytes + pad]
    _arrays.append(a)
    return a


class At:
    """a pointer `off` bytes into the plane (or the workspace, "ws") called `name`"""

    def __init__(self, name, off=0):
        self.name, self.off = name, off


class Family:
    def __init__(self, host, opt_cls, buf_cls, defaults, planes, cams=False, counts=False, ws_bytes=None, ws_sized=False):
        self.host, self.device = host, host + "_device"
        self.opt_cls, self.buf_cls, self.defaults = opt_cls, buf_cls, defaults
        self.has_cams, self.has_counts, self.ws_bytes, self.ws_sized = cams, counts, ws_bytes, ws_sized
        self.mem = {k: _block(n) for k, n in planes.items()}
        self.mem["ws"] = _block(ws_bytes or 16, pad=N * 12 + PAD)      # room for the largest plane, placed anywhere in it
        if counts:
            self.mem["counts"] = _block(N * 4)

    def _address(self, v, own):
        if isinstance(v, At):
            return self.mem[v.name].ctypes.data + v.off
        return v if v is None or isinstance(v, int) else self.mem[own].ctypes.data

    def call(self, lib, L, device, opt=(), buf=(), **extra):
        """one call of the host (device = False) or the device entry.  opt / buf: None for a null struct, else the fields to change;
        "reserved" takes the index of the reserved field to set.  extra: cams, counts, cap, ws, ws_bytes, device_id."""
        o = None
        if opt is not None:
            o = self.opt_cls()
            for k, v in dict(self.defaults, **dict(opt)).items():
                if k == "reserved":
                    o.reserved[v] = 1
                else:
                    setattr(o, k, v)
        b = None
        if buf is not None:
            b = self.buf_cls()
            for k, _ in self.buf_cls._fields_:
                if k != "reserved":
                    setattr(b, k, self.mem[k].ctypes.data)
            for k, v in dict(buf).items():
                if k == "reserved":
                    b.reserved[v] = self.mem["ws"].ctypes.data
                else:
                    setattr(b, k, self._address(v, k))
        args = [C.byref(o) if o is not None else None]
        if self.has_cams:
            cams = np.zeros(V, dtype=L.CAMERA)
            cams["look_at"] = np.eye(4, dtype=np.float32)
            how = extra.get("cams", "good")
            if how == "singular":
                cams[1]["look_at"][:] = 0.0
            args.append(None if how is None else L.ptr(cams))
        args.append(C.byref(b) if b is not None else None)
        if self.has_counts:
            args += [self._address(extra.get("counts", At("counts")), "counts"), extra.get("cap", 4)]
        if not device:
            args.append(extra.get("device_id", 0))
        else:
            if self.ws_bytes:
                args.append(self._address(extra.get("ws", At("ws")), "ws"))
            if self.ws_sized:
                args.append(extra.get("ws_bytes", self.ws_bytes))
            args.append(None)                                       # the stream
        rc = getattr(lib, self.device if device else self.host)(*args)
        return rc, lib.mipt_last_error().decode()


def _families(L):
    f3, f1 = N * 12, N * 4
    denoise = dict(hdr=f3, normal=f3, depth=f1, albedo=f3, out=f3)
    variance = dict(hdr=f3, normal=f3, depth=f1, albedo=f3, variance=f1, length=f1, out=f3, variance_out=f1)
    upsample = dict(lo_hdr=N_LO * 12, lo_normal=N_LO * 12, lo_depth=N_LO * 4, lo_albedo=N_LO * 12, lo_material=N_LO * 4,
                    normal=f3, depth=f1, albedo=f3, material=f1, out=f3, weight=f1)
    temporal = dict(hdr=f3, position=f3, normal=f3, depth=f1, material=f1, albedo=f3, history_in=HIST, history_out=HIST, out=f3,
                    length=f1, variance=f1)
    sample_map = dict(variance=f1, hdr=f3, albedo=f3, counts=f1)
    frame = dict(width=W, height=H, n_views=V)
    t_opt = dict(frame, alpha_min=0.0, max_history=32.0, normal_tol=0.1, depth_tol=0.1)
    s_opt = dict(frame, min_samples=1, max_samples=8, budget=2.0)
    return dict(
        denoise=Family("mipt_denoise", L.MiptDenoiseOptions, L.MiptDenoiseBuffers,
                       dict(frame, iterations=3, sigma_color=4.0, sigma_normal=0.5, sigma_depth=0.5), denoise, ws_bytes=N * 48, ws_sized=True),
        variance=Family("mipt_denoise_variance", L.MiptVarianceOptions, L.MiptVarianceBuffers,
                        dict(frame, iterations=3, sigma_luminance=4.0, sigma_normal=0.5, sigma_depth=0.5, short_history=4.0), variance,
                        ws_bytes=N * 48, ws_sized=True),
        upsample=Family("mipt_upsample", L.MiptUpsampleOptions, L.MiptUpsampleBuffers,
                        dict(frame, scale=SCALE, sigma_normal=0.5, sigma_depth=0.5), upsample, ws_bytes=N_LO * 32, ws_sized=True),
        temporal=Family("mipt_temporal", L.MiptTemporalOptions, L.MiptTemporalBuffers, t_opt, temporal, cams=True),
        temporal_counts=Family("mipt_temporal_counts", L.MiptTemporalOptions, L.MiptTemporalBuffers, t_opt, temporal, cams=True, counts=True),
        sample_map=Family("mipt_sample_map", L.MiptSampleMapOptions, L.MiptSampleMapBuffers, s_opt, sample_map, ws_bytes=32),
        sample_map_fill=Family("mipt_sample_map_fill", L.MiptSampleMapFillOptions, L.MiptSampleMapBuffers, dict(s_opt, rounds=2), sample_map,
                               ws_bytes=64),
    )


INF, NAN = float("inf"), float("nan")
BIG = dict(width=65536, height=65536)                              # 2 views of 2^32 pixels
BIG_TEXT = "2 views of 65536x65536: n_views*width*height must stay below 2^32"
ONLY = " (only out == hdr is allowed)"

# (where, call arguments, the message after "<entry>: ").  where: "both" entries, the "host" or the "device" entry only.
# The first block of every family is its single faults, the second its pairs of faults: the one reported is the one checked first.
FRAME = [
    ("both", dict(opt=None), "null opt"),
    ("both", dict(buf=None), "null buffers"),
    ("both", dict(opt=dict(width=0)), "width and height must be greater than 0"),
    ("both", dict(opt=dict(height=0)), "width and height must be greater than 0"),
    ("both", dict(opt=dict(n_views=0)), "n_views == 0"),
    ("both", dict(opt=BIG), BIG_TEXT),
    ("both", dict(opt=dict(flags=4)), "flags 0x4: must be 0"),
    ("both", dict(opt=dict(reserved=0)), "reserved option fields must be 0"),
    ("both", dict(opt=dict(reserved=6)), "reserved option fields must be 0"),
    ("both", dict(buf=dict(reserved=0)), "reserved buffer pointers must be NULL"),
    ("both", dict(buf=dict(reserved=2)), "reserved buffer pointers must be NULL"),
    ("both", dict(opt=dict(flags=0x10, reserved=1)), "flags 0x10: must be 0"),
    ("both", dict(opt=dict(reserved=1), buf=dict(reserved=1)), "reserved option fields must be 0"),
    ("both", dict(opt=None, buf=None), "null opt"),
]
SIGMAS = [
    ("both", dict(opt=dict(sigma_normal=-1.0)), "sigma_normal -1: it and 1 / sigma_normal^2 must be finite and greater than 0"),
    ("both", dict(opt=dict(sigma_normal=1e-20)), "sigma_normal 1e-20: it and 1 / sigma_normal^2 must be finite and greater than 0"),
    ("both", dict(opt=dict(sigma_depth=NAN)), "sigma_depth nan: it and 1 / sigma_depth^2 must be finite and greater than 0"),
    ("both", dict(opt=dict(sigma_depth=1e20)), "sigma_depth 1e+20: it and 1 / sigma_depth^2 must be finite and greater than 0"),
    ("both", dict(opt=dict(sigma_normal=0.0, sigma_depth=0.0)), "sigma_normal 0: it and 1 / sigma_normal^2 must be finite and greater than 0"),
]


def _workspace(need_fn, need, first, second, anchor):
    """the device entries that take a sized workspace; first / second: the first two planes of the table, anchor = the first"""
    return [
        ("device", dict(ws=None), "null workspace"),
        ("device", dict(ws_bytes=need - 1), f"workspace of {need - 1} bytes is too small: {need_fn}() is {need}"),
        ("device", dict(ws_bytes=0), f"workspace of 0 bytes is too small: {need_fn}() is {need}"),
        ("device", dict(ws=At("ws", 4)), "workspace must be 16-byte aligned"),
        ("device", dict(buf={first: At(first, 2)}), f"{first} must be 4-byte aligned"),
        ("device", dict(buf={second: At(second, 1)}), f"{second} must be 4-byte aligned"),
        ("device", dict(buf={first: At("ws")}), f"{first} overlaps the workspace"),
        ("device", dict(buf={second: At("ws", need - 4)}), f"{second} overlaps the workspace"),
        ("device", dict(), f"{anchor} is not device memory"),
        ("device", dict(ws=None, ws_bytes=0), "null workspace"),
        ("device", dict(ws=At("ws", 8), ws_bytes=need - 16), f"workspace of {need - 16} bytes is too small: {need_fn}() is {need}"),
        ("device", dict(ws=At("ws", 8), buf={first: At(first, 2)}), "workspace must be 16-byte aligned"),
        ("device", dict(buf={first: At("ws", 2)}), f"{first} must be 4-byte aligned"),
        ("device", dict(buf={first: At("ws"), second: At(second, 2)}), f"{first} overlaps the workspace"),
        ("device", dict(buf={first: At(first, 2), second: At("ws")}), f"{first} must be 4-byte aligned"),
        ("device", dict(buf={second: At("ws", 2)}), f"{second} must be 4-byte aligned"),
    ]


CASES = dict(
    denoise=FRAME + SIGMAS + _workspace("mipt_denoise_workspace_bytes", N * 48, "hdr", "normal", "hdr") + [
        ("both", dict(buf=dict(hdr=None)), "null hdr"),
        ("both", dict(buf=dict(out=None)), "null out"),
        ("both", dict(opt=dict(iterations=0)), "iterations 0: must be 1 ... 8"),
        ("both", dict(opt=dict(iterations=9)), "iterations 9: must be 1 ... 8"),
        ("both", dict(opt=dict(sigma_color=0.0)), "sigma_color must be finite and greater than 0"),
        ("both", dict(opt=dict(sigma_color=INF)), "sigma_color must be finite and greater than 0"),
        ("both", dict(opt=dict(sigma_color=1e-20)), "sigma_color 1e-20: 1 / (sigma_color * 2^-0)^2 is not finite and greater than 0"),
        ("both", dict(opt=dict(sigma_color=2e-19)), "sigma_color 2e-19: 1 / (sigma_color * 2^-2)^2 is not finite and greater than 0"),
        ("both", dict(buf=dict(normal=At("hdr", 4))), "normal overlaps hdr" + ONLY),
        ("both", dict(buf=dict(out=At("hdr", 4))), "out overlaps hdr" + ONLY),
        ("both", dict(buf=dict(out=At("albedo", 4))), "out overlaps albedo" + ONLY),
        ("both", dict(buf=dict(hdr=None, out=None)), "null hdr"),
        ("both", dict(opt=dict(width=0), buf=dict(out=None)), "null out"),
        ("both", dict(opt=dict(iterations=0, **BIG)), BIG_TEXT),
        ("both", dict(opt=dict(iterations=0, flags=1)), "iterations 0: must be 1 ... 8"),
        ("both", dict(opt=dict(sigma_color=NAN), buf=dict(reserved=0)), "reserved buffer pointers must be NULL"),
        ("both", dict(opt=dict(sigma_color=NAN, sigma_normal=NAN)), "sigma_color must be finite and greater than 0"),
        ("both", dict(opt=dict(sigma_depth=-2.0), buf=dict(normal=At("hdr"))), "sigma_depth -2: it and 1 / sigma_depth^2 must be finite and greater than 0"),
        ("device", dict(buf=dict(normal=At("hdr")), ws=None), "normal overlaps hdr" + ONLY),
    ],
    variance=FRAME + SIGMAS + _workspace("mipt_denoise_variance_workspace_bytes", N * 48, "hdr", "normal", "hdr") + [
        ("both", dict(buf=dict(hdr=None)), "null hdr"),
        ("both", dict(buf=dict(out=None)), "null out"),
        ("both", dict(buf=dict(variance=None)), "null variance: variance and length are given together or not at all"),
        ("both", dict(buf=dict(length=None)), "null length: variance and length are given together or not at all"),
        ("both", dict(opt=dict(iterations=0)), "iterations 0: must be 1 ... 8"),
        ("both", dict(opt=dict(sigma_luminance=0.0)), "sigma_luminance must be finite and greater than 0"),
        ("both", dict(opt=dict(short_history=-1.0)), "short_history must be finite and at least 0"),
        ("both", dict(opt=dict(short_history=INF)), "short_history must be finite and at least 0"),
        ("both", dict(buf=dict(variance_out=At("variance"))), "variance_out overlaps variance" + ONLY),
        ("both", dict(buf=dict(out=At("hdr", 4))), "out overlaps hdr" + ONLY),
        ("both", dict(opt=dict(width=0), buf=dict(out=None)), "null out"),
        ("both", dict(opt=dict(width=0), buf=dict(length=None)), "null length: variance and length are given together or not at all"),
        ("both", dict(opt=dict(iterations=9, flags=1)), "iterations 9: must be 1 ... 8"),
        ("both", dict(opt=dict(sigma_luminance=NAN), buf=dict(reserved=0)), "reserved buffer pointers must be NULL"),
        ("both", dict(opt=dict(sigma_luminance=NAN, short_history=NAN)), "sigma_luminance must be finite and greater than 0"),
        ("both", dict(opt=dict(short_history=NAN, sigma_normal=NAN)), "short_history must be finite and at least 0"),
        ("both", dict(opt=dict(sigma_depth=-2.0), buf=dict(normal=At("hdr"))), "sigma_depth -2: it and 1 / sigma_depth^2 must be finite and greater than 0"),
        ("device", dict(buf=dict(length=At("variance")), ws=None), "length overlaps variance" + ONLY),
    ],
    upsample=FRAME + SIGMAS + _workspace("mipt_upsample_workspace_bytes", N_LO * 32, "lo_hdr", "lo_normal", "lo_hdr") + [
        ("both", dict(buf=dict(lo_hdr=None)), "null lo_hdr"),
        ("both", dict(buf=dict(out=None)), "null out"),
        ("both", dict(opt=dict(scale=1)), "scale 1: must be 2 ... 8"),
        ("both", dict(opt=dict(scale=9)), "scale 9: must be 2 ... 8"),
        ("both", dict(opt=dict(scale=3)), "width 8 is not a multiple of scale 3"),
        ("both", dict(opt=dict(scale=8)), "height 4 is not a multiple of scale 8"),
        ("both", dict(buf=dict(lo_normal=None)), "null lo_normal: normal is given at both resolutions or at neither"),
        ("both", dict(buf=dict(material=None)), "null material: material is given at both resolutions or at neither"),
        ("both", dict(buf=dict(weight=At("out", 4))), "weight overlaps out"),
        ("both", dict(buf=dict(lo_normal=At("lo_hdr", 4))), "lo_normal overlaps lo_hdr"),
        ("both", dict(buf=dict(material=At("lo_hdr"))), "material overlaps lo_hdr"),
        ("both", dict(opt=dict(width=0), buf=dict(lo_hdr=None)), "null lo_hdr"),
        ("both", dict(opt=dict(scale=0, n_views=0)), "n_views == 0"),
        ("both", dict(opt=dict(width=65537, height=65536)), "width 65537 is not a multiple of scale 2"),
        ("both", dict(opt=dict(scale=9, **BIG)), "scale 9: must be 2 ... 8"),
        ("both", dict(opt=dict(flags=2), buf=dict(lo_depth=None)), "flags 0x2: must be 0"),
        ("both", dict(opt=dict(sigma_normal=NAN), buf=dict(lo_depth=None)), "null lo_depth: depth is given at both resolutions or at neither"),
        ("both", dict(opt=dict(sigma_depth=-2.0), buf=dict(weight=At("out"))), "sigma_depth -2: it and 1 / sigma_depth^2 must be finite and greater than 0"),
        ("device", dict(buf=dict(weight=At("out")), ws=None), "weight overlaps out"),
    ],
    sample_map=FRAME + [
        ("both", dict(buf=dict(variance=None)), "null variance"),
        ("both", dict(buf=dict(counts=None)), "null counts"),
        ("both", dict(buf=dict(hdr=None)), "null hdr: albedo is given only with hdr"),
        ("both", dict(opt=dict(max_samples=0)), "max_samples 0: must be 1 ... 65535"),
        ("both", dict(opt=dict(max_samples=65536)), "max_samples 65536: must be 1 ... 65535"),
        ("both", dict(opt=dict(min_samples=9)), "min_samples 9: must be at most max_samples 8"),
        ("both", dict(opt=dict(budget=0.5)), "budget 0.5: must be finite and in [min_samples, max_samples] = [1, 8]"),
        ("both", dict(opt=dict(budget=NAN)), "budget nan: must be finite and in [min_samples, max_samples] = [1, 8]"),
        ("both", dict(buf=dict(counts=At("variance", 4))), "counts overlaps variance"),
        ("both", dict(buf=dict(albedo=At("hdr", 4))), "albedo overlaps hdr"),
        ("both", dict(opt=dict(width=0), buf=dict(counts=None)), "null counts"),
        ("both", dict(opt=dict(width=0), buf=dict(hdr=None)), "null hdr: albedo is given only with hdr"),
        ("both", dict(opt=dict(max_samples=0), buf=dict(reserved=3)), "reserved buffer pointers must be NULL"),
        ("both", dict(opt=dict(max_samples=0, budget=NAN)), "max_samples 0: must be 1 ... 65535"),
        ("both", dict(opt=dict(max_samples=0), buf=dict(counts=At("variance"))), "max_samples 0: must be 1 ... 65535"),
        ("device", dict(ws=None), "null workspace"),
        ("device", dict(ws=At("ws", 4)), "workspace must be 16-byte aligned"),
        ("device", dict(buf=dict(variance=At("variance", 2))), "variance must be 4-byte aligned"),
        ("device", dict(buf=dict(hdr=At("ws", 28), albedo=None)), "hdr overlaps the workspace"),
        ("device", dict(buf=dict(hdr=At("ws", 32), albedo=None)), "variance is not device memory"),
        ("device", dict(), "variance is not device memory"),
        ("device", dict(ws=At("ws", 8), buf=dict(variance=At("variance", 2))), "workspace must be 16-byte aligned"),
        ("device", dict(buf=dict(variance=At("ws", 2))), "variance must be 4-byte aligned"),
        ("device", dict(buf=dict(variance=At("ws"), hdr=At("hdr", 2))), "variance overlaps the workspace"),
        ("device", dict(buf=dict(variance=At("variance", 2), hdr=At("ws"))), "variance must be 4-byte aligned"),
        ("device", dict(buf=dict(counts=At("variance")), ws=None), "counts overlaps variance"),
    ],
)
# the fill form: the same but for the planes held against the workspace, which has another size here
CASES["sample_map_fill"] = [c for c in CASES["sample_map"] if "hdr" not in (c[1].get("buf") or {}) or c[0] != "device"] + [
    ("both", dict(opt=dict(rounds=0)), "rounds 0: must be 1 ... 8"),
    ("both", dict(opt=dict(rounds=9)), "rounds 9: must be 1 ... 8"),
    ("both", dict(opt=dict(rounds=0), buf=None), "null buffers"),
    ("both", dict(opt=dict(rounds=0), buf=dict(variance=None)), "rounds 0: must be 1 ... 8"),
    ("both", dict(opt=dict(rounds=0, width=0)), "rounds 0: must be 1 ... 8"),
    ("device", dict(buf=dict(hdr=At("ws", 60), albedo=None)), "hdr overlaps the workspace"),          # two rounds: 64 bytes
    ("device", dict(buf=dict(hdr=At("ws", 28), albedo=None)), "hdr overlaps the workspace"),
    ("device", dict(opt=dict(rounds=1), buf=dict(hdr=At("ws", 32), albedo=None)), "variance is not device memory"),
]
_TEMPORAL = FRAME + [
    ("both", dict(cams=None), "null cameras"),
    ("both", dict(opt=None, cams=None), "null opt"),
    ("both", dict(buf=None, cams=None), "null cameras"),
] + [("both", dict(buf={k: None}), f"null {k}") for k in ("hdr", "position", "normal", "depth", "material", "history_out", "out")] + [
    ("both", dict(opt=dict(alpha_min=1.5)), "alpha_min 1.5: must be 0 ... 1"),
    ("both", dict(opt=dict(alpha_min=NAN)), "alpha_min nan: must be 0 ... 1"),
    ("both", dict(opt=dict(max_history=0.5)), "max_history 0.5: must be finite and at least 1"),
    ("both", dict(opt=dict(normal_tol=-1.0)), "normal_tol -1: must be finite and at least 0"),
    ("both", dict(opt=dict(depth_tol=INF)), "depth_tol inf: must be finite and at least 0"),
    ("both", dict(cams="singular"), "cameras[1].look_at is singular or not finite: it has no inverse to reproject with"),
    ("both", dict(buf=dict(position=At("hdr", 4))), "position overlaps hdr" + ONLY),
    ("both", dict(buf=dict(out=At("hdr", 4))), "out overlaps hdr" + ONLY),
    ("both", dict(buf=dict(history_out=At("history_in", 16))), "history_out overlaps history_in" + ONLY),
    ("both", dict(buf=dict(length=At("history_in", HIST - N * 4))), "length overlaps history_in" + ONLY),
    ("both", dict(opt=dict(width=0), buf=dict(material=None)), "null material"),
    ("both", dict(buf=dict(hdr=None, out=None)), "null hdr"),
    ("both", dict(opt=dict(flags=1, alpha_min=2.0)), "flags 0x1: must be 0"),
    ("both", dict(opt=dict(alpha_min=2.0, reserved=0)), "alpha_min 2: must be 0 ... 1"),
    ("both", dict(opt=dict(depth_tol=NAN, reserved=0)), "depth_tol nan: must be finite and at least 0"),
    ("both", dict(opt=dict(max_history=0.0, normal_tol=NAN)), "max_history 0: must be finite and at least 1"),
    ("both", dict(opt=dict(alpha_min=2.0), buf=dict(position=At("hdr"))), "alpha_min 2: must be 0 ... 1"),
    ("both", dict(cams="singular", buf=dict(position=At("hdr"))), "cameras[1].look_at is singular or not finite: it has no inverse to reproject with"),
    ("both", dict(cams="singular", buf=dict(reserved=4)), "reserved buffer pointers must be NULL"),
    ("device", dict(buf=dict(hdr=At("hdr", 2))), "hdr must be 4-byte aligned"),
    ("device", dict(buf=dict(material=At("material", 1))), "material must be 4-byte aligned"),
    ("device", dict(buf=dict(history_in=At("history_in", 4))), "history_in must be 16-byte aligned"),
    ("device", dict(buf=dict(history_out=At("history_out", 8))), "history_out must be 16-byte aligned"),
    ("device", dict(), "hdr is not device memory"),
    ("device", dict(buf=dict(albedo=None, history_in=None, length=None, variance=None)), "hdr is not device memory"),
    ("device", dict(buf=dict(history_in=At("history_in", 4), depth=At("depth", 2))), "depth must be 4-byte aligned"),
    ("device", dict(buf=dict(history_in=At("history_in", 4), variance=At("variance", 2))), "history_in must be 16-byte aligned"),
    ("device", dict(buf=dict(hdr=At("hdr", 2), position=At("hdr", 6))), "position overlaps hdr" + ONLY),
]
CASES["temporal"] = _TEMPORAL
CASES["temporal_counts"] = _TEMPORAL + [
    ("both", dict(counts=None), "null counts"),
    ("both", dict(cap=0), "samples_cap 0: must be 1 ... 65535"),
    ("both", dict(cap=65536), "samples_cap 65536: must be 1 ... 65535"),
    ("both", dict(counts=None, cams="singular"), "null counts"),
    ("both", dict(counts=None, cap=0), "null counts"),
    ("both", dict(counts=None, buf=dict(reserved=0)), "reserved buffer pointers must be NULL"),
    ("both", dict(cap=0, buf=dict(position=At("hdr"))), "samples_cap 0: must be 1 ... 65535"),
    ("device", dict(counts=At("counts", 2)), "counts must be 4-byte aligned"),
    ("device", dict(counts=At("hdr", 4)), "counts overlaps hdr"),
    ("device", dict(counts=At("history_out", HIST - N * 4)), "counts overlaps history_out"),
    ("device", dict(counts=At("counts", 2), buf=dict(hdr=At("hdr", 2))), "counts must be 4-byte aligned"),
    ("device", dict(counts=At("hdr", 2)), "counts must be 4-byte aligned"),
    ("device", dict(counts=At("depth"), buf=dict(hdr=At("hdr", 2))), "counts overlaps depth"),
    ("device", dict(counts=At("depth"), cams="singular"), "cameras[1].look_at is singular or not finite: it has no inverse to reproject with"),
    ("device", dict(counts=At("depth"), buf=dict(position=At("hdr"))), "position overlaps hdr" + ONLY),
]


@pytest.fixture(scope="module")
def families(rrt):
    from rust_ray_tracing_amd import _lib as L
    return rrt.load(), L, _families(L)


@pytest.mark.parametrize("family", sorted(CASES))
def test_every_refusal_has_its_code_and_its_whole_message(families, family):
    lib, L, fams = families
    fam = fams[family]
    seen = 0
    for where, kw, text in CASES[family]:
        for device in (False, True):
            if where != ("device" if device else "host") and where != "both":
                continue
            who = fam.device if device else fam.host
            rc, msg = fam.call(lib, L, device, **kw)
            assert (rc, msg) == (L.ERR_INVALID_ARG, f"{who}: {text}"), (who, kw)
            seen += 1
    assert seen >= len(CASES[family])


@pytest.mark.parametrize("family", sorted(CASES))
def test_the_host_entry_names_the_device_it_could_not_select(families, family):
    """the one refusal of a host entry that is HIP's: its text for an ordinal that does not exist, after our own"""
    lib, L, fams = families
    fam = fams[family]
    rc, msg = fam.call(lib, L, False, device_id=NO_DEVICE)
    assert rc == L.ERR_HIP
    assert msg in [f"{fam.host}: hipSetDevice(device_id = {NO_DEVICE}) failed: {t}" for t in HIP_TEXTS], msg
    # any of our own checks comes first
    rc, msg = fam.call(lib, L, False, device_id=NO_DEVICE, opt=dict(flags=1))
    assert (rc, msg) == (L.ERR_INVALID_ARG, f"{fam.host}: flags 0x1: must be 0")


def test_no_plane_was_written(families):
    """runs last: whatever the cases above handed to the library is still zero"""
    assert len(_arrays) > 50
    for a in _arrays:
        assert not a.any()
