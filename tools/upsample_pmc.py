"""Driver for a counter run over the guided upsampling: a few mipt_upsample_device calls at 1920x1080 on
synthetic planes, nothing else on the device, so that a profiler's per-kernel counters belong to upsample_pack_kernel and
upsample_kernel alone.  The planes are made so that every tap takes part and is weighted (one material, smooth normals and depths):
the most loads the kernel can issue.  Counters are collected in runs of their own, one group per run, e.g.

    rocprofv3 --pmc TCP_TOTAL_CACHE_ACCESSES_sum TCP_TCC_READ_REQ_sum --output-format csv -d out/l1 -- python tools/upsample_pmc.py
    rocprofv3 --pmc TCC_HIT_sum TCC_MISS_sum TCC_EA0_RDREQ_sum --output-format csv -d out/l2 -- python tools/upsample_pmc.py

    python tools/upsample_pmc.py [--scale 2] [--calls 3]
"""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--scale", type=int, default=2)
    ap.add_argument("--calls", type=int, default=3)
    args = ap.parse_args()

    import torch

    import rust_ray_tracing_amd as rrt
    from rust_ray_tracing_amd import _lib as L

    if not torch.cuda.is_available():
        raise SystemExit("upsample_pmc.py runs on an MI355X: no HIP device visible")
    lib = rrt.load()
    dev = torch.device("cuda:0")
    w, h, k = args.width, args.height, args.scale
    lw, lh = w // k, h // k
    g = torch.Generator(device=dev).manual_seed(1)

    def planes(ww, hh):
        n = torch.tensor([0.0, 0.0, 1.0], device=dev) + 0.05 * torch.randn((1, hh, ww, 3), generator=g, device=dev)
        return dict(normal=n.contiguous(), depth=2.0 + 0.1 * torch.rand((1, hh, ww), generator=g, device=dev),
                    albedo=0.1 + 0.9 * torch.rand((1, hh, ww, 3), generator=g, device=dev), material=torch.zeros((1, hh, ww), dtype=torch.int32, device=dev))

    lo, hi = planes(lw, lh), planes(w, h)
    keep = dict(lo_hdr=torch.rand((1, lh, lw, 3), generator=g, device=dev), out=torch.empty((1, h, w, 3), device=dev), weight=torch.empty((1, h, w), device=dev))
    for name in lo:
        keep["lo_" + name], keep[name] = lo[name], hi[name]
    need = int(lib.mipt_upsample_workspace_bytes(w, h, 1, k))
    workspace = torch.empty((need // 16, 4), dtype=torch.float32, device=dev)
    o = L.MiptUpsampleOptions()
    o.width, o.height, o.n_views, o.scale, o.sigma_normal, o.sigma_depth = w, h, 1, k, 0.5, 0.5
    b = L.MiptUpsampleBuffers()
    for name, t in keep.items():
        setattr(b, name, t.data_ptr())
    torch.cuda.synchronize()
    for _ in range(args.calls):
        L.check(lib.mipt_upsample_device(C.byref(o), C.byref(b), C.c_void_p(workspace.data_ptr()), need, None), "mipt_upsample_device")
        torch.cuda.synchronize()
    print(f"{args.calls} calls, {w}x{h} from {lw}x{lh}, pixels without an accepted tap: {int((keep['weight'] == 0).sum().item())}")


if __name__ == "__main__":
    main()
