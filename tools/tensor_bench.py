#!/usr/bin/env python3
"""Measure mi_display_tensor at 4K10 4:2:0 -> 224 x 224 float16 CHW (GPU), beside the route it
replaces, in the same run, with HIP events around `--iters` back-to-back calls after `--warmup`
calls (median of `--rounds` rounds):

  tensor        mi_display_tensor: resident picture -> normalised float16 (3, 224, 224);
  rgb_planar    mi_display_picture MI_OUT_RGB_PLANAR of the same picture (the first step of the
                replaced route, on its own);
  replaced      that call, then torch.nn.functional.interpolate(mode="bilinear", antialias=True) in
                float32 and the normalisation in torch, to the same float16 tensor.

The calls rotate over `--pictures` resident source pictures (12 x 24.9 MB by default, more than the
256 MiB Infinity Cache), so every call's source planes come from HBM, for the three cases alike.
Reported per case: microseconds per call; for the tensor path also the source bytes (1.5 W H B,
the floor of a pass that reads the planes once) and the fraction of the HBM peak they imply at
that time. The replaced route's result is not the same tensor: torch's filter is the same triangle
in float, but it drops the taps outside the picture where mi_display_tensor repeats the edge
sample. The largest difference is reported over the whole tensor and over its interior (without
the outermost output row and column on each side, the only ones whose taps leave the picture);
neither is asserted.

--filter NAME (triangle, catmull_rom, mitchell, cubic_075: rav1d_amd.display.Resample's presets)
measures mi_display_tensor_rs with that filter in place of mi_display_tensor; the replaced route
then interpolates with mode="bicubic" for the cubics. Without it the call is mi_display_tensor.

    python tools/tensor_bench.py [--out profiles/tensor_bench.json] [--width 3840 --height 2160]
                                 [--filter catmull_rom]
"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0      # MI355X HBM3E, specification


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tensor_bench.json"))
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--bpc", type=int, default=10)
    ap.add_argument("--size", type=int, nargs=2, default=(224, 224), metavar=("W", "H"))
    ap.add_argument("--pictures", type=int, default=12)
    ap.add_argument("--iters", type=int, default=120)
    ap.add_argument("--warmup", type=int, default=24)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--filter", default=None, choices=["triangle", "catmull_rom", "mitchell", "cubic_075"],
                    help="resize through mi_display_tensor_rs with this filter (default: mi_display_tensor)")
    args = ap.parse_args()

    import numpy as np
    import torch
    import torch.nn.functional as F

    from rav1d_amd import lib
    from rav1d_amd.av1dec import MiColorInfo
    from rav1d_amd.display import DisplayImage, Resample, tensor_image
    from rav1d_amd.frame import Context, Frame

    if not torch.cuda.is_available():
        sys.exit("tensor_bench needs a GPU: nothing is measured without one")
    L = lib()
    w, h, bpc, layout = args.width, args.height, args.bpc, 1
    ow, oh = args.size
    pxb = 1 if bpc == 8 else 2
    m = float((1 << bpc) - 1)
    mean, std = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
    rng = np.random.default_rng(0)
    ctx = Context(0)
    sources = []
    for _ in range(args.pictures):
        src = Frame(w, h, bpc, layout)
        for p in range(3):
            pw, ph = src.dims(p)
            src.set_plane_np(p, rng.integers(0, 1 << bpc, (ph, pw)))
        sources.append(src)
    color = MiColorInfo(1, 1, 1, 0, 0)      # BT.709, limited range, centred chroma
    stream = torch.cuda.current_stream()
    sp = ctypes.c_void_p(stream.cuda_stream)

    out = torch.empty((3, oh, ow), dtype=torch.float16, device="cuda")
    tim = tensor_image(out, bpc, None, mean, std)
    image = DisplayImage(w, h, bpc, layout, "rgb")
    dim = image.image()
    pics = [s.picture() for s in sources]
    # the C entries directly, on prebuilt arguments: the host side of a call stays well below the
    # device time, so the events time the device
    targs = [(ctx.h, ctypes.byref(p), ctypes.byref(tim), ctypes.byref(color), None, sp) for p in pics]
    rs = Resample(args.filter) if args.filter else None
    rargs = [(ctx.h, ctypes.byref(p), ctypes.byref(tim), ctypes.byref(color), None, ctypes.byref(rs), None, sp)
             for p in pics] if rs is not None else None
    mode = "bilinear" if args.filter in (None, "triangle") else "bicubic"
    dargs = [(ctx.h, ctypes.byref(p), ctypes.byref(dim), ctypes.byref(color), None, sp) for p in pics]
    mean_t = torch.tensor(mean, dtype=torch.float32, device="cuda").view(3, 1, 1)
    std_t = torch.tensor(std, dtype=torch.float32, device="cuda").view(3, 1, 1)
    old = torch.empty((3, oh, ow), dtype=torch.float16, device="cuda")
    state = dict(k=0)

    def next_k():
        state["k"] = (state["k"] + 1) % len(pics)
        return state["k"]

    def tensor():
        if rargs is not None:
            if L.mi_display_tensor_rs(*rargs[next_k()]) != 0:
                raise RuntimeError("mi_display_tensor_rs failed")
        elif L.mi_display_tensor(*targs[next_k()]) != 0:
            raise RuntimeError("mi_display_tensor failed")

    def rgb_planar():
        if L.mi_display_picture(*dargs[next_k()]) != 0:
            raise RuntimeError("mi_display_picture failed")

    def replaced():
        rgb_planar()
        # (the 16-bit words are held in int16 storage; 10-bit samples are below 2^15)
        x = image.rgb.to(torch.float32).unsqueeze(0)
        y = F.interpolate(x, size=(oh, ow), mode=mode, antialias=True, align_corners=False)[0]
        old.copy_((y / m - mean_t) / std_t)

    def timed(fn):
        """Median over rounds of the mean microseconds of `iters` back-to-back calls."""
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        us = []
        for _ in range(args.rounds):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            for _ in range(args.iters):
                fn()
            b.record(stream)
            b.synchronize()
            us.append(a.elapsed_time(b) * 1e3 / args.iters)
        return float(np.median(us)), [round(v, 2) for v in us]

    # same picture through both routes, for the difference of the results
    state["k"] = -1
    tensor()
    state["k"] = -1
    replaced()
    torch.cuda.synchronize()
    delta = (out.float() - old.float()).abs()
    diff, diff_interior = float(delta.max()), float(delta[:, 1:-1, 1:-1].max())

    # alternate the cases, the new path on both sides of the replaced route
    results = {}
    order = [("tensor", tensor), ("rgb_planar", rgb_planar), ("replaced", replaced), ("tensor_again", tensor)]
    for name, fn in order:
        us, rounds = timed(fn)
        results[name] = dict(us=round(us, 2), rounds_us=rounds)
        print(json.dumps({name: results[name]}), flush=True)
    src_bytes = int(1.5 * w * h * pxb)
    t_us = (results["tensor"]["us"] + results["tensor_again"]["us"]) / 2
    doc = dict(tool="tools/tensor_bench.py", device=torch.cuda.get_device_name(0), width=w, height=h, bpc=bpc,
               layout="4:2:0", out_w=ow, out_h=oh, dtype="float16", order="CHW", filter=args.filter, pictures=args.pictures,
               iters=args.iters, warmup=args.warmup, rounds=args.rounds,
               timing="HIP events around back-to-back calls rotating over the source pictures; median of rounds",
               results=results, tensor_us=round(t_us, 2), source_bytes=src_bytes,
               tensor_source_gbps=round(src_bytes / t_us / 1e3, 1), hbm_peak_gbps=HBM_PEAK_GBS,
               tensor_fraction_of_hbm_peak=round(src_bytes / t_us / 1e3 / HBM_PEAK_GBS, 4),
               speedup_over_replaced=round(results["replaced"]["us"] / t_us, 2),
               max_abs_difference_of_results=diff, max_abs_difference_interior=diff_interior)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps({k: doc[k] for k in ("tensor_us", "tensor_source_gbps", "tensor_fraction_of_hbm_peak",
                                          "speedup_over_replaced", "max_abs_difference_of_results",
                                          "max_abs_difference_interior")}))
    print("wrote", args.out)


if __name__ == "__main__":
    main()
