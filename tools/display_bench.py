#!/usr/bin/env python3
"""Measure mi_display_picture at 4K10 4:2:0 (GPU): to P010, planar RGB and packed RGBA, with and
without film grain, each beside a hipMemcpyAsync device-to-device copy that moves the same
number of bytes (a copy of n bytes reads n and writes n, so n = (read + write) / 2), timed in the
same run with HIP events around `--iters` back-to-back calls after `--warmup` calls.

Reported per case: microseconds per call, the algorithmic bytes (1.5 W H B read, W H B times
1.5 / 3 / 4 written; with grain, the grain pass's 1.5 W H B read and written on top), the copy's
microseconds for those bytes, and the call's rate as a fraction of the copy's.

    python tools/display_bench.py [--out profiles/display_bench.json] [--width 3840 --height 2160]
"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "display_bench.json"))
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--bpc", type=int, default=10)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()

    import numpy as np
    import torch

    from rav1d_amd.av1dec import MiColorInfo
    from rav1d_amd import lib
    from rav1d_amd.display import DisplayImage
    from rav1d_amd.frame import Context, Frame, film_grain_data
    from rav1d_amd.synth import make_fg_params

    if not torch.cuda.is_available():
        sys.exit("display_bench needs a GPU: nothing is measured without one")
    L = lib()
    hip = L      # (dlsym on the library's handle reaches the HIP runtime it is linked with)
    hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    D2D = 3

    w, h, bpc, layout = args.width, args.height, args.bpc, 1
    pxb = 1 if bpc == 8 else 2
    rng = np.random.default_rng(0)
    ctx = Context(0)
    src = Frame(w, h, bpc, layout)
    for p in range(3):
        pw, ph = src.dims(p)
        src.set_plane_np(p, rng.integers(0, 1 << bpc, (ph, pw)))
    fg = film_grain_data(make_fg_params(rng, layout))
    color = MiColorInfo(1, 1, 1, 0, 0)      # BT.709, limited range, centred chroma
    stream = torch.cuda.current_stream()
    sp = ctypes.c_void_p(stream.cuda_stream)

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

    whb = w * h * pxb
    results = []
    for fmt, out_factor in (("nv12", 1.5), ("rgb", 3.0), ("rgba", 4.0)):
        image = DisplayImage(w, h, bpc, layout, fmt)
        for grain in (False, True):
            nbytes = int((1.5 + out_factor) * whb + (3.0 * whb if grain else 0))
            n = nbytes // 2
            a, b = torch.empty(n, dtype=torch.uint8, device="cuda"), torch.empty(n, dtype=torch.uint8, device="cuda")

            def copy():
                if hip.hipMemcpyAsync(a.data_ptr(), b.data_ptr(), n, D2D, sp) != 0:
                    raise RuntimeError("hipMemcpyAsync failed")

            # the C entry directly, on prebuilt arguments: the host side of a call stays well
            # below the device time, so the events time the device
            pic, im = src.picture(), image.image()
            argv = (ctx.h, ctypes.byref(pic), ctypes.byref(im), ctypes.byref(color),
                    ctypes.byref(fg) if grain else None, sp)

            def call(argv=argv):
                if L.mi_display_picture(*argv) != 0:
                    raise RuntimeError("mi_display_picture failed")

            # copy, call, copy: the copy on both sides of the call, in the same run
            c0, _ = timed(copy)
            us, rounds = timed(call)
            c1, _ = timed(copy)
            cus = (c0 + c1) / 2
            results.append(dict(format=fmt, grain=grain, us=round(us, 2), rounds_us=rounds, bytes=nbytes,
                                gbps=round(nbytes / us / 1e3, 1), copy_us=round(cus, 2),
                                copy_gbps=round(nbytes / cus / 1e3, 1), fraction_of_copy=round(cus / us, 3)))
            print(json.dumps(results[-1]), flush=True)
    doc = dict(tool="tools/display_bench.py", device=torch.cuda.get_device_name(0), width=w, height=h, bpc=bpc,
               layout="4:2:0", iters=args.iters, warmup=args.warmup, rounds=args.rounds,
               timing="HIP events around back-to-back calls; median of rounds", results=results)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
