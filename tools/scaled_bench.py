#!/usr/bin/env python3
"""Measure mi_display_scaled at 4K10 4:2:0 (GPU), beside the two existing output paths on the same
pictures in the same run, with HIP events around `--iters` back-to-back calls after `--warmup`
calls (median of `--rounds` rounds; every round's figure is kept, so the spread is visible):

  scaled_p010        (a) -> 1920 x 1080, 10 bits (P010);
  scaled_nv12        (b) -> 1920 x 1080, 8 bits (NV12);
  ladder             (c) 1920 x 1080, 1280 x 720 and 640 x 360 at 8 bits in one call;
  ladder_3_calls     (c) the same three rungs as three calls;
  tensor_u8_chw      mi_display_tensor writing uint8 CHW at 1920 x 1080: the project's other resize;
  picture_1to1       mi_display_picture MI_OUT_SEMIPLANAR 1:1 (P010): the existing YUV output.

The cases alternate, the two that are compared most closely (scaled_nv12, tensor_u8_chw) on both
sides of the others. The calls rotate over `--pictures` resident source pictures (12 x 24.9 MB by
default, more than the 256 MiB Infinity Cache), so every call's source planes come from HBM.
Reported per case: microseconds per call, and for the scaled cases the bytes a pass that reads the
source once and writes the rungs once would move, with the rate they imply at that time.

--filter NAME (triangle, catmull_rom, mitchell, cubic_075: rav1d_amd.display.Resample's presets)
measures mi_display_scaled_rs and mi_display_tensor_rs with that filter in place of
mi_display_scaled and mi_display_tensor. Without it the calls are those two.

    python tools/scaled_bench.py [--out profiles/scaled_bench.json] [--width 3840 --height 2160]
                                 [--filter mitchell]
"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0      # MI355X HBM3E, specification
LADDER = [(1920, 1080), (1280, 720), (640, 360)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scaled_bench.json"))
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--bpc", type=int, default=10)
    ap.add_argument("--pictures", type=int, default=12)
    ap.add_argument("--iters", type=int, default=120)
    ap.add_argument("--warmup", type=int, default=24)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--only", default=None, help="run one case without writing --out (for a kernel trace)")
    ap.add_argument("--filter", default=None, choices=["triangle", "catmull_rom", "mitchell", "cubic_075"],
                    help="resize through the _rs entries with this filter (default: the entries without one)")
    args = ap.parse_args()

    import numpy as np
    import torch

    from rav1d_amd import lib
    from rav1d_amd.av1dec import MiColorInfo
    from rav1d_amd.display import DisplayImage, MiScaledImage, Resample, ScaledImage, tensor_image
    from rav1d_amd.frame import Context, Frame

    if not torch.cuda.is_available():
        sys.exit("scaled_bench needs a GPU: nothing is measured without one")
    L = lib()
    w, h, bpc, layout = args.width, args.height, args.bpc, 1
    pxb = 1 if bpc == 8 else 2
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
    pics = [s.picture() for s in sources]
    state = dict(k=0)
    rs = Resample(args.filter) if args.filter else None

    def scaled_entry(pic, ims, n):
        if rs is not None:
            return L.mi_display_scaled_rs(ctx.h, pic, ims, n, ctypes.byref(color), ctypes.byref(rs), None, sp)
        return L.mi_display_scaled(ctx.h, pic, ims, n, ctypes.byref(color), None, sp)

    def next_pic():
        state["k"] = (state["k"] + 1) % len(pics)
        return ctypes.byref(pics[state["k"]])

    def rungs(sizes, obpc):
        images = [ScaledImage(W, H, obpc, layout) for W, H in sizes]
        return images, (MiScaledImage * len(images))(*[im.image() for im in images])

    keep = []

    def scaled(sizes, obpc, one_call=True):
        images, ims = rungs(sizes, obpc)
        keep.append(images)
        singles = [(MiScaledImage * 1)(ims[i]) for i in range(len(images))]

        def fn():
            pic = next_pic()
            if one_call:
                if scaled_entry(pic, ims, len(images)) != 0:
                    raise RuntimeError("mi_display_scaled failed")
            else:
                for one in singles:
                    if scaled_entry(pic, one, 1) != 0:
                        raise RuntimeError("mi_display_scaled failed")
        out_bytes = sum(int(1.5 * W * H) * (1 if obpc == 8 else 2) for W, H in sizes)
        return fn, out_bytes

    out_t = torch.empty((3, LADDER[0][1], LADDER[0][0]), dtype=torch.uint8, device="cuda")
    tim = tensor_image(out_t, bpc)
    image = DisplayImage(w, h, bpc, layout, "nv12")
    dim = image.image()

    def tensor():
        if rs is not None:
            if L.mi_display_tensor_rs(ctx.h, next_pic(), ctypes.byref(tim), ctypes.byref(color), None, ctypes.byref(rs), None, sp) != 0:
                raise RuntimeError("mi_display_tensor_rs failed")
        elif L.mi_display_tensor(ctx.h, next_pic(), ctypes.byref(tim), ctypes.byref(color), None, sp) != 0:
            raise RuntimeError("mi_display_tensor failed")

    def picture():
        if L.mi_display_picture(ctx.h, next_pic(), ctypes.byref(dim), ctypes.byref(color), None, sp) != 0:
            raise RuntimeError("mi_display_picture failed")

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

    p010, p010_bytes = scaled(LADDER[:1], 10)
    nv12, nv12_bytes = scaled(LADDER[:1], 8)
    ladder, ladder_bytes = scaled(LADDER, 8)
    ladder3, _ = scaled(LADDER, 8, one_call=False)
    cases = dict(scaled_nv12=nv12, tensor_u8_chw=tensor, scaled_p010=p010, picture_1to1=picture, ladder=ladder,
                 ladder_3_calls=ladder3)
    if args.only:
        us, rounds = timed(cases[args.only])
        print(json.dumps({args.only: dict(us=round(us, 2), rounds_us=rounds)}))
        return
    order = ["scaled_nv12", "tensor_u8_chw", "scaled_p010", "picture_1to1", "ladder", "ladder_3_calls", "tensor_u8_chw",
             "scaled_nv12"]
    results = {}
    for name in order:
        us, rounds = timed(cases[name])
        key = name if name not in results else name + "_again"
        results[key] = dict(us=round(us, 2), rounds_us=rounds)
        print(json.dumps({key: results[key]}), flush=True)
    src_bytes = int(1.5 * w * h * pxb)

    def mean2(name):
        return (results[name]["us"] + results[name + "_again"]["us"]) / 2

    def traffic(us, out_bytes, reads=1):
        moved = reads * src_bytes + out_bytes
        return dict(bytes=moved, gbps=round(moved / us / 1e3, 1), fraction_of_hbm_peak=round(moved / us / 1e3 / HBM_PEAK_GBS, 4))

    nv12_us, tensor_us = mean2("scaled_nv12"), mean2("tensor_u8_chw")
    doc = dict(tool="tools/scaled_bench.py", device=torch.cuda.get_device_name(0), width=w, height=h, bpc=bpc,
               layout="4:2:0", ladder=LADDER, filter=args.filter, pictures=args.pictures, iters=args.iters, warmup=args.warmup,
               rounds=args.rounds,
               timing="HIP events around back-to-back calls rotating over the source pictures; median of rounds",
               results=results, source_bytes=src_bytes, hbm_peak_gbps=HBM_PEAK_GBS,
               scaled_nv12_us=round(nv12_us, 2), tensor_u8_chw_us=round(tensor_us, 2),
               scaled_nv12_over_tensor=round(nv12_us / tensor_us, 3),
               scaled_nv12_over_picture_1to1=round(nv12_us / results["picture_1to1"]["us"], 3),
               ladder_over_3_calls=round(results["ladder"]["us"] / results["ladder_3_calls"]["us"], 3),
               minimum_traffic=dict(scaled_nv12=traffic(nv12_us, nv12_bytes),
                                    scaled_p010=traffic(results["scaled_p010"]["us"], p010_bytes),
                                    ladder=traffic(results["ladder"]["us"], ladder_bytes)))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps({k: doc[k] for k in ("scaled_nv12_us", "tensor_u8_chw_us", "scaled_nv12_over_tensor",
                                          "scaled_nv12_over_picture_1to1", "ladder_over_3_calls")}))
    print("wrote", args.out)


if __name__ == "__main__":
    main()
