#!/usr/bin/env python3
"""Measure the colour-volume stage (mi_display_picture_tm, mi_display_tensor_tm) on a resident 4K10
4:2:0 picture (GPU), each tone-mapped path beside the plain path it extends, timed in the same run
with HIP events around `--iters` back-to-back calls after `--warmup` calls, the plain path on both
sides of the tone-mapped one:

  rgba10           mi_display_picture, packed RGBA at 10 bits (no stage);
  rgba8_tm         mi_display_picture_tm, PQ / BT.2020 -> sRGB / BT.709, packed RGBA at 8 bits;
  rgba10_tm        the same to 10 bits: the bytes of rgba10, so the difference is the stage alone;
  tensor           mi_display_tensor to float16 CHW at --size;
  tensor_tm        mi_display_tensor_tm, the same tone map at 8 bits, to the same tensor.

The planes hold uniformly random codes, so the table gathers have no locality beyond the tables'
size: decoded pictures are smoother. No threshold is asserted; the ratios are recorded.

    python tools/tonemap_bench.py [--out profiles/tonemap_bench.json] [--note TEXT]

With --yuv the run measures the tone-mapped YUV outputs instead (mi_display_yuv_tm,
mi_display_scaled_tm: the same source to 8-bit NV12, BT.709 limited), each row between two takes of
the existing call it stands beside, into profiles/yuv_tm_bench.json by default:

  rgb8_tm          mi_display_picture_tm, planar R'G'B' at 8 bits: reads what the Q kernel reads;
  nv12_tm          mi_display_yuv_tm at the source's size;
  nv12_tm_chr2     the same with co-located chroma (chr 2: the decimation reads the row above too);
  scaled_1080      plain mi_display_scaled, one 1920 x 1080 8-bit rung (no tone map);
  scaled_1080_tm   mi_display_scaled_tm, the same rung;
  ladder           plain mi_display_scaled, 1920 x 1080, 1280 x 720 and 640 x 360 in one call;
  ladder_tm        mi_display_scaled_tm, the same three rungs.

With --hlg the run measures HLG sources (the same picture read as trc 18 on a context with
rav1d_amd.display.enable_hlg, rendered for the tone map's dst_peak), each row between two takes of
its PQ counterpart, into profiles/hlg_bench.json by default; the ratios HLG / PQ are recorded:

  rgba8_hlg        mi_display_picture_tm beside rgba8_tm;
  tensor_hlg       mi_display_tensor_tm beside tensor_tm;
  nv12_hlg         mi_display_yuv_tm beside nv12_tm.

--fold FILE... (with --hlg) folds earlier outputs of this tool into the document: runs of the
existing rows on the library before a change and on the one after it, alternating in one session,
told apart by --note ("parent#1", "change#1", "parent#2", ...). Per row it records every value, the
spread the parent's runs show between themselves, and whether every run of the change lies within
that spread of the parent's range.

A variant build of the library (MI_BUILD_VARIANT of rav1d_amd/build.py, loaded with MI_LIB) is
measured by the same command with another --out; --note says which it was.
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
    ap.add_argument("--out", default=None, help="default: profiles/tonemap_bench.json, with --yuv profiles/yuv_tm_bench.json, "
                    "with --hlg profiles/hlg_bench.json")
    ap.add_argument("--yuv", action="store_true", help="measure the tone-mapped YUV outputs and their baselines")
    ap.add_argument("--hlg", action="store_true", help="measure HLG sources, each row between two takes of its PQ counterpart")
    ap.add_argument("--fold", nargs="*", default=[], metavar="FILE", help="with --hlg: earlier outputs of this tool (parent#n / "
                    "change#n notes) to fold into the document")
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--bpc", type=int, default=10)
    ap.add_argument("--size", type=int, nargs=2, default=(224, 224), metavar=("W", "H"))
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--note", default="")
    args = ap.parse_args()
    if args.yuv and args.hlg:
        sys.exit("--yuv and --hlg are two runs")
    if args.out is None:
        name = "yuv_tm_bench.json" if args.yuv else "hlg_bench.json" if args.hlg else "tonemap_bench.json"
        args.out = os.path.join(ROOT, "profiles", name)

    import numpy as np
    import torch

    from rav1d_amd import LIB_PATH, lib
    from rav1d_amd.av1dec import MiColorInfo
    from rav1d_amd.display import DisplayImage, ToneMap, tensor_image
    from rav1d_amd.frame import Context, Frame

    if not torch.cuda.is_available():
        sys.exit("tonemap_bench needs a GPU: nothing is measured without one")
    L = lib()
    w, h, bpc, layout = args.width, args.height, args.bpc, 1
    ow, oh = args.size
    rng = np.random.default_rng(0)
    ctx = Context(0)
    src = Frame(w, h, bpc, layout)
    for p in range(3):
        pw, ph = src.dims(p)
        src.set_plane_np(p, rng.integers(0, 1 << bpc, (ph, pw)))
    color = MiColorInfo(9, 16, 9, 0, 0)      # HDR10: BT.2020 primaries and matrix, PQ, limited range
    tm8, tm10 = ToneMap(1, 13, 8, 1000.0, 100.0), ToneMap(1, 13, 10, 1000.0, 100.0)
    stream = torch.cuda.current_stream()
    sp = ctypes.c_void_p(stream.cuda_stream)
    pic = src.picture()
    mean, std = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)

    im10, im8 = DisplayImage(w, h, bpc, layout, "rgba"), DisplayImage(w, h, bpc, layout, "rgba", out_bpc=8)
    im10t = DisplayImage(w, h, bpc, layout, "rgba", out_bpc=10)
    d10, d8, d10t = im10.image(), im8.image(), im10t.image()
    out = torch.empty((3, oh, ow), dtype=torch.float16, device="cuda")
    out_t = torch.empty((3, oh, ow), dtype=torch.float16, device="cuda")
    t_plain, t_tm = tensor_image(out, bpc, None, mean, std), tensor_image(out_t, 8, None, mean, std)
    # the C entries directly, on prebuilt arguments: the host side of a call stays well below the
    # device time, so the events time the device
    ref = ctypes.byref

    def entry(fn, *argv):
        def run():
            if fn(*argv) != 0:
                raise RuntimeError(f"{fn.__name__} failed")
        return run

    cases = {
        "rgba10": entry(L.mi_display_picture, ctx.h, ref(pic), ref(d10), ref(color), None, sp),
        "rgba8_tm": entry(L.mi_display_picture_tm, ctx.h, ref(pic), ref(d8), ref(color), ref(tm8), None, sp),
        "rgba10_tm": entry(L.mi_display_picture_tm, ctx.h, ref(pic), ref(d10t), ref(color), ref(tm10), None, sp),
        "tensor": entry(L.mi_display_tensor, ctx.h, ref(pic), ref(t_plain), ref(color), None, sp),
        "tensor_tm": entry(L.mi_display_tensor_tm, ctx.h, ref(pic), ref(t_tm), ref(color), ref(tm8), None, sp),
    }

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

    if args.yuv:
        return yuv_rows(args, L, ctx, pic, color, tm8, sp, timed, entry, (w, h, bpc, layout))
    if args.hlg:
        return hlg_rows(args, L, ctx, pic, color, tm8, sp, timed, entry, (w, h, bpc, layout), cases, t_tm)

    results = {}
    order = ["rgba10", "rgba8_tm", "rgba10_tm", "rgba10", "tensor", "tensor_tm", "tensor"]
    for name in order:
        us, rounds = timed(cases[name])
        key = name if name not in results else name + "_again"
        results[key] = dict(us=round(us, 2), rounds_us=rounds)
        print(json.dumps({key: results[key]}), flush=True)
    plain = (results["rgba10"]["us"] + results["rgba10_again"]["us"]) / 2
    tplain = (results["tensor"]["us"] + results["tensor_again"]["us"]) / 2
    doc = dict(tool="tools/tonemap_bench.py", device=torch.cuda.get_device_name(0), library=os.path.basename(LIB_PATH),
               note=args.note, width=w, height=h, bpc=bpc, layout="4:2:0", out_w=ow, out_h=oh,
               source="PQ / BT.2020 (pri 9, trc 16, mtrx 9, limited), uniformly random codes",
               tonemap="to sRGB / BT.709, src_peak 1000, dst_peak 100", iters=args.iters, warmup=args.warmup,
               rounds=args.rounds, timing="HIP events around back-to-back calls; median of rounds", results=results,
               rgba10_us=round(plain, 2), tensor_us=round(tplain, 2),
               ratio_rgba8_tm_to_rgba10=round(results["rgba8_tm"]["us"] / plain, 3),
               ratio_rgba10_tm_to_rgba10=round(results["rgba10_tm"]["us"] / plain, 3),
               ratio_tensor_tm_to_tensor=round(results["tensor_tm"]["us"] / tplain, 3))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps({k: doc[k] for k in ("rgba10_us", "tensor_us", "ratio_rgba8_tm_to_rgba10", "ratio_rgba10_tm_to_rgba10",
                                          "ratio_tensor_tm_to_tensor")}))
    print("wrote", args.out)


def yuv_rows(args, L, ctx, pic, color, tm8, sp, timed, entry, geom):
    """The --yuv run, on main's source picture, context and timer: the three tone-mapped YUV rows,
    each between two takes of its baseline."""
    import torch

    from rav1d_amd import LIB_PATH
    from rav1d_amd.display import DisplayImage, MiScaledImage, ScaledImage, YuvTarget
    w, h, bpc, layout = geom
    ref = ctypes.byref
    target = YuvTarget(1, 0)
    color2 = type(color)(color.pri, color.trc, color.mtrx, color.range, 2)
    rgb8 = DisplayImage(w, h, bpc, layout, "rgb", out_bpc=8)
    nv12 = DisplayImage(w, h, bpc, layout, "nv12", out_bpc=8)
    d_rgb8, d_nv12 = rgb8.image(), nv12.image()
    sizes = [(1920, 1080), (1280, 720), (640, 360)]
    plain = [ScaledImage(W, H, 8, layout) for W, H in sizes]
    mapped = [ScaledImage(W, H, 8, layout) for W, H in sizes]
    ims_plain = (MiScaledImage * 3)(*[im.image() for im in plain])
    ims_tm = (MiScaledImage * 3)(*[im.image() for im in mapped])
    cases = {
        "rgb8_tm": entry(L.mi_display_picture_tm, ctx.h, ref(pic), ref(d_rgb8), ref(color), ref(tm8), None, sp),
        "nv12_tm": entry(L.mi_display_yuv_tm, ctx.h, ref(pic), ref(d_nv12), ref(color), ref(tm8), ref(target), None, sp),
        "nv12_tm_chr2": entry(L.mi_display_yuv_tm, ctx.h, ref(pic), ref(d_nv12), ref(color2), ref(tm8), ref(target), None, sp),
        "scaled_1080": entry(L.mi_display_scaled, ctx.h, ref(pic), ims_plain, 1, ref(color), None, sp),
        "scaled_1080_tm": entry(L.mi_display_scaled_tm, ctx.h, ref(pic), ims_tm, 1, ref(color), ref(tm8), ref(target), None, None, sp),
        "ladder": entry(L.mi_display_scaled, ctx.h, ref(pic), ims_plain, 3, ref(color), None, sp),
        "ladder_tm": entry(L.mi_display_scaled_tm, ctx.h, ref(pic), ims_tm, 3, ref(color), ref(tm8), ref(target), None, None, sp),
    }
    results = {}
    for name in ["rgb8_tm", "nv12_tm", "rgb8_tm", "nv12_tm_chr2", "scaled_1080", "scaled_1080_tm", "scaled_1080", "ladder", "ladder_tm", "ladder"]:
        us, rounds = timed(cases[name])
        key = name if name not in results else name + "_again"
        results[key] = dict(us=round(us, 2), rounds_us=rounds)
        print(json.dumps({key: results[key]}), flush=True)
    base = {k: (results[k]["us"] + results[k + "_again"]["us"]) / 2 for k in ("rgb8_tm", "scaled_1080", "ladder")}
    doc = dict(tool="tools/tonemap_bench.py --yuv", device=torch.cuda.get_device_name(0), library=os.path.basename(LIB_PATH),
               note=args.note, width=w, height=h, bpc=bpc, layout="4:2:0", rungs=sizes,
               source="PQ / BT.2020 (pri 9, trc 16, mtrx 9, limited, chr 0), uniformly random codes",
               tonemap="to sRGB / BT.709 at 8 bits, src_peak 1000, dst_peak 100; target BT.709 limited, NV12",
               iters=args.iters, warmup=args.warmup, rounds=args.rounds,
               timing="HIP events around back-to-back calls; median of rounds; each baseline before and after its row",
               results=results, rgb8_tm_us=round(base["rgb8_tm"], 2), scaled_1080_us=round(base["scaled_1080"], 2),
               ladder_us=round(base["ladder"], 2),
               ratio_nv12_tm_to_rgb8_tm=round(results["nv12_tm"]["us"] / base["rgb8_tm"], 3),
               ratio_nv12_tm_chr2_to_rgb8_tm=round(results["nv12_tm_chr2"]["us"] / base["rgb8_tm"], 3),
               ratio_scaled_1080_tm_to_scaled_1080=round(results["scaled_1080_tm"]["us"] / base["scaled_1080"], 3),
               ratio_ladder_tm_to_ladder=round(results["ladder_tm"]["us"] / base["ladder"], 3))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps({k: doc[k] for k in ("rgb8_tm_us", "scaled_1080_us", "ladder_us", "ratio_nv12_tm_to_rgb8_tm",
                                          "ratio_scaled_1080_tm_to_scaled_1080", "ratio_ladder_tm_to_ladder")}))
    print("wrote", args.out)


def fold(files):
    """The runs of the existing rows in `files` (outputs of this tool), grouped by the note's name
    before '#': per mode and row every value in microseconds, the spread of the parent's runs, the
    difference of the means, and whether every run of the change lies within the parent's range
    widened by that spread."""
    runs = {}
    for path in files:
        with open(path) as f:
            doc = json.load(f)
        side = doc.get("note", "").split("#")[0]
        for row, v in doc["results"].items():
            runs.setdefault(doc["tool"], {}).setdefault(row, {}).setdefault(side, []).append(v["us"])
    out = {}
    for mode, rows in runs.items():
        out[mode] = {}
        for row, sides in rows.items():
            rec = dict(sides)
            parent, change = sides.get("parent", []), sides.get("change", [])
            if len(parent) >= 2 and change:
                spread = max(parent) - min(parent)
                rec["parent_spread_us"] = round(spread, 2)
                rec["change_minus_parent_us"] = round(sum(change) / len(change) - sum(parent) / len(parent), 2)
                rec["within_parent_spread"] = all(min(parent) - spread <= c <= max(parent) + spread for c in change)
            out[mode][row] = rec
    return out


def hlg_rows(args, L, ctx, pic, color, tm8, sp, timed, entry, geom, cases, t_tm):
    """The --hlg run, on main's source picture, context and timer: the three HLG rows, each between
    two takes of its PQ counterpart (main's rgba8_tm and tensor_tm, --yuv's nv12_tm)."""
    import torch

    from rav1d_amd import LIB_PATH
    from rav1d_amd.display import DisplayImage, YuvTarget, enable_hlg
    w, h, bpc, layout = geom
    ref = ctypes.byref
    enable_hlg(ctx)
    hlg = type(color)(color.pri, 18, color.mtrx, color.range, color.chr)
    target = YuvTarget(1, 0)
    im8, nv12 = DisplayImage(w, h, bpc, layout, "rgba", out_bpc=8), DisplayImage(w, h, bpc, layout, "nv12", out_bpc=8)
    d8, d_nv12 = im8.image(), nv12.image()
    cases = dict(cases)
    cases.update({
        "rgba8_hlg": entry(L.mi_display_picture_tm, ctx.h, ref(pic), ref(d8), ref(hlg), ref(tm8), None, sp),
        "tensor_hlg": entry(L.mi_display_tensor_tm, ctx.h, ref(pic), ref(t_tm), ref(hlg), ref(tm8), None, sp),
        "nv12_tm": entry(L.mi_display_yuv_tm, ctx.h, ref(pic), ref(d_nv12), ref(color), ref(tm8), ref(target), None, sp),
        "nv12_hlg": entry(L.mi_display_yuv_tm, ctx.h, ref(pic), ref(d_nv12), ref(hlg), ref(tm8), ref(target), None, sp),
    })
    results = {}
    pairs = [("rgba8_tm", "rgba8_hlg"), ("tensor_tm", "tensor_hlg"), ("nv12_tm", "nv12_hlg")]
    for pq, row in pairs:
        for name in (pq, row, pq):
            us, rounds = timed(cases[name])
            key = name if name not in results else name + "_again"
            results[key] = dict(us=round(us, 2), rounds_us=rounds)
            print(json.dumps({key: results[key]}), flush=True)
    doc = dict(tool="tools/tonemap_bench.py --hlg", device=torch.cuda.get_device_name(0), library=os.path.basename(LIB_PATH),
               note=args.note, width=w, height=h, bpc=bpc, layout="4:2:0", out_w=args.size[0], out_h=args.size[1],
               source="BT.2020 (pri 9, mtrx 9, limited, chr 0) read as PQ (trc 16) and as HLG (trc 18), uniformly random codes",
               tonemap="to sRGB / BT.709 at 8 bits, src_peak 1000 (PQ only), dst_peak 100; NV12 target BT.709 limited",
               iters=args.iters, warmup=args.warmup, rounds=args.rounds,
               timing="HIP events around back-to-back calls; median of rounds; the PQ row before and after its HLG row",
               results=results)
    for pq, row in pairs:
        base = (results[pq]["us"] + results[pq + "_again"]["us"]) / 2
        doc[pq + "_us"] = round(base, 2)
        doc[f"ratio_{row}_to_{pq}"] = round(results[row]["us"] / base, 3)
    if args.fold:
        doc["existing_rows"] = fold(args.fold)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in doc.items() if k.startswith("ratio_")}))
    print("wrote", args.out)


if __name__ == "__main__":
    main()
