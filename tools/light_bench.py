#!/usr/bin/env python3
"""Measure mi_picture_light_level (csrc/light.hip) and the split table key of the colour-volume stage
on a resident 4K10 4:2:0 picture (GPU), timed with HIP events around `--iters` back-to-back calls
after `--warmup` calls, median of `--rounds`; each baseline is taken before and after its rows:

  random content (uniformly random codes) and flat content (a constant picture: every lane of every
  wave counts into one bin), each:
    rgb10            mi_display_picture, planar R'G'B' at 10 bits: reads the same bytes, and
                     stores three planes more (the baseline);
    light            mi_picture_light_level, the entry;
    light_v0 .. v2   mi_picture_light_level_variant: one LDS atomic per pixel; equal neighbours of
                     a lane combined; a uniform wave combined as well (the entry);
  a tone-mapped call whose peak changes with every call:
    scaled_1080_tm       mi_display_scaled_tm, one 1920 x 1080 8-bit rung, one src_peak;
    scaled_1080_tm_alt   the same, src_peak alternating between 1000 and 4000 nits call by call:
                         every call rebuilds tables. host_us is the wall time of a call on the host
                         (the table build is host work), us the time between the events.

No threshold is asserted; the ratios are recorded.

    python tools/light_bench.py [--out profiles/light_level_bench.json] [--note TEXT]

--peaks-only measures the last two rows alone: a library from before mi_picture_light_level (loaded
with MI_LIB) runs them, which is how the split key is compared with what it replaced.
"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "light_level_bench.json"))
    ap.add_argument("--peaks-only", action="store_true", help="only the tone-mapped rows (any library)")
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--bpc", type=int, default=10)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--note", default="")
    args = ap.parse_args()

    import numpy as np
    import torch

    from rav1d_amd import LIB_PATH
    from rav1d_amd.av1dec import MiColorInfo
    from rav1d_amd.display import DisplayImage, MiScaledImage, ScaledImage, ToneMap, YuvTarget
    from rav1d_amd.frame import Context, Frame

    if not torch.cuda.is_available():
        sys.exit("light_bench needs a GPU: nothing is measured without one")
    # (the library as ctypes finds it: a library from before this entry has no signatures for it)
    L = ctypes.CDLL(LIB_PATH)
    w, h, bpc, layout = args.width, args.height, args.bpc, 1
    rng = np.random.default_rng(0)
    ctx = Context(0)
    color = MiColorInfo(9, 16, 9, 0, 0)      # HDR10: BT.2020 primaries and matrix, PQ, limited range
    stream = torch.cuda.current_stream()
    sp = ctypes.c_void_p(stream.cuda_stream)
    ref = ctypes.byref

    def source(flat):
        src = Frame(w, h, bpc, layout)
        for p in range(3):
            pw, ph = src.dims(p)
            if flat:
                src.set_plane_np(p, np.full((ph, pw), (1 << bpc) // 2 if p else 600))
            else:
                src.set_plane_np(p, rng.integers(0, 1 << bpc, (ph, pw)))
        return src

    def entry(fn, *argv):
        def run():
            if fn(*argv) != 0:
                raise RuntimeError(f"{fn.__name__} failed")
        return run

    def timed(fn):
        """Median over rounds of the mean microseconds of `iters` back-to-back calls: between the
        events, and on the host (the calls alone, before the wait)."""
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        us, host = [], []
        for _ in range(args.rounds):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            t0 = time.perf_counter()
            for _ in range(args.iters):
                fn()
            host.append((time.perf_counter() - t0) * 1e6 / args.iters)
            b.record(stream)
            b.synchronize()
            us.append(a.elapsed_time(b) * 1e3 / args.iters)
        return dict(us=round(float(np.median(us)), 2), host_us=round(float(np.median(host)), 2),
                    rounds_us=[round(v, 2) for v in us])

    results, summary = {}, {}

    def rows(prefix, cases, order):
        for name in order:
            key = f"{prefix}{name}"
            key = key if key not in results else key + "_again"
            results[key] = timed(cases[name])
            print(json.dumps({key: results[key]}), flush=True)

    if not args.peaks_only:
        hist = torch.zeros(1 << bpc, dtype=torch.int32, device="cuda")
        hp = ctypes.c_void_p(hist.data_ptr())
        rgb = DisplayImage(w, h, bpc, layout, "rgb")
        d_rgb = rgb.image()
        for kind in ("random", "flat"):
            src = source(kind == "flat")
            pic = src.picture()
            cases = {"rgb10": entry(L.mi_display_picture, ctx.h, ref(pic), ref(d_rgb), ref(color), None, sp),
                     "light": entry(L.mi_picture_light_level, ctx.h, ref(pic), ref(color), hp, sp)}
            for v in range(3):
                cases[f"light_v{v}"] = entry(L.mi_picture_light_level_variant, ctx.h, ref(pic), ref(color), hp, v, sp)
            rows(kind + "_", cases, ["rgb10", "light", "light_v0", "light_v1", "light_v2", "rgb10"])
            base = (results[f"{kind}_rgb10"]["us"] + results[f"{kind}_rgb10_again"]["us"]) / 2
            summary[f"{kind}_rgb10_us"] = round(base, 2)
            for n in ("light", "light_v0", "light_v1", "light_v2"):
                summary[f"{kind}_ratio_{n}_to_rgb10"] = round(results[f"{kind}_{n}"]["us"] / base, 3)
            torch.cuda.synchronize()
            assert int(hist.sum().item()) == w * h
        for n in ("light", "light_v0"):
            summary[f"flat_to_random_{n}"] = round(results[f"flat_{n}"]["us"] / results[f"random_{n}"]["us"], 3)

    src = source(False)
    pic = src.picture()
    target = YuvTarget(1, 0)
    rung = ScaledImage(1920, 1080, 8, layout)
    ims = (MiScaledImage * 1)(rung.image())
    tms = [ToneMap(1, 13, 8, 1000.0, 100.0), ToneMap(1, 13, 8, 4000.0, 100.0)]
    flip = [0]

    def alternating():
        flip[0] ^= 1
        if L.mi_display_scaled_tm(ctx.h, ref(pic), ims, 1, ref(color), ref(tms[flip[0]]), ref(target), None, None, sp) != 0:
            raise RuntimeError("mi_display_scaled_tm failed")

    cases = {"scaled_1080_tm": entry(L.mi_display_scaled_tm, ctx.h, ref(pic), ims, 1, ref(color), ref(tms[0]), ref(target),
                                     None, None, sp),
             "scaled_1080_tm_alt": alternating}
    rows("", cases, ["scaled_1080_tm", "scaled_1080_tm_alt", "scaled_1080_tm"])
    steady = (results["scaled_1080_tm"]["us"] + results["scaled_1080_tm_again"]["us"]) / 2
    summary["scaled_1080_tm_us"] = round(steady, 2)
    summary["scaled_1080_tm_alt_us"] = results["scaled_1080_tm_alt"]["us"]
    summary["scaled_1080_tm_alt_host_us"] = results["scaled_1080_tm_alt"]["host_us"]
    summary["ratio_alt_to_steady"] = round(results["scaled_1080_tm_alt"]["us"] / steady, 3)

    doc = dict(tool="tools/light_bench.py" + (" --peaks-only" if args.peaks_only else ""),
               device=torch.cuda.get_device_name(0), library=os.path.basename(LIB_PATH), note=args.note, width=w, height=h,
               bpc=bpc, layout="4:2:0", source="PQ / BT.2020 (pri 9, trc 16, mtrx 9, limited, chr 0); random: uniformly "
               "random codes; flat: Y 600, U = V = 512", iters=args.iters, warmup=args.warmup, rounds=args.rounds,
               timing="HIP events around back-to-back calls; median of rounds; each baseline before and after its rows; "
               "host_us: wall time of the calls on the host", results=results, **summary)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(summary))
    print("wrote", args.out)


if __name__ == "__main__":
    main()
