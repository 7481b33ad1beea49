"""What explicit per-layer rates cost an encode, and how far below their
targets the layers land (jp2hip_set_layer_rates).

Cost: the benchmark's C2 image, device-resident, on one warmed context, in two
phases of two settings in turn -- the rates are no part of the plan cache's
key, so the two settings of a phase share its recipe's plan throughout:

  rate           the default lossy recipe: -rate 3, slope prediction on
  rates          six rates, 3 bpp at the top and halving below, slope prediction on
  rate_noskip    -rate 3 with slope_skip = 0
  rates_noskip   the six rates with slope_skip = 0

Undershoot: per layer (target - bytes) / target, target = floor(rate * W * H / 8),
bytes = the report's bytes through the layer + 2 (EOC), for the C2 encode by
rates and (--c3) for C3's lossless recipe with a lossless top layer over
0.5, 1, 2, 4 and 8 bpp.  One JSON line; no threshold here: the numbers go into
DESIGN.md.

    python tests/tools/rate_cost.py [--c3]
"""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "jp2-bucketeer_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import imaging as im  # noqa: E402
import jp2hip  # noqa: E402
from devmem import DeviceBytes  # noqa: E402

SETTINGS = ("rate", "rates", "rate_noskip", "rates_noskip")
RATES_C2 = [3.0 / 32, 3.0 / 16, 3.0 / 8, 0.75, 1.5, 3.0]
RATES_C3 = [0.5, 1.0, 2.0, 4.0, 8.0, 0.0]


def undershoot(rep, rates, w, h):
    out = []
    for l, r in enumerate(rates):
        if r > 0.0:
            target = math.floor(r * w * h / 8)
            out.append({"layer": l, "target": target, "bytes": int(rep.bytes[l]) + 2,
                        "undershoot": round((target - int(rep.bytes[l]) - 2) / target, 6)})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15, help="encodes of each setting after the warm-up")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--c3", action="store_true", help="also the undershoot of C3's lossless recipe by rates")
    args = ap.parse_args()
    img = im.synth_rgb8(4000, 6000, seed=1234)
    tif = im.tiff_bytes(img)
    lay, _offs = jp2hip.tiff_layout(tif)
    rc = {k: jp2hip.recipe(jp2hip.LOSSY, slope_skip=0 if k.endswith("noskip") else 1) for k in SETTINGS}
    d = DeviceBytes(tif)
    enc = jp2hip.Encoder(0)
    ms, waits, iters, files, reps = ({k: [] for k in SETTINGS}, {k: set() for k in SETTINGS},
                                     {k: set() for k in SETTINGS}, {}, {})
    try:
        n = 2 * (args.warmup + args.reps)
        for i in range(2 * n):
            k = SETTINGS[2 * (i // n) + i % 2]
            enc.set_layer_rates(RATES_C2 if k.startswith("rates") else None)
            out, st = enc.encode_device(d.ptr, d.nbytes, lay, jp2hip.LOSSY, rc[k], copy=False)
            if k not in files:
                files[k] = len(out)
                reps[k] = enc.layer_report()
            out.close()
            if i % n >= 2 * args.warmup:
                ms[k].append(st.total_ms)
                waits[k].add(st.host_waits)
                iters[k].add(st.rate_iterations)
    finally:
        enc.close()
        d.free()
    res = {"image": "c2", "shape": list(img.shape), "reps": args.reps, "layer_rates": RATES_C2, "file_bytes": files}
    for k in SETTINGS:
        res[k] = {"median_ms": round(statistics.median(ms[k]), 3), "min_ms": round(min(ms[k]), 3),
                  "max_ms": round(max(ms[k]), 3), "host_waits": sorted(waits[k]), "iterations": sorted(iters[k])}
    res["rates_minus_rate_ms"] = round(res["rates"]["median_ms"] - res["rate"]["median_ms"], 3)
    res["rates_noskip_minus_rate_noskip_ms"] = round(res["rates_noskip"]["median_ms"] - res["rate_noskip"]["median_ms"], 3)
    res["undershoot_c2"] = undershoot(reps["rates"], RATES_C2, img.shape[1], img.shape[0])
    res["undershoot_c2_noskip"] = undershoot(reps["rates_noskip"], RATES_C2, img.shape[1], img.shape[0])
    if args.c3:
        img = im.synth_u16(8000, 10000, comps=3, seed=2)
        tif = im.tiff_bytes(img, rows_per_strip=64)
        lay, _offs = jp2hip.tiff_layout(tif)
        d = DeviceBytes(tif)
        enc = jp2hip.Encoder(0)
        try:
            enc.set_layer_rates(RATES_C3)
            rcp = jp2hip.recipe(jp2hip.LOSSLESS, tile_w=1024, tile_h=1024)
            out, st = enc.encode_device(d.ptr, d.nbytes, lay, jp2hip.LOSSLESS, rcp, copy=False)
            res["c3"] = {"rates": RATES_C3, "file_bytes": len(out), "iterations": st.rate_iterations,
                         "host_waits": st.host_waits, "total_ms": round(st.total_ms, 3),
                         "undershoot": undershoot(enc.layer_report(), RATES_C3, img.shape[1], img.shape[0])}
            out.close()
        finally:
            enc.close()
            d.free()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
