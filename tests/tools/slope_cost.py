"""What fixed-slope layers and the layer report cost an encode
(jp2hip_set_layer_slopes, jp2hip_set_layer_report).

Encodes the benchmark's C2 image, device-resident, on one context -- three
settings in turn on one recipe (so the plan is reused throughout), after a
warm-up of each, then the fourth, whose recipe differs, on its own -- and
prints one JSON line with the medians of stats.total_ms and their spread:

  rate          the default lossy recipe: 3 bpp, slope prediction on
  slope         slope-driven at the thresholds the rate-driven encode chose
                (its layer report's), which codes every plane and runs no rate loop
  slope_report  the same with the layer report's distortion enabled; the
                report's kernels and its host wait are slope_report - slope
  rate_noskip   rate-driven with slope_skip = 0 (every plane coded, as a
                slope-driven encode codes them)

No threshold here: the numbers go into DESIGN.md.

    python tests/tools/slope_cost.py
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "jp2-bucketeer_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import imaging as im  # noqa: E402
import jp2hip  # noqa: E402
from devmem import DeviceBytes  # noqa: E402

TURN = ("rate", "slope", "slope_report")
SETTINGS = TURN + ("rate_noskip",)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15, help="encodes of each setting after the warm-up")
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    img = im.synth_rgb8(4000, 6000, seed=1234)
    tif = im.tiff_bytes(img)
    lay, _offs = jp2hip.tiff_layout(tif)
    rc = {k: jp2hip.recipe(jp2hip.LOSSY, slope_skip=0 if k == "rate_noskip" else 1) for k in SETTINGS}
    d = DeviceBytes(tif)
    enc = jp2hip.Encoder(0)
    ms, waits, files = {k: [] for k in SETTINGS}, {k: set() for k in SETTINGS}, {}
    try:
        out, _ = enc.encode_device(d.ptr, d.nbytes, lay, jp2hip.LOSSY, rc["rate"])
        files["rate"] = out
        rep = enc.layer_report()
        slopes = list(rep.threshold[:rep.layers])
        n = len(TURN) * (args.warmup + args.reps)
        for i in range(n + args.warmup + args.reps):
            k = TURN[i % len(TURN)] if i < n else "rate_noskip"
            enc.set_layer_slopes(slopes if k.startswith("slope") else None)
            enc.set_layer_report(1 if k == "slope_report" else 0)
            out, st = enc.encode_device(d.ptr, d.nbytes, lay, jp2hip.LOSSY, rc[k], copy=False)
            if k not in files:
                files[k] = out.tobytes()
            out.close()
            if len(TURN) * args.warmup <= i < n or i >= n + args.warmup:
                ms[k].append(st.total_ms)
                waits[k].add(st.host_waits)
            if k == "slope_report":
                dist = list(enc.layer_report().distortion[:rep.layers])
    finally:
        enc.close()
        d.free()
    res = {"image": "c2", "shape": list(img.shape), "reps": args.reps, "thresholds": slopes,
           "log2_thresholds": [round(jp2hip.slope_to_log2(s, 8), 2) for s in slopes],
           "distortion": dist, "file_bytes": {k: len(files[k]) for k in SETTINGS},
           "slope_file_is_rate_file": files["slope"] == files["rate"],
           "slope_file_is_rate_noskip_file": files["slope"] == files["rate_noskip"]}
    for k in SETTINGS:
        res[k] = {"median_ms": round(statistics.median(ms[k]), 3), "min_ms": round(min(ms[k]), 3),
                  "max_ms": round(max(ms[k]), 3), "host_waits": sorted(waits[k])}
    res["slope_minus_rate_ms"] = round(res["slope"]["median_ms"] - res["rate"]["median_ms"], 3)
    res["slope_minus_rate_noskip_ms"] = round(res["slope"]["median_ms"] - res["rate_noskip"]["median_ms"], 3)
    res["report_on_minus_off_ms"] = round(res["slope_report"]["median_ms"] - res["slope"]["median_ms"], 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
