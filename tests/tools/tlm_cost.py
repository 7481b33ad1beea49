"""What the TLM marker segments cost an encode (jp2hip_set_organisation).

Encodes a device-resident image on one context with tlm off and on,
alternating, after a warm-up of both, and prints one JSON line: the medians
of stats.total_ms, their spread (min, max) and the host waits of each.  The
yardstick is the tlm-off encode of the same run: no threshold here, the
numbers go into DESIGN.md.

    python tests/tools/tlm_cost.py c2    # 6000 x 4000 RGB8, lossy (the benchmark's image)
    python tests/tools/tlm_cost.py c3    # 10000 x 8000 RGB16, lossless
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("image", choices=("c2", "c3"))
    ap.add_argument("--reps", type=int, default=15, help="encodes of each setting after the warm-up")
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    if args.image == "c2":
        img, conv = im.synth_rgb8(4000, 6000, seed=1234), jp2hip.LOSSY
    else:
        img, conv = im.synth_u16(8000, 10000, comps=3, seed=2), jp2hip.LOSSLESS
    tif = im.tiff_bytes(img)
    lay, _offs = jp2hip.tiff_layout(tif)
    rc = jp2hip.recipe(conv)
    d = DeviceBytes(tif)
    enc = jp2hip.Encoder(0)
    ms, waits, size = {0: [], 1: []}, {0: set(), 1: set()}, {}
    try:
        for i in range(2 * (args.warmup + args.reps)):
            tlm = i & 1
            enc.set_organisation(tlm=tlm)
            out, st = enc.encode_device(d.ptr, d.nbytes, lay, conv, rc, copy=False)
            size[tlm] = len(out)
            out.close()
            if i >= 2 * args.warmup:
                ms[tlm].append(st.total_ms)
                waits[tlm].add(st.host_waits)
    finally:
        enc.close()
        d.free()
    res = {"image": args.image, "shape": list(img.shape), "bits": img.dtype.itemsize * 8,
           "conversion": "lossy" if conv == jp2hip.LOSSY else "lossless", "reps": args.reps,
           "tlm_bytes": size[1] - size[0] if conv == jp2hip.LOSSLESS else None, "file_bytes": [size[0], size[1]]}
    for tlm in (0, 1):
        k = "tlm_on" if tlm else "tlm_off"
        res[k] = {"median_ms": round(statistics.median(ms[tlm]), 3), "min_ms": round(min(ms[tlm]), 3),
                  "max_ms": round(max(ms[tlm]), 3), "host_waits": sorted(waits[tlm])}
    res["median_on_minus_off_ms"] = round(res["tlm_on"]["median_ms"] - res["tlm_off"]["median_ms"], 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
