"""What the tile-part divisions L and C cost an encode
(jp2hip_set_tile_part_divisions).

Encodes a device-resident image on one context with the letters off and on,
alternating, after a warm-up of both, and prints one JSON line: the medians
of stats.total_ms, their spread (min, max), the host waits and the tile-part
counts of each.  The yardstick is the letters-off encode of the same run: no
threshold here, the numbers go into DESIGN.md.  (Every switch rebuilds and
uploads the tier-2 tables, off -> on and on -> off alike, so both sides of the
comparison pay that.)

    python tests/tools/tparts_cost.py c2    # 6000 x 4000 RGB8, lossy, LRCP + L
    python tests/tools/tparts_cost.py c3    # 10000 x 8000 RGB16, lossless, RLCP + R + L
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
        rc = jp2hip.recipe(conv, progression=jp2hip.ORDER_LRCP, tparts_r=0)
    else:
        img, conv = im.synth_u16(8000, 10000, comps=3, seed=2), jp2hip.LOSSLESS
        rc = jp2hip.recipe(conv, progression=jp2hip.ORDER_RLCP, tparts_r=1)
    tif = im.tiff_bytes(img)
    lay, _offs = jp2hip.tiff_layout(tif)
    d = DeviceBytes(tif)
    enc = jp2hip.Encoder(0)
    ms, waits, size, parts = {0: [], 1: []}, {0: set(), 1: set()}, {}, {}
    try:
        for i in range(2 * (args.warmup + args.reps)):
            on = i & 1
            enc.set_tile_part_divisions("L" if on else 0)
            out, st = enc.encode_device(d.ptr, d.nbytes, lay, conv, rc, copy=False)
            size[on] = len(out)
            if on not in parts:
                parts[on] = len(im.tile_parts(im.codestream(out.tobytes())))
            out.close()
            if i >= 2 * args.warmup:
                ms[on].append(st.total_ms)
                waits[on].add(st.host_waits)
    finally:
        enc.close()
        d.free()
    res = {"image": args.image, "shape": list(img.shape), "bits": img.dtype.itemsize * 8,
           "conversion": "lossy" if conv == jp2hip.LOSSY else "lossless", "reps": args.reps,
           "order": "LRCP" if args.image == "c2" else "RLCP", "tparts_r": rc.tparts_r, "letters": "L",
           "tile_parts": [parts[0], parts[1]], "file_bytes": [size[0], size[1]]}
    for on in (0, 1):
        k = "letters_on" if on else "letters_off"
        res[k] = {"median_ms": round(statistics.median(ms[on]), 3), "min_ms": round(min(ms[on]), 3),
                  "max_ms": round(max(ms[on]), 3), "host_waits": sorted(waits[on])}
    res["median_on_minus_off_ms"] = round(res["letters_on"]["median_ms"] - res["letters_off"]["median_ms"], 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
