"""Rate of the sample expansion (k_expand) on the GPU (measurement tool, not a test).

Encodes a C-class scan, 10000 x 8000, as a 1-bit WhiteIsZero TIFF and as an
8-bit palette TIFF on a context in profile mode and prints, per source, the
median ingest_ms (the span of the expansion's own timing events) and the
bytes it moved per second -- packed source read plus 8-bit copy written --
against the HBM peak bench.py quotes.  Each file is also checked against the
8-bit encode of the expanded pixels on the same context.

    python tests/tools/expand_rate.py [--width 10000] [--height 8000] [--reps 5]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "..", "jp2-bucketeer_amd"))

import imaging as im  # noqa: E402
import jp2hip  # noqa: E402
import pixel_format_cases as pf  # noqa: E402

HBM_PEAK = 8.0e12  # bench.py


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=10000)
    ap.add_argument("--height", type=int, default=8000)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    h, w = args.height, args.width
    enc = jp2hip.Encoder(0, profile=True)
    conv = jp2hip.LOSSY
    for name, bits, photo in (("bilevel_white_is_zero", 1, pf.WHITE_IS_ZERO), ("palette8", 8, pf.PALETTE)):
        idx = pf.indices(h, w, bits, 7)
        cm = pf.random_colormap(8, 8) if photo == pf.PALETTE else None
        tif = pf.make_tiff(idx, bits, photo, colormap=cm, rows_per_strip=64)
        px = pf.expand(idx, bits, photo, cm)
        ref, _ = enc.encode_tiff(im.tiff_bytes(px, rows_per_strip=64), conv)
        times, totals = [], []
        for _ in range(args.reps + 1):
            out, st = enc.encode_tiff(tif, conv)
            times.append(st.ingest_ms)
            totals.append(st.total_ms)
        assert out == ref, name
        ms = statistics.median(times[1:])
        moved = ((w * bits + 7) // 8) * h + px.nbytes
        print(json.dumps({"source": name, "width": w, "height": h, "expand_ms": round(ms, 4),
                          "expand_ms_all": [round(t, 4) for t in times[1:]],
                          "bytes_moved": moved, "TB_per_s": round(moved / (ms * 1e-3) / 1e12, 3),
                          "of_hbm_peak": round(moved / (ms * 1e-3) / HBM_PEAK, 3),
                          "encode_total_ms": round(statistics.median(totals[1:]), 2)}), flush=True)
    enc.close()


if __name__ == "__main__":
    main()
