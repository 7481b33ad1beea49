"""Rate of the orientation stage (k_orient) on the GPU (measurement tool, not a test).

Encodes C-class scans -- 8000 rows of 10000 and of 10001 columns, RGB8 and
RGB16 -- with source orientation 3 (the flipping form) and 6 (the transposing
form) on a context in profile mode and prints, per case, the median ingest_ms
(the span of the stage's own timing events: an uncompressed 8- / 16-bit source
launches nothing else in front of the DWT) and the bytes it moved per second
-- stored image read plus upright copy written -- against the HBM peak
bench.py quotes.  Each file is also checked against the encode, on the same
context with orientation off, of the upright pixels.

    python tests/tools/orient_rate.py [--height 8000] [--reps 5]
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
import orientation_cases as oc  # noqa: E402

HBM_PEAK = 8.0e12  # bench.py


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=8000)
    ap.add_argument("--widths", type=int, nargs="+", default=[10000, 10001])
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    h = args.height
    enc = jp2hip.Encoder(0, profile=True)
    conv = jp2hip.LOSSY
    for w in args.widths:
        for name in ("rgb8", "rgb16"):
            px = im.synth_rgb8(h, w, seed=7) if name == "rgb8" else im.synth_u16(h, w, comps=3, seed=7)
            tif = im.tiff_bytes(px, rows_per_strip=64)
            for o in (3, 6):
                ref, _ = enc.encode_tiff(im.tiff_bytes(oc.upright(px, o), rows_per_strip=64), conv)
                enc.set_source_orientation(o)
                times, totals = [], []
                for _ in range(args.reps + 1):
                    out, st = enc.encode_tiff(tif, conv)
                    times.append(st.ingest_ms)
                    totals.append(st.total_ms)
                enc.set_source_orientation(jp2hip.ORIENT_OFF)
                assert out == ref, (name, w, o)
                ms = statistics.median(times[1:])
                moved = 2 * px.nbytes
                print(json.dumps({"source": name, "width": w, "height": h, "orientation": o,
                                  "orient_ms": round(ms, 4), "orient_ms_all": [round(t, 4) for t in times[1:]],
                                  "bytes_moved": moved, "TB_per_s": round(moved / (ms * 1e-3) / 1e12, 3),
                                  "of_hbm_peak": round(moved / (ms * 1e-3) / HBM_PEAK, 3),
                                  "encode_total_ms": round(statistics.median(totals[1:]), 2)}), flush=True)
    enc.close()


if __name__ == "__main__":
    main()
