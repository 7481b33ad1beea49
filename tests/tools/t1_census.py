#!/usr/bin/env python3
"""What the image-driven suites reach in tier-1, against the crafted corpus.

Runs the CPU oracle, with its tier-1 census on, over tests/sweep_cases.py and
tests/recipe_axes_cases.py (the images behind the GPU parity sweeps) and over
tests/t1_block_cases.py, and prints the census cells the former leave at zero
that the corpus reaches, the rarest cells of each, and the per-block maxima.
CPU only; a few minutes.  DESIGN.md records one run.

    python tests/tools/t1_census.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import oracle_lib as ol  # noqa: E402
import recipe_axes_cases as ra  # noqa: E402
import sweep_cases as sc  # noqa: E402
import t1_block_cases as tc  # noqa: E402

BAND = ("LL/LH", "HL", "HH")
PASS = ("SPP", "CUP")
RL = ("four zeros", "r=0", "r=1", "r=2", "r=3", "denied: own state", "denied: neighbour", "denied: short stripe")
MQ = ("MPS", "MPS renorm+xchg", "MPS renorm", "LPS xchg", "LPS", "SWITCH")
BO = ("after 0xFF", "plain", "carry", "carry makes 0xFF")
FL = ("C >= tempc", "C < tempc", "0xFF dropped", "last byte kept")
MAXIMA = ("decisions in one plane", "decisions in one block", "SPP depth")


def cell_name(name, idx):
    if name == "zc":
        c, h, v, d, p, b = idx
        return f"ZC {BAND[c]} h={h} v={v} d={d} {PASS[p]} bit={b}"
    if name == "sc":
        return f"SC h={idx[0] - 1:+d} v={idx[1] - 1:+d} bit={idx[2]}"
    if name == "mr":
        return f"MR ctx={14 + idx[0]} bit={idx[1]}"
    if name == "mq":
        return f"MQ state {idx[0]} {MQ[idx[1]]}"
    return {"rl": "RL " + RL[idx[0]], "byteout": "byteout " + BO[idx[0]], "flush": "flush " + FL[idx[0]]}[name]


def run(cases, image, recipe):
    total = None
    for c in cases:
        ol.census_reset()
        ol.encode(image(c), recipe(c))
        total = ol.census_add(total, ol.census_read())
    return total


def main():
    old = {
        "sweep": run(sc.cases(), sc.image, lambda c: ol.recipe(c["lossless"], **c["recipe"])),
        "recipe_axes": run(ra.cases(), ra.image, lambda c: ol.recipe(c["lossless"], **c["recipe"])),
    }
    both = ol.census_add(ol.census_add(None, old["sweep"]), old["recipe_axes"])
    corpus = run(tc.cases(), tc.image, lambda c: ol.recipe(c["lossless"], **c["recipe"]))
    print(f"{'maximum':28s} {'sweep':>10s} {'recipe_axes':>12s} {'corpus':>10s}")
    for i, n in enumerate(MAXIMA):
        print(f"{n:28s} {old['sweep']['max'][i]:10d} {old['recipe_axes']['max'][i]:12d} {corpus['max'][i]:10d}")
    print(f"\n{'counter':10s} {'cells':>6s} {'empty: sweep':>13s} {'recipe_axes':>12s} {'both':>6s} {'corpus':>7s}")
    for name, shape in ol.CENSUS_LAYOUT[:-1]:
        print(f"{name:10s} {int(np.prod(shape)):6d} {(old['sweep'][name] == 0).sum():13d} "
              f"{(old['recipe_axes'][name] == 0).sum():12d} {(both[name] == 0).sum():6d} {(corpus[name] == 0).sum():7d}")
    print("\ncells the old suites leave empty and the corpus reaches (corpus count):")
    for name, shape in ol.CENSUS_LAYOUT[:-1]:
        for idx in np.ndindex(*shape):
            if both[name][idx] == 0 and corpus[name][idx]:
                print(f"  {cell_name(name, idx):44s} {corpus[name][idx]}")
    print("\ncells the old suites reach fewer than 10 times (old count, corpus count):")
    for name, shape in ol.CENSUS_LAYOUT[:-1]:
        for idx in np.ndindex(*shape):
            if 0 < both[name][idx] < 10:
                print(f"  {cell_name(name, idx):44s} {both[name][idx]:6d} {corpus[name][idx]}")
    for label, c in (("old suites", both), ("corpus", corpus)):
        print(f"\nbyte-out branches, {label}: " + ", ".join(f"{n} {c['byteout'][i]}" for i, n in enumerate(BO)))
        print(f"flush branches, {label}: " + ", ".join(f"{n} {c['flush'][i]}" for i, n in enumerate(FL)))
        print(f"run-length, {label}: " + ", ".join(f"{n} {c['rl'][i]}" for i, n in enumerate(RL)))


if __name__ == "__main__":
    main()
