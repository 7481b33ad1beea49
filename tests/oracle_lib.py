"""ctypes binding of the CPU oracle (oracle/_build/liboracle.so).

TEST INFRASTRUCTURE ONLY: the oracle is the checker, never the thing measured
or shipped.  Built by ``make -C oracle`` (``__graft_entry__.build()`` does it).
"""
from __future__ import annotations

import ctypes
import os
from ctypes import POINTER, Structure, byref, c_double, c_int, c_int32, c_int64, c_size_t, c_uint8

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "oracle", "_build", "liboracle.so")


class OracleRecipe(Structure):
    _fields_ = [("levels", c_int32), ("layers", c_int32), ("tile_w", c_int32), ("tile_h", c_int32),
                ("cblk_w_log2", c_int32), ("cblk_h_log2", c_int32), ("nprecincts", c_int32),
                ("prec_w_log2", c_int32 * 16), ("prec_h_log2", c_int32 * 16),
                ("progression", c_int32), ("sop", c_int32), ("eph", c_int32), ("plt", c_int32),
                ("tparts_r", c_int32), ("guard_bits", c_int32), ("reversible", c_int32),
                ("mct", c_int32), ("qstep", c_double), ("rate_bpp", c_double),
                ("format", c_int32), ("comment", c_int32), ("slope_skip", c_int32),
                ("flush_period", c_int32)]


_L = None


def lib():
    global _L
    if _L is None:
        if not os.path.exists(LIB):
            import subprocess
            subprocess.run(["make", "-C", os.path.join(ROOT, "oracle")], check=True,
                           capture_output=True)
        L = ctypes.CDLL(LIB)
        L.oracle_recipe_init.argtypes = [POINTER(OracleRecipe), c_int]
        L.oracle_encode.argtypes = [ctypes.c_void_p, c_int, c_int, c_int, c_int,
                                    POINTER(OracleRecipe), POINTER(POINTER(c_uint8)),
                                    POINTER(c_size_t)]
        L.oracle_encode_tiff.argtypes = [ctypes.c_void_p, c_size_t, POINTER(OracleRecipe),
                                         POINTER(POINTER(c_uint8)), POINTER(c_size_t)]
        L.oracle_fdwt.argtypes = [ctypes.c_void_p, c_int, c_int, c_int, c_int]
        L.oracle_t1_encode.argtypes = [ctypes.c_void_p, c_int, c_int, c_int, c_int,
                                       ctypes.c_void_p, c_int, POINTER(c_int), ctypes.c_void_p,
                                       ctypes.c_void_p, POINTER(c_int)]
        L.oracle_t1_census_reset.argtypes = []
        L.oracle_t1_census_reset.restype = None
        L.oracle_t1_census_read.argtypes = [ctypes.c_void_p, c_int]
        L.oracle_pcrd_census_reset.argtypes = []
        L.oracle_pcrd_census_reset.restype = None
        L.oracle_pcrd_census_read.argtypes = [ctypes.c_void_p, c_int]
        L.oracle_pcrd_export_enable.argtypes = [c_int]
        L.oracle_pcrd_export_enable.restype = None
        L.oracle_pcrd_export_segments.argtypes = [ctypes.c_void_p] * 4 + [c_int]
        L.oracle_pcrd_export_layers.argtypes = [ctypes.c_void_p] * 5 + [c_int]
        L.oracle_pcrd_export_block.argtypes = [c_int] + [ctypes.c_void_p] * 2 + [POINTER(c_double)] + \
            [ctypes.c_void_p] * 3 + [POINTER(c_int)]
        L.oracle_pcrd_export_iterations.argtypes = []
        L.oracle_free.argtypes = [ctypes.c_void_p]
        L.oracle_last_error.restype = ctypes.c_char_p
        _L = L
    return _L


def recipe(lossless: bool, **overrides) -> OracleRecipe:
    r = OracleRecipe()
    lib().oracle_recipe_init(byref(r), 1 if lossless else 0)
    for k, v in overrides.items():
        if k in ("prec_w_log2", "prec_h_log2"):
            arr = getattr(r, k)
            for i, x in enumerate(v):
                arr[i] = x
        else:
            setattr(r, k, v)
    return r


def copy_recipe(src) -> OracleRecipe:
    """Oracle recipe with the same field values as a jp2hip Recipe."""
    r = OracleRecipe()
    for name, _ in OracleRecipe._fields_:
        v = getattr(src, name)
        if name in ("prec_w_log2", "prec_h_log2"):
            arr = getattr(r, name)
            for i in range(16):
                arr[i] = v[i]
        else:
            setattr(r, name, v)
    return r


def _take(out, n) -> bytes:
    try:
        return ctypes.string_at(out, n.value)
    finally:
        lib().oracle_free(out)


def encode(img: np.ndarray, rcp: OracleRecipe) -> bytes:
    a = np.ascontiguousarray(img)
    if a.ndim == 2:
        h, w, nc = a.shape[0], a.shape[1], 1
    else:
        h, w, nc = a.shape
    bits = a.dtype.itemsize * 8
    out = POINTER(c_uint8)()
    n = c_size_t()
    if lib().oracle_encode(a.ctypes.data, w, h, nc, bits, byref(rcp), byref(out), byref(n)):
        raise RuntimeError(lib().oracle_last_error().decode())
    return _take(out, n)


def encode_tiff(data: bytes, rcp: OracleRecipe) -> bytes:
    buf = ctypes.create_string_buffer(data, len(data))
    out = POINTER(c_uint8)()
    n = c_size_t()
    if lib().oracle_encode_tiff(buf, len(data), byref(rcp), byref(out), byref(n)):
        raise RuntimeError(lib().oracle_last_error().decode())
    return _take(out, n)


def fdwt(plane: np.ndarray, levels: int, reversible: bool) -> np.ndarray:
    a = np.ascontiguousarray(plane.astype(np.int32 if reversible else np.float32))
    lib().oracle_fdwt(a.ctypes.data, a.shape[1], a.shape[0], levels, 1 if reversible else 0)
    return a


def t1_encode(sm: np.ndarray, band: int, lossless: bool):
    """Tier-1 of one block of sign-magnitude int32 samples -> (bytes, rates, dists, P)."""
    a = np.ascontiguousarray(sm.astype(np.int32))
    h, w = a.shape
    cap = w * h * 8 + 256
    buf = (c_uint8 * cap)()
    rates = np.zeros(100, np.int32)
    dists = np.zeros(100, np.int64)
    n = c_int()
    P = c_int()
    np_ = lib().oracle_t1_encode(a.ctypes.data, w, h, band, 1 if lossless else 0, buf, cap,
                                 byref(n), rates.ctypes.data, dists.ctypes.data, byref(P))
    if np_ < 0:
        raise RuntimeError(lib().oracle_last_error().decode())
    return bytes(buf[:n.value]), rates[:np_].copy(), dists[:np_].copy(), P.value


# Tier-1 census: the cell layout of g_cen in oracle/jp2_oracle.c, as
# (name, shape) in storage order.
CENSUS_LAYOUT = (
    ("zc", (3, 3, 3, 5, 2, 2)),  # band class (LL/LH, HL, HH), h, v, d, pass (SPP, CUP), decision
    ("sc", (3, 3, 2)),           # horizontal contribution + 1, vertical + 1, coded bit
    ("mr", (3, 2)),              # context 14, 15, 16; decision
    ("rl", (8,)),                # RL_* below
    ("mq", (47, 6)),             # table index; MQ_* below
    ("byteout", (4,)),           # BO_* below
    ("flush", (4,)),             # FL_* below
    ("max", (3,)),               # MAX_* below
)
RL_ZEROS, RL_R0, RL_R1, RL_R2, RL_R3, RL_DENIED_OWN, RL_DENIED_NEIGHBOUR, RL_DENIED_SHORT = range(8)
MQ_MPS, MQ_MPS_RENORM_XCHG, MQ_MPS_RENORM, MQ_LPS_XCHG, MQ_LPS, MQ_SWITCH = range(6)
BO_AFTER_FF, BO_PLAIN, BO_CARRY, BO_CARRY_TO_FF = range(4)
FL_C_GE_TEMPC, FL_C_LT_TEMPC, FL_DROP_FF, FL_KEEP = range(4)
MAX_PLANE_DECISIONS, MAX_BLOCK_DECISIONS, MAX_SPP_DEPTH = range(3)
CENSUS_CELLS = sum(int(np.prod(shape)) for _, shape in CENSUS_LAYOUT)


def census_reset():
    lib().oracle_t1_census_reset()


def census_read() -> dict:
    """The counters since the last census_reset(), one int64 array per
    CENSUS_LAYOUT entry."""
    n = lib().oracle_t1_census_read(None, 0)
    assert n == CENSUS_CELLS, (n, CENSUS_CELLS)
    cells = np.zeros(n, np.int64)
    lib().oracle_t1_census_read(cells.ctypes.data, n)
    out, at = {}, 0
    for name, shape in CENSUS_LAYOUT:
        k = int(np.prod(shape))
        out[name] = cells[at:at + k].reshape(shape).copy()
        at += k
    return out


def census_add(total: dict | None, c: dict) -> dict:
    """Accumulate census `c` into `total`: counts add, maxima take the max."""
    if total is None:
        return {k: v.copy() for k, v in c.items()}
    for k, v in c.items():
        total[k] = np.maximum(total[k], v) if k == "max" else total[k] + v
    return total


# PCRD census: the cells of oracle/jp2_oracle.h's PC_* enum, in order.  The
# *_max_* cells hold maxima, the others counts.
PCRD_CELLS = (
    "hull_skip_dd", "hull_pop_dr", "hull_pop_slope", "hull_pop_slope_equal", "hull_pop_to_base", "hull_pop_reads_stack",
    "hull_max_pops_one_pass", "hull_max_points", "hull_block_no_pass", "hull_np_mult8", "hull_np_not_mult8",
    "hull_np_gt88",
    "sel_takes_nothing", "sel_takes_all", "sel_tie_1", "sel_tie_2_64", "sel_tie_gt64", "sel_tie_blocks_differ",
    "sel_tie_one_block", "sel_same_as_layer_before", "sel_layers_1", "sel_layers_32",
    "rate_iterations_1", "rate_iterations_2", "rate_iterations_3", "rate_iterations_4", "rate_iterations_5",
    "rate_iterations_6", "rate_iterations_7", "rate_iterations_8", "rate_stopped_under_target",
    "rate_stopped_over_at_8", "rate_first_budget_negative", "rate_budget_clamped_in_step", "rate_safety_net",
    "lossless_stripes_1", "lossless_stripes_2", "lossless_stripes_3_or_more", "lossless_stripe_no_bytes",
)
PCRD_MAX_CELLS = ("hull_max_pops_one_pass", "hull_max_points")


def pcrd_census_reset():
    lib().oracle_pcrd_census_reset()


def pcrd_census_read() -> dict:
    """The PCRD counters since the last pcrd_census_reset(), by cell name."""
    n = lib().oracle_pcrd_census_read(None, 0)
    assert n == len(PCRD_CELLS), (n, len(PCRD_CELLS))
    cells = np.zeros(n, np.int64)
    lib().oracle_pcrd_census_read(cells.ctypes.data, n)
    return {k: int(v) for k, v in zip(PCRD_CELLS, cells)}


def pcrd_census_add(total: dict | None, c: dict) -> dict:
    if total is None:
        return dict(c)
    for k, v in c.items():
        total[k] = max(total[k], v) if k in PCRD_MAX_CELLS else total[k] + v
    return total


def pcrd_export_enable(on: bool):
    lib().oracle_pcrd_export_enable(1 if on else 0)


def pcrd_export() -> dict:
    """The last encode's selection (oracle_pcrd_export_*): `segments` (key,
    bytes, block, group) sorted by key, descending, within each group;
    `layers` (group, layer, budget, K, Kc) of the final iteration; `blocks`
    (rates, dd, weight, hull, hslope, nl) per block; `iterations`."""
    L = lib()
    n = L.oracle_pcrd_export_segments(None, None, None, None, 0)
    keys, nbytes = np.zeros(n, np.uint64), np.zeros(n, np.int32)
    blocks, groups = np.zeros(n, np.int32), np.zeros(n, np.int32)
    L.oracle_pcrd_export_segments(keys.ctypes.data, nbytes.ctypes.data, blocks.ctypes.data, groups.ctypes.data, n)
    m = L.oracle_pcrd_export_layers(None, None, None, None, None, 0)
    bud, K, Kc = np.zeros(m, np.int64), np.zeros(m, np.uint64), np.zeros(m, np.uint64)
    lg, ll = np.zeros(m, np.int32), np.zeros(m, np.int32)
    L.oracle_pcrd_export_layers(bud.ctypes.data, K.ctypes.data, Kc.ctypes.data, lg.ctypes.data, ll.ctypes.data, m)
    out_blocks = []
    rates, dd = np.zeros(100, np.int32), np.zeros(100, np.int64)
    hull, hslope, nl = np.zeros(101, np.int32), np.zeros(101, np.float64), np.zeros(32, np.int32)
    w, nh = c_double(), c_int()
    i = 0
    while True:
        np_ = L.oracle_pcrd_export_block(i, rates.ctypes.data, dd.ctypes.data, byref(w), hull.ctypes.data,
                                         hslope.ctypes.data, nl.ctypes.data, byref(nh))
        if np_ < 0:
            break
        out_blocks.append(dict(rates=[int(x) for x in rates[:np_]], dd=[int(x) for x in dd[:np_]], weight=w.value,
                               hull=[int(x) for x in hull[:nh.value]], hslope=[float(x) for x in hslope[:nh.value]],
                               nl=[int(x) for x in nl]))
        i += 1
    return dict(segments=[(int(k), int(b), int(bl), int(g)) for k, b, bl, g in zip(keys, nbytes, blocks, groups)],
                layers=[dict(group=int(g), layer=int(l), budget=int(b), K=int(k), Kc=int(kc))
                        for g, l, b, k, kc in zip(lg, ll, bud, K, Kc)],
                blocks=out_blocks, iterations=int(L.oracle_pcrd_export_iterations()))
