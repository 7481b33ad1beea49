"""CPU checks of bench.py's arithmetic and fixtures (the GPU legs run on the
MI355X box): the DWT byte model against SURVEY.md 8(d)'s closed form, the
golden SHA-256 lookups the untimed validation uses, and the CLI parses."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import bench  # noqa: E402


@pytest.mark.parametrize("C,s,L,want", [(3, 1, 6, 22.99), (3, 2, 6, 25.99), (1, 2, 7, 8.666), (4, 1, 6, 30.66)])
def test_dwt_bytes_match_survey_formula(C, s, L, want):
    # B_dwt = C [s + 4 + (8/3)(1 - 4^-(L-1))] with 4-byte coefficients
    assert bench.dwt_bytes_per_px(C, s, L, 4) == pytest.approx(C * (s + 4 + 8 / 3 * (1 - 4.0 ** -(L - 1))), rel=1e-12)
    assert bench.dwt_bytes_per_px(C, s, L, 4) == pytest.approx(want, abs=0.01)


def test_golden_lookups_name_committed_fixtures():
    with open(os.path.join(ROOT, "tests", "golden", "golden.json")) as f:
        g = json.load(f)
    assert bench.golden_sha("c3") == g["c3_full"]["oracle_sha256"]
    assert bench.golden_sha("c4") == g["lossless"][0]["oracle_sha256"]
    c2 = [x for x in g["lossy"] if x["name"] == "c2_synth_rgb8_6000x4000"][0]
    assert bench.golden_sha("c2") == c2["oracle_sha256"]
    assert bench.golden_sha("nope") is None
    for k in ("c2", "c3", "c4"):
        assert len(bench.golden_sha(k)) == 64


def test_cli_parses():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr
    for flag in ("--gpus", "--steps", "--warmup", "--workload", "--full", "--dump-outputs"):
        assert flag in r.stdout


class _File:
    """What bench.dump_outputs takes: an encode's Output, here over bytes."""

    def __init__(self, data):
        self.data, self.closed = data, False

    def view(self):
        return memoryview(self.data)

    def close(self):
        self.closed = True


def test_dump_outputs_is_a_fixed_sample(tmp_path):
    import numpy as np
    rng = np.random.default_rng(7)
    files = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in (70001, 1, 65536)]
    for d in ("a", "b"):
        fs = [_File(f) for f in files]
        bench.dump_outputs(str(tmp_path / d), fs)
        assert all(f.closed for f in fs)
    a = {n: np.load(tmp_path / "a" / f"{n}.npy") for n in ("jpx_len", "jpx_bytesum", "jpx_sample")}
    for n, arr in a.items():  # the same files give the same arrays, run after run
        assert np.array_equal(arr, np.load(tmp_path / "b" / f"{n}.npy"))
    assert a["jpx_len"].dtype == np.float64 and a["jpx_sample"].dtype == np.float32
    assert a["jpx_len"].tolist() == [70001, 1, 65536]
    assert a["jpx_bytesum"].tolist() == [float(sum(f)) for f in files]
    k = a["jpx_sample"].shape[1]
    assert a["jpx_sample"].shape == (3, k) and sum(x.nbytes for x in a.values()) <= 64 << 20
    u = np.sort(np.random.default_rng(bench.DUMP_SEED).random(k))
    for i, f in enumerate(files):
        want = np.frombuffer(f, np.uint8)[(u * len(f)).astype(np.int64)]
        assert np.array_equal(a["jpx_sample"][i], want.astype(np.float32))
    # a changed byte shows: in the sum always, in the sample where it is drawn
    g = bytearray(files[0])
    g[(u[0] * len(g)).astype(np.int64)] ^= 1
    bench.dump_outputs(str(tmp_path / "c"), [_File(bytes(g))])
    assert np.load(tmp_path / "c" / "jpx_bytesum.npy")[0] != a["jpx_bytesum"][0]
    assert np.load(tmp_path / "c" / "jpx_sample.npy")[0, 0] != a["jpx_sample"][0, 0]
