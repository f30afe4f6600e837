"""jxg_cjxl --jxg_trace=FILE.csv: the traced encode from the command line.  The
codestream is the one the run without the flag writes, the CSV holds the
summary jxg_search_trace gives, one row per scan index; with --sweep or
--jxg_strategy_in the flag is refused (exit 1)."""
import csv
import subprocess

import numpy as np
import pytest

from sweep_cases import natural as _natural

pytestmark = pytest.mark.gpu

SCAN_IDS = (0, 3, 2, 12, 13, 1)


def _cli(jxg, *args):
    return subprocess.run([jxg.CLI_PATH] + [str(a) for a in args], capture_output=True, text=True)


@pytest.fixture()
def src(tmp_path):
    p = tmp_path / "nat.ppm"
    p.write_bytes(b"P6\n200 136\n255\n" + _natural().tobytes())
    return p


def test_trace_csv_holds_the_summary_and_the_bytes_are_the_same(jxg_mod, tmp_path, src):
    jxg = jxg_mod
    a, b, t = tmp_path / "A.jxl", tmp_path / "B.jxl", tmp_path / "trace.csv"
    r = _cli(jxg, src, a, "--effort=7", "--proposals=PF")
    assert r.returncode == 0, r.stderr
    r = _cli(jxg, src, b, "--effort=7", "--proposals=PF", "--jxg_trace=%s" % t)
    assert r.returncode == 0, r.stderr
    assert a.read_bytes() == b.read_bytes()
    with jxg.Encoder(distance=1.0, effort=7, proposals=3, flags=jxg.FLAGS_CJXL_DEFAULTS) as enc:
        assert enc.encode_traced(_natural()) == a.read_bytes()
        s = enc.search_trace(maps=False)
    rows = list(csv.DictReader(open(t)))
    assert len(rows) == 6
    raw = ("Raw DCT8", "Raw DCT4X4", "Raw DCT2X2", "Raw DCT4X8", "Raw DCT8X4", "Raw IDENTITY")
    for i, row in enumerate(rows):
        assert row["Original Image Name"] == "nat.ppm" and row["Compressed Image Name"] == "B.jxl"
        assert row["Distance"] == "1" and row["Effort"] == "7"
        assert int(row["Scan Index"]) == i and int(row["Strategy"]) == SCAN_IDS[i]
        assert row["Name"] == jxg.STRATEGY_NAMES[SCAN_IDS[i]]
        assert int(row["Blocks"]) == s["blocks"] == 25 * 17 and int(row["Max Px"]) == s["max_px"] == 64
        assert [int(row[k]) for k in raw] == [int(v) for v in s["flip"][:, i]]
        assert int(row["Scan Wins"]) == int(s["flip"][:, i].sum())
        assert int(row["Hook P"]) == int(s["hook_p"][i])
        assert int(row["Merged Over"]) == int(s["merged_over"][i])
        assert [int(row["Margin %d" % k]) for k in range(8)] == [int(v) for v in s["margin"][i]]
        assert int(row["Margin Skipped"]) == int(s["margin_skipped"][i])
    # a second run appends its rows under the one header
    r = _cli(jxg, src, b, "--effort=5", "--jxg_trace=%s" % t)
    assert r.returncode == 0, r.stderr
    rows = list(csv.DictReader(open(t)))
    assert len(rows) == 12 and rows[6]["Effort"] == "5" and rows[6]["Max Px"] == "32"


def test_refused_combinations_exit_1(jxg_mod, tmp_path, src):
    jxg = jxg_mod
    out, t = tmp_path / "out.jxl", tmp_path / "trace.csv"
    lst = tmp_path / "points.txt"
    lst.write_text("1 5\n")
    r = _cli(jxg, src, tmp_path / "sweep", "--sweep=%s" % lst, "--jxg_trace=%s" % t)
    assert r.returncode == 1 and "--jxg_trace" in r.stderr and "--sweep" in r.stderr
    m = tmp_path / "m.pgm"
    m.write_bytes(b"P5\n25 17\n255\n" + np.zeros((17, 25), np.uint8).tobytes())
    r = _cli(jxg, src, out, "--jxg_strategy_in=%s" % m, "--jxg_trace=%s" % t)
    assert r.returncode == 1 and "--jxg_trace" in r.stderr and "--jxg_strategy_in" in r.stderr
    # effort 4 has no search: the library's refusal, exit 1
    r = _cli(jxg, src, out, "--effort=4", "--jxg_trace=%s" % t)
    assert r.returncode == 1 and "unsupported" in r.stderr
    assert not out.exists() and not t.exists()
