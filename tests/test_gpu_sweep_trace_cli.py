"""jxg_cjxl --sweep=LIST --jxg_sweep_trace=FILE.csv: the search-trace summary of
every point of a sweep from the command line.  The codestreams and the exit
status are the run's without the flag, the CSV holds the numbers of
Encoder.sweep(trace=True) in the text harness.sweep_and_compare writes, a point
without a search writes no rows; without --sweep the flag is refused."""
import csv
import subprocess

import numpy as np
import pytest

from sweep_cases import natural
from test_cli_png import png_bytes

pytestmark = pytest.mark.gpu

GRID = ((1.0, 5), (1.0, 7), (1.0, 4))
RAW = ("Raw DCT8", "Raw DCT4X4", "Raw DCT2X2", "Raw DCT4X8", "Raw DCT8X4", "Raw IDENTITY")


def _cli(jxg, *args):
    return subprocess.run([jxg.CLI_PATH] + [str(a) for a in args], capture_output=True, text=True)


@pytest.fixture()
def src(tmp_path):
    p = tmp_path / "nat.png"
    p.write_bytes(png_bytes(np.array(natural()), 2, filt=0))
    return p


def test_sweep_trace_csv(jxg_mod, tmp_path, src):
    from jxg import harness

    jxg = jxg_mod
    lst = tmp_path / "points.txt"
    lst.write_text("".join("%s %d\n" % (jxg.rust_f64(d), e) for d, e in GRID))
    plain, traced, t = tmp_path / "plain", tmp_path / "traced", tmp_path / "T.csv"
    r0 = _cli(jxg, src, plain, "--sweep=%s" % lst, "--proposals=PF")
    assert r0.returncode == 0, r0.stderr
    r1 = _cli(jxg, src, traced, "--sweep=%s" % lst, "--proposals=PF", "--jxg_sweep_trace=%s" % t)
    assert r1.returncode == r0.returncode, r1.stderr
    names = [jxg.comp_image_name("nat", d, e) for d, e in GRID]
    for name in names:
        assert (traced / name).read_bytes() == (plain / name).read_bytes(), name
    # one line on stderr for the point without a search, and only for it
    lines = [ln for ln in r1.stderr.splitlines() if ln.strip()]
    assert len(lines) == len(r0.stderr.splitlines()) + 1
    assert sum("effort 4" in ln for ln in lines) == 1

    pts = [dict(distance=d, effort=e, proposals=3, flags=jxg.FLAGS_CJXL_DEFAULTS) for d, e in GRID]
    img = np.array(natural())
    t_py = tmp_path / "py.csv"
    with jxg.Encoder() as enc:
        got = enc.sweep(img, pts, quality=None, trace=True)
        datas, _ = harness.sweep_and_compare(enc, "nat.png", img, src.stat().st_size, pts,
                                             trace_file=str(t_py))
    for name, (data, _), d2 in zip(names, got, datas):
        assert (plain / name).read_bytes() == data == d2
    rows = list(csv.DictReader(open(t)))
    assert len(rows) == 12 and [r["Effort"] for r in rows] == ["5"] * 6 + ["7"] * 6
    assert got[2][1]["trace"]["blocks"] == 0
    for j, row in enumerate(rows):
        k, i = divmod(j, 6)
        s = got[k][1]["trace"]
        assert row["Original Image Name"] == "nat.png" and row["Compressed Image Name"] == names[k]
        assert row["Distance"] == "1" and int(row["Scan Index"]) == i
        assert int(row["Strategy"]) == jxg.TRACE_SCAN_IDS[i]
        assert row["Name"] == jxg.STRATEGY_NAMES[jxg.TRACE_SCAN_IDS[i]]
        assert int(row["Blocks"]) == s["blocks"] == 25 * 17
        assert int(row["Max Px"]) == s["max_px"] == (32, 64)[k]
        assert [int(row[c]) for c in RAW] == [int(v) for v in s["flip"][:, i]]
        assert int(row["Scan Wins"]) == int(s["flip"][:, i].sum())
        assert int(row["Hook P"]) == int(s["hook_p"][i])
        assert int(row["Merged Over"]) == int(s["merged_over"][i])
        assert [int(row["Margin %d" % n]) for n in range(8)] == [int(v) for v in s["margin"][i]]
        assert int(row["Margin Skipped"]) == int(s["margin_skipped"][i])
    # the harness parses the file, and writes the same text for the same points
    parsed = harness.read_trace_stats(str(t))
    assert len(parsed) == 12
    want = []
    for k in (0, 1):
        want += harness.trace_stats("nat.png", names[k], GRID[k][0], GRID[k][1], got[k][1]["trace"])
    assert parsed == want
    assert t.read_text() == t_py.read_text()


def test_the_flag_needs_a_sweep(jxg_mod, tmp_path, src):
    out, t = tmp_path / "out.jxl", tmp_path / "T.csv"
    r = _cli(jxg_mod, src, out, "--effort=7", "--jxg_sweep_trace=%s" % t)
    assert r.returncode == 1
    assert "--jxg_sweep_trace" in r.stderr and "--sweep" in r.stderr.replace("--jxg_sweep_trace", "")
    assert not out.exists() and not t.exists()
