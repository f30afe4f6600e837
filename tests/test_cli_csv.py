"""jxg_cjxl's CSV text is jxg/harness.py's: the compiled writers of
csrc/jxg_cli_csv.h (tests/native/cli_csv.cpp) against strategy_stats /
rate_stats / ab_stats / trace_stats and their write_*_stats, file bytes against
file bytes, over reports filled by one generator on both sides.  No GPU."""
import ctypes
import functools
import os
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("report", "rates", "ab", "trace")
KEY = ('a,b "q".png', "a-0.5-7.jxl", 0.5, 7)
W, H = 1000, 777


@functools.lru_cache(maxsize=None)
def cli_csv_files():
    """name -> (the file after one run of cli_csv, after a second one)"""
    from test_decode_host import _sanitizer_flags
    import pathlib

    d = pathlib.Path(tempfile.mkdtemp(prefix="cli_csv"))
    flags = ["-O1", "-std=c++17"] + _sanitizer_flags(d)
    exe = str(d / "cli_csv")
    subprocess.check_call(["g++", *flags, os.path.join(ROOT, "tests", "native", "cli_csv.cpp"),
                           "-o", exe])
    out = d / "out"
    out.mkdir()
    files = []
    for _ in range(2):
        r = subprocess.run([exe, str(out)], capture_output=True, text=True)
        assert r.returncode == 0 and not r.stderr, r.stderr
        files.append({n: (out / (n + ".csv")).read_bytes() for n in NAMES})
    return {n: (files[0][n], files[1][n]) for n in NAMES}


class _Lcg:
    def __init__(self):
        self.s = 12345

    def __call__(self):
        self.s = (self.s * 6364136223846793005 + 1442695040888963407) & (2 ** 64 - 1)
        return self.s >> 33


def _words(obj, ctype):
    return (ctype * (ctypes.sizeof(obj) // ctypes.sizeof(ctype))).from_buffer(obj)


def _python_files(jxg_mod, d):
    """the same reports as cli_csv.cpp fills, through the harness's writers"""
    from jxg import harness

    nxt = _Lcg()
    rep = jxg_mod._StrategyReport()
    w = _words(rep, ctypes.c_uint64)
    for i in range(len(w)):
        w[i] = nxt() % 1000003
    for i in range(0, jxg_mod.NUM_STRATEGIES, 4):
        rep.row[i].blocks = 0
    rates = jxg_mod._RateReport()
    w = _words(rates.row, ctypes.c_uint64)
    for i in range(len(w)):
        v = nxt() % 100000007
        w[i] = 0 if i % 5 == 0 else v
    rates.ac_bits = nxt() % 100000007
    rates.stream_bits = nxt() % 100000007
    ab = jxg_mod._AbReport()
    for i in range(len(ab.cell)):
        v = nxt() % 10000019
        ab.cell[i] = v if (i // 6) % 7 == 0 else 0
    tr = jxg_mod._TraceSummary()
    w = _words(tr, ctypes.c_uint32)
    for i in range(len(w)):
        w[i] = nxt() % 4099
    orig, comp, dist, effort = KEY
    rows = {"report": harness.strategy_stats(orig, comp, dist, effort, rep.as_dict(), W, H),
            "rates": harness.rate_stats(orig, comp, dist, effort, rates.as_dict()),
            "ab": harness.ab_stats(orig, comp, comp, dist, effort, ab.as_dict(), W, H),
            "trace": harness.trace_stats(orig, comp, dist, effort, tr.as_dict())}
    write = {"report": harness.write_strategy_stats, "rates": harness.write_rate_stats,
             "ab": harness.write_ab_stats, "trace": harness.write_trace_stats}
    out = {}
    for n in NAMES:
        path = os.path.join(d, n + ".csv")
        write[n](rows[n], path)
        once = open(path, "rb").read()
        write[n](rows[n], path)
        out[n] = (once, open(path, "rb").read())
    return out


@pytest.fixture(scope="module")
def both(jxg_mod, tmp_path_factory):
    return cli_csv_files(), _python_files(jxg_mod, str(tmp_path_factory.mktemp("py_csv")))


@pytest.mark.parametrize("name,lines", zip(NAMES, (21, 28, 106, 7)), ids=NAMES)
def test_the_compiled_writers_give_the_harness_bytes(both, name, lines):
    cli, py = both
    assert cli[name][0] == py[name][0]
    assert len(cli[name][0].splitlines()) == lines


@pytest.mark.parametrize("name", NAMES)
def test_a_second_call_appends_rows_without_a_second_header(both, name):
    cli, py = both
    once, twice = cli[name]
    header, rows = once.split(b"\n", 1)
    assert twice == once + rows and twice.count(header) == 1
    assert twice == py[name][1]
