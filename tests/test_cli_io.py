"""The command-line tools' file readers (csrc/jxg_cli_io.h: PNG, PPM, PGM) in a
stand-alone program under the host sanitizers (tests/native/cli_io.cpp), as
test_decode_host.py does for the codestream decoder: thousands of damaged PNGs,
crafted headers, and the PNG writer against the reader.  No GPU, nothing
loaded into Python."""
import os
import shutil
import subprocess
import time

import numpy as np
import pytest

import cli_cases
from test_cli_png import png_bytes
from test_decode_host import _sanitizer_flags

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
           UBSAN_OPTIONS="print_stacktrace=1")


@pytest.fixture(scope="module")
def cli_io_bin(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no host compiler")
    d = tmp_path_factory.mktemp("cli_io")
    san = _sanitizer_flags(d)
    if not san:
        print("cli_io: the compiler does not accept the sanitizers; built without them")
    flags = ["-O1", "-std=c++17"] + san + os.environ.get("JXG_NATIVE_CFLAGS", "").split()
    exe = d / "cli_io"
    subprocess.check_call(["g++", *flags, os.path.join(ROOT, "tests", "native", "cli_io.cpp"),
                           "-o", str(exe), "-lz"])
    return str(exe)


def _run(exe, *args):
    r = subprocess.run([exe, *map(str, args)], capture_output=True, text=True, timeout=600, env=ENV)
    print(r.stdout.strip())
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr
    return r.stdout


@pytest.mark.parametrize("ctype,ch", [(2, 3), (6, 4), (0, 1), (4, 2)])
def test_damaged_pngs_never_leave_their_buffers(cli_io_bin, tmp_path, ctype, ch):
    """test_cli_png's 37 x 53 image (seven IDAT pieces, rows cycling through the
    five filters) decodes to its source; then 2000 single-byte changes spread
    over the file and 200 truncations: every call returns, no report"""
    rng = np.random.default_rng(ctype * 10 + 7)
    img = rng.integers(0, 256, (37, 53, ch), dtype=np.uint8)
    img[:, :20] = img[:, :1]
    rgb = img[..., :3] if ch >= 3 else np.repeat(img[..., :1], 3, axis=2)
    (tmp_path / "in.png").write_bytes(png_bytes(img, ctype, 7))
    (tmp_path / "in.rgb").write_bytes(np.ascontiguousarray(rgb).tobytes())
    out = _run(cli_io_bin, "mutate", tmp_path / "in.png", tmp_path / "in.rgb", 2000, 200)
    assert "unmutated: ok" in out and "2000 byte changes" in out


@pytest.mark.parametrize("kind,cases", [("png", cli_cases.bad_pngs()), ("ppm", cli_cases.bad_ppms()),
                                        ("pgm", cli_cases.bad_pgms())], ids=["png", "ppm", "pgm"])
def test_crafted_files_are_refused(cli_io_bin, tmp_path, kind, cases):
    """each with a message, probe_dims 0 x 0, and at once: the 2^18 x 2^18
    header over 60 bytes of IDAT allocates nothing"""
    paths = []
    for name, data in cases.items():
        paths.append(tmp_path / (name + "." + kind))
        paths[-1].write_bytes(data)
    t = time.monotonic()
    out = _run(cli_io_bin, "refuse", kind, *paths)
    assert time.monotonic() - t < 5.0
    lines = out.splitlines()
    assert len(lines) == len(cases) and not any(ln.endswith(": read") for ln in lines)
    if kind == "png":
        assert dict(zip(cases, lines))["huge_over_60_bytes"].endswith("truncated PNG")


def test_a_pgm_with_a_comment_reads(cli_io_bin, tmp_path):
    (name, data), = cli_cases.good_pgms().items()
    (tmp_path / "m.pgm").write_bytes(data)
    assert _run(cli_io_bin, "accept", "pgm", tmp_path / "m.pgm").strip().endswith(": read")


def test_png_writer_and_reader_round_trip(cli_io_bin):
    out = _run(cli_io_bin, "roundtrip")
    assert [ln.split(":")[0] for ln in out.splitlines()] == ["1 x 1", "53 x 37", "1500 x 400"]
