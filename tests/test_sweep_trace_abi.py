"""Search-trace summaries in a sweep (jxg_set_sweep_trace / jxg_sweep_trace,
DESIGN.md 3.20) without a device: the pair is exported and refuses a null
context, Python has the rider's row, and the harness's CSV text is the command
line's."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARG = -1


def test_the_pair_is_exported_and_refuses_a_null_context(jxg_mod):
    lib = jxg_mod.load()
    for name in ("jxg_set_sweep_trace", "jxg_sweep_trace"):
        assert hasattr(lib, name), name
        assert name in jxg_mod.EXPORTS
    for on in (0, 1):
        assert lib.jxg_set_sweep_trace(None, on) == INVALID_ARG
    out = (jxg_mod._TraceSummary * 2)()
    ctypes.memset(out, 0xA5, ctypes.sizeof(out))
    assert lib.jxg_sweep_trace(None, out, 2) == INVALID_ARG
    assert bytes(out) == b"\xa5" * ctypes.sizeof(out), "nothing written"


def test_python_has_the_riders_row(jxg_mod):
    rows = [r for r in jxg_mod.Encoder._RIDERS if r[0] == "trace"]
    assert len(rows) == 1
    name, setter, off, getter, ctype, put = rows[0]
    assert (setter, off, getter) == ("jxg_set_sweep_trace", (0,), "jxg_sweep_trace")
    assert ctype is jxg_mod._TraceSummary
    s = jxg_mod._TraceSummary()
    s.blocks = 7
    d = put(s)
    assert list(d) == ["trace"] and d["trace"]["blocks"] == 7
    assert d["trace"]["flip"].shape == (6, 6)


def test_the_header_describes_the_getter():
    src = open(os.path.join(ROOT, "include", "jxg.h")).read()
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*jxg_status jxg_set_sweep_trace\(jxg_ctx\* ctx, int on\);\s*"
                  r"jxg_status jxg_sweep_trace\(jxg_ctx\* ctx, jxg_trace_summary\* out, uint32_t n\);",
                  src, re.S)
    assert m, "the pair's declarations under one comment"
    text = " ".join(m.group(1).replace("*", " ").split())
    for phrase in ("jxg_sweep_trace copies the last sweep's summaries out in point order",
                   "bit-equal", "jxg_search_trace", "jxg_encode_traced_rgb8", "effort < 5",
                   "zero-filled", "blocks == 0", "115 bytes a block", "JXG_ERR_INVALID_ARG"):
        assert phrase in text, phrase
    assert "sweep, sharded or forced" not in src  # (the traced encode's old "no sweep form")


def _cli_header():
    """the header line the compiled writer (csrc/jxg_cli_csv.h) puts into a new file"""
    from test_cli_csv import cli_csv_files

    text = cli_csv_files()["trace"][0].decode().split("\n", 1)[0]
    return text.split(",")


def test_the_harness_header_is_the_command_lines():
    from jxg import harness

    assert harness.TRACE_HEADER == _cli_header()
    assert len(harness.TRACE_HEADER) == 27
    from dataclasses import fields

    assert len(fields(harness.TraceStat)) == len(harness.TRACE_HEADER)


def _summary():
    rng = np.random.default_rng(20)
    return {"blocks": 425, "max_px": 64,
            "flip": rng.integers(0, 50, (6, 6)).astype(np.uint32),
            "hook_p": rng.integers(0, 50, 6).astype(np.uint32),
            "merged_over": rng.integers(0, 50, 6).astype(np.uint32),
            "margin": rng.integers(0, 50, (6, 8)).astype(np.uint32),
            "margin_skipped": rng.integers(0, 50, 6).astype(np.uint32)}


def test_trace_stats_rows(jxg_mod, tmp_path):
    from jxg import harness

    s = _summary()
    rows = harness.trace_stats("photo.png", "photo-1-7.jxl", 1.0, 7, s)
    assert len(rows) == 6
    for i, r in enumerate(rows):
        assert (r.orig_image_name, r.comp_image_name, r.distance, r.effort) == (
            "photo.png", "photo-1-7.jxl", 1.0, 7)
        assert r.scan_index == i and r.strategy == jxg_mod.TRACE_SCAN_IDS[i]
        assert r.name == jxg_mod.STRATEGY_NAMES[r.strategy]
        assert r.blocks == 425 and r.max_px == 64
        assert r.scan_wins == int(s["flip"][:, i].sum())
        assert [r.raw_dct8, r.raw_dct4x4, r.raw_dct2x2, r.raw_dct4x8, r.raw_dct8x4,
                r.raw_identity] == [int(v) for v in s["flip"][:, i]]
        assert r.hook_p == s["hook_p"][i] and r.merged_over == s["merged_over"][i]
        assert [getattr(r, "margin_%d" % k) for k in range(8)] == [int(v) for v in s["margin"][i]]
        assert r.margin_skipped == s["margin_skipped"][i]
        # row() / parse() round-trip, every value column an integer's text
        rec = r.row()
        assert len(rec) == 27 and all(isinstance(v, str) for v in rec)
        assert rec[2] == "1" and all(v.isdigit() for v in rec[3:6] + rec[7:])
        assert harness.TraceStat.parse(rec) == r
    assert [r.name for r in rows] == ["DCT8", "DCT4X4", "DCT2X2", "DCT4X8", "DCT8X4", "IDENTITY"]
    # through a file: one header, rows appended
    f = str(tmp_path / "trace.csv")
    harness.write_trace_stats(rows, f)
    harness.write_trace_stats(rows[:2], f)
    lines = open(f).read().splitlines()
    assert lines[0].split(",") == harness.TRACE_HEADER and len(lines) == 1 + 8
    assert harness.read_trace_stats(f) == rows + rows[:2]


def test_sweep_keyword_exists(jxg_mod):
    import inspect

    for fn in (jxg_mod.Encoder.sweep, jxg_mod.Encoder.sweep_device):
        assert inspect.signature(fn).parameters["trace"].default is False
    from jxg import harness

    assert inspect.signature(harness.sweep_and_compare).parameters["trace_file"].default is None
