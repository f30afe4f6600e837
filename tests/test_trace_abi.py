"""Search trace (jxg_encode_traced_rgb8 / jxg_search_trace): what
holds without a device -- the entry points exist, refuse null arguments, and
the Python mirrors have the header's layout."""
import ctypes
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARG = -1
NEW = ("jxg_encode_traced_rgb8", "jxg_encode_traced_rgb8_device", "jxg_search_trace")


def test_new_symbols_are_exported(jxg_mod):
    lib = jxg_mod.load()
    for name in NEW:
        assert name in jxg_mod.EXPORTS
        assert getattr(lib, name) is not None


def test_null_arguments_are_refused_without_a_device(jxg_mod):
    lib = jxg_mod.load()
    img = np.zeros((16, 16, 3), np.uint8)
    buf = jxg_mod._Buffer()
    buf.size = 7
    for fn in (lib.jxg_encode_traced_rgb8, lib.jxg_encode_traced_rgb8_device):
        assert fn(None, img.ctypes.data, 16, 16, 48, ctypes.byref(buf)) == INVALID_ARG
        assert not buf.data and buf.size == 0  # *out = {NULL, 0}
        assert fn(None, None, 16, 16, 48, None) == INVALID_ARG
    maps, summary = jxg_mod._TraceMaps(), jxg_mod._TraceSummary()
    assert lib.jxg_search_trace(None, None, None) == INVALID_ARG
    assert lib.jxg_search_trace(None, ctypes.byref(maps), ctypes.byref(summary)) == INVALID_ARG


def test_python_mirrors_follow_the_header(jxg_mod):
    src = open(os.path.join(ROOT, "include", "jxg.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} jxg_trace_maps;", src).group(1)
    fields = re.findall(r"(float|uint8_t)\* (\w+);", body)
    assert [n for _, n in fields] == [n for n, _ in jxg_mod._TraceMaps._fields_]
    dtypes = {n: dt for n, _, dt in jxg_mod._TRACE_PLANES}
    for ctype, name in fields:
        assert dtypes[name] == (np.float32 if ctype == "float" else np.uint8), name
    body = re.search(r"typedef struct \{([^}]*)\} jxg_trace_summary;", src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    words = 0
    names = []
    for name, dims in re.findall(r"uint32_t (\w+)((?:\[\d+\])*);", body):
        names.append(name)
        n = 1
        for d in re.findall(r"\[(\d+)\]", dims):
            n *= int(d)
        words += n
    assert names == [n for n, _ in jxg_mod._TraceSummary._fields_]
    assert ctypes.sizeof(jxg_mod._TraceSummary) == 4 * words == 4 * 104
    s = jxg_mod._TraceSummary()
    s.blocks, s.max_px = 425, 64
    s.flip[1 * 6 + 4] = 3
    s.margin[5 * 8 + 7] = 9
    s.margin_skipped[2] = 1
    d = s.as_dict()
    assert d["blocks"] == 425 and d["max_px"] == 64
    assert d["flip"].shape == (6, 6) and d["flip"][1, 4] == 3
    assert d["margin"].shape == (6, 8) and d["margin"][5, 7] == 9
    assert d["margin_skipped"][2] == 1 and d["hook_p"].shape == (6,) and d["merged_over"].shape == (6,)
    assert len(jxg_mod.TRACE_SCAN_IDS) == 6 and len(jxg_mod.TRACE_MERGED_IDS) == 9
    assert len(jxg_mod.TRACE_BIG_IDS) == 6
