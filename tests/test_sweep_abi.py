"""jxg_sweep_rgb8 without a device: the three symbols, the call-level refusals
that need no context (nothing is touched), the Python and harness entry points
and the CLI's --sweep argument handling."""
import ctypes
import subprocess

import pytest

INVALID_ARG = -1
SENTINEL = 0x5A5A5A5A


def test_symbols_exported(jxg_mod):
    lib = jxg_mod.load()
    for name in ("jxg_sweep_rgb8", "jxg_sweep_rgb8_device", "jxg_sweep_timings"):
        assert hasattr(lib, name), name
        assert name in jxg_mod.EXPORTS


def _args(jxg_mod, n=2):
    pts = (jxg_mod._SweepPoint * n)(*[jxg_mod._SweepPoint(1.0, 7, 0, 0) for _ in range(n)])
    outs = (jxg_mod._Buffer * n)()
    for o in outs:
        o.size = SENTINEL
    st = (ctypes.c_int * n)(*[SENTINEL] * n)
    rgb = (ctypes.c_uint8 * (16 * 16 * 3))()
    return pts, outs, st, rgb


@pytest.mark.parametrize("fn", ["jxg_sweep_rgb8", "jxg_sweep_rgb8_device"])
def test_null_context_is_refused_and_touches_nothing(jxg_mod, fn):
    f = getattr(jxg_mod.load(), fn)
    pts, outs, st, rgb = _args(jxg_mod)
    q = (jxg_mod._Quality * 2)()
    for quality, qq in ((0, None), (2, q)):
        assert f(None, ctypes.addressof(rgb), 16, 16, 48, pts, 2, quality, outs, qq, st) == INVALID_ARG
        assert [o.size for o in outs] == [SENTINEL] * 2
        assert list(st) == [SENTINEL] * 2
    # every argument is checked before the context is used: a null context
    # with other bad arguments is still only a refusal
    assert f(None, None, 16, 16, 48, pts, 2, 0, outs, None, st) == INVALID_ARG
    assert f(None, ctypes.addressof(rgb), 16, 16, 48, None, 2, 0, outs, None, st) == INVALID_ARG
    assert f(None, ctypes.addressof(rgb), 16, 16, 48, pts, 0, 0, outs, None, st) == INVALID_ARG
    assert f(None, ctypes.addressof(rgb), 16, 16, 47, pts, 2, 0, outs, None, st) == INVALID_ARG
    assert f(None, ctypes.addressof(rgb), 16, 16, 48, pts, 2, 0, None, None, st) == INVALID_ARG
    assert [o.size for o in outs] == [SENTINEL] * 2


def test_timings_null_arguments(jxg_mod):
    lib = jxg_mod.load()
    s = jxg_mod._SweepStats()
    assert lib.jxg_sweep_timings(None, ctypes.byref(s)) == INVALID_ARG


def test_python_entry_points(jxg_mod):
    from jxg import harness

    for name in ("sweep", "sweep_device", "sweep_timings"):
        assert callable(getattr(jxg_mod.Encoder, name)), name
    assert callable(harness.sweep_and_compare)
    pts = jxg_mod.Encoder._sweep_points([dict(distance=0.5, effort=7, flags=4), (2.0, 5),
                                         (1.0, 8, 3, 16)])
    assert [(p.distance, p.effort, p.proposals, p.flags) for p in pts] == [
        (0.5, 7, 0, 4), (2.0, 5, 0, 0), (1.0, 8, 3, 16)]


def test_cli_sweep_list_errors(jxg_mod, tmp_path):
    """a missing or malformed list ends the process before any device is used"""
    src = tmp_path / "in.ppm"
    src.write_bytes(b"P6\n8 8\n255\n" + bytes(8 * 8 * 3))
    bad = tmp_path / "bad.txt"
    bad.write_text("1.0 seven\n")
    for lst in (tmp_path / "missing.txt", bad):
        p = subprocess.run([jxg_mod.CLI_PATH, str(src), str(tmp_path / "out"), "--sweep=%s" % lst],
                           capture_output=True, text=True)
        assert p.returncode == 1
        assert "--sweep: cannot read the list" in p.stderr
    assert not (tmp_path / "out").exists()
