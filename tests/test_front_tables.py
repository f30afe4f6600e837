"""front_kernel's constant tables, built by the host-only
csrc/jxg_front_tables.cpp and run as itself (no GPU, nothing loaded into
Python): tests/native/front_tables.cpp is built by g++ from that source alone
-- under ASan + UBSan where the compiler has them -- and prints the five table
blobs for fixed inputs.  Their structure is checked here, and their bytes
against digests recorded from the builder's earlier form (set_front_constants
inside the kernel's HIP file), tests/golden/front_tables.json."""
import hashlib
import json
import os
import shutil
import struct
import subprocess

import pytest

from test_decode_host import _sanitizer_flags

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "jpeg-xl-lossy-image-compression-thesis_amd", "csrc")
NT = 6  # table indices: DCT8, DCT4X4, DCT4X8, DCT8X4, DCT2X2, IDENTITY
QKIND = [0, 1, 2, 2, 4, 3]  # their weight kinds (quant_weights)


@pytest.fixture(scope="module")
def blobs(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no host compiler")
    d = tmp_path_factory.mktemp("ft")
    san = _sanitizer_flags(d)
    if not san:
        print("front_tables: the compiler does not accept the sanitizers; built without them")
    flags = ["-O1", "-std=c++17", "-Wall", "-ffp-contract=off"] + san + os.environ.get(
        "JXG_NATIVE_CFLAGS", "").split()
    exe = d / "front_tables"
    subprocess.check_call(["g++", *flags, os.path.join(ROOT, "tests", "native", "front_tables.cpp"),
                           os.path.join(PKG, "jxg_front_tables.cpp"), "-o", str(exe)])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr
    print("front_tables sanitizers: %s" % ("on" if san else "NOT available"))
    out = {}
    for ln in r.stdout.splitlines():
        name, hexs = ln.split()
        out[name] = bytes.fromhex(hexs)
    assert list(out) == ["wperm", "iwperm", "sdperm", "btab", "zz"]
    return out


def _floats(b):
    return struct.unpack("<%df" % (len(b) // 4), b)


def _source(w):
    """(kind, channel, position) of a synthetic weight (64 (3 kind + c + 1) + pos) * 0.625"""
    n = w / 0.625
    assert n == int(n)
    g, pos = divmod(int(n), 64)
    return (g - 1) // 3, (g - 1) % 3, pos


def test_sizes(blobs):
    assert [len(blobs[k]) for k in ("wperm", "iwperm", "sdperm", "btab", "zz")] == [
        NT * 3 * 64 * 4, NT * 64 * 4, NT * 3 * 64 * 4, 256 * 4, NT * 64]


@pytest.mark.parametrize("ti", range(NT))
def test_slots_cover_the_block(blobs, ti):
    """the 64 (lane r, value k) slots of a table index take their weights from
    64 distinct coefficient positions of the index's weight kind, the same
    positions in the three channels"""
    w = _floats(blobs["wperm"])
    pos = []
    for c in range(3):
        src = [_source(w[(ti * 3 + c) * 64 + i]) for i in range(64)]
        assert {(s[0], s[1]) for s in src} == {(QKIND[ti], c)}
        pos.append([s[2] for s in src])
        assert sorted(pos[c]) == list(range(64))
    assert pos[0] == pos[1] == pos[2]
    if ti == 0:  # DCT8: slot (r, k) is the raster position k * 8 + r
        assert pos[0] == [(i & 7) * 8 + (i >> 3) for i in range(64)]
    # only slot (0, 0) maps to the DC position
    assert pos[0][0] == 0


@pytest.mark.parametrize("ti", range(NT))
def test_zigzag_is_a_permutation(blobs, ti):
    zz = list(blobs["zz"][ti * 64:(ti + 1) * 64])
    assert sorted(zz) == list(range(64))
    assert zz[0] == 0  # DC first


def test_inverse_weights(blobs):
    """iwperm is 1 / (the Y weight at the same slot), rounded once"""
    w, iw = _floats(blobs["wperm"]), _floats(blobs["iwperm"])
    for ti in range(NT):
        for i in range(64):
            wy = w[(ti * 3 + 1) * 64 + i]
            assert abs(wy * iw[ti * 64 + i] - 1.0) <= 2.0 ** -24, (ti, i)


def test_bytes_equal_the_recorded_digests(blobs):
    with open(os.path.join(ROOT, "tests", "golden", "front_tables.json")) as f:
        want = json.load(f)["sha256"]
    assert sorted(want) == sorted(blobs)
    for name, b in blobs.items():
        assert hashlib.sha256(b).hexdigest() == want[name], name
