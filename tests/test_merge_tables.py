"""The merge stage's host-built tables (csrc/jxg_tables.cpp build_merge_tables:
per-shape weights, distortion weights, inverse Y weights and natural orders in
row quads, Lee constants, LLF scales), run as itself (no GPU, nothing loaded
into Python): tests/native/merge_tables.cpp is built by g++ -- under ASan +
UBSan where the compiler has them -- and prints the eight blobs.  The builder
takes the nine shapes from csrc/jxg_shapes.h; the blobs' structure is checked
here against a restatement of that table, and their bytes against digests
recorded from the builder's earlier form (its own kShapeDims),
tests/golden/merge_tables.json."""
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
HIP_INC = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")
# kShapes order: (blocks down, blocks across)
SHAPES = [(2, 1), (1, 2), (2, 2), (4, 2), (2, 4), (4, 4), (8, 4), (4, 8), (8, 8)]
STOT = sum(64 * cy * cx for cy, cx in SHAPES)
NAMES = ["wk", "sdk", "iwy", "nat", "lee_c", "lee_s", "llf_p", "llf_ib"]


@pytest.fixture(scope="module")
def blobs(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no host compiler")
    if not os.path.exists(os.path.join(HIP_INC, "hip", "hip_runtime.h")):
        pytest.skip("no HIP headers")
    d = tmp_path_factory.mktemp("mt")
    san = _sanitizer_flags(d)
    if not san:
        print("merge_tables: the compiler does not accept the sanitizers; built without them")
    flags = ["-O1", "-std=c++17", "-Wall", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__",
             "-isystem", HIP_INC] + san + os.environ.get("JXG_NATIVE_CFLAGS", "").split()
    exe = d / "merge_tables"
    subprocess.check_call(["g++", *flags, os.path.join(ROOT, "tests", "native", "merge_tables.cpp"),
                           os.path.join(PKG, "jxg_tables.cpp"), os.path.join(PKG, "jxg_dequant.cpp"),
                           "-o", str(exe)])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr
    print("merge_tables sanitizers: %s" % ("on" if san else "NOT available"))
    out = {}
    for ln in r.stdout.splitlines():
        name, hexs = ln.split()
        out[name] = bytes.fromhex(hexs)
    assert list(out) == NAMES
    return out


def _floats(b):
    return struct.unpack("<%df" % (len(b) // 4), b)


def _shape_slices():
    off = 0
    for cy, cx in SHAPES:
        yield cy, cx, off
        off += 64 * cy * cx


def test_sizes(blobs):
    assert STOT == 10752
    assert [len(blobs[k]) for k in NAMES] == [
        3 * STOT * 4, 3 * STOT * 4, STOT * 4, STOT * 2, 7 * 32 * 4, 7 * 64 * 4, 4 * 8 * 4, 4 * 64 * 4]


def test_llf_positions_carry_no_weight(blobs):
    """row quads [ky / 4][kx][ky % 4]: the first cy x cx positions of a shape
    have weight and distortion weight 0 in every channel, all others a
    positive weight"""
    wk, sdk = _floats(blobs["wk"]), _floats(blobs["sdk"])
    for cy, cx, off in _shape_slices():
        R, C = 8 * cy, 8 * cx
        for c in range(3):
            for ky in range(R):
                for kx in range(C):
                    i = c * STOT + off + ((ky >> 2) * C + kx) * 4 + (ky & 3)
                    if ky < cy and kx < cx:
                        assert wk[i] == 0.0 and sdk[i] == 0.0, (cy, cx, c, ky, kx)
                    else:
                        assert wk[i] > 0.0 and sdk[i] > 0.0, (cy, cx, c, ky, kx)


def test_natural_order_is_a_permutation_per_shape(blobs):
    nat = struct.unpack("<%dH" % STOT, blobs["nat"])
    for cy, cx, off in _shape_slices():
        n = 64 * cy * cx
        assert sorted(nat[off:off + n]) == list(range(n)), (cy, cx)


def test_inverse_y_weights(blobs):
    """iwy is 1 / (the Y weight of the shape's kind at the same position),
    rounded once; the LLF positions keep the kind's weight there"""
    wk, iwy = _floats(blobs["wk"]), _floats(blobs["iwy"])
    for cy, cx, off in _shape_slices():
        R, C = 8 * cy, 8 * cx
        for ky in range(R):
            for kx in range(C):
                i = off + ((ky >> 2) * C + kx) * 4 + (ky & 3)
                assert iwy[i] > 0.0
                if not (ky < cy and kx < cx):
                    assert abs(wk[STOT + i] * iwy[i] - 1.0) <= 2.0 ** -24, (cy, cx, ky, kx)


def test_bytes_equal_the_recorded_digests(blobs):
    with open(os.path.join(ROOT, "tests", "golden", "merge_tables.json")) as f:
        want = json.load(f)["sha256"]
    assert sorted(want) == sorted(blobs)
    for name, b in blobs.items():
        assert hashlib.sha256(b).hexdigest() == want[name], name
