"""tests/native/ac_model.cpp built once per session (helper of test_ac_model.py
and test_ac_bands.py; not a conftest): g++ compiles the program against
csrc/jxg_acmodel.h, jxg_acrec.h and jxg_shapes.h, gcc the oracle's tables
(oracle/entropy.c), under ASan + UBSan where the compiler has them.  Nothing
is loaded into Python."""
import os
import shutil
import subprocess

import pytest

from test_decode_host import _sanitizer_flags

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_built = []


def build(tmp_path_factory):
    """the program's path (built by the first caller of the session)"""
    if _built:
        return _built[0]
    if shutil.which("g++") is None or shutil.which("gcc") is None:
        pytest.skip("no host compiler")
    d = tmp_path_factory.mktemp("acm")
    san = _sanitizer_flags(d)
    print("ac_model sanitizers: %s" % ("on" if san else "NOT available"))
    extra = os.environ.get("JXG_NATIVE_CFLAGS", "").split()
    obj = d / "entropy.o"
    subprocess.check_call(["gcc", "-O1", "-c", *san, os.path.join(ROOT, "oracle", "entropy.c"),
                           "-o", str(obj)])
    exe = d / "ac_model"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", *san, *extra,
                           os.path.join(ROOT, "tests", "native", "ac_model.cpp"), str(obj),
                           "-o", str(exe)])
    _built.append(str(exe))
    return _built[0]


def run(exe, mode=None, stdin=""):
    """the program's output lines"""
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe] + ([mode] if mode else []), input=stdin, capture_output=True,
                       text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr
    return r.stdout.splitlines()
