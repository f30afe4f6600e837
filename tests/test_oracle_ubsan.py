"""The oracle under UBSan, stand-alone: oracle/Makefile's `ubsan` target builds
jxo_cli (its own main) with -fsanitize=undefined,float-cast-overflow
-fno-sanitize-recover, and the binary runs as a child process on three frames
of tests/highrate_cases.py at the floor of the distance range, far below it
and at 0.001, under both presets.  Every run must exit 0 and write the bytes
of the plain build.  (Before the floor, 1e-12 ended in "runtime error: ... is
outside the range of representable values of type 'int'" at front.c's quant
field conversion.)  Nothing is loaded into Python under a sanitizer and nothing
is preloaded."""
import os
import subprocess

import pytest

import highrate_cases as H

ORACLE_DIR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle")
FRAMES = ("white72", "edge72", "corners72")
DISTANCES = ("1e-6", "1e-12", "0.001")


def _links_ubsan(tmp):
    src = tmp / "probe.c"
    src.write_text("int main(void) { return 0; }\n")
    cc = os.environ.get("CC", "gcc")
    try:
        p = subprocess.run([cc, "-fsanitize=undefined,float-cast-overflow", "-o",
                            str(tmp / "probe"), str(src)], capture_output=True, text=True)
    except OSError as e:
        return False, str(e)
    return p.returncode == 0, p.stderr.strip()[-300:]


@pytest.fixture(scope="module")
def ubsan_cli(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("ubsan")
    ok, why = _links_ubsan(tmp)
    if not ok:
        pytest.skip("this toolchain cannot link UBSan: %s" % why)
    out = tmp / "bin"
    subprocess.check_call(["make", "-s", "-C", ORACLE_DIR, "ubsan", "UBSAN_OUT=%s" % out])
    return str(out / "jxo_cli")


@pytest.fixture(scope="module")
def ppms(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("ppm")
    paths = {}
    for name in FRAMES:
        img = H.images()[name]
        paths[name] = tmp / (name + ".ppm")
        paths[name].write_bytes(b"P6\n%d %d\n255\n" % (img.shape[1], img.shape[0]) + img.tobytes())
    return paths


@pytest.mark.parametrize("setting", [H.CJXL7, H.PLAIN5], ids=H.setting_id)
@pytest.mark.parametrize("name", FRAMES)
def test_ubsan_clean_and_same_bytes(oracle, ubsan_cli, ppms, tmp_path, name, setting):
    e, p, coder, mask = setting
    for d in DISTANCES:
        out = tmp_path / ("%s-%s.jxl" % (name, d))
        argv = [ubsan_cli, str(ppms[name]), str(out), "--distance=%s" % d, "--effort=%d" % e,
                "--proposals=%s" % ("PF" if p == 3 else "none"),
                "--coder=%s" % ("ans" if coder else "prefix"), "--filters=%d" % mask]
        r = subprocess.run(argv, capture_output=True, text=True)
        assert r.returncode == 0, (d, r.stderr[-600:])
        assert "runtime error" not in r.stderr, (d, r.stderr[-600:])
        ref = oracle.encode(H.images()[name], float(d), e, p, coder, mask)
        assert out.read_bytes() == ref.bytes, d
    assert (tmp_path / ("%s-1e-12.jxl" % name)).read_bytes() == \
        (tmp_path / ("%s-1e-6.jxl" % name)).read_bytes()
