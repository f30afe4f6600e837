"""jxg_cjxl --jxg_ab=FILE.csv [--jxg_ab_base=...]: the codestreams written are
those of a run without the option, and the rows are harness.ab_stats of the
Python report of the same two encodes."""
import subprocess

import pytest

from sweep_cases import natural as _natural

pytestmark = pytest.mark.gpu

def _report(jxg, distance, effort, base, proposals):
    """(side B's codestream, A/B report) of two fresh encoders at cjxl's defaults"""
    img = _natural()
    kw = dict(distance=distance, effort=effort, flags=jxg.FLAGS_CJXL_DEFAULTS)
    with jxg.Encoder(proposals=base, **kw) as ea, jxg.Encoder(proposals=proposals, **kw) as eb:
        ea.encode(img)
        data = eb.encode(img)
        return data, jxg.ab_report(ea, eb, img)


def _run(jxg, *args):
    p = subprocess.run([jxg.CLI_PATH] + [str(a) for a in args], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr


def test_cli_one_encode(jxg_mod, tmp_path):
    from jxg import harness

    jxg = jxg_mod
    src = tmp_path / "nat.ppm"
    src.write_bytes(b"P6\n200 136\n255\n" + _natural().tobytes())
    plain, out = tmp_path / "plain.jxl", tmp_path / "nat-1-7.jxl"
    csv_cli, csv_py = tmp_path / "cli.csv", tmp_path / "py.csv"
    _run(jxg, src, plain, "--distance=1", "--effort=7", "--proposals=PF")
    _run(jxg, src, out, "--distance=1", "--effort=7", "--proposals=PF", "--jxg_ab=%s" % csv_cli)
    data, rep = _report(jxg, 1.0, 7, 0, 3)
    assert out.read_bytes() == plain.read_bytes() == data
    rows = harness.ab_stats("nat.ppm", "nat-1-7.jxl", "nat-1-7.jxl", 1.0, 7, rep, 200, 136)
    assert len(rows) > 1 and any(r.from_strategy != r.to_strategy for r in rows)
    harness.write_ab_stats(rows, str(csv_py))
    assert csv_cli.read_text() == csv_py.read_text()
    assert harness.read_ab_stats(str(csv_cli)) == rows
    # another base, appended to the same file
    _run(jxg, src, out, "--distance=1", "--effort=7", "--proposals=PF", "--jxg_ab=%s" % csv_cli,
         "--jxg_ab_base=P")
    assert out.read_bytes() == data
    harness.write_ab_stats(harness.ab_stats("nat.ppm", "nat-1-7.jxl", "nat-1-7.jxl", 1.0, 7,
                                            _report(jxg, 1.0, 7, 1, 3)[1], 200, 136), str(csv_py))
    assert csv_cli.read_text() == csv_py.read_text()


def test_cli_sweep(jxg_mod, tmp_path):
    from jxg import harness

    jxg = jxg_mod
    src = tmp_path / "nat.ppm"
    src.write_bytes(b"P6\n200 136\n255\n" + _natural().tobytes())
    lst = tmp_path / "points.txt"
    lst.write_text("1 5\n4 7\n2 8\n")
    plain, outdir = tmp_path / "plain", tmp_path / "sweep"
    csv_cli, csv_py = tmp_path / "cli.csv", tmp_path / "py.csv"
    _run(jxg, src, plain, "--sweep=%s" % lst, "--proposals=F")
    _run(jxg, src, outdir, "--sweep=%s" % lst, "--proposals=F", "--jxg_ab=%s" % csv_cli)
    assert sorted(f.name for f in outdir.iterdir()) == sorted(f.name for f in plain.iterdir())
    for d, e in ((1.0, 5), (4.0, 7), (2.0, 8)):
        name = jxg.comp_image_name("nat", d, e)
        data, rep = _report(jxg, d, e, 0, 2)
        assert (outdir / name).read_bytes() == (plain / name).read_bytes() == data
        harness.write_ab_stats(harness.ab_stats("nat.ppm", name, name, d, e, rep, 200, 136),
                               str(csv_py))
    assert csv_cli.read_text() == csv_py.read_text()
