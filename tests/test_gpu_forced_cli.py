"""jxg_cjxl --jxg_strategy_in / --jxg_qf_in / --jxg_strategy_out / --jxg_qf_out:
the forced encode from the command line, maps as binary PGMs (one byte per
block).  An encode's own strategy map, fed back, writes the same codestream; a
map of the wrong geometry or one the validator refuses exits 1 and names the
block."""
import subprocess

import numpy as np
import pytest

from sweep_cases import natural as _natural

pytestmark = pytest.mark.gpu

BXS, BYS = 25, 17  # the 200 x 136 image's blocks


def _cli(jxg, *args):
    return subprocess.run([jxg.CLI_PATH] + [str(a) for a in args], capture_output=True, text=True)


def _pgm(path, m):
    m = np.ascontiguousarray(m, np.uint8)
    path.write_bytes(b"P5\n%d %d\n255\n" % (m.shape[1], m.shape[0]) + m.tobytes())
    return path


def _read_pgm(path):
    raw = path.read_bytes()
    head = b"P5\n%d %d\n255\n" % (BXS, BYS)
    assert raw.startswith(head) and len(raw) == len(head) + BXS * BYS
    return np.frombuffer(raw[len(head):], np.uint8).reshape(BYS, BXS)


@pytest.fixture()
def src(tmp_path):
    p = tmp_path / "nat.ppm"
    p.write_bytes(b"P6\n200 136\n255\n" + _natural().tobytes())
    return p


def test_the_written_map_fed_back_gives_the_same_file(jxg_mod, tmp_path, src):
    jxg = jxg_mod
    a, b, c = tmp_path / "A.jxl", tmp_path / "B.jxl", tmp_path / "C.jxl"
    s, q, s2, q2 = (tmp_path / n for n in ("S.pgm", "Q.pgm", "S2.pgm", "Q2.pgm"))
    r = _cli(jxg, src, a, "--effort=7", "--jxg_strategy_out=%s" % s, "--jxg_qf_out=%s" % q)
    assert r.returncode == 0, r.stderr
    r = _cli(jxg, src, b, "--effort=7", "--jxg_strategy_in=%s" % s, "--jxg_strategy_out=%s" % s2)
    assert r.returncode == 0, r.stderr
    assert a.read_bytes() == b.read_bytes()
    assert s.read_bytes() == s2.read_bytes()
    # the maps are the library's: the search encode's KEEP_MAPS arrays
    with jxg.Encoder(distance=1.0, effort=7, flags=jxg.FLAGS_CJXL_DEFAULTS | jxg.FLAG_KEEP_MAPS) as enc:
        assert enc.encode(_natural()) == a.read_bytes()
        st = enc.stats()
    assert np.array_equal(_read_pgm(s), st["acs"]) and np.array_equal(_read_pgm(q), st["qf"])
    assert (st["acs"] & 0x80).any(), "no merged varblock: the case shows nothing"
    # with the quant field too: the maps come back (bytes are the library test's matter)
    r = _cli(jxg, src, c, "--jxg_strategy_in=%s" % s, "--jxg_qf_in=%s" % q,
             "--jxg_strategy_out=%s" % s2, "--jxg_qf_out=%s" % q2)
    assert r.returncode == 0, r.stderr
    assert s2.read_bytes() == s.read_bytes() and q2.read_bytes() == q.read_bytes()
    maps = jxg.decode_maps(c.read_bytes())
    assert np.array_equal(maps["acs"], st["acs"]) and np.array_equal(maps["qf"], st["qf"])


def test_refused_maps_exit_1_and_name_the_block(jxg_mod, tmp_path, src):
    jxg = jxg_mod
    out = tmp_path / "out.jxl"
    # wrong geometry
    r = _cli(jxg, src, out, "--jxg_strategy_in=%s" % _pgm(tmp_path / "w.pgm", np.zeros((17, 24))))
    assert r.returncode == 1 and "24 x 17" in r.stderr and "25 x 17" in r.stderr, r.stderr
    # two 16x16 varblocks overlapping at block (3, 3) = 78
    m = jxg.make_strategy_map(BYS, BXS, [(4, 2, 2)])
    m[3, 3] = 4
    m[3, 4] = m[4, 3] = m[4, 4] = 0x84
    r = _cli(jxg, src, out, "--jxg_strategy_in=%s" % _pgm(tmp_path / "o.pgm", m))
    assert r.returncode == 1 and "block 78 (row 3, column 3)" in r.stderr, r.stderr
    # a 128 px kind
    m = np.zeros((BYS, BXS), np.uint8)
    m[1, 2] = 21
    r = _cli(jxg, src, out, "--jxg_strategy_in=%s" % _pgm(tmp_path / "u.pgm", m))
    assert r.returncode == 1 and "block 27 (row 1, column 2)" in r.stderr, r.stderr
    # a quant field of the wrong geometry, a quant field alone, not a PGM
    ok = _pgm(tmp_path / "ok.pgm", np.zeros((BYS, BXS)))
    r = _cli(jxg, src, out, "--jxg_strategy_in=%s" % ok,
             "--jxg_qf_in=%s" % _pgm(tmp_path / "q.pgm", np.zeros((16, 25))))
    assert r.returncode == 1 and "25 x 16" in r.stderr, r.stderr
    r = _cli(jxg, src, out, "--jxg_qf_in=%s" % ok)
    assert r.returncode == 1 and "--jxg_strategy_in" in r.stderr
    r = _cli(jxg, src, out, "--jxg_strategy_in=%s" % src)
    assert r.returncode == 1 and "PGM" in r.stderr
    assert not out.exists()
    # with --sweep: a usage error
    lst = tmp_path / "points.txt"
    lst.write_text("1 5\n")
    r = _cli(jxg, src, tmp_path / "sweep", "--sweep=%s" % lst, "--jxg_strategy_in=%s" % ok)
    assert r.returncode == 1 and "--sweep" in r.stderr
