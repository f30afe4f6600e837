"""jxg_rate_report[_device], the sweep's rate reports, the harness file and the
CLI option against tests/rate_ref.py.  Every field is an integer, so every
comparison is exact equality: no tolerance anywhere.  The reference prices the
encoder's own codestream through the oracle decoder -- the stream's histograms
and codes, not the tables the kernel reads."""
import ctypes
import subprocess

import numpy as np
import pytest

import rate_ref
from sweep_cases import INVALID_ARG, RefusedAndGood, cached, natural as _natural, poisoned
from sweep_cases import points as _points, qbits as _qbits, same
from test_recon_cases import CASES, case_flags, case_image

pytestmark = pytest.mark.gpu

KEYS = ("tokens", "cost", "ac_bits", "stream_bits", "ans", "groups")
# prefix-code twins: 128 / 256 px varblocks across bands, both hooks, every filter
TWINS = [tuple(c[:8]) + (0, c[9]) for c in CASES
         if c[0] in ("gradient_e8", "natural_hooks", "natural_d1_all")]
TWINS = [(c[0] + "_prefix",) + c[1:] for c in TWINS]
ALL = CASES + TWINS


_same = same(KEYS, lambda a, b, k: a["tokens"].dtype == np.uint64)


def _check(jxg, enc, data, w, h):
    """the report of enc's last encode (to data) against the reference; the
    device variant; a second call"""
    import torch

    ref = rate_ref.reference(data)
    got = enc.rate_report(block_map=True)
    for k in ("tokens", "cost"):
        assert got[k].shape == (27, 3) and got[k].dtype == np.uint64
        assert np.array_equal(got[k], ref[k]), (k, got[k].tolist(), ref[k].tolist())
    bmap = got["block_cost"]
    assert bmap.dtype == np.uint32 and bmap.shape == ((h + 7) // 8, (w + 7) // 8)
    assert np.array_equal(bmap, ref["block_cost"]), np.argwhere(bmap != ref["block_cost"])[:8]
    total = int(got["cost"].sum())
    assert int(bmap.astype(np.uint64).sum()) == total
    assert got["groups"] == ref["groups"] and got["ans"] == ref["ans"]
    assert got["stream_bits"] == 8 * len(data)
    assert got["ac_bits"] == sum(ref["group_bits"]), "the bits the reader consumed"
    if not got["ans"]:
        assert total == 256 * got["ac_bits"]
    if got["groups"] > 1:
        assert 0 <= 8 * sum(ref["group_bytes"]) - got["ac_bits"] < 8 * got["groups"]
    # the map in device memory, pre-filled: identical and no word left
    d_map = torch.full(bmap.shape, -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    again = enc.rate_report_device(d_map.data_ptr())
    assert _same(again, got)
    assert np.array_equal(d_map.cpu().numpy().view(np.uint32), bmap)
    assert _same(enc.rate_report_device(), got)
    third = enc.rate_report(block_map=True)
    assert _same(third, got) and third["block_cost"].tobytes() == bmap.tobytes()
    return got


@pytest.mark.parametrize("case", ALL, ids=[c[0] for c in ALL])
def test_report_equals_the_reference(jxg_mod, case):
    img = case_image(case)
    with jxg_mod.Encoder(distance=case[5], effort=case[6], proposals=case[7],
                         flags=case_flags(jxg_mod, case)) as enc:
        data = enc.encode(img)
        got = _check(jxg_mod, enc, data, case[2], case[3])
    assert got["ans"] == case[8]
    print(case[0], got["ac_bits"], got["stream_bits"],
          {jxg_mod.STRATEGY_NAMES[t]: int(got["cost"][t].sum()) for t in range(27)
           if got["tokens"][t].sum()})


def test_big_varblocks_are_present(jxg_mod):
    """the gradient_e8 cases are the whole-group path: 128 / 256 px varblocks"""
    case = CASES[2]
    with jxg_mod.Encoder(distance=case[5], effort=case[6], proposals=case[7],
                         flags=case_flags(jxg_mod, case)) as enc:
        enc.encode(case_image(case))
        got = enc.rate_report()
    assert any(int(got["tokens"][t].sum()) for t in range(21, 27)), got["tokens"].tolist()


@pytest.mark.parametrize("coder", ["ans", "prefix"])
def test_pass_group_and_band_edges(jxg_mod, coder):
    """520 x 264 at cjxl's defaults: 3 x 2 pass groups, partial right and bottom
    groups, a partial last band (33 block rows), 65 x 33 blocks"""
    from jxg.synth import synth_rgb8

    img = synth_rgb8(520, 264, 0x4A584C31)
    flags = jxg_mod.FLAGS_CJXL_DEFAULTS
    if coder == "prefix":
        flags &= ~jxg_mod.FLAG_ANS
    with jxg_mod.Encoder(distance=1.0, effort=7, flags=flags) as enc:
        data = enc.encode(img)
        got = _check(jxg_mod, enc, data, 520, 264)
    assert got["groups"] == 6 and got["block_cost"].shape == (33, 65)


def test_nothing_is_disturbed(jxg_mod):
    from jxg.synth import natural_rgb8

    img = natural_rgb8(333, 222, 8)
    with jxg_mod.Encoder(distance=2.0, effort=8, flags=jxg_mod.FLAGS_CJXL_DEFAULTS) as enc:
        first = enc.encode(img)
        r0 = enc.rate_report(block_map=True)
        rec = enc.reconstruct()
        s0 = enc.strategy_report(img)
        r1 = enc.rate_report(block_map=True)
        assert np.array_equal(enc.reconstruct(), rec)
        s1 = enc.strategy_report(img)
        r2 = enc.rate_report(block_map=True)
        second = enc.encode(img)
        r3 = enc.rate_report(block_map=True)
    assert first == second
    for r in (r1, r2, r3):
        assert _same(r, r0) and r["block_cost"].tobytes() == r0["block_cost"].tobytes()
    assert all(np.array_equal(s0[k], s1[k]) for k in ("blocks", "nonzeros", "sse", "qf_sum"))
    # the rows partition the same varblocks the strategy report counts
    assert [bool(v) for v in r0["tokens"].sum(axis=1)] == [bool(v) for v in s0["varblocks"]]


# ---- sweeps ----
def _fresh(jxg, img, points):
    """[(bytes, rate report)] of fresh one-at-a-time contexts"""
    out = []
    for p in points:
        with jxg.Encoder(**p) as enc:
            data = enc.encode(img)
            out.append((data, enc.rate_report()))
    return out


def _natural_refs(jxg):
    return cached("rate refs", lambda: _fresh(jxg, _natural(), _points(jxg)))


@pytest.mark.parametrize("quality", [None, "psnr", "msssim"])
def test_sweep_rates_equal_fresh_contexts(jxg_mod, quality):
    img, pts = _natural(), _points(jxg_mod)
    refs = _natural_refs(jxg_mod)
    with jxg_mod.Encoder(distance=3.0, effort=6) as enc:
        off = enc.sweep(img, pts, quality=quality)
        on = enc.sweep(img, pts, quality=quality, rates=True)
        tm = enc.sweep_timings()
        again = enc.sweep(img, pts, quality=quality)
    assert tm["points"] == 6
    for i, ((data, q), (odata, oq), (adata, aq), (rdata, rrep)) in enumerate(
            zip(on, off, again, refs)):
        assert data == odata == adata == rdata, "point %d: codestream" % i
        assert _same(q["rates"], rrep), "point %d: rates" % i
        assert q["rates"]["stream_bits"] == 8 * len(data)
        if quality is None:
            assert oq is None and aq is None and set(q) == {"rates"}
        else:
            assert "rates" not in oq and "rates" not in aq
            assert _qbits(q) == _qbits(oq) == _qbits(aq), "point %d: quality" % i
    rates = [q["rates"] for _, q in on]
    assert rates[1]["ans"] == 0 and rates[0]["ans"] == 1
    assert not _same(rates[0], rates[3]) and not _same(rates[0], rates[2])


def test_sweep_rates_with_strategies(jxg_mod):
    """both switches on: each result is what it is alone"""
    img, pts = _natural(), _points(jxg_mod)[1:4]
    refs = _natural_refs(jxg_mod)[1:4]
    with jxg_mod.Encoder() as enc:
        alone = enc.sweep(img, pts, quality="ssim", strategies=True)
        both = enc.sweep(img, pts, quality="ssim", strategies=True, rates=True)
        assert enc.sweep_timings()["ms_metrics"] > 0
    for (data, q), (adata, aq), (rdata, rrep) in zip(both, alone, refs):
        assert data == adata == rdata and _same(q["rates"], rrep)
        assert _qbits(q) == _qbits(aq)
        assert all(np.array_equal(q["strategies"][k], aq["strategies"][k])
                   for k in ("varblocks", "blocks", "pixels", "nonzeros", "qf_sum", "sse"))


def test_sweep_msssim_results_unchanged(jxg_mod):
    """a frame MS-SSIM is defined for: its results with the rates switch on"""
    from jxg.synth import natural_rgb8

    img = natural_rgb8(256, 192, 11)
    pts = _points(jxg_mod)[2:4]
    with jxg_mod.Encoder() as enc:
        off = enc.sweep(img, pts, quality="msssim")
        on = enc.sweep(img, pts, quality="msssim", rates=True)
    for (data, q), (odata, oq), (rdata, rrep) in zip(on, off, _fresh(jxg_mod, img, pts)):
        assert data == odata == rdata
        assert 0.0 < q["ms_ssim"] < 1.0 and _qbits(q) == _qbits(oq)
        assert _same(q["rates"], rrep)


def test_sweep_of_batched_small_frames(jxg_mod):
    """768 x 512: the size the pipeline batches four to a launch"""
    from jxg.synth import synth_rgb8

    img = synth_rgb8(768, 512, 0x4A584C32)
    d = jxg_mod.FLAGS_CJXL_DEFAULTS
    pts = [dict(distance=1.0, effort=7, proposals=0, flags=d),
           dict(distance=2.0, effort=7, proposals=1, flags=d),
           dict(distance=1.0, effort=5, proposals=0, flags=d & ~jxg_mod.FLAG_ANS),
           dict(distance=6.0, effort=8, proposals=2, flags=d),
           dict(distance=1.0, effort=7, proposals=0, flags=d)]
    with jxg_mod.Encoder() as enc:
        on = enc.sweep(img, pts, quality=None, rates=True)
    for i, ((data, q), (rdata, rrep)) in enumerate(zip(on, _fresh(jxg_mod, img, pts))):
        assert data == rdata and _same(q["rates"], rrep), "point %d" % i
        assert q["rates"]["groups"] == 6


def test_sweep_refused_point_and_state(jxg_mod):
    lib = jxg_mod.load()
    img = np.array(_natural())
    good = _points(jxg_mod)[0]
    reps = poisoned(jxg_mod._RateReport, 2)

    with jxg_mod.Encoder() as enc:
        sweep = RefusedAndGood(jxg_mod, enc, good)
        st = sweep.st
        assert lib.jxg_sweep_rates(enc._ctx, reps, 2) == INVALID_ARG, "no sweep yet"
        assert sweep(0)[0] == INVALID_ARG and list(st) == [INVALID_ARG, 0]
        assert lib.jxg_sweep_rates(enc._ctx, reps, 2) == INVALID_ARG, "switch off"
        assert lib.jxg_set_sweep_rates(None, 1) == INVALID_ARG
        assert lib.jxg_set_sweep_rates(enc._ctx, 1) == 0
        for quality in (0, 1):
            ret, datas = sweep(quality)
            assert ret == INVALID_ARG and list(st) == [INVALID_ARG, 0] and datas[0] is None
            assert lib.jxg_sweep_rates(enc._ctx, reps, 1) == INVALID_ARG, "wrong n"
            assert lib.jxg_sweep_rates(enc._ctx, reps, 3) == INVALID_ARG, "wrong n"
            assert lib.jxg_sweep_rates(enc._ctx, None, 2) == INVALID_ARG
            assert lib.jxg_sweep_rates(None, reps, 2) == INVALID_ARG
            assert lib.jxg_sweep_rates(enc._ctx, reps, 2) == 0
            assert bytes(reps[0]) == bytes(ctypes.sizeof(jxg_mod._RateReport)), \
                "a refused point is zero-filled"
            ref_data, ref_rep = _natural_refs(jxg_mod)[0]
            assert datas[1] == ref_data and _same(reps[1].as_dict(), ref_rep)
        assert lib.jxg_set_sweep_rates(enc._ctx, 0) == 0
        assert sweep(1)[0] == INVALID_ARG
        assert lib.jxg_sweep_rates(enc._ctx, reps, 2) == INVALID_ARG, "after a sweep without"
        enc.submit(img)
        assert lib.jxg_set_sweep_rates(enc._ctx, 1) == INVALID_ARG, "frames pending"
        assert lib.jxg_sweep_rates(enc._ctx, reps, 2) == INVALID_ARG, "frames pending"
        enc.receive()


# ---- refusals ----
def test_refusals(jxg_mod):
    import torch

    lib = jxg_mod.load()
    img = np.array(_natural())
    rep = jxg_mod._RateReport()
    bmap = np.zeros((17, 25), np.uint32)
    d_map = torch.zeros((17, 25), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    host = (lib.jxg_rate_report, bmap.ctypes.data)
    dev = (lib.jxg_rate_report_device, d_map.data_ptr())

    def status(enc, which, with_map=False):
        fn, ptr = which
        return fn(enc._ctx, ctypes.byref(rep), ptr if with_map else None)

    with jxg_mod.Encoder(distance=1.0, effort=7, flags=jxg_mod.FLAG_ANS) as enc:
        for which in (host, dev):
            fn, ptr = which
            assert status(enc, which) == INVALID_ARG, "before any encode"
            enc.encode(img)
            assert status(enc, which) == 0 and status(enc, which, True) == 0
            assert fn(None, ctypes.byref(rep), None) == INVALID_ARG
            assert fn(enc._ctx, None, None) == INVALID_ARG
            data = enc.encode_batch([img, img])[0]
            assert status(enc, which) == INVALID_ARG, "after encode_batch"
            enc.encode(img)
            assert status(enc, which) == 0
            enc.decode(data)
            assert status(enc, which) == INVALID_ARG, "after a decode"
            enc.encode(img)
            enc.submit(img)
            assert status(enc, which) == INVALID_ARG, "while a frame is pending"
            enc.receive()
            assert status(enc, which) == INVALID_ARG, "after submit / receive"
            enc.encode(img)
            assert status(enc, which) == 0
            enc.sweep(img, [_points(jxg_mod)[0]], quality=None, rates=True)
            assert status(enc, which) == INVALID_ARG, "after a sweep"
            assert lib.jxg_warmup(enc._ctx, 200, 136) == 0
            assert status(enc, which) == INVALID_ARG, "after a warm-up encode"
        with pytest.raises(jxg_mod.JxgError):
            enc.rate_report()
    # a sharded encode (one rank of one): not a one-at-a-time encode either
    # (a frame of several pass groups: shard_begin takes no other)
    from jxg.synth import synth_rgb8

    big = synth_rgb8(520, 264, 0x4A584C31)
    hist_words, cap = jxg_mod.shard_sizes(520, 264, 1)
    d_img = torch.from_numpy(big).cuda()
    d_hist = torch.zeros(hist_words, dtype=torch.int32, device="cuda")
    d_xbuf = torch.zeros(max(cap, 1), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    with jxg_mod.Encoder(distance=1.0, effort=7, flags=jxg_mod.FLAG_ANS) as enc:
        enc.encode(big)
        assert lib.jxg_rate_report(enc._ctx, ctypes.byref(rep), None) == 0
        enc.shard_begin(d_img.data_ptr(), 520, 264, 0, 1, d_hist.data_ptr(), d_xbuf.data_ptr())
        assert lib.jxg_rate_report(enc._ctx, ctypes.byref(rep), None) == INVALID_ARG
        assert enc.shard_end(d_hist.data_ptr(), d_xbuf.data_ptr()) > 0
        assert lib.jxg_rate_report(enc._ctx, ctypes.byref(rep), None) == INVALID_ARG, "sharded"


# ---- harness and CLI ----
def test_harness_rows_equal_the_reports(jxg_mod, tmp_path):
    from jxg import harness

    img, pts = _natural(), _points(jxg_mod)[:3]
    plain, with_stats = str(tmp_path / "r0.csv"), str(tmp_path / "r1.csv")
    rfile = str(tmp_path / "rate_stats.csv")
    with jxg_mod.Encoder() as enc:
        d0, rec0 = harness.sweep_and_compare(enc, "nat.png", img, 4321, pts, result_file=plain)
        d1, rec1 = harness.sweep_and_compare(enc, "nat.png", img, 4321, pts,
                                             result_file=with_stats, rate_file=rfile)
    assert d0 == d1 and rec0 == rec1
    assert open(plain).read() == open(with_stats).read(), "the 17-column file is unchanged"
    want = []
    for p, (_, rep) in zip(pts, _natural_refs(jxg_mod)):
        name = jxg_mod.comp_image_name("nat", p["distance"], p["effort"])
        want += harness.rate_stats("nat.png", name, p["distance"], p["effort"], rep)
    got = harness.read_rate_stats(rfile)
    assert got == want and len(got) >= 3 + 1
    for (_, rep) in _natural_refs(jxg_mod)[:3]:
        rows = [r for r in got if r.stream_bits == rep["stream_bits"]]
        assert sum(r.bits_x + r.bits_y + r.bits_b for r in rows) * 256 == int(rep["cost"].sum())
    assert harness.STRATEGY_HEADER[6] == "Varblocks" and len(harness.RATE_HEADER) == 14


def test_cli_rates(jxg_mod, tmp_path):
    from jxg import harness

    img = _natural()
    src = tmp_path / "nat.ppm"
    src.write_bytes(b"P6\n200 136\n255\n" + img.tobytes())
    # one encode
    out, csv_cli, csv_py = tmp_path / "nat-1-7.jxl", tmp_path / "cli.csv", tmp_path / "py.csv"
    p = subprocess.run([jxg_mod.CLI_PATH, str(src), str(out), "--distance=1", "--effort=7",
                        "--proposals=PF", "--jxg_rates=%s" % csv_cli],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    ref_data, ref_rep = _natural_refs(jxg_mod)[2]   # d1 e7 PF at cjxl's defaults
    assert out.read_bytes() == ref_data
    harness.write_rate_stats(harness.rate_stats("nat.ppm", "nat-1-7.jxl", 1.0, 7, ref_rep),
                             str(csv_py))
    assert csv_cli.read_text() == csv_py.read_text()
    # every point of a sweep, appended to the same file
    lst = tmp_path / "points.txt"
    lst.write_text("1 5\n4 7\n")
    outdir = tmp_path / "sweep"
    p = subprocess.run([jxg_mod.CLI_PATH, str(src), str(outdir), "--sweep=%s" % lst,
                        "--jxg_rates=%s" % csv_cli], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    for i, (d, e) in ((0, (1.0, 5)), (3, (4.0, 7))):
        data, rep = _natural_refs(jxg_mod)[i]
        name = jxg_mod.comp_image_name("nat", d, e)
        assert (outdir / name).read_bytes() == data
        harness.write_rate_stats(harness.rate_stats("nat.ppm", name, d, e, rep), str(csv_py))
    assert csv_cli.read_text() == csv_py.read_text()
