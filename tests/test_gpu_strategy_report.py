"""jxg_strategy_report_rgb8[_device], the sweep's reports, the harness file and
the CLI option against tests/strategy_ref.py.  Every field is an integer sum,
so every comparison is exact equality: no tolerance anywhere.  The maps of the
reference come from the codestream through the host decoder (jxg.decode_maps
without a context), not from the buffers the kernels read."""
import ctypes
import subprocess

import numpy as np
import pytest

from strategy_ref import FIELDS, reference_block_sse, reference_report
from sweep_cases import INVALID_ARG, RefusedAndGood, cached, natural as _natural, poisoned
from sweep_cases import points as _points, qbits as _qbits, same
from test_recon_cases import CASES, case_flags, case_image

pytestmark = pytest.mark.gpu

MERGED = set(range(4, 12)) | set(range(18, 27))


_same = same(FIELDS, lambda a, b, k: a[k].dtype == b[k].dtype)


def _check(jxg, enc, img, data):
    """the report of enc's last encode (of img, to data) against the reference"""
    import torch

    h, w = img.shape[:2]
    maps = jxg.decode_maps(data)
    dec = enc.reconstruct()
    got = enc.strategy_report(img, block_map=True)
    ref = reference_report(maps["acs"], maps["qf"], maps["ac"], img, dec, w, h)
    for k in FIELDS:
        assert np.array_equal(got[k], ref[k]), (k, got[k].tolist(), ref[k].tolist())
    bmap = got["block_sse"]
    assert bmap.dtype == np.uint32 and bmap.shape == ((h + 7) // 8, (w + 7) // 8)
    assert np.array_equal(bmap, reference_block_sse(img, dec))
    d_orig, d_comp = torch.from_numpy(np.array(img)).cuda(), torch.from_numpy(dec).cuda()
    torch.cuda.synchronize()
    sse = enc.compare_device(d_orig.data_ptr(), d_comp.data_ptr(), w, h, ssim=False)["sse"]
    assert int(bmap.astype(np.uint64).sum()) == sse and int(got["sse"].sum()) == sse
    assert int(got["pixels"].sum()) == w * h and int(got["blocks"].sum()) == bmap.size
    # the device entry point, a padded stride, the map in device memory; identical bytes
    stride = w * 3 + 13
    d_pad = torch.zeros((h, stride), dtype=torch.uint8, device="cuda")
    d_pad[:, :w * 3] = d_orig.reshape(h, w * 3)
    d_map = torch.full(bmap.shape, -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    again = enc.strategy_report_device(d_pad.data_ptr(), stride, d_map.data_ptr())
    assert _same(again, got)
    assert np.array_equal(d_map.cpu().numpy().view(np.uint32), bmap)
    third = enc.strategy_report(img, block_map=True)
    assert _same(third, got) and third["block_sse"].tobytes() == bmap.tobytes()
    return got


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_report_equals_the_reference(jxg_mod, case):
    img = case_image(case)
    with jxg_mod.Encoder(distance=case[5], effort=case[6], proposals=case[7],
                         flags=case_flags(jxg_mod, case)) as enc:
        data = enc.encode(img)
        got = _check(jxg_mod, enc, img, data)
    print(case[0], {jxg_mod.STRATEGY_NAMES[t]: int(got["blocks"][t]) for t in range(27)
                    if got["blocks"][t]})


def test_pass_group_and_tile_edges(jxg_mod):
    """520 x 264 at cjxl's defaults: 3 x 2 pass groups, 9 x 5 tiles, the last of
    each partial in both directions"""
    from jxg.synth import synth_rgb8

    img = synth_rgb8(520, 264, 0x4A584C31)
    with jxg_mod.Encoder(distance=1.0, effort=7, flags=jxg_mod.FLAGS_CJXL_DEFAULTS) as enc:
        data = enc.encode(img)
        got = _check(jxg_mod, enc, img, data)
    assert any(got["blocks"][t] for t in MERGED), got["blocks"].tolist()


def test_encoder_is_not_disturbed(jxg_mod):
    from jxg.synth import natural_rgb8

    img = natural_rgb8(333, 222, 8)
    with jxg_mod.Encoder(distance=2.0, effort=8, flags=jxg_mod.FLAGS_CJXL_DEFAULTS) as enc:
        first = enc.encode(img)
        rec = enc.reconstruct()
        r1 = enc.strategy_report(img)
        assert np.array_equal(enc.reconstruct(), rec)
        second = enc.encode(img)
        r2 = enc.strategy_report(img)
    assert first == second and _same(r1, r2)


# ---- sweeps ----
def _fresh(jxg, img, points):
    """[(bytes, report)] of fresh one-at-a-time contexts, through the device entry point"""
    import torch

    d_orig = torch.from_numpy(np.array(img)).cuda()
    torch.cuda.synchronize()
    out = []
    for p in points:
        with jxg.Encoder(**p) as enc:
            data = enc.encode(img)
            out.append((data, enc.strategy_report_device(d_orig.data_ptr())))
    return out


def _natural_refs(jxg):
    return cached("strategy refs", lambda: _fresh(jxg, _natural(), _points(jxg)))


@pytest.mark.parametrize("quality", ["psnr", "ssim", "msssim"])
def test_sweep_reports_equal_fresh_contexts(jxg_mod, quality):
    img, pts = _natural(), _points(jxg_mod)
    refs = _natural_refs(jxg_mod)
    with jxg_mod.Encoder(distance=3.0, effort=6) as enc:
        off = enc.sweep(img, pts, quality=quality)
        on = enc.sweep(img, pts, quality=quality, strategies=True)
        tm = enc.sweep_timings()
        again = enc.sweep(img, pts, quality=quality)
    assert tm["points"] == 6 and tm["ms_metrics"] > 0
    for i, ((data, q), (odata, oq), (adata, aq), (rdata, rrep)) in enumerate(
            zip(on, off, again, refs)):
        assert data == odata == adata == rdata, "point %d: codestream" % i
        assert "strategies" not in oq and "strategies" not in aq
        assert _same(q["strategies"], rrep), "point %d: report" % i
        assert int(q["strategies"]["sse"].sum()) == q["sse"]
        assert _qbits(q) == _qbits(oq) == _qbits(aq), "point %d: quality" % i
        if quality == "msssim":   # 136 rows: under MS-SSIM's 176
            assert np.isnan(q["ms_ssim"])
    reps = [q["strategies"] for _, q in on]
    assert not _same(reps[0], reps[3]) and not _same(reps[0], reps[2])


def test_sweep_msssim_results_unchanged(jxg_mod):
    """a frame MS-SSIM is defined for: its results with the report switch on"""
    from jxg.synth import natural_rgb8

    img = natural_rgb8(256, 192, 11)
    pts = _points(jxg_mod)[2:4]
    with jxg_mod.Encoder() as enc:
        off = enc.sweep(img, pts, quality="msssim")
        on = enc.sweep(img, pts, quality="msssim", strategies=True)
    refs = _fresh(jxg_mod, img, pts)
    for (data, q), (odata, oq), (rdata, rrep) in zip(on, off, refs):
        assert data == odata == rdata
        assert 0.0 < q["ms_ssim"] < 1.0 and _qbits(q) == _qbits(oq)
        assert _same(q["strategies"], rrep)


def test_sweep_refused_point_and_state(jxg_mod):
    lib = jxg_mod.load()
    img = np.array(_natural())
    good = _points(jxg_mod)[0]
    reps = poisoned(jxg_mod._StrategyReport, 2)

    with jxg_mod.Encoder() as enc:
        sweep = RefusedAndGood(jxg_mod, enc, good)
        st = sweep.st
        assert lib.jxg_sweep_report(enc._ctx, reps, 2) == INVALID_ARG, "no sweep yet"
        assert sweep(1)[0] == INVALID_ARG and list(st) == [INVALID_ARG, 0]
        assert lib.jxg_sweep_report(enc._ctx, reps, 2) == INVALID_ARG, "switch off"
        assert lib.jxg_set_sweep_report(None, 1) == INVALID_ARG
        assert lib.jxg_set_sweep_report(enc._ctx, 1) == 0
        ret, datas = sweep(1)
        assert ret == INVALID_ARG and list(st) == [INVALID_ARG, 0] and datas[0] is None
        assert lib.jxg_sweep_report(enc._ctx, reps, 1) == INVALID_ARG, "wrong n"
        assert lib.jxg_sweep_report(enc._ctx, reps, 3) == INVALID_ARG, "wrong n"
        assert lib.jxg_sweep_report(enc._ctx, None, 2) == INVALID_ARG
        assert lib.jxg_sweep_report(None, reps, 2) == INVALID_ARG
        assert lib.jxg_sweep_report(enc._ctx, reps, 2) == 0
        assert bytes(reps[0]) == bytes(27 * 64), "a refused point is zero-filled"
        ref_data, ref_rep = _natural_refs(jxg_mod)[0]
        assert datas[1] == ref_data and _same(reps[1].as_dict(), ref_rep)
        assert sweep(0)[0] == INVALID_ARG
        assert lib.jxg_sweep_report(enc._ctx, reps, 2) == INVALID_ARG, "after a quality-0 sweep"
        enc.submit(img)
        assert lib.jxg_set_sweep_report(enc._ctx, 0) == INVALID_ARG, "frames pending"
        assert lib.jxg_sweep_report(enc._ctx, reps, 2) == INVALID_ARG, "frames pending"
        enc.receive()
        with pytest.raises(ValueError):
            enc.sweep(img, [good], quality=None, strategies=True)


def test_sweep_of_batched_small_frames(jxg_mod):
    """768 x 512: the size the pipeline batches four to a launch"""
    from jxg.synth import synth_rgb8

    img = synth_rgb8(768, 512, 0x4A584C32)
    d = jxg_mod.FLAGS_CJXL_DEFAULTS
    pts = [dict(distance=1.0, effort=7, proposals=0, flags=d),
           dict(distance=2.0, effort=7, proposals=1, flags=d),
           dict(distance=1.0, effort=5, proposals=0, flags=d),
           dict(distance=6.0, effort=8, proposals=2, flags=d),
           dict(distance=1.0, effort=7, proposals=0, flags=d)]
    with jxg_mod.Encoder() as enc:
        on = enc.sweep(img, pts, quality="psnr", strategies=True)
    for i, ((data, q), (rdata, rrep)) in enumerate(zip(on, _fresh(jxg_mod, img, pts))):
        assert data == rdata and _same(q["strategies"], rrep), "point %d" % i
        assert int(q["strategies"]["sse"].sum()) == q["sse"]
        assert int(q["strategies"]["pixels"].sum()) == 768 * 512


# ---- refusals ----
def test_refusals(jxg_mod):
    import torch

    lib = jxg_mod.load()
    img = np.array(_natural())
    w, h = 200, 136
    rep = jxg_mod._StrategyReport()
    bmap = np.zeros((17, 25), np.uint32)
    d_img = torch.from_numpy(img).cuda()
    torch.cuda.synchronize()
    host = (lib.jxg_strategy_report_rgb8, img.ctypes.data)
    dev = (lib.jxg_strategy_report_rgb8_device, d_img.data_ptr())

    def status(enc, which, stride=3 * w):
        fn, ptr = which
        return fn(enc._ctx, ptr, stride, ctypes.byref(rep), None)

    with jxg_mod.Encoder(distance=1.0, effort=7, flags=jxg_mod.FLAG_ANS) as enc:
        for which in (host, dev):
            fn, ptr = which
            assert status(enc, which) == INVALID_ARG, "before any encode"
            enc.encode(img)
            assert status(enc, which) == 0
            assert fn(enc._ctx, ptr, 3 * w, ctypes.byref(rep), bmap.ctypes.data
                      if which is host else None) == 0
            assert status(enc, which, 3 * w - 1) == INVALID_ARG, "stride too small"
            assert fn(None, ptr, 3 * w, ctypes.byref(rep), None) == INVALID_ARG
            assert fn(enc._ctx, None, 3 * w, ctypes.byref(rep), None) == INVALID_ARG
            assert fn(enc._ctx, ptr, 3 * w, None, None) == INVALID_ARG
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
            enc.sweep(img, [_points(jxg_mod)[0]], quality="psnr", strategies=True)
            assert status(enc, which) == INVALID_ARG, "after a sweep"
        with pytest.raises(jxg_mod.JxgError):
            enc.strategy_report(img)
        enc.encode(img)
        with pytest.raises(ValueError):
            enc.strategy_report(img[:-1])


# ---- harness and CLI ----
def test_harness_rows_equal_the_reports(jxg_mod, tmp_path):
    from jxg import harness

    img, pts = _natural(), _points(jxg_mod)[:3]
    plain, with_stats = str(tmp_path / "r0.csv"), str(tmp_path / "r1.csv")
    sfile = str(tmp_path / "strategy_stats.csv")
    with jxg_mod.Encoder() as enc:
        d0, rec0 = harness.sweep_and_compare(enc, "nat.png", img, 4321, pts, result_file=plain)
        d1, rec1 = harness.sweep_and_compare(enc, "nat.png", img, 4321, pts,
                                             result_file=with_stats, strategy_file=sfile)
    assert d0 == d1 and rec0 == rec1
    assert open(plain).read() == open(with_stats).read(), "the 17-column file is unchanged"
    want = []
    for p, (_, rep) in zip(pts, _natural_refs(jxg_mod)):
        name = jxg_mod.comp_image_name("nat", p["distance"], p["effort"])
        want += harness.strategy_stats("nat.png", name, p["distance"], p["effort"], rep, 200, 136)
    got = harness.read_strategy_stats(sfile)
    assert got == want and len(got) >= 3 + 1
    assert sum(r.pixels for r in got) == 3 * 200 * 136


def test_cli_report(jxg_mod, tmp_path):
    from jxg import harness

    img = _natural()
    src = tmp_path / "nat.ppm"
    src.write_bytes(b"P6\n200 136\n255\n" + img.tobytes())
    # one encode
    out, csv_cli, csv_py = tmp_path / "nat-1-7.jxl", tmp_path / "cli.csv", tmp_path / "py.csv"
    p = subprocess.run([jxg_mod.CLI_PATH, str(src), str(out), "--distance=1", "--effort=7",
                        "--proposals=PF", "--jxg_report=%s" % csv_cli],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    ref_data, ref_rep = _natural_refs(jxg_mod)[2]   # d1 e7 PF at cjxl's defaults
    assert out.read_bytes() == ref_data
    harness.write_strategy_stats(
        harness.strategy_stats("nat.ppm", "nat-1-7.jxl", 1.0, 7, ref_rep, 200, 136), str(csv_py))
    assert csv_cli.read_text() == csv_py.read_text()
    # every point of a sweep, appended to the same file
    lst = tmp_path / "points.txt"
    lst.write_text("1 5\n4 7\n")
    outdir = tmp_path / "sweep"
    p = subprocess.run([jxg_mod.CLI_PATH, str(src), str(outdir), "--sweep=%s" % lst,
                        "--jxg_report=%s" % csv_cli], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    for i, (d, e) in ((0, (1.0, 5)), (3, (4.0, 7))):
        data, rep = _natural_refs(jxg_mod)[i]
        name = jxg_mod.comp_image_name("nat", d, e)
        assert (outdir / name).read_bytes() == data
        harness.write_strategy_stats(
            harness.strategy_stats("nat.ppm", name, d, e, rep, 200, 136), str(csv_py))
    assert csv_cli.read_text() == csv_py.read_text()
