"""MS-SSIM on the GPU (jxg_msssim_rgb8[_device], the sweep's lanes, the
harness column) against tests/msssim_ref.py.

Tolerances: the per-window values use the reference's op order, only the
order of each mean's summation differs, so every cs[j] / ssim[j] matches to the
existing SSIM tolerance (rel 1e-12, abs 1e-15); ms_ssim is a product of five
powers with exponents <= 1 of factors each within 1e-12, so rel 1e-11.  All
reference means of the parity inputs are above 0.88 (asserted), so nothing
hides behind a near-zero mean."""
import ctypes
import math
import struct

import numpy as np
import pytest

import msssim_ref
from sweep_cases import INVALID_ARG, qbits
from test_gpu_metrics import _pair

pytestmark = pytest.mark.gpu



@pytest.fixture(scope="module")
def enc(jxg_mod):
    with jxg_mod.Encoder(distance=1.0, effort=7) as e:
        yield e


def _bits(r):
    return struct.pack("<11d", r["ms_ssim"], *r["cs"], *r["ssim"])


def _synth_pair():
    from jxg.synth import synth_rgb8

    s = synth_rgb8(320, 200, 0x4A584C00)
    rng = np.random.default_rng(1)
    m = np.clip(s.astype(np.int32) + rng.integers(-6, 7, s.shape), 0, 255).astype(np.uint8)
    return s, m


_cases = {}


def _case(name):
    """(a, b, reference), computed once"""
    if name not in _cases:
        if name == "synth":
            a, b = _synth_pair()
        else:
            h, w = name
            a, b = _pair(h, w, h * 1000 + w)
        ref = msssim_ref.msssim(a, b)
        for x in (a, b):
            x.setflags(write=False)
        _cases[name] = (a, b, ref)
    return _cases[name]


@pytest.mark.parametrize("name", [(176, 176), (177, 191), (530, 700), "synth"], ids=str)
def test_parity_with_the_reference(enc, name):
    a, b, ref = _case(name)
    got = enc.msssim(a, b)
    print(name, "gpu", got, "ref", ref)
    assert min(ref["cs"] + ref["ssim"]) > 0.88
    for j in range(5):
        assert got["cs"][j] == pytest.approx(ref["cs"][j], rel=1e-12, abs=1e-15), j
        assert got["ssim"][j] == pytest.approx(ref["ssim"][j], rel=1e-12, abs=1e-15), j
    assert got["ms_ssim"] == pytest.approx(ref["ms_ssim"], rel=1e-11)
    assert struct.pack("<d", got["ssim"][0]) == struct.pack("<d", enc.compare(a, b)["ssim"])


def test_synth_scales_differ():
    """a swapped weight or level would show: the frame's cs are far apart"""
    _, _, ref = _case("synth")
    assert ref["cs"] == pytest.approx([0.90, 0.977, 0.997, 0.9998, 0.99998], abs=6e-3)
    assert all(ref["cs"][j] < ref["cs"][j + 1] for j in range(4))


def test_identical_images_give_exactly_one(enc):
    a, _, _ = _case((177, 191))
    got = enc.msssim(a, a)
    assert got["ms_ssim"] == 1.0 and got["cs"] == [1.0] * 5 and got["ssim"] == [1.0] * 5


def test_inverted_noise_gives_exactly_zero(enc):
    a, _ = _pair(200, 240, 3)
    got = enc.msssim(a, 255 - a)
    ref = msssim_ref.msssim(a, 255 - a)
    assert got["ms_ssim"] == 0.0 and math.copysign(1.0, got["ms_ssim"]) == 1.0
    assert all(v < 0.0 for v in got["cs"][:4])
    assert got["cs"] == pytest.approx(ref["cs"], rel=1e-12, abs=1e-15)


@pytest.mark.parametrize("h,w", [(175, 400), (400, 175)])
def test_under_176_is_all_nan(enc, h, w):
    a, b = _pair(h, w, 2)
    got = enc.msssim(a, b)
    assert math.isnan(got["ms_ssim"])
    assert all(math.isnan(v) for v in got["cs"] + got["ssim"])
    assert enc.compare(a, b)["ssim"] > 0.0


def test_invalid_arguments(jxg_mod):
    lib = jxg_mod.load()
    a, b, _ = _case((176, 176))
    a, b = np.array(a), np.array(b)
    w = h = 176
    out = jxg_mod._Msssim()
    o = ctypes.byref(out)
    with jxg_mod.Encoder() as e:
        ctx, pa, pb = e._ctx, a.ctypes.data, b.ctypes.data
        for fn in (lib.jxg_msssim_rgb8, lib.jxg_msssim_rgb8_device):
            assert fn(None, pa, 3 * w, pb, 3 * w, w, h, o) == INVALID_ARG
            assert fn(ctx, None, 3 * w, pb, 3 * w, w, h, o) == INVALID_ARG
            assert fn(ctx, pa, 3 * w, None, 3 * w, w, h, o) == INVALID_ARG
            assert fn(ctx, pa, 3 * w, pb, 3 * w, w, h, None) == INVALID_ARG
            assert fn(ctx, pa, 3 * w - 1, pb, 3 * w, w, h, o) == INVALID_ARG
            assert fn(ctx, pa, 3 * w, pb, 3 * w - 1, w, h, o) == INVALID_ARG
        assert lib.jxg_set_sweep_msssim(None, 1) == INVALID_ARG
        assert lib.jxg_sweep_msssim(None, o, 1) == INVALID_ARG
        assert lib.jxg_sweep_msssim(ctx, None, 1) == INVALID_ARG
        assert lib.jxg_sweep_msssim(ctx, o, 1) == INVALID_ARG  # no sweep yet
        # while a streamed frame is pending
        e.submit(a)
        assert lib.jxg_msssim_rgb8(ctx, pa, 3 * w, pb, 3 * w, w, h, o) == INVALID_ARG
        assert lib.jxg_set_sweep_msssim(ctx, 1) == INVALID_ARG
        with pytest.raises(jxg_mod.JxgError):
            e.msssim(a, b)
        e.receive()
        assert lib.jxg_msssim_rgb8(ctx, pa, 3 * w, pb, 3 * w, w, h, o) == 0
        assert out.ms_ssim == e.msssim(a, b)["ms_ssim"]


def test_device_pointers_with_unaligned_rows(enc):
    import torch

    a, b, _ = _case((177, 191))
    h, w = 177, 191
    stride = 3 * w + 5  # rows not 4-byte aligned
    da = torch.full((h, stride), 0xA5, dtype=torch.uint8, device="cuda")
    db = torch.full((h, stride), 0x5A, dtype=torch.uint8, device="cuda")
    da[:, :3 * w] = torch.from_numpy(np.array(a).reshape(h, 3 * w)).cuda()
    db[:, :3 * w] = torch.from_numpy(np.array(b).reshape(h, 3 * w)).cuda()
    torch.cuda.synchronize()
    got = enc.msssim_device(da.data_ptr(), db.data_ptr(), w, h, stride, stride)
    assert _bits(got) == _bits(enc.msssim(a, b))


def test_two_calls_are_bit_equal(enc):
    a, b, _ = _case((530, 700))
    first = enc.msssim(a, b)
    assert _bits(enc.msssim(a, b)) == _bits(first)
    with enc.__class__() as other:
        assert _bits(other.msssim(a, b)) == _bits(first)


# ---- sweep ----
def _points(jxg):
    d = jxg.FLAGS_CJXL_DEFAULTS
    return [
        dict(distance=1.0, effort=7, proposals=0, flags=d),   # cjxl defaults
        dict(distance=3.0, effort=5, proposals=0, flags=0),   # prefix codes
        dict(distance=0.5, effort=8, proposals=0, flags=d),
        dict(distance=1.0, effort=7, proposals=3, flags=d),   # P + F
    ]


def _qbits(q):
    return qbits(q, ms=False)


_sweep_state = {}


def _sweep_img():
    from jxg.synth import synth_rgb8

    if "img" not in _sweep_state:
        _sweep_state["img"] = synth_rgb8(256, 192, 0x4A584C41)
        _sweep_state["img"].setflags(write=False)
    return _sweep_state["img"]


def _one_at_a_time(jxg):
    """per point: the msssim_device of a fresh context's encode + reconstruct_device"""
    import torch

    if "ref" not in _sweep_state:
        img = _sweep_img()
        h, w = img.shape[:2]
        d_orig = torch.from_numpy(np.array(img)).cuda()
        d_comp = torch.empty_like(d_orig)
        torch.cuda.synchronize()
        ref = []
        for p in _points(jxg):
            with jxg.Encoder(**p) as e:
                e.encode(img)
                e.reconstruct_device(d_comp.data_ptr())
                ref.append(e.msssim_device(d_orig.data_ptr(), d_comp.data_ptr(), w, h))
        _sweep_state["ref"] = ref
    return _sweep_state["ref"]


def test_sweep_results_and_unchanged_outputs(jxg_mod):
    import torch

    img = _sweep_img()
    h, w = img.shape[:2]
    pts = _points(jxg_mod)
    ref = _one_at_a_time(jxg_mod)
    with jxg_mod.Encoder(distance=4.0, effort=6) as e:
        plain = e.sweep(img, pts, quality="ssim")
        tm_plain = e.sweep_timings()
        got = e.sweep(img, pts, quality="msssim")
        tm = e.sweep_timings()
        d_img = torch.from_numpy(np.array(img)).cuda()
        torch.cuda.synchronize()
        dev = e.sweep_device(d_img.data_ptr(), w, h, pts, quality="msssim")
        # the wrapper put the switch back: a plain quality-2 sweep as before
        again = e.sweep(img, pts, quality="ssim")
        out = (jxg_mod._Msssim * len(pts))()
        assert jxg_mod.load().jxg_sweep_msssim(e._ctx, out, len(pts)) == INVALID_ARG
    assert tm["points"] == tm_plain["points"] == 4 and tm["ms_metrics"] > 0
    for i in range(len(pts)):
        assert got[i][0] == plain[i][0] == dev[i][0] == again[i][0], "point %d: bytes" % i
        assert _qbits(got[i][1]) == _qbits(plain[i][1]) == _qbits(dev[i][1]), "point %d: q" % i
        assert _qbits(again[i][1]) == _qbits(plain[i][1])
        assert "ms_ssim" not in plain[i][1] and "ms_ssim" not in again[i][1]
        for res in (got[i][1], dev[i][1]):
            assert struct.pack("<d", res["ms_ssim"]) == struct.pack("<d", ref[i]["ms_ssim"]), i
            assert res["cs"] == ref[i]["cs"], i
        assert 0.0 < got[i][1]["ms_ssim"] < 1.0
    assert len({r["ms_ssim"] for r in ref}) == 4  # the points' results differ


def test_sweep_abi_entries_refusals_and_switch(jxg_mod):
    lib = jxg_mod.load()
    img = np.array(_sweep_img())
    h, w = img.shape[:2]
    ref = _one_at_a_time(jxg_mod)
    good = _points(jxg_mod)
    bad = dict(distance=0.0, effort=7, proposals=0, flags=0)
    pts = [good[0], bad, good[1]]
    n = len(pts)
    c_pts = (jxg_mod._SweepPoint * n)(*jxg_mod.Encoder._sweep_points(pts))
    outs = (jxg_mod._Buffer * n)()
    qs = (jxg_mod._Quality * n)()
    st = (ctypes.c_int * n)()
    ms = (jxg_mod._Msssim * n)()
    with jxg_mod.Encoder() as e:
        ctx = e._ctx

        def sweep(quality):
            ret = lib.jxg_sweep_rgb8(ctx, img.ctypes.data, w, h, 3 * w, c_pts, n, quality, outs,
                                     qs if quality else None, st)
            for i in range(n):
                lib.jxg_buffer_free(ctypes.byref(outs[i]))
            return ret

        assert lib.jxg_set_sweep_msssim(ctx, 1) == 0
        assert sweep(2) == INVALID_ARG and list(st) == [0, INVALID_ARG, 0]
        assert lib.jxg_sweep_msssim(ctx, ms, n - 1) == INVALID_ARG
        assert lib.jxg_sweep_msssim(ctx, ms, n + 1) == INVALID_ARG
        assert lib.jxg_sweep_msssim(ctx, ms, n) == 0
        assert _bits(ms[0].as_dict()) == _bits(ref[0])
        assert _bits(ms[2].as_dict()) == _bits(ref[1])
        assert bytes(ms[1]) == bytes(ctypes.sizeof(jxg_mod._Msssim))  # refused: zero-filled
        assert struct.pack("<d", ms[0].ssim[0]) == struct.pack("<d", qs[0].ssim)
        # quality 1 and 0 sweeps compute none, whatever the switch says
        assert sweep(1) == INVALID_ARG
        assert lib.jxg_sweep_msssim(ctx, ms, n) == INVALID_ARG
        assert sweep(2) == INVALID_ARG
        assert lib.jxg_sweep_msssim(ctx, ms, n) == 0
        # switched off: the sweep computes none
        assert lib.jxg_set_sweep_msssim(ctx, 0) == 0
        assert sweep(2) == INVALID_ARG
        assert lib.jxg_sweep_msssim(ctx, ms, n) == INVALID_ARG


def test_sweep_under_176_gives_nan_and_the_ssim_stays(jxg_mod):
    from jxg.synth import synth_rgb8

    img = synth_rgb8(160, 200, 0x4A584C42)
    pts = _points(jxg_mod)[:2]
    with jxg_mod.Encoder() as e:
        plain = e.sweep(img, pts, quality="ssim")
        got = e.sweep(img, pts, quality="msssim")
    for (d0, q0), (d1, q1) in zip(plain, got):
        assert d0 == d1 and _qbits(q0) == _qbits(q1) and 0.0 < q1["ssim"] <= 1.0
        assert math.isnan(q1["ms_ssim"]) and all(math.isnan(v) for v in q1["cs"])


# ---- harness ----
def test_harness_column(jxg_mod, tmp_path):
    from jxg import harness

    img = np.array(_sweep_img())
    pts = _points(jxg_mod)[:2]
    ref = _one_at_a_time(jxg_mod)
    f_sweep, f_loop = str(tmp_path / "sweep.csv"), str(tmp_path / "loop.csv")
    f_off, f_off_loop = str(tmp_path / "off.csv"), str(tmp_path / "off_loop.csv")
    with jxg_mod.Encoder() as e:
        datas, recs = harness.sweep_and_compare(e, "photo-m.png", img, 4321, pts,
                                                result_file=f_sweep, ms_ssim=True)
        _, recs_off = harness.sweep_and_compare(e, "photo-m.png", img, 4321, pts,
                                                result_file=f_off)
        host = harness.compare_to_orig(e, "photo-m.png", img, 4321, "x.jxl", datas[0],
                                       len(datas[0]), 1.0, 7, decode_with=e, ms_ssim=True)
        batch = harness.compare_batch_to_orig(
            e, [("photo-m.png", img, 4321, "x.jxl", datas[0], len(datas[0]), 1.0, 7)], e,
            ms_ssim=True)
    want = []
    for p in pts:
        name = jxg_mod.comp_image_name("photo-m", p["distance"], p["effort"])
        with jxg_mod.Encoder(**p) as e:
            d, r = harness.encode_and_compare(e, "photo-m.png", img, 4321, name, p["distance"],
                                              p["effort"], result_file=f_loop, ms_ssim=True)
            harness.encode_and_compare(e, "photo-m.png", img, 4321, name, p["distance"],
                                       p["effort"], result_file=f_off_loop)
        want.append(r)
    assert recs == want
    assert [r.ms_ssim for r in recs] == [ref[0]["ms_ssim"], ref[1]["ms_ssim"]]
    assert open(f_sweep).read() == open(f_loop).read()
    # the decoded file's MS-SSIM is the reconstruction's (the decoder is bit-exact)
    assert host.ms_ssim == recs[0].ms_ssim and batch == [host]
    # the default: column 13 stays the reference's 0.0, rows as before
    assert all(r.ms_ssim == 0.0 for r in recs_off)
    assert open(f_off).read() == open(f_off_loop).read()
    rows_on = open(f_sweep).read().splitlines()
    rows_off = open(f_off).read().splitlines()
    assert rows_on[0] == rows_off[0]
    for on, off, r in zip(rows_on[1:], rows_off[1:], recs):
        on, off = on.split(","), off.split(",")
        assert on[13] == jxg_mod.rust_f64(r.ms_ssim) and off[13] == "0"
        assert on[:13] + on[14:] == off[:13] + off[14:]
