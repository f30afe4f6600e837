"""jxg_ab_report_rgb8[_device], the sweep's A/B reports and the harness file
against tests/ab_ref.py.  Every field is an integer, so every comparison is
exact equality: no tolerance anywhere.  The reference is fed from calls other
tests pin: jxg.decode_maps of each codestream (host path), the block error map
of strategy_report and the first-block cost map of rate_report."""
import ctypes

import numpy as np
import pytest

import ab_ref
from sweep_cases import INVALID_ARG, natural as _natural, qbits, same
from test_ab_ref import PAIRS, pair_image
from test_recon_cases import case_flags, gradient_rgb8

pytestmark = pytest.mark.gpu

KEYS = ("blocks", "pixels", "sse_a", "sse_b", "cost_a", "cost_b")


_same = same(KEYS, lambda a, b, k: a[k].dtype == np.uint64 and a[k].shape == (27, 27))


def _params(jxg, side):
    d, e, p, coder, mask = side
    return dict(distance=d, effort=e, proposals=p, flags=case_flags(jxg, (0,) * 8 + (coder, mask)))


_cache = {}


def _pair(jxg, pair):
    """the pair's image, and per side (params, codestream, strategy report with
    its block map, rate report with its block map, decoded strategy bytes) of
    a fresh one-at-a-time encoder; computed once, read only"""
    if pair[0] not in _cache:
        img = pair_image(pair)
        img.setflags(write=False)
        sides = []
        for side in pair[2:4]:
            prm = _params(jxg, side)
            with jxg.Encoder(**prm) as enc:
                data = enc.encode(img)
                sides.append((prm, data, enc.strategy_report(img, block_map=True),
                              enc.rate_report(block_map=True), jxg.decode_maps(data)["acs"]))
        _cache[pair[0]] = (img, sides)
    return _cache[pair[0]]


def _reference(img, sa, sb):
    h, w = img.shape[:2]
    return ab_ref.reference(sa[4], sb[4], sa[2]["block_sse"], sb[2]["block_sse"],
                            sa[3]["block_cost"], sb[3]["block_cost"], w, h)


def _marginals(got, sa, sb):
    """rows sum to side A's strategy / rate reports, columns to side B's"""
    for axis, s, e, c in ((1, sa, "sse_a", "cost_a"), (0, sb, "sse_b", "cost_b")):
        assert np.array_equal(got["blocks"].sum(axis=axis), s[2]["blocks"])
        assert np.array_equal(got["pixels"].sum(axis=axis), s[2]["pixels"])
        assert np.array_equal(got[e].sum(axis=axis), s[2]["sse"])
        assert np.array_equal(got[c].sum(axis=axis), s[3]["cost"].sum(axis=1))


@pytest.mark.parametrize("pair", PAIRS, ids=[p[0] for p in PAIRS])
def test_report_equals_the_reference(jxg_mod, pair):
    import torch

    jxg = jxg_mod
    img, (sa, sb) = _pair(jxg, pair)
    h, w = img.shape[:2]
    ref = _reference(img, sa, sb)
    with jxg.Encoder(**sa[0]) as ea, jxg.Encoder(**sb[0]) as eb:
        assert ea.encode(img) == sa[1] and eb.encode(img) == sb[1]
        got = jxg.ab_report(ea, eb, img, block_delta=True)
        for k in KEYS:
            assert got[k].shape == (27, 27) and got[k].dtype == np.uint64
            assert np.array_equal(got[k], ref[k]), (k, np.argwhere(got[k] != ref[k])[:8].tolist())
        dl = got["block_delta"]
        assert dl.dtype == np.int32 and dl.shape == (2, (h + 7) // 8, (w + 7) // 8)
        assert np.array_equal(dl, ref["block_delta"]), np.argwhere(dl != ref["block_delta"])[:8]
        _marginals(got, sa, sb)
        off = got["blocks"] - np.diag(np.diag(got["blocks"]))
        print(pair[0], int(off.sum()), int((off != 0).sum()))
        assert (off != 0).sum() >= 20 or off.sum() >= 1000
        # the map in device memory, pre-filled: identical and no word left
        d_img = torch.from_numpy(np.array(img)).cuda()
        d_map = torch.full(dl.shape, -1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        again = jxg.ab_report_device(ea, eb, d_img.data_ptr(), block_delta_ptr=d_map.data_ptr())
        assert _same(again, got)
        assert np.array_equal(d_map.cpu().numpy(), dl)
        assert _same(jxg.ab_report_device(ea, eb, d_img.data_ptr()), got)
        third = jxg.ab_report(ea, eb, img, block_delta=True)
        assert _same(third, got) and third["block_delta"].tobytes() == dl.tobytes()
        # swapped: the transpose, the _a / _b fields exchanged, the deltas negated
        sw = jxg.ab_report(eb, ea, img, block_delta=True)
        for k, ks in (("blocks", "blocks"), ("pixels", "pixels"), ("sse_a", "sse_b"),
                      ("sse_b", "sse_a"), ("cost_a", "cost_b"), ("cost_b", "cost_a")):
            assert np.array_equal(sw[k], got[ks].T), k
        assert np.array_equal(sw["block_delta"], -dl)


def test_same_encoder_is_diagonal(jxg_mod):
    jxg = jxg_mod
    img, (sa, sb) = _pair(jxg, PAIRS[1])
    with jxg.Encoder(**sb[0]) as enc:
        assert enc.encode(img) == sb[1]
        got = jxg.ab_report(enc, enc, img, block_delta=True)
    for k in KEYS:
        assert np.array_equal(got[k], np.diag(np.diag(got[k]))), k
    assert not got["block_delta"].any()
    assert np.array_equal(np.diag(got["blocks"]), sb[2]["blocks"])
    assert np.array_equal(np.diag(got["pixels"]), sb[2]["pixels"])
    for k in ("sse_a", "sse_b"):
        assert np.array_equal(np.diag(got[k]), sb[2]["sse"])
    for k in ("cost_a", "cost_b"):
        assert np.array_equal(np.diag(got[k]), sb[3]["cost"].sum(axis=1))


def test_nothing_is_disturbed(jxg_mod):
    """the reports and the decoded image of both contexts before and after, in
    any order; a re-encode gives the same bytes"""
    jxg = jxg_mod
    img, (sa, sb) = _pair(jxg, PAIRS[2])

    def state(enc):
        s, r = enc.strategy_report(img, block_map=True), enc.rate_report(block_map=True)
        return (enc.reconstruct().tobytes(), s["block_sse"].tobytes(), r["block_cost"].tobytes(),
                [s[k].tobytes() for k in ("varblocks", "blocks", "pixels", "nonzeros", "qf_sum",
                                          "sse")], [r[k].tobytes() for k in ("tokens", "cost")])

    with jxg.Encoder(**sa[0]) as ea, jxg.Encoder(**sb[0]) as eb:
        assert ea.encode(img) == sa[1] and eb.encode(img) == sb[1]
        first = jxg.ab_report(ea, eb, img)          # before any other report
        a0, b0 = state(ea), state(eb)
        second = jxg.ab_report(ea, eb, img)
        assert state(eb) == b0 and state(ea) == a0
        ea.rate_report()
        third = jxg.ab_report(ea, eb, img)
        eb.reconstruct()
        fourth = jxg.ab_report(ea, eb, img)
        assert ea.encode(img) == sa[1] and eb.encode(img) == sb[1]
        fifth = jxg.ab_report(ea, eb, img)
        assert state(ea) == a0 and state(eb) == b0
    for r in (second, third, fourth, fifth):
        assert _same(r, first)
    assert _same(first, _reference(img, sa, sb))


def test_refusals(jxg_mod):
    import torch

    jxg = jxg_mod
    lib = jxg.load()
    img, (sa, sb) = _pair(jxg, PAIRS[0])
    img = np.array(img)
    other = pair_image(PAIRS[1])
    rep = jxg._AbReport()
    d_img = torch.from_numpy(img).cuda()
    torch.cuda.synchronize()
    calls = ((lib.jxg_ab_report_rgb8, img.ctypes.data), (lib.jxg_ab_report_rgb8_device,
                                                          d_img.data_ptr()))
    with jxg.Encoder(**sa[0]) as ea, jxg.Encoder(**sb[0]) as eb:
        for fn, ptr in calls:
            def status(a=ea._ctx, b=eb._ctx, p=ptr, stride=600, out=ctypes.byref(rep)):
                return fn(a, b, p, stride, out, None)

            def good():
                assert status() == 0
                assert _same(rep.as_dict(), _reference(img, sa, sb))

            ea.encode(img)
            # (eb before its first encode on the first round, after a sweep on the second)
            assert status() == INVALID_ARG, "a context that never encoded / swept last"
            assert status(a=eb._ctx, b=ea._ctx) == INVALID_ARG
            eb.encode(img)
            good()
            assert status(a=None) == INVALID_ARG and status(b=None) == INVALID_ARG
            assert status(p=None) == INVALID_ARG and status(out=None) == INVALID_ARG
            assert status(stride=599) == INVALID_ARG, "a short stride"
            good()
            eb.encode(other)
            assert status() == INVALID_ARG, "different sizes"
            assert status(a=eb._ctx, b=ea._ctx) == INVALID_ARG, "different sizes"
            eb.encode(img)
            good()
            data = ea.encode_batch([img, img])[0]
            assert status() == INVALID_ARG, "after encode_batch"
            ea.encode(img)
            good()
            eb.decode(data)
            assert status() == INVALID_ARG, "after a decode"
            eb.encode(img)
            ea.submit(img)
            assert status() == INVALID_ARG, "while a frame is pending"
            ea.receive()
            assert status() == INVALID_ARG, "after submit / receive"
            ea.encode(img)
            good()
            eb.sweep(img, [sb[0]], quality="psnr")
        with pytest.raises(jxg.JxgError):
            jxg.ab_report(ea, eb, img)


# ---- sweeps ----
BASE = [-1, 0, 0, -1, 3, 1]   # a chain 0 -> 1 -> 5, a shared baseline, two uncompared points


def _points(jxg):
    d = jxg.FLAGS_CJXL_DEFAULTS
    return [
        dict(distance=1.0, effort=7, proposals=0, flags=d),
        dict(distance=1.0, effort=7, proposals=3, flags=d),                   # both hooks
        dict(distance=4.0, effort=7, proposals=0, flags=d),
        dict(distance=2.0, effort=5, proposals=0, flags=d & ~jxg.FLAG_ANS),   # prefix codes
        dict(distance=2.0, effort=7, proposals=2, flags=d & ~jxg.FLAG_ANS),
        dict(distance=1.0, effort=8, proposals=1, flags=d),
    ]


def _fresh(jxg):
    """per point its codestream and, where BASE names one, the A/B report of
    fresh one-at-a-time encoders of the two points"""
    if "fresh" not in _cache:
        img, pts = _natural(), _points(jxg)
        out = []
        for i, p in enumerate(pts):
            with jxg.Encoder(**p) as eb:
                data = eb.encode(img)
                rep = None
                if BASE[i] >= 0:
                    with jxg.Encoder(**pts[BASE[i]]) as ea:
                        ea.encode(img)
                        rep = jxg.ab_report(ea, eb, img)
                out.append((data, rep))
        _cache["fresh"] = out
    return _cache["fresh"]


def _qbits(q):
    return qbits(q, ms=False)


@pytest.mark.parametrize("quality", ["psnr", "ssim"])
def test_sweep_ab_equals_fresh_encoders(jxg_mod, quality):
    jxg = jxg_mod
    img, pts, fresh = _natural(), _points(jxg), _fresh(jxg)
    with jxg.Encoder(distance=3.0, effort=6) as enc:
        off = enc.sweep(img, pts, quality=quality)
        on = enc.sweep(img, pts, quality=quality, ab=BASE)
        assert enc.sweep_timings()["ms_metrics"] > 0
        again = enc.sweep(img, pts, quality=quality)
        full = enc.sweep(img, pts, quality=quality, ab=BASE, strategies=True, rates=True)
        alone = enc.sweep(img, pts, quality=quality, strategies=True, rates=True)
    for i in range(6):
        (data, q), (odata, oq), (adata, aq), (fdata, frep) = on[i], off[i], again[i], fresh[i]
        assert data == odata == adata == fdata == full[i][0], "point %d: codestream" % i
        assert _qbits(q) == _qbits(oq) == _qbits(aq) == _qbits(full[i][1]), "point %d: q" % i
        assert "ab" not in oq and "ab" not in aq
        assert "strategies" not in q and "rates" not in q, "their own switches decide"
        if BASE[i] < 0:
            assert "ab" not in q and "ab" not in full[i][1]
            continue
        assert _same(q["ab"], frep), "point %d" % i
        assert _same(full[i][1]["ab"], frep), "point %d with the other switches" % i
        assert q["ab"]["blocks"].sum() == 17 * 25
    for (_, q), (_, aq) in zip(full, alone):
        assert all(np.array_equal(q["strategies"][k], aq["strategies"][k])
                   for k in ("varblocks", "blocks", "pixels", "nonzeros", "qf_sum", "sse"))
        assert all(np.array_equal(q["rates"][k], aq["rates"][k])
                   for k in ("tokens", "cost", "ac_bits", "stream_bits"))
    # the chain's reports differ from each other: not one table copied around
    assert not _same(on[1][1]["ab"], on[2][1]["ab"]) and not _same(on[1][1]["ab"], on[5][1]["ab"])


def test_sweep_refused_baseline_and_arguments(jxg_mod):
    jxg = jxg_mod
    lib = jxg.load()
    img, pts, fresh = _natural(), _points(jxg), _fresh(jxg)
    bad = list(pts)
    bad[0] = dict(distance=1.0, effort=0)   # refused: the baseline of points 1 and 2
    zero = bytes(ctypes.sizeof(jxg._AbReport))
    with jxg.Encoder() as enc:
        res = enc.sweep(img, bad, quality="psnr", strict=False, ab=BASE)
        assert res[0] == (None, INVALID_ARG)
        for i in (1, 2):   # dependants of the refused point: zero-filled
            assert res[i][0] == fresh[i][0]
            assert all(not res[i][1]["ab"][k].any() for k in KEYS)
        assert res[4][0] == fresh[4][0] and _same(res[4][1]["ab"], fresh[4][1])
        # point 5 compares with point 1, which completed although its own baseline did not
        assert _same(res[5][1]["ab"], fresh[5][1])
        for kw in (dict(quality=None, ab=BASE), dict(ab=BASE[:5]), dict(ab=[0] + BASE[1:]),
                   dict(ab=[-1, 0, 2, -1, 3, 1]), dict(ab=[-2] + BASE[1:])):
            with pytest.raises(ValueError):
                enc.sweep(img, pts, **kw)
        # the C level
        n = 6
        c_pts = (jxg._SweepPoint * n)(*jxg.Encoder._sweep_points(pts))
        outs, qs, st = (jxg._Buffer * n)(), (jxg._Quality * n)(), (ctypes.c_int * n)()
        reps = (jxg._AbReport * n)()
        base = (ctypes.c_int32 * n)(*BASE)
        cimg = np.array(img)

        def sweep(npts, quality=1):
            ret = lib.jxg_sweep_rgb8(enc._ctx, cimg.ctypes.data, 200, 136, 600, c_pts, npts,
                                     quality, outs, qs if quality else None, st)
            for o in outs:
                lib.jxg_buffer_free(ctypes.byref(o))
            return ret

        assert sweep(n) == 0
        assert lib.jxg_sweep_ab(enc._ctx, reps, n) == INVALID_ARG, "a sweep with the switch off"
        assert lib.jxg_set_sweep_ab(None, base, n) == INVALID_ARG
        assert lib.jxg_set_sweep_ab(enc._ctx, (ctypes.c_int32 * 2)(-1, 1), 2) == INVALID_ARG
        assert lib.jxg_set_sweep_ab(enc._ctx, (ctypes.c_int32 * 2)(-2, 0), 2) == INVALID_ARG
        assert lib.jxg_set_sweep_ab(enc._ctx, base, n) == 0
        base[1] = 5   # (the array was copied)
        assert sweep(n - 1) == INVALID_ARG, "another n with the switch on"
        assert lib.jxg_sweep_ab(enc._ctx, reps, n) == INVALID_ARG, "nothing touched"
        assert sweep(n, quality=0) == 0
        assert lib.jxg_sweep_ab(enc._ctx, reps, n) == INVALID_ARG, "quality 0 computes none"
        assert sweep(n) == 0
        assert lib.jxg_sweep_ab(enc._ctx, reps, n - 1) == INVALID_ARG, "wrong n"
        assert lib.jxg_sweep_ab(enc._ctx, None, n) == INVALID_ARG
        assert lib.jxg_sweep_ab(None, reps, n) == INVALID_ARG
        assert lib.jxg_sweep_ab(enc._ctx, reps, n) == 0
        for i in range(n):
            if BASE[i] < 0:
                assert bytes(reps[i]) == zero
            else:
                assert _same(reps[i].as_dict(), fresh[i][1]), "point %d" % i
        enc.submit(cimg)
        assert lib.jxg_set_sweep_ab(enc._ctx, base, n) == INVALID_ARG, "frames pending"
        assert lib.jxg_sweep_ab(enc._ctx, reps, n) == INVALID_ARG, "frames pending"
        enc.receive()
        assert lib.jxg_set_sweep_ab(enc._ctx, None, 0) == 0
        assert sweep(n - 1) == 0, "off again: any n"
        assert lib.jxg_sweep_ab(enc._ctx, reps, n - 1) == INVALID_ARG


# ---- harness ----
def test_harness_rows_parse_back_to_the_report(jxg_mod, tmp_path):
    from jxg import harness

    jxg = jxg_mod
    img, pts, fresh = _natural(), _points(jxg), _fresh(jxg)
    plain, with_ab = str(tmp_path / "r0.csv"), str(tmp_path / "r1.csv")
    afile = str(tmp_path / "ab_stats.csv")
    with jxg.Encoder() as enc:
        d0, rec0 = harness.sweep_and_compare(enc, "nat.png", img, 4321, pts, result_file=plain)
        d1, rec1 = harness.sweep_and_compare(enc, "nat.png", img, 4321, pts, result_file=with_ab,
                                             ab_file=afile, ab_base=BASE)
        with pytest.raises(ValueError):
            harness.sweep_and_compare(enc, "nat.png", img, 4321, pts, ab_file=afile)
    assert d0 == d1 and rec0 == rec1
    assert open(plain).read() == open(with_ab).read(), "the 17-column file is unchanged"
    names = [jxg.comp_image_name("nat", p["distance"], p["effort"]) for p in pts]
    want = []
    for i, p in enumerate(pts):
        if BASE[i] >= 0:
            want += harness.ab_stats("nat.png", names[BASE[i]], names[i], p["distance"],
                                     p["effort"], fresh[i][1], 200, 136)
    got = harness.read_ab_stats(afile)
    assert got == want and len(harness.AB_HEADER) == 18
    # the rows of a pair parse back to its report
    for i in (1, 2, 4, 5):
        rep = fresh[i][1]
        rows = [r for r in got if (r.comp_image_name_a, r.comp_image_name_b, r.effort) ==
                (names[BASE[i]], names[i], pts[i]["effort"])]
        assert len(rows) == int((rep["blocks"] != 0).sum()) and len(rows) > 3
        back = {k: np.zeros((27, 27), np.uint64) for k in KEYS}
        for r in rows:
            f, t = r.from_strategy, r.to_strategy
            assert (r.from_name, r.to_name) == (jxg.STRATEGY_NAMES[f], jxg.STRATEGY_NAMES[t])
            back["blocks"][f, t], back["pixels"][f, t] = r.blocks, r.pixels
            back["sse_a"][f, t], back["sse_b"][f, t] = r.sse_a, r.sse_b
            back["cost_a"][f, t], back["cost_b"][f, t] = int(r.bits_a * 256), int(r.bits_b * 256)
            assert r.diff_sse == r.sse_b - r.sse_a and r.diff_bits == r.bits_b - r.bits_a
        assert _same(back, rep)
        assert all(r.area_share == r.pixels / (200.0 * 136.0) for r in rows)


def test_whole_group_rate_path_on_both_sides(jxg_mod):
    """cjxl's defaults at effort 8 on the 512 x 512 gradient: both sides price
    their tokens with one workgroup per pass group"""
    jxg = jxg_mod
    img = gradient_rgb8(512, 512, 512 * 7 + 512)
    sides = []
    with jxg.Encoder(distance=1.0, effort=8, flags=jxg.FLAGS_CJXL_DEFAULTS) as ea, \
            jxg.Encoder(distance=2.0, effort=8, flags=jxg.FLAGS_CJXL_DEFAULTS) as eb:
        for enc in (ea, eb):
            data = enc.encode(img)
            sides.append((None, data, enc.strategy_report(img, block_map=True),
                          enc.rate_report(block_map=True), jxg.decode_maps(data)["acs"]))
        got = jxg.ab_report(ea, eb, img, block_delta=True)
    ref = _reference(img, *sides)
    assert _same(got, ref) and np.array_equal(got["block_delta"], ref["block_delta"])
    _marginals(got, *sides)
    assert got["blocks"][21:27].sum() and got["blocks"][:, 21:27].sum(), "128 px shapes, both sides"
