"""Distances below 0.1 on the GPU (tests/highrate_cases.py: the frames, the
table and what each case reaches; tests/test_highrate_cases.py asserts that
from the oracle).  Down there the three quantizers (jxg_front.hip quant_lane /
quant_xb, jxg_merge_kernel.h quant_pass, jxg_bigvb.hip vb_quant) clamp at +-32767
and pack it as int16, the rate runs at 15-bit magnitudes, the token record
(tok 63, nbits 13, 13 extra bits) is at the edge of every field in both rANS
kernels, the prefix writer, the histogram / clustering, the rate kernel and the
decoder kernel, the raw quant field is 256 and the global scale 73727.

Every comparison with the oracle is exact: maps, token counts and codestream
bytes.  The pixel comparisons (enc.reconstruct() against the Python decoder's
float64 image) use test_gpu_recon.py's bound: no sample differs by more than 1
and at most 0.5 % of the samples differ; the reference differs from its own
f32-staged version on none (tests/test_highrate_cases.py)."""
import subprocess

import numpy as np
import pytest

import highrate_cases as H
import rate_ref
from highrate_cases import CJXL7, CJXL8, PLAIN5
from strategy_ref import FIELDS, reference_block_sse, reference_report

pytestmark = pytest.mark.gpu


def _encoder(jxg, distance, setting, keep_maps=False):
    return jxg.Encoder(distance=distance, effort=setting[0], proposals=setting[1],
                       flags=H.jxg_flags(jxg, setting, keep_maps))


def _assert_matches(got, st, ref, what):
    assert np.array_equal(st["acs"], ref.acs), what
    assert np.array_equal(st["qf"], ref.qf), what
    assert np.array_equal(st["dc"], ref.dc), what
    assert np.array_equal(st["ac"], ref.ac), what
    assert np.array_equal(st["ac_tokens"], ref.ac_tokens), what
    assert (st["global_scale"], st["quant_dc"]) == (ref.global_scale, ref.quant_dc), what
    assert got == ref.bytes, what


@pytest.mark.parametrize("setting", H.SETTINGS, ids=H.setting_id)
def test_encode_parity(jxg_mod, setting):
    """one context per (setting, distance), its frames back to back: a saturated
    frame leaves nothing behind for the next"""
    by_distance = {}
    for name, d, s in H.ALL_CASES:
        if s == setting:
            by_distance.setdefault(d, []).append(name)
    assert H.FLOOR in by_distance and len(by_distance) >= 2
    for d, names in by_distance.items():
        with _encoder(jxg_mod, d, setting, keep_maps=True) as enc:
            for name in names + names[:1]:
                got = enc.encode(H.images()[name])
                _assert_matches(got, enc.stats(), H.oracle_ref(name, d, setting), (name, d))
    # below the floor: the floor's bytes and maps
    with _encoder(jxg_mod, 1e-12, setting, keep_maps=True) as enc:
        for name in by_distance[H.FLOOR]:
            got = enc.encode(H.images()[name])
            _assert_matches(got, enc.stats(), H.oracle_ref(name, H.FLOOR, setting), (name, 1e-12))


def test_refused_distances_stay_refused(jxg_mod):
    for d in (0.0, -1e-6, float("nan"), 25.000002):
        with pytest.raises(jxg_mod.JxgError):
            jxg_mod.Encoder(distance=d)
    tiny = float(np.nextafter(np.float32(0), np.float32(1)))
    with jxg_mod.Encoder(distance=tiny, effort=5, proposals=3) as enc:
        assert enc.encode(H.images()["edge72"]) == H.oracle_ref("edge72", H.FLOOR, PLAIN5).bytes


@pytest.mark.parametrize("name", ["half264", "white72"])
def test_streamed_and_batched_ans(jxg_mod, name):
    """the one-lane-per-chain rANS kernel (streamed frames) and the batched
    launch (small frames share one) code the 13-bit tokens like a single encode"""
    img = H.images()[name]
    other = H.images()["tri64" if name == "half264" else "corners72"]
    ref = H.oracle_ref(name, 0.001, CJXL7).bytes
    ref_other = H.oracle_ref("tri64" if name == "half264" else "corners72", 0.001, CJXL7).bytes
    with _encoder(jxg_mod, 0.001, CJXL7) as enc:
        single = enc.encode(img)
        assert single == ref
        frames = [img, other, img, img]
        for f in frames:
            enc.submit(f)
        streamed = []
        while enc.pending():
            streamed.append(enc.receive())
        assert streamed == [ref, ref_other, ref, ref]
        assert enc.encode_batch(frames) == [ref, ref_other, ref, ref]
        assert enc.encode(img) == ref


def test_sharded_equals_single(jxg_mod):
    from test_gpu_shard import sharded_encode

    for setting in (CJXL7, PLAIN5):
        ref = H.oracle_ref("half264", 0.001, setting).bytes
        e, p = setting[:2]
        got = sharded_encode(jxg_mod, np.array(H.images()["half264"]), 2, 0.001, e, p,
                             H.jxg_flags(jxg_mod, setting))
        if setting[2] == H.ANS:
            # ANS shards carry one preset per rank: compare what they decode to
            with _encoder(jxg_mod, 0.001, setting) as enc:
                single = enc.encode(H.images()["half264"])
                assert single == ref
                maps = jxg_mod.decode_maps(got)
                want = jxg_mod.decode_maps(single)
                assert all(np.array_equal(maps[k], want[k]) for k in want)
                assert np.array_equal(enc.decode(got), enc.decode(single))
        else:
            assert got == ref


@pytest.mark.parametrize("case", H.RECON_CASES, ids=H.case_id)
def test_reconstruct_and_decode(jxg_mod, case):
    name, d, setting = case
    img = H.images()[name]
    ref = H.oracle_ref(*case)
    with _encoder(jxg_mod, d, setting) as enc:
        data = enc.encode(img)
        assert data == ref.bytes
        rec = enc.reconstruct()
        dec = enc.decode(data)
        maps_gpu = jxg_mod.decode_maps(data, enc)
    maps_host = jxg_mod.decode_maps(data)
    want = H.reference_rgb(*case)
    assert rec.shape == want.shape == img.shape and rec.dtype == np.uint8
    diff = np.abs(rec.astype(np.int32) - want.astype(np.int32))
    share = float(np.count_nonzero(diff)) / diff.size
    print("recon %s: max |diff| %d, differing share %.3g" % (H.case_id(case), diff.max(), share))
    assert diff.max() <= 1, "a sample differs by %d" % diff.max()
    assert share <= H.RECON_MAX_SHARE, "%.4f %% of the samples differ" % (100 * share)
    assert np.array_equal(dec, rec)
    for maps in (maps_gpu, maps_host):
        assert np.array_equal(maps["acs"], ref.acs)
        assert np.array_equal(maps["qf"], ref.qf)
        assert np.array_equal(maps["dc"], ref.dc)
        assert np.array_equal(maps["ac"], ref.ac)
        assert np.array_equal(maps["cmap"], ref.cmap)
    if H.reach(ref)["merged"]["sat"]:
        assert (np.abs(maps_gpu["ac"]) == 32767).sum() >= 24


def _check_rates(got, data, w, h):
    ref = rate_ref.reference(data)
    for k in ("tokens", "cost"):
        assert np.array_equal(got[k], ref[k]), (k, got[k].tolist(), ref[k].tolist())
    assert got["groups"] == ref["groups"] and got["ans"] == ref["ans"]
    assert got["stream_bits"] == 8 * len(data)
    assert got["ac_bits"] == sum(ref["group_bits"]), "the AC streams as the reader consumed them"
    if "block_cost" in got:
        assert got["block_cost"].shape == ((h + 7) // 8, (w + 7) // 8)
        assert np.array_equal(got["block_cost"], ref["block_cost"])
        assert int(got["block_cost"].astype(np.uint64).sum()) == int(got["cost"].sum())
    if not got["ans"]:
        assert int(got["cost"].sum()) == 256 * got["ac_bits"]


@pytest.mark.parametrize("case", [("half264", 0.001, CJXL7), ("half264", 0.001, PLAIN5),
                                  ("tri64", 0.001, CJXL8)], ids=H.case_id)
def test_rate_report(jxg_mod, case):
    name, d, setting = case
    img = H.images()[name]
    with _encoder(jxg_mod, d, setting) as enc:
        data = enc.encode(img)
        assert data == H.oracle_ref(*case).bytes
        got = enc.rate_report(block_map=True)
    assert got["ans"] == setting[2]
    _check_rates(got, data, img.shape[1], img.shape[0])


def test_strategy_report(jxg_mod):
    case = ("half264", 0.004, PLAIN5)
    img = H.images()["half264"]
    h, w = img.shape[:2]
    ref = H.oracle_ref(*case)
    with _encoder(jxg_mod, case[1], case[2]) as enc:
        data = enc.encode(img)
        assert data == ref.bytes
        dec = enc.reconstruct()
        got = enc.strategy_report(img, block_map=True)
    want = reference_report(ref.acs, ref.qf, ref.ac, img, dec, w, h)
    for k in FIELDS:
        assert np.array_equal(got[k], want[k]), (k, got[k].tolist(), want[k].tolist())
    assert np.array_equal(got["block_sse"], reference_block_sse(img, dec))
    assert int(got["qf_sum"].sum()) >= 141 * got["block_sse"].size  # stored qf 141 .. 255, + 1 raw


SWEEP_DISTANCES = (0.05, 0.0111, 0.0108, 0.004, 0.001, 1e-6, 1e-12)


def test_sweep(jxg_mod):
    img = H.images()["tri64"]
    h, w = img.shape[:2]
    flags = jxg_mod.FLAGS_CJXL_DEFAULTS
    pts = [{"distance": d, "effort": 7, "proposals": 0, "flags": flags} for d in SWEEP_DISTANCES]
    with jxg_mod.Encoder(distance=1.0, effort=3) as enc:
        got = enc.sweep(img, pts, quality="psnr", rates=True)
    assert len(got) == len(pts)
    for (data, q), p in zip(got, pts):
        with jxg_mod.Encoder(**p) as enc:
            fresh = enc.encode(img)
            rates = enc.rate_report()
        assert data == fresh, p["distance"]
        for k in ("tokens", "cost", "ac_bits", "stream_bits", "ans", "groups"):
            assert np.array_equal(q["rates"][k], rates[k]), (p["distance"], k)
        _check_rates(q["rates"], data, w, h)
    psnr = [q["psnr"] for _, q in got]
    print("sweep tri64:", ["%g: %d bytes, %.3f dB" % (d, len(b), v)
                           for d, (b, _), v in zip(SWEEP_DISTANCES, got, psnr)])
    assert all(b >= a for a, b in zip(psnr, psnr[1:])), psnr
    assert got[-1][0] == got[-2][0] and got[-1][1]["sse"] == got[-2][1]["sse"]
    assert got[-1][0] == H.oracle_ref("tri64", H.FLOOR, (7, 0, H.ANS, 7)).bytes


def test_cli(jxg_mod, tmp_path):
    img = H.images()["half264"]
    src = tmp_path / "in.ppm"
    src.write_bytes(b"P6\n%d %d\n255\n" % (img.shape[1], img.shape[0]) + img.tobytes())
    outs = {}
    for d in ("0.001", "1e-6", "1e-12"):
        out = tmp_path / ("out-%s.jxl" % d)
        p = subprocess.run([jxg_mod.CLI_PATH, str(src), str(out), "--distance=%s" % d, "--effort=7"],
                           capture_output=True, text=True)
        assert p.returncode == 0, p.stderr
        outs[d] = out.read_bytes()
    with jxg_mod.Encoder(distance=0.001, effort=7, flags=jxg_mod.FLAGS_CJXL_DEFAULTS) as enc:
        assert enc.encode(img) == outs["0.001"]
    assert outs["0.001"] == H.oracle_ref("half264", 0.001, (7, 0, H.ANS, 7)).bytes
    assert outs["1e-12"] == outs["1e-6"] == H.oracle_ref("half264", H.FLOOR, (7, 0, H.ANS, 7)).bytes
