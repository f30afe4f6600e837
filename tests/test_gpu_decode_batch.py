"""The batch decoder (jxg_decode_batch_rgb8[_device], csrc/jxg_decode_batch.cpp,
decode_batch_kernel of csrc/jxg_decode.hip): many codestreams in one call, the
pass groups of all frames in one or two launches.  Every output is
byte-identical to Encoder.decode of that stream alone -- same walk, same
reconstruction kernels, so an identity, not a tolerance.  Only well-formed
streams reach the GPU; the refused ones are refused on the host
(tests/test_decode_host.py)."""
import ctypes
import subprocess

import numpy as np
import pytest

from test_gpu_decode import DEC_PARAMS, _by_name, _encoded
from test_recon_cases import CASES

pytestmark = pytest.mark.gpu

OK, INVALID_ARG, UNSUPPORTED = 0, -1, -5

_single = {}


def _streams(jxg_mod):
    """the 14 reconstruction cases' codestreams, in CASES order"""
    return [_encoded(jxg_mod, c)[0] for c in CASES]


def _decoded(jxg_mod, data):
    """Encoder.decode of one stream alone, once per stream"""
    if data not in _single:
        with jxg_mod.Encoder(**DEC_PARAMS) as dec:
            _single[data] = dec.decode(data)
    return _single[data]


def _two_lf(jxg_mod, w, h):
    from jxg.synth import synth_rgb8

    key = ("two_lf", w, h)
    if key not in _single:
        with jxg_mod.Encoder(distance=1.0, effort=7, flags=jxg_mod.FLAG_ANS) as enc:
            _single[key] = enc.encode(synth_rgb8(w, h, 0x4A584C00))
    return _single[key]


def _assert_all_equal(jxg_mod, got, datas):
    assert len(got) == len(datas)
    for i, (g, d) in enumerate(zip(got, datas)):
        want = _decoded(jxg_mod, d)
        assert g.shape == want.shape and g.dtype == np.uint8, i
        assert np.array_equal(g, want), "frame %d differs from its single decode" % i


def _eight_presets(jxg_mod):
    """a stream whose symbol tables do not fit LDS: the 14 cases' all do (one
    preset: at most eight 1.5 KB alias tables, or small prefix tables), so none
    of them takes the kernel with the tables in memory.  2100x600 sharded over
    8 ranks carries 8 HF presets (tests/test_shard_host.py CASES)."""
    from jxg.synth import synth_rgb8
    from test_gpu_shard import sharded_encode

    if "presets8" not in _single:
        _single["presets8"] = sharded_encode(jxg_mod, synth_rgb8(2100, 600, 2700), 8,
                                             flags=jxg_mod.FLAG_ANS)
    assert jxg_mod.stream_info(_single["presets8"])["num_hf_presets"] == 8
    return _single["presets8"]


def _mixed(jxg_mod):
    return _streams(jxg_mod) + [_eight_presets(jxg_mod)]


def test_mixed_batch(jxg_mod):
    """all 14 cases in one call: 1x1 .. 768x520, prefix and ANS, the e8 tables,
    every filter combination; and, with the 8-preset stream, both launch classes"""
    datas = _mixed(jxg_mod)
    with jxg_mod.Encoder(**DEC_PARAMS) as dec:
        got = dec.decode_batch(datas)
        t = dec.decode_batch_timings()
    _assert_all_equal(jxg_mod, got, datas)
    groups = sum(jxg_mod.stream_info(d)["num_groups"] for d in datas)
    print("mixed batch: %d staged + %d unstaged work items, %d pass groups, %d chunk(s)" % (
        t["items_staged"], t["items_unstaged"], groups, t["chunks"]))
    assert t["items_staged"] + t["items_unstaged"] == groups
    assert t["frames"] == len(datas) and t["chunks"] == 1
    assert t["items_staged"] > 0 and t["items_unstaged"] > 0, "a launch class is empty"


def test_multi_lf_group_and_multi_preset_frames(jxg_mod):
    from jxg.synth import synth_rgb8
    from test_gpu_shard import sharded_encode

    img = synth_rgb8(520, 300, 520 * 3 + 300)
    sharded = sharded_encode(jxg_mod, img, 2, flags=jxg_mod.FLAG_ANS)
    assert jxg_mod.stream_info(sharded)["num_hf_presets"] == 2
    datas = [_two_lf(jxg_mod, 2056, 24), sharded, _two_lf(jxg_mod, 24, 2056)]
    assert [jxg_mod.stream_info(d)["num_lf_groups"] for d in datas] == [2, 1, 2]
    with jxg_mod.Encoder(**DEC_PARAMS) as dec:
        got = dec.decode_batch(datas)
    _assert_all_equal(jxg_mod, got, datas)


def test_order_and_aliasing(jxg_mod):
    datas = _mixed(jxg_mod)
    rev = datas[::-1]
    rep = [datas[2], datas[7], datas[2], datas[13], datas[2]]
    with jxg_mod.Encoder(**DEC_PARAMS) as dec:
        _assert_all_equal(jxg_mod, dec.decode_batch(rev), rev)
        _assert_all_equal(jxg_mod, dec.decode_batch(rep), rep)
        one = dec.decode_batch([datas[1]])
        assert len(one) == 1 and np.array_equal(one[0], dec.decode(datas[1]))


def test_chunking(jxg_mod):
    """budgets that give chunks of one frame, of two or three, and one chunk"""
    names = ("natural_d1_plain", "natural_d1.5_epf", "natural_d1_all", "natural_d4_epf3",
             "natural_d1_gab", "natural_hooks", "natural_d1_plain")
    datas = [_encoded(jxg_mod, _by_name(n))[0] for n in names]  # 200x136, ANS
    # A 200x136 frame's footprint in units of fp = 25 * 17 blocks * 398 bytes of
    # maps and coefficients: those (1.005 with the 256-byte alignment), the
    # tables (7.4 KB context map + at most eight 1.5 KB alias tables: 0.05 ..
    # 0.12) and the stream (under fp / 8 here), so 1.06 .. 1.25.  Two frames per
    # chunk: 2 * 1.25 <= budget < 3 * 1.06; three: 3 * 1.25 <= budget < 4 * 1.06.
    fp = 25 * 17 * 398
    assert all(len(d) < fp // 8 for d in datas)
    with jxg_mod.Encoder(**DEC_PARAMS) as dec:
        for budget, chunks in ((1, 7), (int(2.8 * fp), 4), (int(4.0 * fp), 3), (0, 1),
                               (1 << 40, 1)):
            dec.set_decode_batch_bytes(budget)
            got = dec.decode_batch(datas)
            t = dec.decode_batch_timings()
            print("budget %d: %d chunks" % (budget, t["chunks"]))
            assert t["chunks"] == chunks, budget
            assert t["items_staged"] + t["items_unstaged"] == len(datas)
            _assert_all_equal(jxg_mod, got, datas)


def test_more_work_than_is_resident(jxg_mod):
    """400 x the 9-group ANS frame: 3600 one-wave workgroups (about 1500 are
    resident at a time), about 120 MB of arena"""
    data = _two_lf(jxg_mod, 2056, 24)
    assert jxg_mod.stream_info(data)["num_groups"] == 9
    want = _decoded(jxg_mod, data)
    with jxg_mod.Encoder(**DEC_PARAMS) as dec:
        got = dec.decode_batch([data] * 400)
        t = dec.decode_batch_timings()
    assert t["items_staged"] + t["items_unstaged"] == 3600 and t["chunks"] == 1
    assert len(got) == 400
    bad = [i for i, g in enumerate(got) if not np.array_equal(g, want)]
    assert not bad, "frames %s differ from the single decode" % bad[:10]


def _batch_call(jxg_mod, enc, datas, outs, strides, device=False, n=None):
    """the C call itself -> (return value, statuses)"""
    lib = jxg_mod.load()
    n = len(datas) if n is None else n
    m = max(len(datas), 1)
    c_datas = (ctypes.c_char_p * m)(*datas)
    c_sizes = (ctypes.c_size_t * m)(*[len(d) if d else 0 for d in datas])
    c_outs = (ctypes.c_void_p * m)(*outs)
    c_strides = (ctypes.c_size_t * m)(*strides)
    st = (ctypes.c_int * m)(*([7] * m))
    fn = lib.jxg_decode_batch_rgb8_device if device else lib.jxg_decode_batch_rgb8
    ret = fn(enc._ctx, c_datas, c_sizes, n, c_outs, c_strides, st)
    return ret, list(st)


def test_a_refused_frame_in_the_middle(jxg_mod):
    from test_decode_host import _Bits, _flip

    good_a = _encoded(jxg_mod, _by_name("natural_d1_plain"))[0]  # 200x136
    good_b = _encoded(jxg_mod, _by_name("natural_d12_all"))[0]   # 333x222
    truncated = good_b[:len(good_b) // 2]
    # the passes selector next to x_qm / b_qm: a frame of several passes
    unsupported = _flip(good_a, _Bits(good_a).passes, 2, 1)
    lib = jxg_mod.load()
    assert lib.jxg_decode_maps(None, truncated, len(truncated), None, None, None, None,
                               None) == INVALID_ARG
    assert lib.jxg_decode_maps(None, unsupported, len(unsupported), None, None, None, None,
                               None) == UNSUPPORTED
    datas = [good_a, truncated, unsupported, good_b]
    shapes = [(136, 200), (222, 333), (136, 200), (222, 333)]
    outs = [np.full((h, w, 3), 0xA5, np.uint8) for h, w in shapes]
    with jxg_mod.Encoder(**DEC_PARAMS) as dec:
        ret, st = _batch_call(jxg_mod, dec, datas, [o.ctypes.data for o in outs],
                              [w * 3 for _, w in shapes])
        assert st == [OK, INVALID_ARG, UNSUPPORTED, OK]
        assert ret == INVALID_ARG, "the first bad frame's status"
        assert np.array_equal(outs[0], _decoded(jxg_mod, good_a))
        assert np.array_equal(outs[3], _decoded(jxg_mod, good_b))
        assert np.all(outs[1] == 0xA5) and np.all(outs[2] == 0xA5), "a refused frame was written"
        # the Python form
        arrays, sts = dec.decode_batch(datas, strict=False)
        assert sts == [OK, INVALID_ARG, UNSUPPORTED, OK]
        assert arrays[1] is None and arrays[2] is None
        assert np.array_equal(arrays[0], outs[0]) and np.array_equal(arrays[3], outs[3])
        with pytest.raises(jxg_mod.JxgError):
            dec.decode_batch(datas)
        # unsupported first: the return value follows the index order
        ret, st = _batch_call(jxg_mod, dec, [unsupported, truncated],
                              [outs[2].ctypes.data, outs[1].ctypes.data], [600, 999])
        assert (ret, st) == (UNSUPPORTED, [UNSUPPORTED, INVALID_ARG])
        # a stride below 3 * w, a null stream, an empty one, a null output: that frame's
        for o in outs:
            o[:] = 0xA5
        ret, st = _batch_call(jxg_mod, dec, [good_a, good_b, None, good_a, good_a],
                              [outs[0].ctypes.data, outs[1].ctypes.data, outs[2].ctypes.data,
                               None, outs[2].ctypes.data], [600, 998, 600, 600, 600])
        assert (ret, st) == (INVALID_ARG, [OK, INVALID_ARG, INVALID_ARG, INVALID_ARG, OK])
        assert np.array_equal(outs[0], _decoded(jxg_mod, good_a)) and np.all(outs[1] == 0xA5)
        assert np.array_equal(outs[2], outs[0])
        c_datas = (ctypes.c_char_p * 1)(good_a)
        c_outs = (ctypes.c_void_p * 1)(outs[0].ctypes.data)
        one = (ctypes.c_size_t * 1)(600)
        zero = (ctypes.c_size_t * 1)(0)
        st1 = (ctypes.c_int * 1)(7)
        assert lib.jxg_decode_batch_rgb8(dec._ctx, c_datas, zero, 1, c_outs, one, st1) == INVALID_ARG
        assert st1[0] == INVALID_ARG
        # call-level: nothing touched, no status written
        sizes = (ctypes.c_size_t * 1)(len(good_a))
        st1[0] = 7
        outs[0][:] = 0xA5
        assert lib.jxg_decode_batch_rgb8(dec._ctx, c_datas, sizes, 0, c_outs, one, st1) == INVALID_ARG
        assert lib.jxg_decode_batch_rgb8(None, c_datas, sizes, 1, c_outs, one, st1) == INVALID_ARG
        assert lib.jxg_decode_batch_rgb8(dec._ctx, None, sizes, 1, c_outs, one, st1) == INVALID_ARG
        assert lib.jxg_decode_batch_rgb8(dec._ctx, c_datas, None, 1, c_outs, one, st1) == INVALID_ARG
        assert lib.jxg_decode_batch_rgb8(dec._ctx, c_datas, sizes, 1, None, one, st1) == INVALID_ARG
        assert lib.jxg_decode_batch_rgb8(dec._ctx, c_datas, sizes, 1, c_outs, None, st1) == INVALID_ARG
        assert lib.jxg_decode_batch_rgb8_device(dec._ctx, c_datas, sizes, 0, c_outs, one,
                                                st1) == INVALID_ARG
        assert lib.jxg_decode_batch_timings(dec._ctx, None) == INVALID_ARG
        assert st1[0] == 7 and np.all(outs[0] == 0xA5)
        # statuses may be NULL
        assert lib.jxg_decode_batch_rgb8(dec._ctx, c_datas, sizes, 1, c_outs, one, None) == OK
        assert np.array_equal(outs[0], _decoded(jxg_mod, good_a))


def test_pending_streamed_frame_refuses_the_call(jxg_mod):
    from jxg.synth import natural_rgb8

    img = natural_rgb8(200, 136, 5)
    with jxg_mod.Encoder(distance=1.0, effort=7, flags=jxg_mod.FLAGS_CJXL_DEFAULTS) as enc:
        data = enc.encode(img)
        out = np.full((136, 200, 3), 0xA5, np.uint8)
        enc.submit(img)
        assert enc.pending() == 1
        ret, st = _batch_call(jxg_mod, enc, [data], [out.ctypes.data], [600])
        assert ret == INVALID_ARG and st == [7] and np.all(out == 0xA5)
        with pytest.raises(jxg_mod.JxgError):
            enc.decode_batch([data], strict=False)
        assert enc.receive() == data
        ret, st = _batch_call(jxg_mod, enc, [data], [out.ctypes.data], [600])
        assert (ret, st) == (OK, [OK])
        assert np.array_equal(out, _decoded(jxg_mod, data))


def test_context_hygiene(jxg_mod):
    from jxg.synth import natural_rgb8

    datas = _mixed(jxg_mod)
    small = [datas[5], datas[6]]  # 1x1, 9x7
    img = natural_rgb8(200, 136, 5)
    params = dict(distance=1.0, effort=7, flags=jxg_mod.FLAGS_CJXL_DEFAULTS)
    with jxg_mod.Encoder(**params) as fresh:
        first = fresh.encode(img)
        rec = fresh.reconstruct()
    with jxg_mod.Encoder(**params) as enc:
        assert enc.encode(img) == first
        # a large batch, then a small one in the same (larger) arena
        _assert_all_equal(jxg_mod, enc.decode_batch(datas), datas)
        _assert_all_equal(jxg_mod, enc.decode_batch(small), small)
        _assert_all_equal(jxg_mod, enc.decode_batch(datas[:3]), datas[:3])
        with pytest.raises(jxg_mod.JxgError):
            enc.reconstruct()  # as after Encoder.decode
        assert enc.encode(img) == first
        assert np.array_equal(enc.reconstruct(), rec)
        # the single decoder and the batch on one context
        assert np.array_equal(enc.decode(datas[2]), _decoded(jxg_mod, datas[2]))
        _assert_all_equal(jxg_mod, enc.decode_batch(small), small)
        assert enc.encode(img) == first


def test_strides_and_device_outputs(jxg_mod):
    import torch

    datas = [_encoded(jxg_mod, _by_name(n))[0] for n in ("natural_d1_all", "natural_d12_all", "9x7")]
    dims = [(200, 136), (333, 222), (9, 7)]
    strides = [w * 3 + pad for (w, _), pad in zip(dims, (40, 1, 0))]
    bufs = [torch.full((h, s), 0xA5, dtype=torch.uint8, device="cuda")
            for (_, h), s in zip(dims, strides)]
    torch.cuda.synchronize()
    with jxg_mod.Encoder(**DEC_PARAMS) as dec:
        st = dec.decode_batch_device(datas, [b.data_ptr() for b in bufs], strides)
        host = dec.decode_batch(datas)
        # padded host rows
        outs = [np.full((h, s), 0xA5, np.uint8) for (_, h), s in zip(dims, strides)]
        ret, st_host = _batch_call(jxg_mod, dec, datas, [o.ctypes.data for o in outs], strides)
    assert st == [OK] * 3 and (ret, st_host) == (OK, [OK] * 3)
    _assert_all_equal(jxg_mod, host, datas)
    for (w, h), buf, out, want in zip(dims, bufs, outs, host):
        got = buf.cpu().numpy()
        for rows in (got, out):
            assert np.array_equal(rows[:, :w * 3].reshape(h, w, 3), want)
            assert np.all(rows[:, w * 3:] == 0xA5), "bytes past 3 * width were written"


def test_cli_batch(jxg_mod, tmp_path):
    names = ("natural_d1_all", "gradient_e8", "natural_prefix")
    datas = [_encoded(jxg_mod, _by_name(n))[0] for n in names]
    lines, single = [], []
    for i, (d, ext) in enumerate(zip(datas, ("ppm", "png", "ppm"))):
        src = tmp_path / ("in%d.jxl" % i)
        src.write_bytes(d)
        one = tmp_path / ("single%d.%s" % (i, ext))
        p = subprocess.run([jxg_mod.DJXL_PATH, str(src), str(one)], capture_output=True, text=True)
        assert p.returncode == 0, p.stderr
        single.append(one.read_bytes())
        lines.append("%s\t%s\n" % (src, tmp_path / ("batch%d.%s" % (i, ext))))
    lst = tmp_path / "list.txt"
    lst.write_text("".join(lines))
    p = subprocess.run([jxg_mod.DJXL_PATH, "--batch=%s" % lst], capture_output=True, text=True)
    assert p.returncode == 0 and p.stderr == "", p.stderr
    for i, ext in enumerate(("ppm", "png", "ppm")):
        assert (tmp_path / ("batch%d.%s" % (i, ext))).read_bytes() == single[i]
    w, h = 200, 136
    head = b"P6\n%d %d\n255\n" % (w, h)
    assert single[0] == head + _decoded(jxg_mod, datas[0]).tobytes()
    # a missing input and a stream the decoder refuses: one line each, the others written
    bad = tmp_path / "bad.jxl"
    bad.write_bytes(datas[1][:len(datas[1]) // 2])
    missing = tmp_path / "missing.jxl"
    outs = [tmp_path / ("again%d.ppm" % i) for i in range(4)]
    lst.write_text("%s\t%s\n%s\t%s\n%s\t%s\n%s\t%s\n" % (
        tmp_path / "in0.jxl", outs[0], missing, outs[1], bad, outs[2], tmp_path / "in2.jxl", outs[3]))
    p = subprocess.run([jxg_mod.DJXL_PATH, "--batch=%s" % lst], capture_output=True, text=True)
    assert p.returncode == 1
    err = p.stderr.strip().splitlines()
    assert err == ["cannot read %s" % missing, "%s: invalid argument" % bad]
    assert outs[0].read_bytes() == single[0] and outs[3].read_bytes() == single[2]
    assert not outs[1].exists() and not outs[2].exists()


def test_harness_compares_a_batch(jxg_mod, tmp_path):
    from jxg import harness
    from test_recon_cases import case_image

    cases = [_by_name(n) for n in ("natural_d1_all", "natural_d12_all", "natural_prefix")]
    items = []
    for c in cases:
        data = _encoded(jxg_mod, c)[0]
        items.append((c[0] + ".png", case_image(c), 12345 + len(data), c[0] + ".jxl", data,
                      len(data), c[5], c[6]))
    with jxg_mod.Encoder(**DEC_PARAMS) as dec:
        one_csv, batch_csv = str(tmp_path / "one.csv"), str(tmp_path / "batch.csv")
        ref = [harness.compare_to_orig(dec, it[0], it[1], it[2], it[3], it[4], it[5], it[6], it[7],
                                       result_file=one_csv, decode_with=dec) for it in items]
        got = harness.compare_batch_to_orig(dec, items, dec, result_file=batch_csv)
    assert got == ref
    assert all(0.0 < r.mse for r in got)
    assert open(batch_csv).read() == open(one_csv).read()
