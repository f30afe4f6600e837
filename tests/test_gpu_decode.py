"""The decoder on the GPU (jxg_decode_rgb8[_device], jxg_decode_maps with a
context; csrc/jxg_decode.hip runs the pass groups, csrc/jxg_recon.hip the
pixels): decoding the codestream of an encode gives the bytes
jxg_reconstruct_rgb8 gives from the encoder's own buffers -- same inputs, same
kernels, so an identity, not a tolerance -- for one-at-a-time, streamed, batch
and sharded (several HF presets) frames, and the GPU's maps equal the host
path's.  Only well-formed streams reach the GPU here; corrupted input is the
business of tests/test_decode_host.py.

Against the float64 oracle decoder the bound is the one of
tests/test_gpu_recon.py: no sample differs by more than 1 and at most 0.5 % of
the samples differ (f32 kernels, values on a rounding boundary)."""
import struct
import subprocess
import zlib

import numpy as np
import pytest

from test_recon_cases import CASES, case_flags, case_image

pytestmark = pytest.mark.gpu

MAX_SHARE = 0.005
MAPS = ("acs", "qf", "dc", "ac", "cmap")
# a decoding context whose parameters differ from every encoding one: nothing
# may be taken from the context
DEC_PARAMS = dict(distance=3.0, effort=5, flags=0)

_cache = {}


def _by_name(name):
    return next(c for c in CASES if c[0] == name)


def _encoded(jxg_mod, case):
    """(codestream, reconstruction from the encoder's buffers), once per case"""
    if case[0] not in _cache:
        d, e, p = case[5:8]
        with jxg_mod.Encoder(distance=d, effort=e, proposals=p,
                             flags=case_flags(jxg_mod, case)) as enc:
            data = enc.encode(case_image(case))
            _cache[case[0]] = (data, enc.reconstruct())
    return _cache[case[0]]


def _assert_close_to_oracle(got, ref, what):
    assert got.shape == ref.shape and got.dtype == np.uint8
    diff = np.abs(got.astype(np.int32) - ref.astype(np.int32))
    share = float(np.count_nonzero(diff)) / diff.size
    print("decode %s: max |diff| %d, differing share %.3g" % (what, diff.max(), share))
    assert diff.max() <= 1, "a sample differs by %d" % diff.max()
    assert share <= MAX_SHARE, "%.4f %% of the samples differ" % (100 * share)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_decode_equals_reconstruct(jxg_mod, decoder, case):
    data, rec = _encoded(jxg_mod, case)
    host = jxg_mod.decode_maps(data)
    with jxg_mod.Encoder(**DEC_PARAMS) as dec:
        dev = jxg_mod.decode_maps(data, dec)
        got = dec.decode(data)
    for k in MAPS:
        assert np.array_equal(dev[k], host[k]), k
    assert np.array_equal(got, rec), "decode differs from reconstruct of the same encode"
    _assert_close_to_oracle(got, decoder.decode(data).rgb, case[0])


@pytest.mark.parametrize("w,h", [(2056, 24), (24, 2056)])
def test_two_lf_groups(jxg_mod, decoder, w, h):
    from jxg.synth import synth_rgb8

    img = synth_rgb8(w, h, 0x4A584C00)
    with jxg_mod.Encoder(distance=1.0, effort=7, flags=jxg_mod.FLAG_ANS) as enc:
        data = enc.encode(img)
        rec = enc.reconstruct()
    assert jxg_mod.stream_info(data)["num_lf_groups"] == 2
    host = jxg_mod.decode_maps(data)
    with jxg_mod.Encoder(**DEC_PARAMS) as dec:
        dev = jxg_mod.decode_maps(data, dec)
        got = dec.decode(data)
    for k in MAPS:
        assert np.array_equal(dev[k], host[k]), k
    assert np.array_equal(got, rec)
    _assert_close_to_oracle(got, decoder.decode(data).rgb, "%dx%d" % (w, h))


def test_x_qm_b_qm_scales(jxg_mod, decoder):
    """the frame header's x_qm / b_qm scales (this encoder writes 2 / 2) reach the
    dequantization: a stream edited to 4 / 1 decodes as the oracle decoder reads it"""
    from test_decode_host import _Bits, _flip

    data, rec = _encoded(jxg_mod, _by_name("natural_d1_plain"))
    bits = _Bits(data)
    assert (int.from_bytes(data, "little") >> bits.x_qm) & 63 == 2 | 2 << 3
    edited = _flip(data, bits.x_qm, 6, 4 | 1 << 3)
    ref = decoder.decode(edited)
    assert (ref.x_qm, ref.b_qm) == (4, 1)
    with jxg_mod.Encoder(**DEC_PARAMS) as dec:
        got = dec.decode(edited)
    assert not np.array_equal(got, rec)
    _assert_close_to_oracle(got, ref.rgb, "x_qm 4, b_qm 1")


def test_multi_preset_stream(jxg_mod):
    """a sharded ANS stream (one HF preset per rank) decodes to the pixels of
    the single-context ANS encode of the same image"""
    from jxg.synth import synth_rgb8
    from test_gpu_shard import sharded_encode

    w, h = 520, 300
    img = synth_rgb8(w, h, w * 3 + h)
    sharded = sharded_encode(jxg_mod, img, 2, flags=jxg_mod.FLAG_ANS)
    with jxg_mod.Encoder(distance=1.0, effort=7, flags=jxg_mod.FLAG_ANS) as enc:
        single = enc.encode(img)
    assert sharded != single
    assert jxg_mod.stream_info(sharded)["num_hf_presets"] == 2
    assert jxg_mod.stream_info(single)["num_hf_presets"] == 1
    with jxg_mod.Encoder(**DEC_PARAMS) as dec:
        a = dec.decode(sharded)
        b = dec.decode(single)
        ma, mb = jxg_mod.decode_maps(sharded, dec), jxg_mod.decode_maps(single, dec)
    assert np.array_equal(a, b)
    for k in MAPS:
        assert np.array_equal(ma[k], mb[k]), k


def test_streamed_and_batch_frames(jxg_mod):
    from jxg.synth import natural_rgb8

    img = natural_rgb8(333, 222, 8)
    other = natural_rgb8(333, 222, 9)
    params = dict(distance=2.0, effort=7, flags=jxg_mod.FLAGS_CJXL_DEFAULTS)
    with jxg_mod.Encoder(**params) as enc:
        one = enc.encode(img)
        rec = enc.reconstruct()
        enc.submit(other)
        enc.submit(img)
        enc.receive()
        streamed = enc.receive()
        batch = enc.encode_batch([other, img])[1]
    with jxg_mod.Encoder(**DEC_PARAMS) as dec:
        assert np.array_equal(dec.decode(streamed), rec)
        assert np.array_equal(dec.decode(batch), rec)
        assert np.array_equal(dec.decode(one), rec)


def test_harness_decodes_the_file(jxg_mod):
    """compare_to_orig(decode_with=): the record from the codestream's bytes equals
    the record from the image Encoder.decode gives for them"""
    from jxg import harness

    case = _by_name("natural_d1_all")
    img = case_image(case)
    data, _ = _encoded(jxg_mod, case)
    with jxg_mod.Encoder(**DEC_PARAMS) as dec:
        via = harness.compare_to_orig(dec, "img.png", img, 12345, "img-1-7.jxl", data, len(data),
                                      1.0, 7, decode_with=dec)
        ref = harness.compare_to_orig(dec, "img.png", img, 12345, "img-1-7.jxl", dec.decode(data),
                                      len(data), 1.0, 7)
        q = dec.compare(img, dec.decode(data))
    assert via == ref
    assert via.mse == q["mse"] and via.psnr == q["psnr"] and via.ssim == q["ssim"]
    assert via.comp_file_size == len(data) and 0.0 < via.mse


def test_host_and_device_variants_agree(jxg_mod):
    import torch

    case = _by_name("natural_d1_all")
    data, rec = _encoded(jxg_mod, case)
    w, h = case[2], case[3]
    stride = w * 3 + 40
    with jxg_mod.Encoder(**DEC_PARAMS) as dec:
        host = dec.decode(data)
        buf = torch.full((h, stride), 0xA5, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        dec.decode_device(data, buf.data_ptr(), stride)
        got = buf.cpu().numpy()
        tight = torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        dec.decode_device(data, tight.data_ptr())
    assert np.array_equal(host, rec)
    assert np.array_equal(got[:, :w * 3].reshape(h, w, 3), host)
    assert np.all(got[:, w * 3:] == 0xA5), "bytes past 3 * width were written"
    assert np.array_equal(tight.cpu().numpy(), host)


def test_state_rules(jxg_mod):
    from jxg.synth import natural_rgb8

    img = natural_rgb8(200, 136, 5)
    small = natural_rgb8(64, 40, 6)
    lib = jxg_mod.load()
    out = np.zeros((136, 200, 3), np.uint8)
    with jxg_mod.Encoder(distance=1.0, effort=7, flags=jxg_mod.FLAGS_CJXL_DEFAULTS) as enc:
        first = enc.encode(img)
        rec = enc.reconstruct()
        other = enc.encode(small)

        def status(data=first, stride=600, ptr=out.ctypes.data):
            return lib.jxg_decode_rgb8(enc._ctx, data, len(data) if data else 10, ptr, stride)

        # decoding between two encodes leaves the second encode's bytes alone
        assert enc.encode(img) == first
        assert enc.decode(other).shape == (40, 64, 3)  # (a smaller frame: no buffer regrows)
        assert enc.encode(img) == first
        assert np.array_equal(enc.decode(first), rec)
        with pytest.raises(jxg_mod.JxgError):
            enc.reconstruct()  # the decode used the context's buffers
        assert enc.encode(img) == first
        assert np.array_equal(enc.reconstruct(), rec)
        # arguments
        assert status() == 0
        assert np.array_equal(out, rec)
        # a refused call leaves the context alone: the last encode still reconstructs
        assert enc.encode(img) == first
        assert status(stride=599) == -1, "stride too small"
        assert np.array_equal(enc.reconstruct(), rec)
        assert status(data=None) == -1
        assert status(ptr=None) == -1
        assert lib.jxg_decode_rgb8(enc._ctx, first, 0, out.ctypes.data, 600) == -1
        assert lib.jxg_decode_rgb8(None, first, len(first), out.ctypes.data, 600) == -1
        assert lib.jxg_decode_rgb8_device(enc._ctx, first, len(first), None, 600) == -1
        assert lib.jxg_decode_rgb8_device(enc._ctx, None, 10, None, 600) == -1
        # a pending streamed frame
        enc.submit(img)
        assert enc.pending() == 1
        assert status() == -1, "while a frame is pending"
        assert lib.jxg_decode_maps(enc._ctx, first, len(first), None, None, None, None, None) == -1
        assert enc.receive() == first
        assert status() == 0


def _read_png(raw):
    """8-bit RGB PNG -> (H, W, 3), any filter type"""
    assert raw[:8] == b"\x89PNG\r\n\x1a\n"
    p, idat, w, h = 8, b"", 0, 0
    while p < len(raw):
        n, t = struct.unpack(">I4s", raw[p:p + 8])
        body = raw[p + 8:p + 8 + n]
        assert struct.unpack(">I", raw[p + 8 + n:p + 12 + n])[0] == zlib.crc32(t + body) & 0xFFFFFFFF
        if t == b"IHDR":
            w, h, depth, ctype, _, _, inter = struct.unpack(">IIBBBBB", body)
            assert (depth, ctype, inter) == (8, 2, 0)
        elif t == b"IDAT":
            idat += body
        p += 12 + n
    rows = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(h, 1 + 3 * w)
    out = np.zeros((h, 3 * w), np.int32)
    for y in range(h):
        ft, cur = int(rows[y, 0]), rows[y, 1:].astype(np.int32)
        prev = out[y - 1] if y else np.zeros(3 * w, np.int32)
        if ft == 0:
            out[y] = cur
        elif ft == 2:
            out[y] = (cur + prev) & 0xFF
        else:
            for x in range(3 * w):
                a = out[y, x - 3] if x >= 3 else 0
                c = prev[x - 3] if x >= 3 else 0
                b = prev[x]
                if ft == 1:
                    pred = a
                elif ft == 3:
                    pred = (a + b) // 2
                else:
                    pa, pb, pc = abs(b - c), abs(a - c), abs(a + b - 2 * c)
                    pred = a if pa <= pb and pa <= pc else (b if pb <= pc else c)
                out[y, x] = (cur[x] + pred) & 0xFF
    return out.astype(np.uint8).reshape(h, w, 3)


def test_cli(jxg_mod, tmp_path):
    from jxg.synth import natural_rgb8

    img = natural_rgb8(333, 222, 8)
    src = tmp_path / "in.ppm"
    src.write_bytes(b"P6\n333 222\n255\n" + img.tobytes())
    jxl, ppm, png = tmp_path / "out.jxl", tmp_path / "r.ppm", tmp_path / "r.png"
    p = subprocess.run([jxg_mod.CLI_PATH, str(src), str(jxl), "--distance=2", "--effort=7"],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    for dst in (ppm, png):
        p = subprocess.run([jxg_mod.DJXL_PATH, str(jxl), str(dst)], capture_output=True, text=True)
        assert p.returncode == 0, p.stderr
    with jxg_mod.Encoder(**DEC_PARAMS) as dec:
        want = dec.decode(jxl.read_bytes())
    raw = ppm.read_bytes()
    head = b"P6\n333 222\n255\n"
    assert raw.startswith(head) and len(raw) == len(head) + img.size
    assert np.array_equal(np.frombuffer(raw[len(head):], np.uint8).reshape(222, 333, 3), want)
    assert np.array_equal(_read_png(png.read_bytes()), want)
    # and through jxg_cjxl's own PNG reader: the same codestream as from the PPM of it
    back = tmp_path / "back.jxl"
    again = tmp_path / "again.jxl"
    for s, o in ((png, back), (ppm, again)):
        p = subprocess.run([jxg_mod.CLI_PATH, str(s), str(o), "--distance=2", "--effort=7"],
                           capture_output=True, text=True)
        assert p.returncode == 0, p.stderr
    assert back.read_bytes() == again.read_bytes()
    # garbage
    bad = tmp_path / "bad.jxl"
    bad.write_bytes(b"this is not a codestream at all")
    p = subprocess.run([jxg_mod.DJXL_PATH, str(bad), str(tmp_path / "x.ppm")], capture_output=True,
                       text=True)
    assert p.returncode == 1
    assert "invalid argument" in p.stderr and len(p.stderr.strip().splitlines()) == 1
    assert not (tmp_path / "x.ppm").exists()
