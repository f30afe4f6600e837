"""Decode-side reconstruction on the GPU (jxg_reconstruct_rgb8[_device],
csrc/jxg_recon.hip): the decoded image of the frame a context encoded last,
computed from its device-resident coefficients, against the oracle decoder
(oracle/jxl_decode.py, float64) reading the codestream.

Parity bound: the decoder is float64 and the kernels are f32, so a sample whose
value sits on a rounding boundary may land on the other side: no sample may
differ by more than 1 and at most 0.5 % of the samples may differ.  (The
reference rounded to f32 between its stages differs from itself on at most
9e-5 of the samples of these cases, always by 1.)"""
import subprocess

import numpy as np
import pytest

from test_recon_cases import CASES, case_flags, case_image

pytestmark = pytest.mark.gpu

MAX_SHARE = 0.005

_cache = {}


def _run_case(jxg_mod, decoder, case):
    """(image, codestream, GPU reconstruction, decoder's image), once per case"""
    name = case[0]
    if name not in _cache:
        img = case_image(case)
        d, e, p = case[5:8]
        with jxg_mod.Encoder(distance=d, effort=e, proposals=p,
                             flags=case_flags(jxg_mod, case)) as enc:
            data = enc.encode(img)
            rec = enc.reconstruct()
        _cache[name] = (img, data, rec, decoder.decode(data).rgb)
    return _cache[name]


def _by_name(name):
    return next(c for c in CASES if c[0] == name)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_matches_the_decoder(jxg_mod, decoder, case):
    img, _, rec, ref = _run_case(jxg_mod, decoder, case)
    assert rec.shape == ref.shape == img.shape
    assert rec.dtype == np.uint8
    diff = np.abs(rec.astype(np.int32) - ref.astype(np.int32))
    share = float(np.count_nonzero(diff)) / diff.size
    print("recon %s: max |diff| %d, differing share %.3g" % (case[0], diff.max(), share))
    assert diff.max() <= 1, "a sample differs by %d" % diff.max()
    assert share <= MAX_SHARE, "%.4f %% of the samples differ" % (100 * share)


def test_host_and_device_variants_agree(jxg_mod):
    import torch

    case = _by_name("natural_d1_all")
    img = case_image(case)
    h, w = img.shape[:2]
    stride = w * 3 + 40
    with jxg_mod.Encoder(distance=case[5], effort=case[6], flags=case_flags(jxg_mod, case)) as enc:
        enc.encode(img)
        host = enc.reconstruct()
        buf = torch.full((h, stride), 0xA5, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        enc.reconstruct_device(buf.data_ptr(), stride)
        got = buf.cpu().numpy()
        # and with the default stride
        tight = torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        enc.reconstruct_device(tight.data_ptr())
    assert np.array_equal(got[:, :w * 3].reshape(h, w, 3), host)
    assert np.all(got[:, w * 3:] == 0xA5), "bytes past 3 * width were written"
    assert np.array_equal(tight.cpu().numpy(), host)


@pytest.mark.parametrize("keep", [False, True])
def test_encoder_is_not_disturbed(jxg_mod, oracle, keep):
    case = _by_name("natural_d12_all")
    img = case_image(case)
    d, e, p, coder, mask = case[5:]
    flags = case_flags(jxg_mod, case) | (jxg_mod.FLAG_KEEP_MAPS if keep else 0)
    ref = oracle.encode(img, d, e, p, coder, mask)
    with jxg_mod.Encoder(distance=d, effort=e, proposals=p, flags=flags) as enc:
        first = enc.encode(img)
        rec1 = enc.reconstruct()
        rec2 = enc.reconstruct()
        second = enc.encode(img)
        st = enc.stats()
        rec3 = enc.reconstruct()
    assert first == ref.bytes and second == first
    assert np.array_equal(rec1, rec2) and np.array_equal(rec1, rec3)
    if keep:
        assert np.array_equal(st["acs"], ref.acs)
        assert np.array_equal(st["qf"], ref.qf)
        assert np.array_equal(st["dc"], ref.dc)
        assert np.array_equal(st["ac"], ref.ac)


def test_state_rules(jxg_mod):
    from jxg.synth import natural_rgb8

    img = natural_rgb8(200, 136, 5)
    lib = jxg_mod.load()
    out = np.zeros((136, 200, 3), np.uint8)

    def status(enc, stride=600):
        return lib.jxg_reconstruct_rgb8(enc._ctx, out.ctypes.data, stride)

    with jxg_mod.Encoder(distance=1.0, effort=7, flags=jxg_mod.FLAG_ANS) as enc:
        assert status(enc) == -1, "before any encode"
        with pytest.raises(jxg_mod.JxgError):
            enc.reconstruct()
        enc.encode(img)
        assert status(enc) == 0
        assert status(enc, 599) == -1, "stride too small"
        assert lib.jxg_reconstruct_rgb8(enc._ctx, None, 600) == -1
        assert lib.jxg_reconstruct_rgb8_device(enc._ctx, None, 600) == -1
        assert lib.jxg_reconstruct_rgb8(None, out.ctypes.data, 600) == -1
        enc.encode_batch([img, img])
        assert status(enc) == -1, "after encode_batch"
        enc.encode(img)
        assert status(enc) == 0
        enc.submit(img)
        assert enc.pending() == 1
        assert status(enc) == -1, "while a frame is pending"
        enc.receive()
        assert status(enc) == -1, "after submit / receive"
        enc.encode(img)
        first = enc.reconstruct()
        assert status(enc) == 0
    assert np.array_equal(out, first)


def test_reconstruction_is_live(jxg_mod, decoder):
    from jxg import harness
    from jxg.synth import natural_rgb8

    img = natural_rgb8(200, 136, 5)
    recs, psnr = {}, {}
    for d in (1.0, 6.0):
        with jxg_mod.Encoder(distance=d, effort=7, flags=jxg_mod.FLAGS_CJXL_DEFAULTS) as enc:
            enc.encode(img)
            recs[d] = enc.reconstruct()
            psnr[d] = enc.compare(img, recs[d], ssim=False)["psnr"]
    assert not np.array_equal(recs[1.0], recs[6.0])
    assert psnr[1.0] > psnr[6.0]

    # encode_and_compare == compare_to_orig of the decoder's image, within what
    # 0.5 % of the samples moving by 1 can change: a sample with difference d
    # from the original changes its square by at most 2 |d| + 1, and over n
    # moved samples sum |d_i| <= sqrt(n * SSE) (Cauchy-Schwarz), so
    # |SSE' - SSE| <= 2 sqrt(n SSE) + n
    with jxg_mod.Encoder(distance=2.0, effort=7, flags=jxg_mod.FLAGS_CJXL_DEFAULTS) as enc:
        data, res = harness.encode_and_compare(enc, "img.png", img, 12345, "img-2-7.jxl", 2.0, 7)
        assert data == enc.encode(img)
        ref = enc.compare(img, decoder.decode(data).rgb)
    assert res.comp_file_size == len(data) and res.orig_file_size == 12345
    assert res.orig_raw_size == res.comp_raw_size == img.size
    n = MAX_SHARE * ref["samples"]
    bound = (2.0 * np.sqrt(n * ref["sse"]) + n) / ref["sse"]
    print("mse %.6f vs %.6f, relative bound %.4f" % (res.mse, ref["mse"], bound))
    assert abs(res.mse - ref["mse"]) <= bound * ref["mse"]
    assert res.psnr == pytest.approx(10 * np.log10(255.0 ** 2 / res.mse))
    assert 0.0 < res.ssim <= 1.0


def test_cli_writes_the_reconstruction(jxg_mod, tmp_path):
    from jxg.synth import natural_rgb8

    img = natural_rgb8(333, 222, 8)
    src = tmp_path / "in.ppm"
    src.write_bytes(b"P6\n333 222\n255\n" + img.tobytes())
    plain, out, rec = tmp_path / "plain.jxl", tmp_path / "out.jxl", tmp_path / "r.ppm"
    argv = [jxg_mod.CLI_PATH, str(src)]
    p = subprocess.run(argv + [str(plain), "--distance=2", "--effort=7"], capture_output=True,
                       text=True)
    assert p.returncode == 0, p.stderr
    p = subprocess.run(argv + [str(out), "--distance=2", "--effort=7", "--jxg_recon=%s" % rec],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    assert out.read_bytes() == plain.read_bytes()
    raw = rec.read_bytes()
    head = b"P6\n333 222\n255\n"
    assert raw.startswith(head) and len(raw) == len(head) + img.size
    got = np.frombuffer(raw[len(head):], np.uint8).reshape(222, 333, 3)
    with jxg_mod.Encoder(distance=2.0, effort=7, flags=jxg_mod.FLAGS_CJXL_DEFAULTS) as enc:
        assert enc.encode(img) == out.read_bytes()
        assert np.array_equal(enc.reconstruct(), got)
