"""One context kept across frames, as the drop-in boundary uses it (one
context per (distance, effort), every image of a corpus through it): the
sequences of tests/reuse_cases.py on one Encoder, every frame against the
oracle -- bytes, and under KEEP_MAPS the maps -- through jxg_encode_rgb8, its
device variant and the streaming pipeline with all frames in flight; and a walk
over the other entry points on one context, every result bit-equal to a fresh
context's.  What the sequences reach (boundaries, content classes, quant-table
kinds) is asserted from the oracle in tests/test_reuse_cases.py.

A context carries its buffers (they only grow), the plan upload key, the
cached context map, the statistics arena, the LF look-back words, the ready
flags and the notes on its last encode from frame to frame; a mistake in any
of them changes nothing on a fresh context, which is what every other parity
test uses."""
import ctypes
import struct

import numpy as np
import pytest

import reuse_cases as R

pytestmark = pytest.mark.gpu

MAPS = ("acs", "qf", "dc", "ac", "ac_tokens")
INVALID_ARG = -1


def _maps_differ(st, ref):
    return [k for k in MAPS if not np.array_equal(st[k], getattr(ref, k))]


def _check_frames(preset, got, stats, decoder):
    """every frame of the preset's sequence against the oracle; names every
    frame that differs, not only the first"""
    refs = R.oracle_refs(preset)
    seq = R.SEQUENCES[R.PRESETS[preset][6]]
    assert len(got) == len(refs) == len(seq)
    bad = []
    for i, (data, ref) in enumerate(zip(got, refs)):
        what = []
        if data != ref.bytes:
            what.append("bytes (%d vs %d)" % (len(data), len(ref.bytes)))
        if stats is not None:
            what += _maps_differ(stats[i], ref)
        if preset == "e8_cjxl":
            kinds = tuple(sorted(decoder.decode(data, groups=[]).qm_params))
            if kinds != R.E8_QM_KINDS[i]:
                what.append("qm_params %r" % (kinds,))
        if what:
            bad.append("frame %d (%s %dx%d): %s" % (i, seq[i][0], seq[i][2], seq[i][3],
                                                    ", ".join(what)))
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("preset", list(R.PRESETS))
def test_sequence_encode(jxg_mod, oracle, decoder, preset):
    keep = R.PRESETS[preset][5]
    got, stats = [], [] if keep else None
    with R.encoder(jxg_mod, preset) as enc:
        for img in R.preset_frames(preset):
            got.append(enc.encode(img))
            if keep:
                stats.append(enc.stats())
    _check_frames(preset, got, stats, decoder)


@pytest.mark.parametrize("preset", list(R.PRESETS))
def test_sequence_encode_device(jxg_mod, oracle, decoder, preset):
    import torch

    keep = R.PRESETS[preset][5]
    frames = R.preset_frames(preset)
    dev = [torch.from_numpy(np.array(f)).cuda() for f in frames]
    torch.cuda.synchronize()
    got, stats = [], [] if keep else None
    with R.encoder(jxg_mod, preset) as enc:
        for f, t in zip(frames, dev):
            got.append(enc.encode_device(t.data_ptr(), f.shape[1], f.shape[0]))
            if keep:
                stats.append(enc.stats())
    _check_frames(preset, got, stats, decoder)


@pytest.mark.parametrize("preset", list(R.PRESETS))
def test_sequence_streamed(jxg_mod, oracle, decoder, preset):
    """all frames in flight: small frames go four to a lane, and a lane slot
    meets a new size each time; then the sequence once more one at a time on
    the same context"""
    frames = R.preset_frames(preset)
    with R.encoder(jxg_mod, preset) as enc:
        for img in frames:
            enc.submit(img)
        assert enc.pending() == len(frames)
        got = [enc.receive() for _ in frames]
        assert enc.pending() == 0
        again = [enc.encode(img) for img in frames]
    _check_frames(preset, got, None, decoder)
    _check_frames(preset, again, None, decoder)


# ---------------------------------------------------------------------------
# the entry-point walk
# ---------------------------------------------------------------------------
WALK = dict(distance=1.0, effort=7, proposals=0)  # with FLAGS_CJXL_DEFAULTS


def _walk_images():
    from jxg.synth import natural_rgb8, synth_rgb8
    from test_gpu_parity import smooth_rgb8

    imgs = {"A": natural_rgb8(333, 250, 8), "B": smooth_rgb8(520, 264, 520 * 31 + 264),
            "C": synth_rgb8(200, 136, 0x4A584C31), "D": natural_rgb8(264, 200, 9),
            "E": smooth_rgb8(136, 72, 136 * 31 + 72), "F": synth_rgb8(67, 41, 0x4A584C32)}
    for v in imgs.values():
        v.setflags(write=False)
    return imgs


def _sweep_points(jxg):
    d = jxg.FLAGS_CJXL_DEFAULTS
    return [dict(distance=2.0, effort=5, proposals=0, flags=d),
            dict(distance=1.0, effort=8, proposals=0, flags=d),
            dict(distance=4.0, effort=7, proposals=3, flags=d & ~jxg.FLAG_ANS)]


def _bits(v):
    """a result as something == compares bit for bit (floats by their bits, NaN
    included; arrays by shape, type and bytes)"""
    if isinstance(v, dict):
        return {k: _bits(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [_bits(x) for x in v]
    if isinstance(v, np.ndarray):
        return (v.shape, v.dtype.str, v.tobytes())
    if isinstance(v, float):
        return struct.pack("<d", v)
    return v


def _recon_status(jxg, enc):
    """jxg_reconstruct_rgb8's status, into a buffer no frame of the walk outgrows"""
    out = np.empty((1024, 1024, 3), np.uint8)
    return jxg.load().jxg_reconstruct_rgb8(enc._ctx, out.ctypes.data, 1024 * 3)


def _trace_status(jxg, enc):
    s = jxg._TraceSummary()
    return jxg.load().jxg_search_trace(enc._ctx, None, ctypes.byref(s))


def test_entry_point_walk(jxg_mod, oracle):
    jxg = jxg_mod
    imgs = _walk_images()
    flags = jxg.FLAGS_CJXL_DEFAULTS
    pts = _sweep_points(jxg)

    def ref_bytes(name, point=None):
        p = point or dict(WALK, flags=flags)
        coder = 1 if p["flags"] & jxg.FLAG_ANS else 0
        return oracle.encode(imgs[name], p["distance"], p["effort"], p["proposals"], coder,
                             R.CJXL).bytes

    streams = {k: ref_bytes(k) for k in "ABCDEF"}
    # streams of other distances: a decode rebuilds the reconstruction tables
    # for their global scale, and the encode after it for the context's again
    streams["D2"], streams["D4"] = ref_bytes("D", pts[0]), ref_bytes("D", pts[2])
    assert len({jxg.stream_info(streams[k])["global_scale"] for k in ("D", "D2", "D4")}) == 3
    # the map of a fresh search, for the forced encode
    with jxg.Encoder(flags=flags | jxg.FLAG_KEEP_MAPS, **WALK) as enc:
        assert enc.encode(imgs["C"]) == streams["C"]
        acs_c = enc.stats()["acs"]
    assert (acs_c & 0x80).any()

    # name, the operation, the codestreams in its result (-> the oracle's),
    # reconstruct's and search_trace's status afterwards
    ops = [
        ("encode A, reconstruct",
         lambda e: (e.encode(imgs["A"]), e.reconstruct()),
         lambda r: [(r[0], streams["A"])], 0, INVALID_ARG),
        ("encode_traced B, search_trace",
         lambda e: (e.encode_traced(imgs["B"]), e.search_trace(), e.reconstruct()),
         lambda r: [(r[0], streams["B"])], 0, 0),
        ("encode_forced C",
         lambda e: (e.encode_forced(imgs["C"], acs_c), e.reconstruct()),
         lambda r: [(r[0], streams["C"])], 0, INVALID_ARG),
        ("sweep D",
         lambda e: e.sweep(imgs["D"], pts, quality="ssim"),
         lambda r: [(r[i][0], ref_bytes("D", pts[i])) for i in range(3)],
         INVALID_ARG, INVALID_ARG),
        ("encode E, rate_report, strategy_report",
         lambda e: (e.encode(imgs["E"]), e.rate_report(block_map=True),
                    e.strategy_report(imgs["E"], block_map=True)),
         lambda r: [(r[0], streams["E"])], 0, INVALID_ARG),
        ("decode B, D at d2",
         lambda e: (e.decode(streams["B"]), e.decode(streams["D2"])), lambda r: [],
         INVALID_ARG, INVALID_ARG),
        ("decode_batch A F D at d4 B C",
         lambda e: e.decode_batch([streams[k] for k in ("A", "F", "D4", "B", "C")]),
         lambda r: [], INVALID_ARG, INVALID_ARG),
        ("compare and msssim A",
         lambda e: (e.compare(imgs["A"], recon_a), e.msssim(imgs["A"], recon_a)),
         lambda r: [], INVALID_ARG, INVALID_ARG),
        ("encode_batch F F' F",
         lambda e: e.encode_batch([imgs["F"], imgs["F"][::-1], imgs["F"]]),
         lambda r: [(r[0], streams["F"]), (r[2], streams["F"])], INVALID_ARG, INVALID_ARG),
        ("encode A, reconstruct, again",
         lambda e: (e.encode(imgs["A"]), e.reconstruct()),
         lambda r: [(r[0], streams["A"])], 0, INVALID_ARG),
    ]

    # what a fresh context returns for each operation alone
    fresh = []
    recon_a = None
    for name, op, _, _, _ in ops:
        if name.startswith("compare"):
            recon_a = fresh[0][1]
        with jxg.Encoder(flags=flags, **WALK) as enc:
            fresh.append(op(enc))

    bad = []
    with jxg.Encoder(flags=flags, **WALK) as enc:
        for i, (name, op, codestreams, recon_st, trace_st) in enumerate(ops):
            got = op(enc)
            if _bits(got) != _bits(fresh[i]):
                bad.append("%s: differs from a fresh context's result" % name)
            for data, want in codestreams(got):
                if data != want:
                    bad.append("%s: a codestream differs from the oracle's" % name)
            if _recon_status(jxg, enc) != recon_st:
                bad.append("%s: reconstruct's status afterwards is not %d" % (name, recon_st))
            if _trace_status(jxg, enc) != trace_st:
                bad.append("%s: search_trace's status afterwards is not %d" % (name, trace_st))
    assert not bad, "\n".join(bad)
    # the walk compared something: the reports and the trace are not empty
    assert fresh[1][1]["blocks"] == 65 * 33
    assert int(fresh[4][1]["ac_bits"]) > 0 and int(fresh[4][2]["varblocks"].sum()) > 0
    assert all(q is not None and q["sse"] > 0 for _, q in fresh[3])
