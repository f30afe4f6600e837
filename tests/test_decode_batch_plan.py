"""The batch decoder's host-only planner (csrc/jxg_decode_plan.cpp), run as
itself: tests/native/decode_batch_plan.cpp is built by g++ from that file alone
-- under ASan + UBSan where the compiler has them -- and prints the chunks,
arena slices and work lists of frames described in a text file.  No GPU,
nothing loaded into Python."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from test_decode_host import _sanitizer_flags

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "jpeg-xl-lossy-image-compression-thesis_amd", "csrc")
ALIGN = 256
SLICES = ("acs", "qf", "dc", "ac", "cmap", "stream", "sec", "tab")


def lds_rule(nhist, tab_bytes):
    """decode_groups_lds of csrc/jxg_decode.hip, restated: [non-zero map 3 KB |
    512 pending coefficients | 7425 context-map bytes | 12-byte descriptors |
    tables], parts 8-byte aligned, within 60 KB -> (LDS bytes, staged)"""
    base = 3 * 1024 + 512 * 4 + ((7425 + 7) & ~7) + ((nhist * 12 + 7) & ~7)
    staged = 0 < tab_bytes <= 60 * 1024 - base
    return base + (((tab_bytes + 7) & ~7) if staged else 0), staged


def frame(w, h, stream_bytes, nhist, tab_bytes, bits, table_bytes=None):
    """a frame line: blocks, tiles, stream words, table blob, nhist, tab_bytes, sections"""
    bxs, bys = (w + 7) // 8, (h + 7) // 8
    ntiles = ((bxs + 7) // 8) * ((bys + 7) // 8)
    if table_bytes is None:
        table_bytes = nhist * 12 + tab_bytes + 7425
    return dict(bxs=bxs, bys=bys, ntiles=ntiles, words=(stream_bytes + 7) // 8 + 3,
                table=table_bytes, nhist=nhist, tab_bytes=tab_bytes, bits=list(bits))


def slice_bytes(f):
    nb = f["bxs"] * f["bys"]
    return dict(acs=nb, qf=nb, dc=nb * 12, ac=nb * 384, cmap=2 * f["ntiles"],
                stream=f["words"] * 8, sec=16 * len(f["bits"]), tab=f["table"])


def footprint(f):
    return sum((b + ALIGN - 1) // ALIGN * ALIGN for b in slice_bytes(f).values())


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no host compiler")
    d = tmp_path_factory.mktemp("dbp")
    san = _sanitizer_flags(d)
    if not san:
        print("decode_batch_plan: the compiler does not accept the sanitizers; built without them")
    flags = ["-O1", "-std=c++17", "-Wall"] + san + os.environ.get("JXG_NATIVE_CFLAGS", "").split()
    exe = d / "decode_batch_plan"
    subprocess.check_call(["g++", *flags,
                           os.path.join(ROOT, "tests", "native", "decode_batch_plan.cpp"),
                           os.path.join(PKG, "jxg_decode_plan.cpp"), "-o", str(exe)])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1")
    count = [0]

    def run(frames, budget):
        count[0] += 1
        path = d / ("frames%d.txt" % count[0])
        path.write_text("".join(
            " ".join(map(str, [f["bxs"], f["bys"], f["ntiles"], f["words"], f["table"], f["nhist"],
                               f["tab_bytes"], len(f["bits"])] + f["bits"])) + "\n"
            for f in frames))
        r = subprocess.run([str(exe), str(path), str(budget)], capture_output=True, text=True,
                           timeout=120, env=env)
        assert r.returncode == 0, r.stdout + r.stderr
        assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr
        info, chunks = [], []
        for ln in r.stdout.splitlines():
            t = ln.split()
            if t[0] == "frame":
                v = list(map(int, t[1:]))
                info.append(dict(footprint=v[1], lds=v[2], staged=bool(v[3]),
                                 bytes=dict(zip(SLICES, v[4:]))))
            elif t[0] == "chunk":
                v = list(map(int, t[1:]))
                chunks.append(dict(first=v[1], end=v[2], bytes=v[3], nstatus=v[4], lds_staged=v[5],
                                   lds_unstaged=v[6], at={}, base={}))
            elif t[0] == "at":
                v = list(map(int, t[1:]))
                chunks[-1]["at"][v[0]] = dict(zip(SLICES + ("end",), v[1:10]))
                chunks[-1]["base"][v[0]] = v[10]
            else:
                chunks[-1][t[0]] = [tuple(map(int, w.split(":"))) for w in t[1:]]
        assert len(info) == len(frames)
        return info, chunks

    print("decode_batch_plan sanitizers: %s" % ("on" if san else "NOT available"))
    return run


def mixed_frames():
    """sizes from 1x1 to 8K, both launch classes, equal section lengths (ties),
    empty sections, a frame of no groups"""
    rng = np.random.default_rng(7)

    def secs(n, top):
        return [int(v) for v in rng.integers(0, top, n)]

    return [
        frame(1, 1, 40, 3, 12 * 128, [200]),
        frame(1920, 1080, 670000, 8, 8 * 128 * 12, secs(40, 400000)),
        frame(768, 520, 90000, 8, 12288, [5000, 5000, 0, 5000, 77, 77, 9, 123456, 5000]),
        frame(200, 136, 9000, 40, 200000, [70000]),           # prefix tables beyond LDS
        frame(520, 300, 60000, 16, 2 * 8 * 128 * 12, secs(6, 90000)),  # two presets
        frame(64, 64, 100, 1, 0, []),                         # no groups, no tables
        frame(7680, 4320, 10670000, 8, 12288, secs(510, 700000)),
        frame(2056, 24, 30000, 8, 12288, [5000] * 9),
        frame(333, 222, 20000, 300, 45292, secs(2, 100000)),  # tables 4 bytes too large for LDS
        frame(333, 222, 20000, 300, 45288, secs(2, 100000)),  # and the largest that fit
        frame(9, 7, 64, 2, 3072, [0]),
    ]


def check_plan(frames, info, chunks, budget):
    n = len(frames)
    # frames: footprint, slice sizes and the launch class
    for f, i in zip(frames, info):
        assert i["bytes"] == slice_bytes(f)
        assert i["footprint"] == footprint(f)
        assert (i["lds"], i["staged"]) == lds_rule(f["nhist"], f["tab_bytes"])
    # chunks partition 0 .. n-1 in order
    assert [c["first"] for c in chunks] == [0] + [c["end"] for c in chunks[:-1]]
    assert chunks[-1]["end"] == n and all(c["first"] < c["end"] for c in chunks)
    for k, c in enumerate(chunks):
        ids = list(range(c["first"], c["end"]))
        assert sorted(c["at"]) == ids
        fp = sum(info[i]["footprint"] for i in ids)
        assert c["bytes"] == fp
        if len(ids) > 1:
            assert fp <= budget, "a chunk of several frames over the budget"
        # greedy: the next frame would not have fitted
        if c["end"] < n:
            assert fp + info[c["end"]]["footprint"] > budget
        # arena slices: aligned, inside the arena, disjoint
        spans = []
        for i in ids:
            at = c["at"][i]
            for s in SLICES:
                assert at[s] % ALIGN == 0, (i, s)
                spans.append((at[s], at[s] + info[i]["bytes"][s]))
            assert at["end"] <= c["bytes"]
        spans.sort()
        for (a0, a1), (b0, _) in zip(spans, spans[1:]):
            assert a0 <= a1 <= b0
        assert not spans or spans[-1][1] <= c["bytes"]
        # status words: one per group, frames in order
        base = 0
        for i in ids:
            assert c["base"][i] == base
            base += len(frames[i]["bits"])
        assert c["nstatus"] == base
        # every (frame, group) once, in its frame's class, longest first
        want = {(i, g) for i in ids for g in range(len(frames[i]["bits"]))}
        got = c["staged"] + c["unstaged"]
        assert len(got) == len(want) and set(got) == want
        for name, staged in (("staged", True), ("unstaged", False)):
            items = c[name]
            assert all(info[i]["staged"] == staged for i, _ in items)
            keys = [(-frames[i]["bits"][g], i, g) for i, g in items]
            assert keys == sorted(keys), "%s list of chunk %d is not longest first" % (name, k)
            lds = [info[i]["lds"] for i in ids if info[i]["staged"] == staged and frames[i]["bits"]]
            assert c["lds_" + name] == (max(lds) if lds else 0)


def test_mixed_frames_default_budget(planner):
    frames = mixed_frames()
    info, chunks = planner(frames, 0)
    check_plan(frames, info, chunks, 2 << 30)
    assert len(chunks) == 1
    assert chunks[0]["staged"] and chunks[0]["unstaged"], "both launch classes"
    # the sizes the default is stated for: blocks * 398 bytes (12.9 MB, 206.3 MB) + the stream
    assert 32400 * 398 + 670000 < info[1]["footprint"] < 32400 * 398 + 700000
    assert 518400 * 398 + 10670000 < info[6]["footprint"] < 518400 * 398 + 10750000
    assert 64 * info[1]["footprint"] <= 2 << 30 and 9 * info[6]["footprint"] <= 2 << 30


def test_budgets(planner):
    """1 byte, exactly one frame, a few frames, huge: n, n, some, 1 chunks"""
    frames = [frame(1920, 1080, 670000, 8, 12288, [1000 * (g % 7) for g in range(40)])
              for _ in range(7)]
    fp = footprint(frames[0])
    for budget, nchunks in ((1, 7), (fp, 7), (2 * fp, 4), (3 * fp + 5, 3), (7 * fp - 1, 2),
                            (7 * fp, 1), (1 << 62, 1)):
        info, chunks = planner(frames, budget)
        check_plan(frames, info, chunks, budget)
        assert len(chunks) == nchunks, budget


def test_oversize_frame_is_alone(planner):
    small = frame(200, 136, 9000, 8, 12288, [70000])
    big = frame(7680, 4320, 10670000, 8, 12288, [1000] * 510)
    frames = [small, small, big, small, big, big, small]
    budget = 3 * footprint(small)
    assert footprint(big) > budget
    info, chunks = planner(frames, budget)
    check_plan(frames, info, chunks, budget)
    assert [(c["first"], c["end"]) for c in chunks] == [(0, 2), (2, 3), (3, 4), (4, 5), (5, 6),
                                                        (6, 7)]


def test_mixed_frames_small_budgets(planner):
    frames = mixed_frames()
    for budget in (1, footprint(frames[1]), 30 << 20, 250 << 20):
        info, chunks = planner(frames, budget)
        check_plan(frames, info, chunks, budget)


def test_ties_break_by_frame_then_group(planner):
    frames = [frame(768, 520, 90000, 8, 12288, [64, 64, 64]),
              frame(200, 136, 9000, 40, 200000, [64]),
              frame(768, 520, 90000, 8, 12288, [64, 128, 64])]
    info, chunks = planner(frames, 0)
    check_plan(frames, info, chunks, 2 << 30)
    assert chunks[0]["staged"] == [(2, 1), (0, 0), (0, 1), (0, 2), (2, 0), (2, 2)]
    assert chunks[0]["unstaged"] == [(1, 0)]


def test_empty_inputs(planner):
    """no frames; frames without groups; zero-length sections; an empty frame"""
    info, chunks = planner([], 0)
    assert info == [] and chunks == []
    frames = [frame(64, 64, 100, 1, 0, []), frame(8, 8, 0, 0, 0, [0, 0]),
              dict(bxs=0, bys=0, ntiles=0, words=0, table=0, nhist=0, tab_bytes=0, bits=[])]
    info, chunks = planner(frames, 0)
    check_plan(frames, info, chunks, 2 << 30)
    assert chunks[0]["staged"] == [] and chunks[0]["unstaged"] == [(1, 0), (1, 1)]
    assert info[2]["footprint"] == 0
