#!/usr/bin/env python3
"""Times of jxg_sweep_rgb8 on the reference harness's grid
-- 10 distances x 5 efforts (benchmark.rs:637-642), cjxl's default flags --
against the loop it replaces on the same build: one cached context per point,
each doing encode + reconstruct_device + compare_device.

    python tools/sweep_timing.py [--reps 5] [--sizes 8k,768] [--queues N] [--cli]
    python tools/sweep_timing.py --strategies [--reps 5] [--sizes 8k,768] [--queues N]
    python tools/sweep_timing.py --rates | --ab | --trace [the same options]

Per frame size (the 8K synthetic frame and a 768 x 512 one), input (host /
device) and quality level (0 none, 1 sse/psnr, 2 also ssim): warm contexts,
`--reps` repetitions with sweep and loop alternating, median and min..max of
the host wall time, the jxg_sweep_timings split of the median sweep, and the
device memory one sweeping context holds next to the 50 cached ones.  --queues
sets GPU_MAX_HW_QUEUES before HIP starts (the pipeline has queues - 1 lanes).
--cli: `jxg_cjxl IN OUTDIR --sweep=LIST` of the grid against 50 plain jxg_cjxl
processes.  Prints one JSON line per measurement; the outputs of sweep and loop
are compared before anything is timed.
--strategies: the cost of the strategy reports: the grid's
`sweep_device` at quality 1 and 2 with jxg_set_sweep_report off and on,
alternating; wall time and the ms_recon / ms_metrics of the median sweep.  On a
library without the switch (JXG_LIB_PATH pointing at the parent commit's build)
only the switch-off rows are measured, for the comparison on one box.
--rates: the cost of the rate reports: the grid's
`sweep_device` at quality 0 and 1 with jxg_set_sweep_rates off and on,
alternating; then the kernel alone -- the ms_metrics (events) of a one-point
sweep, switch on minus off -- and the wall time of rate_report_device.  On a
library without the switch only the switch-off rows are measured.
--ab: the cost of the A/B reports: the grid as a 100-point
`sweep_device` at quality 1 -- 50 base points, then 50 P+F points each compared
with its base -- with jxg_set_sweep_ab off and on, alternating; then the added
kernels alone by the events of a two-point sweep, and the wall time of
ab_report_device after two encodes.  On a library without the switch only the
switch-off rows are measured.
--trace: the cost of the search-trace summaries: the grid's
`sweep_device` at quality 0 and 2 with jxg_set_sweep_trace off and on,
alternating; jxg_sweep_timings' ms_call (median, min..max) and the ms_encode of
the median sweep, and the device memory the sweeping context holds without and
with the lanes' trace planes.  On a library without the switch only the
switch-off rows are measured."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "jpeg-xl-lossy-image-compression-thesis_amd"))

DISTANCES = [0.5, 1.0, 1.5, 3.0, 4.0, 6.0, 8.0, 10.0, 12.0, 14.0]
EFFORTS = [5, 6, 7, 8, 9]
SIZES = {"8k": (7680, 4320, 2), "768": (768, 512, 5)}
QUALITY = {0: None, 1: "psnr", 2: "ssim"}


def spread(v):
    return {"median": round(statistics.median(v), 3), "min": round(min(v), 3),
            "max": round(max(v), 3)}


def used_mib(torch):
    free, total = torch.cuda.mem_get_info()
    return (total - free) / 2.0 ** 20


def library(args):
    import torch

    import jxg
    from jxg.synth import SEED_BASE, synth_rgb8_device

    points = [dict(distance=d, effort=e, proposals=0, flags=jxg.FLAGS_CJXL_DEFAULTS)
              for d in DISTANCES for e in EFFORTS]
    for name in args.sizes.split(","):
        w, h, seed = SIZES[name]
        d_img = synth_rgb8_device(w, h, SEED_BASE + seed, 0)
        d_rec = torch.empty_like(d_img)
        torch.cuda.synchronize()
        img = d_img.cpu().numpy()
        base = used_mib(torch)
        sweeper = jxg.Encoder()
        sweeper.sweep_device(d_img.data_ptr(), w, h, points, quality="ssim")  # warm, all buffers
        sweeper.sweep(img, points[:1], quality=None)                          # (the upload buffer)
        mem_sweep = used_mib(torch) - base
        cached = [jxg.Encoder(**p) for p in points]

        def loop(host, level):
            out = []
            for enc in cached:
                data = enc.encode(img) if host else enc.encode_device(d_img.data_ptr(), w, h)
                q = None
                if level:
                    enc.reconstruct_device(d_rec.data_ptr())
                    q = enc.compare_device(d_img.data_ptr(), d_rec.data_ptr(), w, h,
                                           ssim=level == 2)
                out.append((data, q))
            return out

        def sweep(host, level):
            if host:
                return sweeper.sweep(img, points, quality=QUALITY[level])
            return sweeper.sweep_device(d_img.data_ptr(), w, h, points, quality=QUALITY[level])

        want = loop(False, 2)  # warm every cached context, and the reference results
        mem_loop = used_mib(torch) - base - mem_sweep
        got = sweep(False, 2)
        assert [g[0] for g in got] == [r[0] for r in want], "sweep bytes differ from the loop's"
        assert all(repr(g[1]) == repr(r[1]) for g, r in zip(got, want)), "quality differs"
        print(json.dumps({"frame": "%s %dx%d synth_rgb8" % (name, w, h), "points": len(points),
                          "queues": os.environ.get("GPU_MAX_HW_QUEUES", "default"),
                          "lanes": sweeper.sweep_timings()["lanes"],
                          "bytes_total": sum(len(g[0]) for g in got),
                          "mib_one_sweeping_context": round(mem_sweep, 1),
                          "mib_50_cached_contexts": round(mem_loop, 1)}), flush=True)
        for host in (False, True):
            for level in (0, 1, 2):
                t_sweep, t_loop, split = [], [], []
                for rep in range(args.reps + 1):
                    t0 = time.perf_counter()
                    sweep(host, level)
                    t1 = time.perf_counter()
                    tm = sweeper.sweep_timings()
                    t2 = time.perf_counter()
                    loop(host, level)
                    t3 = time.perf_counter()
                    if rep:
                        t_sweep.append((t1 - t0) * 1e3)
                        t_loop.append((t3 - t2) * 1e3)
                        split.append(tm)
                mid = sorted(range(len(t_sweep)), key=lambda i: t_sweep[i])[len(t_sweep) // 2]
                res = {"frame": name, "input": "host" if host else "device", "quality": level,
                       "reps": args.reps, "ms_sweep_wall": spread(t_sweep),
                       "ms_loop_wall": spread(t_loop),
                       "loop_over_sweep": round(statistics.median(t_loop) /
                                                statistics.median(t_sweep), 2),
                       "ms_sweep_per_point": round(statistics.median(t_sweep) / len(points), 3),
                       "ms_loop_per_point": round(statistics.median(t_loop) / len(points), 3),
                       "sweep_timings_of_median": {k: round(v, 3) if isinstance(v, float) else v
                                                   for k, v in split[mid].items()}}
                print(json.dumps(res), flush=True)
        for enc in cached:
            enc.close()
        sweeper.close()
        del cached, d_img, d_rec


def strategies(args):
    import torch

    import jxg
    from jxg.synth import SEED_BASE, synth_rgb8_device

    has_switch = hasattr(jxg.load(), "jxg_set_sweep_report")
    points = [dict(distance=d, effort=e, proposals=0, flags=jxg.FLAGS_CJXL_DEFAULTS)
              for d in DISTANCES for e in EFFORTS]
    for name in args.sizes.split(","):
        w, h, seed = SIZES[name]
        d_img = synth_rgb8_device(w, h, SEED_BASE + seed, 0)
        torch.cuda.synchronize()
        sweeper = jxg.Encoder()

        def sweep(level, on):
            kw = {"strategies": True} if on else {}
            return sweeper.sweep_device(d_img.data_ptr(), w, h, points, quality=QUALITY[level],
                                        **kw)

        want = sweep(2, False)  # warm, all buffers
        if has_switch:
            got = sweep(2, True)
            assert [g[0] for g in got] == [r[0] for r in want], "bytes differ with the switch on"
            for g, r in zip(got, want):
                assert int(g[1]["strategies"]["sse"].sum()) == g[1]["sse"] == r[1]["sse"]
                assert int(g[1]["strategies"]["pixels"].sum()) == w * h
        modes = (False, True) if has_switch else (False,)
        for level in (1, 2):
            wall = {m: [] for m in modes}
            split = {m: [] for m in modes}
            for rep in range(args.reps + 1):
                for m in modes:
                    t0 = time.perf_counter()
                    sweep(level, m)
                    t1 = time.perf_counter()
                    if rep:
                        wall[m].append((t1 - t0) * 1e3)
                        split[m].append(sweeper.sweep_timings())
            res = {"frame": name, "strategies": True, "library": os.path.relpath(jxg.LIB_PATH, ROOT), "quality": level,
                   "points": len(points), "reps": args.reps,
                   "queues": os.environ.get("GPU_MAX_HW_QUEUES", "default"),
                   "lanes": sweeper.sweep_timings()["lanes"]}
            for m in modes:
                mid = sorted(range(len(wall[m])), key=lambda i: wall[m][i])[len(wall[m]) // 2]
                key = "on" if m else "off"
                res["ms_wall_" + key] = spread(wall[m])
                res["ms_recon_" + key] = round(split[m][mid]["ms_recon"], 3)
                res["ms_metrics_" + key] = round(split[m][mid]["ms_metrics"], 3)
            if has_switch:
                res["ms_added_per_point"] = round(
                    (statistics.median(wall[True]) - statistics.median(wall[False])) / len(points),
                    4)
            print(json.dumps(res), flush=True)
        sweeper.close()
        del d_img


def rates(args):
    import torch

    import jxg
    from jxg.synth import SEED_BASE, synth_rgb8_device

    has_switch = hasattr(jxg.load(), "jxg_set_sweep_rates")
    points = [dict(distance=d, effort=e, proposals=0, flags=jxg.FLAGS_CJXL_DEFAULTS)
              for d in DISTANCES for e in EFFORTS]
    one = [dict(distance=1.0, effort=7, proposals=0, flags=jxg.FLAGS_CJXL_DEFAULTS)]
    for name in args.sizes.split(","):
        w, h, seed = SIZES[name]
        d_img = synth_rgb8_device(w, h, SEED_BASE + seed, 0)
        torch.cuda.synchronize()
        sweeper = jxg.Encoder()

        def sweep(level, on, pts=points):
            kw = {"rates": True} if on else {}
            return sweeper.sweep_device(d_img.data_ptr(), w, h, pts, quality=QUALITY[level], **kw)

        want = sweep(1, False)  # warm, all buffers
        if has_switch:
            got = sweep(1, True)
            assert [g[0] for g in got] == [r[0] for r in want], "bytes differ with the switch on"
            for g in got:
                assert g[1]["rates"]["stream_bits"] == 8 * len(g[0])
        modes = (False, True) if has_switch else (False,)
        for level in (0, 1):
            wall = {m: [] for m in modes}
            split = {m: [] for m in modes}
            for rep in range(args.reps + 1):
                for m in modes:
                    t0 = time.perf_counter()
                    sweep(level, m)
                    t1 = time.perf_counter()
                    if rep:
                        wall[m].append((t1 - t0) * 1e3)
                        split[m].append(sweeper.sweep_timings())
            res = {"frame": name, "rates": True, "library": os.path.relpath(jxg.LIB_PATH, ROOT),
                   "quality": level, "points": len(points), "reps": args.reps,
                   "queues": os.environ.get("GPU_MAX_HW_QUEUES", "default"),
                   "lanes": sweeper.sweep_timings()["lanes"]}
            for m in modes:
                mid = sorted(range(len(wall[m])), key=lambda i: wall[m][i])[len(wall[m]) // 2]
                key = "on" if m else "off"
                res["ms_wall_" + key] = spread(wall[m])
                res["ms_encode_" + key] = round(split[m][mid]["ms_encode"], 3)
                res["ms_metrics_" + key] = round(split[m][mid]["ms_metrics"], 3)
            if has_switch:
                res["ms_added_per_point"] = round(
                    (statistics.median(wall[True]) - statistics.median(wall[False])) / len(points),
                    4)
            print(json.dumps(res), flush=True)
        if has_switch:
            # the kernel alone (with the table's memset and 1.3 KB copy), by the
            # events around a point's metrics: a one-point sweep (d1 e7, cjxl's
            # defaults) at quality 1, switch off and on, alternating; and the
            # one-at-a-time call's host wall time after an encode of that point
            ms = {False: [], True: []}
            for rep in range(4 * args.reps + 1):
                for m in (False, True):
                    sweep(1, m, one)
                    if rep:
                        ms[m].append(sweeper.sweep_timings()["ms_metrics"])
            with jxg.Encoder(**one[0]) as enc:
                enc.encode_device(d_img.data_ptr(), w, h)
                tokens = int(enc.rate_report_device()["tokens"].sum())
                call = []
                for rep in range(4 * args.reps):
                    t0 = time.perf_counter()
                    enc.rate_report_device()
                    call.append((time.perf_counter() - t0) * 1e3)
            print(json.dumps({"frame": name, "rates": True, "point": "d1 e7", "tokens": tokens,
                              "ms_metrics_off": spread(ms[False]), "ms_metrics_on": spread(ms[True]),
                              "ms_kernel_by_events": round(statistics.median(ms[True]) -
                                                           statistics.median(ms[False]), 4),
                              "ms_rate_report_call_wall": spread(call)}), flush=True)
        sweeper.close()
        del d_img


def ab(args):
    import torch

    import jxg
    from jxg.synth import SEED_BASE, synth_rgb8_device

    has_switch = hasattr(jxg.load(), "jxg_set_sweep_ab")
    grid = [(d, e) for d in DISTANCES for e in EFFORTS]
    flags = jxg.FLAGS_CJXL_DEFAULTS
    # 50 base points, then 50 P+F points each compared with its base
    points = [dict(distance=d, effort=e, proposals=0, flags=flags) for d, e in grid] + \
             [dict(distance=d, effort=e, proposals=3, flags=flags) for d, e in grid]
    base = [-1] * len(grid) + list(range(len(grid)))
    two = [dict(distance=1.0, effort=7, proposals=0, flags=flags),
           dict(distance=1.0, effort=7, proposals=3, flags=flags)]
    for name in args.sizes.split(","):
        w, h, seed = SIZES[name]
        d_img = synth_rgb8_device(w, h, SEED_BASE + seed, 0)
        torch.cuda.synchronize()
        sweeper = jxg.Encoder()

        def sweep(on, pts=points, bs=base, **kw):
            if on:
                kw["ab"] = bs
            return sweeper.sweep_device(d_img.data_ptr(), w, h, pts, quality="psnr", **kw)

        want = sweep(False)  # warm, all buffers
        if has_switch:
            got = sweep(True)
            assert [g[0] for g in got] == [r[0] for r in want], "bytes differ with the switch on"
            for g in got[len(grid):]:
                assert int(g[1]["ab"]["pixels"].sum()) == w * h
                assert int(g[1]["ab"]["sse_b"].sum()) == g[1]["sse"]
        modes = (False, True) if has_switch else (False,)
        wall = {m: [] for m in modes}
        split = {m: [] for m in modes}
        for rep in range(args.reps + 1):
            for m in modes:
                t0 = time.perf_counter()
                sweep(m)
                t1 = time.perf_counter()
                if rep:
                    wall[m].append((t1 - t0) * 1e3)
                    split[m].append(sweeper.sweep_timings())
        res = {"frame": name, "ab": True, "library": os.path.relpath(jxg.LIB_PATH, ROOT),
               "quality": 1, "points": len(points), "reps": args.reps,
               "queues": os.environ.get("GPU_MAX_HW_QUEUES", "default"),
               "lanes": sweeper.sweep_timings()["lanes"]}
        for m in modes:
            mid = sorted(range(len(wall[m])), key=lambda i: wall[m][i])[len(wall[m]) // 2]
            key = "on" if m else "off"
            res["ms_wall_" + key] = spread(wall[m])
            res["ms_recon_" + key] = round(split[m][mid]["ms_recon"], 3)
            res["ms_metrics_" + key] = round(split[m][mid]["ms_metrics"], 3)
        if has_switch:
            res["ms_added_per_pair"] = round(
                (statistics.median(wall[True]) - statistics.median(wall[False])) / len(grid), 4)
        print(json.dumps(res), flush=True)
        if has_switch:
            # the kernels alone, by the events around the metrics of a two-point
            # sweep (d1 e7, none then P+F), alternating.  Against a plain sweep:
            # everything the switch adds (block-map form, rate kernel with its map,
            # two share passes, the snapshot, the transition kernel, the table's
            # copy).  Against a sweep that already runs the strategy and rate
            # reports: the share passes, the snapshot and the transition kernel.
            ms = {k: [] for k in ("plain", "plain_ab", "reports", "reports_ab")}
            for rep in range(4 * args.reps + 1):
                for k in ms:
                    kw = {"strategies": True, "rates": True} if k.startswith("reports") else {}
                    sweep(k.endswith("_ab"), two, [-1, 0], **kw)
                    if rep:
                        ms[k].append(sweeper.sweep_timings()["ms_metrics"])
            with jxg.Encoder(**two[0]) as ea, jxg.Encoder(**two[1]) as eb:
                ea.encode_device(d_img.data_ptr(), w, h)
                eb.encode_device(d_img.data_ptr(), w, h)
                moved = jxg.ab_report_device(ea, eb, d_img.data_ptr())["blocks"]
                call = []
                for rep in range(4 * args.reps):
                    t0 = time.perf_counter()
                    jxg.ab_report_device(ea, eb, d_img.data_ptr())
                    call.append((time.perf_counter() - t0) * 1e3)
            print(json.dumps({
                "frame": name, "ab": True, "pair": "d1 e7 none -> PF",
                "blocks": int(moved.sum()), "blocks_moved": int(moved.sum() - moved.trace()),
                "cells": int((moved != 0).sum()),
                "ms_metrics": {k: spread(v) for k, v in ms.items()},
                "ms_all_added_by_events": round(statistics.median(ms["plain_ab"]) -
                                                statistics.median(ms["plain"]), 4),
                "ms_share_snapshot_transition_by_events": round(
                    statistics.median(ms["reports_ab"]) - statistics.median(ms["reports"]), 4),
                "ms_ab_report_call_wall": spread(call)}), flush=True)
        sweeper.close()
        del d_img


def trace(args):
    import torch

    import jxg
    from jxg.synth import SEED_BASE, synth_rgb8_device

    has_switch = hasattr(jxg.load(), "jxg_set_sweep_trace")
    points = [dict(distance=d, effort=e, proposals=0, flags=jxg.FLAGS_CJXL_DEFAULTS)
              for d in DISTANCES for e in EFFORTS]
    for name in args.sizes.split(","):
        w, h, seed = SIZES[name]
        d_img = synth_rgb8_device(w, h, SEED_BASE + seed, 0)
        torch.cuda.synchronize()
        base = used_mib(torch)
        sweeper = jxg.Encoder()

        def sweep(level, on):
            kw = {"trace": True} if on else {}
            return sweeper.sweep_device(d_img.data_ptr(), w, h, points, quality=QUALITY[level],
                                        **kw)

        want = sweep(2, False)  # warm, all buffers
        mem_off = used_mib(torch) - base
        mem_on = mem_off
        if has_switch:
            got = sweep(2, True)
            mem_on = used_mib(torch) - base
            assert [g[0] for g in got] == [r[0] for r in want], "bytes differ with the switch on"
            nb = ((w + 7) // 8) * ((h + 7) // 8)
            for g, r in zip(got, want):
                assert g[1]["trace"]["blocks"] == nb == int(g[1]["trace"]["flip"].sum())
                assert g[1]["sse"] == r[1]["sse"]
        modes = (False, True) if has_switch else (False,)
        for level in (0, 2):
            wall = {m: [] for m in modes}
            split = {m: [] for m in modes}
            for rep in range(args.reps + 1):
                for m in modes:
                    sweep(level, m)
                    if rep:
                        tm = sweeper.sweep_timings()
                        wall[m].append(tm["ms_call"])
                        split[m].append(tm)
            res = {"frame": name, "trace": True, "library": os.path.relpath(jxg.LIB_PATH, ROOT),
                   "quality": level, "points": len(points), "reps": args.reps,
                   "queues": os.environ.get("GPU_MAX_HW_QUEUES", "default"),
                   "lanes": sweeper.sweep_timings()["lanes"],
                   "mib_switch_off": round(mem_off, 1), "mib_switch_on": round(mem_on, 1)}
            for m in modes:
                mid = sorted(range(len(wall[m])), key=lambda i: wall[m][i])[len(wall[m]) // 2]
                key = "on" if m else "off"
                res["ms_call_" + key] = spread(wall[m])
                res["ms_encode_" + key] = round(split[m][mid]["ms_encode"], 3)
            if has_switch:
                res["ms_added_per_point"] = round(
                    (statistics.median(wall[True]) - statistics.median(wall[False])) / len(points),
                    4)
            print(json.dumps(res), flush=True)
        sweeper.close()
        del d_img


def cli(args):
    import jxg
    from jxg.synth import SEED_BASE, synth_rgb8

    grid = [(d, e) for d in DISTANCES for e in EFFORTS]
    for name in args.sizes.split(","):
        w, h, seed = SIZES[name]
        with tempfile.TemporaryDirectory() as tmp:
            src = os.path.join(tmp, "frame.ppm")
            with open(src, "wb") as f:
                f.write(b"P6\n%d %d\n255\n" % (w, h) + synth_rgb8(w, h, SEED_BASE + seed).tobytes())
            lst = os.path.join(tmp, "grid.txt")
            with open(lst, "w") as f:
                f.writelines("%s %d\n" % (jxg.rust_f64(d), e) for d, e in grid)
            t_sweep, t_runs = [], []
            for rep in range(args.cli_reps):
                t0 = time.perf_counter()
                subprocess.run([jxg.CLI_PATH, src, os.path.join(tmp, "s%d" % rep),
                                "--sweep=" + lst], check=True, capture_output=True)
                t1 = time.perf_counter()
                for d, e in grid:
                    ok, msg = jxg.execute_cjxl(src, os.path.join(tmp, "p%d" % rep,
                                                                 jxg.comp_image_name("frame", d, e)),
                                               d, e)
                    assert ok, msg
                t2 = time.perf_counter()
                t_sweep.append((t1 - t0) * 1e3)
                t_runs.append((t2 - t1) * 1e3)
                for d, e in grid:
                    n = jxg.comp_image_name("frame", d, e)
                    a = open(os.path.join(tmp, "s%d" % rep, n), "rb").read()
                    assert a == open(os.path.join(tmp, "p%d" % rep, n), "rb").read(), n
            print(json.dumps({"frame": name, "cli": True, "points": len(grid),
                              "reps": args.cli_reps, "ms_sweep_process": spread(t_sweep),
                              "ms_50_processes": spread(t_runs)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cli-reps", type=int, default=2)
    ap.add_argument("--sizes", default="8k,768")
    ap.add_argument("--queues", type=int, default=0)
    ap.add_argument("--cli", action="store_true")
    ap.add_argument("--strategies", action="store_true")
    ap.add_argument("--rates", action="store_true")
    ap.add_argument("--ab", action="store_true")
    ap.add_argument("--trace", action="store_true")
    args = ap.parse_args()
    if not 0 <= args.queues <= 32:
        ap.error("--queues: at most 32 hardware queues (0: leave the environment's)")
    if args.queues:
        os.environ["GPU_MAX_HW_QUEUES"] = str(args.queues)
    if args.cli:
        return cli(args)
    import torch  # noqa: F401  (one HIP runtime in the process: DESIGN.md §6)

    if args.strategies:
        return strategies(args)
    if args.rates:
        return rates(args)
    if args.ab:
        return ab(args)
    if args.trace:
        return trace(args)
    library(args)


if __name__ == "__main__":
    main()
