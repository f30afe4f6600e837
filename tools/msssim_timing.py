#!/usr/bin/env python3
"""Times of MS-SSIM on the GPU, at 8K and at 768 x 512.

    python tools/msssim_timing.py [--reps 5] [--calls 20] [--sizes 8k,768] [--queues N]
                                  [--part pair,sweep]

pair:  the synthetic frame against itself with +-6 noise, both on the device:
       `compare_device` with SSIM against `msssim_device`, alternating, `--reps`
       repetitions of `--calls` calls each after a warm call.  Both calls end in
       a stream synchronise, so the host clock around a call is the device time
       of its kernels plus one launch / copy / synchronise round (the same
       round for both); per-call median and min..max over the repetitions.
       The kernels alone: run this part under `rocprofv3 --kernel-trace --stats`.
sweep: the harness's 50-point grid (10 distances x 5 efforts, cjxl's default
       flags) through `sweep_device` with quality "ssim" against the same with
       "msssim", alternating; host wall time and the jxg_sweep_timings split of
       the median sweep.  The two must give the same bytes and quality records.

Prints one JSON line per measurement."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "jpeg-xl-lossy-image-compression-thesis_amd"))

DISTANCES = [0.5, 1.0, 1.5, 3.0, 4.0, 6.0, 8.0, 10.0, 12.0, 14.0]
EFFORTS = [5, 6, 7, 8, 9]
SIZES = {"8k": (7680, 4320, 2), "768": (768, 512, 5)}


def spread(v):
    return {"median": round(statistics.median(v), 3), "min": round(min(v), 3),
            "max": round(max(v), 3)}


def pair(args, torch, jxg, name, d_img):
    w, h, _ = SIZES[name]
    noise = torch.randint(-6, 7, d_img.shape, device=d_img.device, dtype=torch.int16,
                          generator=torch.Generator(device=d_img.device).manual_seed(1))
    d_cmp = (d_img.to(torch.int16) + noise).clamp_(0, 255).to(torch.uint8)
    del noise
    torch.cuda.synchronize()
    a, b = d_img.data_ptr(), d_cmp.data_ptr()
    with jxg.Encoder() as enc:
        q = enc.compare_device(a, b, w, h)
        m = enc.msssim_device(a, b, w, h)
        assert m["ssim"][0] == q["ssim"], "ssim[0] differs from compare_device's"
        t_cmp, t_ms = [], []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            for _ in range(args.calls):
                enc.compare_device(a, b, w, h)
            t1 = time.perf_counter()
            for _ in range(args.calls):
                enc.msssim_device(a, b, w, h)
            t2 = time.perf_counter()
            t_cmp.append((t1 - t0) * 1e3 / args.calls)
            t_ms.append((t2 - t1) * 1e3 / args.calls)
    print(json.dumps({"frame": "%s %dx%d" % (name, w, h), "part": "pair", "reps": args.reps,
                      "calls": args.calls, "ms_compare_ssim": spread(t_cmp),
                      "ms_msssim": spread(t_ms),
                      "msssim_over_compare": round(statistics.median(t_ms) /
                                                   statistics.median(t_cmp), 3),
                      "ms_ssim": m["ms_ssim"], "cs": m["cs"]}), flush=True)


def sweep(args, torch, jxg, name, d_img):
    w, h, _ = SIZES[name]
    points = [dict(distance=d, effort=e, proposals=0, flags=jxg.FLAGS_CJXL_DEFAULTS)
              for d in DISTANCES for e in EFFORTS]
    keys = ("sse", "samples", "mse", "psnr", "ssim")
    with jxg.Encoder() as enc:
        def run(quality):
            return enc.sweep_device(d_img.data_ptr(), w, h, points, quality=quality)

        want = run("ssim")
        got = run("msssim")
        assert [g[0] for g in got] == [r[0] for r in want], "bytes differ with MS-SSIM on"
        assert all(repr([g[1][k] for k in keys]) == repr([r[1][k] for k in keys])
                   for g, r in zip(got, want)), "quality differs with MS-SSIM on"
        t, split = {"ssim": [], "msssim": []}, {"ssim": [], "msssim": []}
        for _ in range(args.reps):
            for quality in ("ssim", "msssim"):
                t0 = time.perf_counter()
                run(quality)
                t[quality].append((time.perf_counter() - t0) * 1e3)
                split[quality].append(enc.sweep_timings())
        res = {"frame": "%s %dx%d" % (name, w, h), "part": "sweep", "points": len(points),
               "reps": args.reps, "queues": os.environ.get("GPU_MAX_HW_QUEUES", "default"),
               "lanes": split["ssim"][0]["lanes"],
               "ms_ssim_range": [min(g[1]["ms_ssim"] for g in got),
                                 max(g[1]["ms_ssim"] for g in got)]}
        for quality in ("ssim", "msssim"):
            v = t[quality]
            mid = sorted(range(len(v)), key=lambda i: v[i])[len(v) // 2]
            res["ms_wall_" + quality] = spread(v)
            res["timings_of_median_" + quality] = {
                k: round(x, 3) if isinstance(x, float) else x for k, x in split[quality][mid].items()}
        res["ms_added_per_point"] = round((statistics.median(t["msssim"]) -
                                           statistics.median(t["ssim"])) / len(points), 3)
        print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--sizes", default="8k,768")
    ap.add_argument("--queues", type=int, default=0)
    ap.add_argument("--part", default="pair,sweep")
    args = ap.parse_args()
    if not 0 <= args.queues <= 32:
        ap.error("--queues: at most 32 hardware queues (0: leave the environment's)")
    if args.queues:
        os.environ["GPU_MAX_HW_QUEUES"] = str(args.queues)
    import torch  # (one HIP runtime in the process: DESIGN.md §6)

    import jxg
    from jxg.synth import SEED_BASE, synth_rgb8_device

    for name in args.sizes.split(","):
        w, h, seed = SIZES[name]
        d_img = synth_rgb8_device(w, h, SEED_BASE + seed, 0)
        torch.cuda.synchronize()
        for part in args.part.split(","):
            {"pair": pair, "sweep": sweep}[part](args, torch, jxg, name, d_img)
        del d_img


if __name__ == "__main__":
    main()
