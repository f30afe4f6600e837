#!/usr/bin/env python3
"""Times of the GPU decoder: jxg_decode_rgb8_device of the
benchmark's headline frame (8K synth_rgb8, d1 e7, cjxl defaults) and of a
1080p frame, split into host parse + tables, LF groups on the host threads,
the pass-group kernel and the reconstruction chain (device time by events),
next to jxg_reconstruct_rgb8_device of the same encode.

    python tools/decode_timing.py [--reps 15] [--recon-only]

Warm context, `--reps` repetitions, median and min..max.  --recon-only: the
reconstruct time alone (what a library without the decoder can run, for the
comparison with the commit before it).  Prints one JSON line per frame."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "jpeg-xl-lossy-image-compression-thesis_amd"))

import torch  # noqa: E402,F401  (one HIP runtime in the process: DESIGN.md §6)

import jxg  # noqa: E402
from jxg.synth import SEED_BASE, synth_rgb8_device  # noqa: E402


def spread(v):
    return {"median": round(statistics.median(v), 3), "min": round(min(v), 3),
            "max": round(max(v), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--recon-only", action="store_true")
    args = ap.parse_args()
    for name, w, h, seed in (("8k", 7680, 4320, SEED_BASE + 2), ("1080p", 1920, 1080, SEED_BASE + 3)):
        with jxg.Encoder(distance=1.0, effort=7, flags=jxg.FLAGS_CJXL_DEFAULTS) as enc:
            img = synth_rgb8_device(w, h, seed, 0)
            out = torch.empty_like(img)
            torch.cuda.synchronize()
            data = enc.encode_device(img.data_ptr(), w, h)
            per_group = enc.stats()["ac_tokens"].sum(axis=1)
            tokens, longest = int(per_group.sum()), int(per_group.max())
            rec = []
            for _ in range(args.reps + 2):
                t0 = time.perf_counter()
                enc.reconstruct_device(out.data_ptr())
                rec.append((time.perf_counter() - t0) * 1e3)
            res = {"frame": "%s %dx%d synth_rgb8 d1 e7 cjxl defaults" % (name, w, h),
                   "bytes": len(data), "ac_tokens": tokens, "reps": args.reps,
                   "ms_reconstruct_device_wall": spread(rec[2:])}
            if not args.recon_only:
                want = out.clone()
                keys = ("ms_head", "ms_lf", "ms_groups", "ms_recon", "ms_call")
                runs = {k: [] for k in keys}
                for i in range(args.reps + 2):
                    enc.decode_device(data, out.data_ptr())
                    if i >= 2:
                        t = enc.decode_timings()
                        for k in keys:
                            runs[k].append(t[k])
                assert torch.equal(out, want), "decode differs from reconstruct"
                for k in keys:
                    res[k] = spread(runs[k])
                # all groups' waves are resident at once, so the kernel lasts as long as
                # its longest chain: its time over that group's tokens is the chain's step
                med = statistics.median(runs["ms_groups"])
                res["ns_per_token_all_groups"] = round(1e6 * med / tokens, 4)
                res["longest_group_tokens"] = longest
                res["ns_per_token_longest_chain"] = round(1e6 * med / longest, 2)
                info = jxg.stream_info(data)
                res["num_groups"], res["num_lf_groups"] = info["num_groups"], info["num_lf_groups"]
            print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
