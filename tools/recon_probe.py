"""Cost of the decode-side reconstruction (jxg_reconstruct_rgb8_device) next to
the one-at-a-time encode of the same frame: the 8K synthetic frame of the
headline (config 2, seed 0x4A584C00 + 2) at d1 e7 with cjxl's defaults,
device-resident; a first encode (buffers, code objects), the encode whose
ms_total is reported, one untimed reconstruct, then 20 timed ones (host wall
clock around the synchronous call).  Prints one JSON line.

Traffic model of the kernel split at these flags (Gaborish + one EPF pass):
the tile kernel reads the quantized AC (3 x int16 per pixel) and writes three
f32 planes; Gaborish reads and writes them; the EPF pass reads them and writes
RGB8 -- 6 + 12 + 24 + 12 + 3 = 57 B per pixel (maps and DC: < 0.3 B)."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "jpeg-xl-lossy-image-compression-thesis_amd"))
import torch  # noqa: F401,E402  (one HIP runtime)

import jxg  # noqa: E402
from jxg.synth import CONFIGS, synth_rgb8_device  # noqa: E402

cfg = int(sys.argv[1]) if len(sys.argv) > 1 else 2
distance = float(sys.argv[2]) if len(sys.argv) > 2 else 1.0
effort = int(sys.argv[3]) if len(sys.argv) > 3 else 7
_, w, h, _ = CONFIGS[cfg]
t = synth_rgb8_device(w, h, 0x4A584C00 + cfg)
out = torch.empty_like(t)
torch.cuda.synchronize()
with jxg.Encoder(distance=distance, effort=effort, flags=jxg.FLAGS_CJXL_DEFAULTS) as enc:
    enc.encode_device(t.data_ptr(), w, h)  # allocations, code objects
    data = enc.encode_device(t.data_ptr(), w, h)
    ms_encode = enc.stats()["ms_total"]
    enc.reconstruct_device(out.data_ptr())
    times = []
    for _ in range(20):
        t0 = time.perf_counter()
        enc.reconstruct_device(out.data_ptr())
        times.append((time.perf_counter() - t0) * 1e3)
    q = enc.compare_device(t.data_ptr(), out.data_ptr(), w, h, ssim=False)
# bytes per pixel of the kernel chain: AC in, planes out; one r+w per filter
# pass but the last, which writes RGB8
gab = 1
epf = 0 if distance < 0.7 else 1 if distance < 1.5 else 2 if distance < 4.0 else 3
passes = gab + epf
bpp = 6 + 12 + 24 * (passes - 1) + 12 + 3 if passes else 6 + 3
med, best = statistics.median(times), min(times)
print(json.dumps({
    "probe": "recon", "width": w, "height": h, "distance": distance, "effort": effort,
    "bytes": len(data), "psnr": round(q["psnr"], 3),
    "recon_ms_median": round(med, 3), "recon_ms_best": round(best, 3),
    "encode_ms_total": round(ms_encode, 3), "filter_passes": passes,
    "model_bytes_per_pixel": bpp,
    "model_gbps_at_median": round(bpp * w * h / (med * 1e-3) / 1e9, 1),
}))
