"""Experiment: N one-at-a-time encodes of each of the two 8K bench frames (d1 e7,
cjxl defaults) through one context (JXG_LIB_PATH selects the build), so a
JXG_MERGE_PROFILE build prints its per-phase cycle sums on destroy
(profiles/r10family/mprof_*.txt)."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "jpeg-xl-lossy-image-compression-thesis_amd"))
import torch  # noqa: F401  (one HIP runtime)
import jxg
from jxg.synth import SEED_BASE, synth_rgb8_device
n = int(sys.argv[1]) if len(sys.argv) > 1 else 2
w, h = 7680, 4320
frames = [synth_rgb8_device(w, h, SEED_BASE + 2 + 100 * f) for f in range(2)]  # bench.py's
torch.cuda.synchronize()
enc = jxg.Encoder(distance=1.0, effort=7, flags=jxg.FLAGS_CJXL_DEFAULTS)
for _ in range(n):
    for t in frames:
        enc.encode_device(t.data_ptr(), w, h)
print("encodes", 2 * n, "ms_front", enc.stats()["ms_front"])
enc.close()
