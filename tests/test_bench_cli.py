"""bench.py's multi-GPU launch contract: with WORLD_SIZE
unset, --gpus N > 1 starts the N ranks itself under torch.distributed.run (a
child process, before the GPU is touched); a launcher's WORLD_SIZE must equal
--gpus.  Those two and the --dump-outputs file format are CPU only (nothing in
them reaches a GPU call); the gpu-marked test runs a small plain benchmark."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_world_size_mismatch_exits_nonzero():
    env = dict(os.environ, WORLD_SIZE="2", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "4"],
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 2
    assert "WORLD_SIZE=2 but --gpus 4" in r.stderr


def test_gpus_n_spawns_ranks(monkeypatch):
    sys.path.insert(0, ROOT)
    import bench

    calls = []

    def fake_call(cmd):
        calls.append(cmd)
        return 7

    monkeypatch.setattr(subprocess, "call", fake_call)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "8", "--steps", "3"])
    try:
        bench.main()
        raise AssertionError("bench.main returned")
    except SystemExit as e:
        assert e.code == 7  # the child's status
    (cmd,) = calls
    assert cmd[1:3] == ["-m", "torch.distributed.run"]
    assert cmd[cmd.index("--nproc-per-node") + 1] == "8"
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1"
    assert cmd[-4:] == [os.path.join(ROOT, "bench.py"), "--gpus", "8", "--steps", "3"][-4:]
    assert cmd[-5] == os.path.join(ROOT, "bench.py")


def test_dump_outputs_arrays(tmp_path, monkeypatch):
    """--dump-outputs' files: the bytes as float32 (whole when they fit, else a
    fixed sorted sample), the length as float64; the same input gives the same
    files"""
    sys.path.insert(0, ROOT)
    import bench

    data = np.random.default_rng(5).integers(0, 256, 1000, dtype=np.uint8).tobytes()
    bench.dump_outputs(str(tmp_path / "a"), data)
    a = np.load(tmp_path / "a" / "codestream.npy")
    assert a.dtype == np.float32 and a.astype(np.uint8).tobytes() == data
    n = np.load(tmp_path / "a" / "codestream_bytes.npy")
    assert n.dtype == np.float64 and n.tolist() == [1000.0]
    monkeypatch.setattr(bench, "DUMP_MAX_VALUES", 64)
    bench.dump_outputs(str(tmp_path / "b"), data)
    bench.dump_outputs(str(tmp_path / "c"), data)
    b = np.load(tmp_path / "b" / "codestream.npy")
    assert b.dtype == np.float32 and b.shape == (64,)
    assert np.array_equal(b, np.load(tmp_path / "c" / "codestream.npy"))
    # a sample of the stream, in stream order: a subsequence of it
    it = iter(a.tolist())
    assert all(v in it for v in b.tolist())
    assert np.load(tmp_path / "b" / "codestream_bytes.npy").tolist() == [1000.0]


@pytest.mark.gpu
def test_plain_run_dumps_the_last_step(tmp_path, oracle):
    """A plain run prints the headline line without the --full measurements
    and --dump-outputs holds the codestream of the last timed step: 3 steps
    over 2 frames end on frame 0, whose bytes the oracle gives."""
    import jxg
    from jxg.synth import CONFIGS, SEED_BASE, synth_rgb8

    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1",
                        "--config", "0", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(tmp_path / "out")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    (line,) = [l for l in r.stdout.splitlines() if l.startswith("{")]
    res = json.loads(line)
    _, w, h, _ = CONFIGS[0]
    assert res["steps"] == 3 and res["unit"] == "MPix/s" and res["higher_is_better"] is True
    assert res["ms_per_step"] > 0
    # value and ms_per_step state the same time (ms_per_step is rounded to 0.001 ms)
    tol = (0.0005 / res["ms_per_step"] + 1e-3) * res["value"] + 0.01
    assert abs(res["value"] - w * h / 1e3 / res["ms_per_step"]) <= tol
    for key in ("roofline", "merge_stage", "ans_chain", "alt_coder", "thesis_proposals",
                "filters_off", "roofline_e4", "quality", "single_image", "cpu_baseline"):
        assert key not in res
    ref = oracle.encode(synth_rgb8(w, h, SEED_BASE + 0), 1.0, 7, 0, 1,
                        jxg.ORACLE_FILTERS_CJXL_DEFAULTS).bytes
    got = np.load(tmp_path / "out" / "codestream.npy")
    assert got.dtype == np.float32
    assert got.astype(np.uint8).tobytes() == ref
    assert np.load(tmp_path / "out" / "codestream_bytes.npy").tolist() == [float(len(ref))]
    assert res["bytes_per_frame"] == len(ref)
