"""jxg -- Python host mirror of the MI355X JPEG XL VarDCT encode path.

Thin ctypes layer over the C ABI in include/jxg.h (libjxg.so, built in-tree
for gfx950).  It mirrors the reference harness's encoder boundary:

* ``execute_cjxl(input, output, distance, effort)`` follows
  ``DockerManager::execute_cjxl`` (benchmark-jpegxl/src/docker_manager.rs:
  100-137): ``mkdir -p dirname(output)``, run the encoder with
  ``--distance=D --effort=E``, return ``(True, stdout)`` on exit 0 and
  ``(False, stderr-or-stdout)`` otherwise;
* ``comp_image_name`` is the ``{stem}-{distance}-{effort}.jxl`` naming of
  benchmark.rs:644-650 (Rust ``{}`` formatting of f64);
* ``calculate_mse`` / ``calculate_psnr`` restate image_reader.rs:555-606.

There is no CPU fallback: importing works anywhere, but every encode goes
through libjxg.so on a HIP device and raises if either is missing.
"""
from __future__ import annotations

import ctypes
import math
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("JXG_LIB_PATH") or os.path.join(HERE, "libjxg.so")  # override: experiments only
CLI_PATH = os.path.join(HERE, "jxg_cjxl")
DJXL_PATH = os.path.join(HERE, "jxg_djxl")

PROPOSAL_P = 1
PROPOSAL_F = 2
FLAG_H1_INT_ABS = 1
FLAG_KEEP_MAPS = 2
FLAG_ANS = 4
FLAG_FORCE_ONE_STREAM = 8  # testing: the split assembly's one-stream fallback (same bytes)
FLAG_GABORISH = 16  # encoder inverse Gaborish + the decoder's Gaborish (cjxl --gaborish=1)
FLAG_EPF = 32  # the decoder's edge-preserving filter, iterations by distance (cjxl --epf=-1)
FLAG_AQ_MASKING = 64  # libjxl-shaped masking quant field (oracle/aq.c) instead of the activity AQ
# JXG_FLAGS_CJXL_DEFAULTS: what `cjxl IN OUT --distance=D --effort=E` encodes
# (docker_manager.rs:126-136) -- jxg_cjxl's defaults, bench.py's headline
FLAGS_CJXL_DEFAULTS = FLAG_ANS | FLAG_GABORISH | FLAG_EPF | FLAG_AQ_MASKING
# the same set as the oracle's filters mask (oracle/jxo.h: GAB 1 | EPF 2 | AQ_MASKING 4; coder 1)
ORACLE_FILTERS_CJXL_DEFAULTS = 7


class JxgError(RuntimeError):
    pass


class _Params(ctypes.Structure):
    _fields_ = [("distance", ctypes.c_float), ("effort", ctypes.c_int),
                ("proposals", ctypes.c_uint32), ("num_devices", ctypes.c_int),
                ("flags", ctypes.c_uint32), ("device", ctypes.c_int)]


class _Buffer(ctypes.Structure):
    _fields_ = [("data", ctypes.POINTER(ctypes.c_uint8)), ("size", ctypes.c_size_t)]


class _Stats(ctypes.Structure):
    _fields_ = [("xsize", ctypes.c_uint32), ("ysize", ctypes.c_uint32),
                ("xsize_blocks", ctypes.c_uint32), ("ysize_blocks", ctypes.c_uint32),
                ("num_groups", ctypes.c_uint32), ("num_lf_groups", ctypes.c_uint32),
                ("global_scale", ctypes.c_uint32), ("quant_dc", ctypes.c_uint32),
                ("bytes", ctypes.c_size_t),
                ("ac_strategy", ctypes.POINTER(ctypes.c_uint8)),
                ("quant_field", ctypes.POINTER(ctypes.c_uint8)),
                ("dc", ctypes.POINTER(ctypes.c_int32)),
                ("ac", ctypes.POINTER(ctypes.c_int32)),
                ("ac_tokens", ctypes.POINTER(ctypes.c_uint32)),
                ("homogeneity", ctypes.POINTER(ctypes.c_float)),
                ("ms_front", ctypes.c_float), ("ms_histogram", ctypes.c_float),
                ("ms_emit", ctypes.c_float), ("ms_assemble", ctypes.c_float),
                ("ms_total", ctypes.c_float), ("ms_host_call", ctypes.c_float),
                ("ms_host_codes", ctypes.c_float), ("ms_host_layout", ctypes.c_float),
                ("ms_front_kernel", ctypes.c_float), ("ms_aq", ctypes.c_float)]


class _StreamInfo(ctypes.Structure):
    _fields_ = [(k, ctypes.c_uint32) for k in (
        "xsize", "ysize", "num_groups", "num_lf_groups", "global_scale", "quant_dc",
        "num_hf_presets", "ans", "gaborish", "epf_iters")]


class _DecodeBatchStats(ctypes.Structure):
    _fields_ = [(k, ctypes.c_uint32) for k in ("frames", "chunks", "items_staged",
                                               "items_unstaged")] + [
        (k, ctypes.c_float) for k in ("ms_parse", "ms_groups", "ms_recon", "ms_call")]


class _Quality(ctypes.Structure):
    _fields_ = [("sse", ctypes.c_uint64), ("samples", ctypes.c_uint64), ("mse", ctypes.c_double),
                ("psnr", ctypes.c_double), ("ssim", ctypes.c_double)]


class _Msssim(ctypes.Structure):
    _fields_ = [("ms_ssim", ctypes.c_double), ("cs", ctypes.c_double * 5),
                ("ssim", ctypes.c_double * 5)]

    def as_dict(self) -> dict:
        return {"ms_ssim": float(self.ms_ssim), "cs": [float(v) for v in self.cs],
                "ssim": [float(v) for v in self.ssim]}


NUM_STRATEGIES = 27
# the project's names of the raw AcStrategy ids 0..26 (rows x columns in pixels;
# the encoder never emits AFV0..3)
STRATEGY_NAMES = (
    "DCT8", "IDENTITY", "DCT2X2", "DCT4X4", "DCT16X16", "DCT32X32", "DCT16X8", "DCT8X16",
    "DCT32X8", "DCT8X32", "DCT32X16", "DCT16X32", "DCT4X8", "DCT8X4", "AFV0", "AFV1", "AFV2",
    "AFV3", "DCT64X64", "DCT64X32", "DCT32X64", "DCT128X128", "DCT128X64", "DCT64X128",
    "DCT256X256", "DCT256X128", "DCT128X256")


class _StrategyRow(ctypes.Structure):
    _fields_ = [("varblocks", ctypes.c_uint64), ("blocks", ctypes.c_uint64),
                ("pixels", ctypes.c_uint64), ("nonzeros", ctypes.c_uint64 * 3),
                ("qf_sum", ctypes.c_uint64), ("sse", ctypes.c_uint64)]


class _StrategyReport(ctypes.Structure):
    _fields_ = [("row", _StrategyRow * NUM_STRATEGIES)]

    def as_dict(self) -> dict:
        """numpy arrays keyed by field name ([27] uint64, nonzeros [27, 3]) + names"""
        t = np.frombuffer(bytes(self), dtype=np.uint64).reshape(NUM_STRATEGIES, 8)
        return {"varblocks": t[:, 0].copy(), "blocks": t[:, 1].copy(), "pixels": t[:, 2].copy(),
                "nonzeros": t[:, 3:6].copy(), "qf_sum": t[:, 6].copy(), "sse": t[:, 7].copy(),
                "names": STRATEGY_NAMES}


RATE_UNIT = 256  # JXG_RATE_UNIT: costs are integers in 1 / 256 bit


class _RateRow(ctypes.Structure):
    _fields_ = [("tokens", ctypes.c_uint64 * 3), ("cost", ctypes.c_uint64 * 3)]


class _RateReport(ctypes.Structure):
    _fields_ = [("row", _RateRow * NUM_STRATEGIES), ("ac_bits", ctypes.c_uint64),
                ("stream_bits", ctypes.c_uint64), ("ans", ctypes.c_uint32),
                ("groups", ctypes.c_uint32)]

    def as_dict(self) -> dict:
        """``tokens`` / ``cost`` [27, 3] uint64 (X, Y, B; cost in 1 / RATE_UNIT bit),
        the four scalars, names"""
        t = np.frombuffer(bytes(self.row), dtype=np.uint64).reshape(NUM_STRATEGIES, 6)
        return {"tokens": t[:, 0:3].copy(), "cost": t[:, 3:6].copy(),
                "ac_bits": int(self.ac_bits), "stream_bits": int(self.stream_bits),
                "ans": int(self.ans), "groups": int(self.groups), "names": STRATEGY_NAMES}


class _AbReport(ctypes.Structure):
    _fields_ = [("cell", ctypes.c_uint64 * (NUM_STRATEGIES * NUM_STRATEGIES * 6))]

    _KEYS = ("blocks", "pixels", "sse_a", "sse_b", "cost_a", "cost_b")

    def as_dict(self) -> dict:
        """six ``[27, 27]`` uint64 arrays indexed ``[from, to]`` (costs in
        1 / RATE_UNIT bit) + names"""
        t = np.frombuffer(bytes(self), dtype=np.uint64).reshape(NUM_STRATEGIES, NUM_STRATEGIES, 6)
        out = {k: t[:, :, i].copy() for i, k in enumerate(self._KEYS)}
        out["names"] = STRATEGY_NAMES
        return out


# search trace (jxg_search_trace): plane orders and the two structures
TRACE_SCAN_IDS = (0, 3, 2, 12, 13, 1)   # DCT8, DCT4X4, DCT2X2, DCT4X8, DCT8X4, IDENTITY
TRACE_MERGED_IDS = (6, 7, 4, 10, 11, 5, 19, 20, 18)
TRACE_BIG_IDS = (22, 23, 21, 25, 26, 24)
# name -> (planes, dtype) of jxg_trace_maps, in the structure's order
_TRACE_PLANES = (("cand8_raw", 6, np.float32), ("cand8", 6, np.float32), ("scan8", 0, np.uint8),
                 ("front8", 0, np.uint8), ("qf8", 0, np.uint8), ("merged", 9, np.float32),
                 ("big", 6, np.float32), ("chosen", 0, np.float32))


class _TraceMaps(ctypes.Structure):
    _fields_ = [(k, ctypes.c_void_p) for k, _, _ in _TRACE_PLANES]


class _TraceSummary(ctypes.Structure):
    _fields_ = [("blocks", ctypes.c_uint32), ("max_px", ctypes.c_uint32),
                ("flip", ctypes.c_uint32 * 36), ("hook_p", ctypes.c_uint32 * 6),
                ("merged_over", ctypes.c_uint32 * 6), ("margin", ctypes.c_uint32 * 48),
                ("margin_skipped", ctypes.c_uint32 * 6)]

    def as_dict(self) -> dict:
        """blocks, max_px and the uint32 arrays flip [6, 6], hook_p [6],
        merged_over [6], margin [6, 8], margin_skipped [6]"""
        arr = lambda a, *shape: np.array(a, dtype=np.uint32).reshape(shape)  # noqa: E731
        return {"blocks": int(self.blocks), "max_px": int(self.max_px),
                "flip": arr(self.flip, 6, 6), "hook_p": arr(self.hook_p, 6),
                "merged_over": arr(self.merged_over, 6), "margin": arr(self.margin, 6, 8),
                "margin_skipped": arr(self.margin_skipped, 6)}


def rate_symbol_cost(f: int) -> int:
    """jxg_rate_symbol_cost: an ANS symbol of normalised frequency f in 1 / 256 bit"""
    return int(load().jxg_rate_symbol_cost(f))


class _SweepPoint(ctypes.Structure):
    _fields_ = [("distance", ctypes.c_float), ("effort", ctypes.c_int),
                ("proposals", ctypes.c_uint32), ("flags", ctypes.c_uint32)]


class _SweepStats(ctypes.Structure):
    _fields_ = [(k, ctypes.c_uint32) for k in ("points", "lanes")] + [
        (k, ctypes.c_float) for k in ("ms_call", "ms_upload", "ms_encode", "ms_recon",
                                      "ms_metrics")]


# every symbol declared in include/jxg.h
EXPORTS = ("jxg_status_str", "jxg_create", "jxg_destroy", "jxg_encode_rgb8",
           "jxg_encode_rgb8_device", "jxg_encode_batch_rgb8", "jxg_get_stats",
           "jxg_buffer_free", "jxg_homogeneity_map", "jxg_shard_sizes", "jxg_shard_begin",
           "jxg_shard_end", "jxg_shard_payload", "jxg_shard_assemble_device",
           "jxg_shard_assemble", "jxg_compare_rgb8", "jxg_compare_rgb8_device",
           "jxg_shard_head", "jxg_shard_write_host", "jxg_host_register", "jxg_host_unregister",
           "jxg_encode_batch_rgb8_device", "jxg_synth_rgb8_device", "jxg_shard_exchange",
           "jxg_submit_rgb8", "jxg_submit_rgb8_device", "jxg_receive", "jxg_pending",
           "jxg_set_input_stream", "jxg_pipeline_depth", "jxg_shard_plan",
           "jxg_shard_submit_device", "jxg_shard_next_head", "jxg_shard_write_next",
           "jxg_shard_write_flush", "jxg_set_pipeline_lanes", "jxg_warmup",
           "jxg_reconstruct_rgb8", "jxg_reconstruct_rgb8_device",
           "jxg_decode_info", "jxg_decode_rgb8", "jxg_decode_rgb8_device", "jxg_decode_maps",
           "jxg_decode_timings", "jxg_decode_batch_rgb8", "jxg_decode_batch_rgb8_device",
           "jxg_set_decode_batch_bytes", "jxg_decode_batch_timings",
           "jxg_sweep_rgb8", "jxg_sweep_rgb8_device", "jxg_sweep_timings",
           "jxg_msssim_rgb8", "jxg_msssim_rgb8_device", "jxg_set_sweep_msssim",
           "jxg_sweep_msssim",
           "jxg_strategy_report_rgb8", "jxg_strategy_report_rgb8_device",
           "jxg_set_sweep_report", "jxg_sweep_report",
           "jxg_rate_symbol_cost", "jxg_rate_report", "jxg_rate_report_device",
           "jxg_set_sweep_rates", "jxg_sweep_rates",
           "jxg_ab_report_rgb8", "jxg_ab_report_rgb8_device",
           "jxg_set_sweep_ab", "jxg_sweep_ab",
           "jxg_check_strategy_map", "jxg_encode_forced_rgb8", "jxg_encode_forced_rgb8_device",
           "jxg_encode_traced_rgb8", "jxg_encode_traced_rgb8_device", "jxg_search_trace",
           "jxg_set_sweep_trace", "jxg_sweep_trace",
)

_lib = None


def load():
    """Load libjxg.so (raises JxgError if it was not built)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise JxgError("libjxg.so not built at %s (run __graft_entry__.build())" % LIB_PATH)
    lib = ctypes.CDLL(LIB_PATH)
    vp = ctypes.c_void_p
    lib.jxg_status_str.restype = ctypes.c_char_p
    lib.jxg_status_str.argtypes = [ctypes.c_int]
    lib.jxg_create.argtypes = [ctypes.POINTER(_Params), ctypes.POINTER(vp)]
    lib.jxg_destroy.argtypes = [vp]
    lib.jxg_destroy.restype = None
    lib.jxg_encode_rgb8.argtypes = [vp, vp, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_size_t,
                                    ctypes.POINTER(_Buffer)]
    lib.jxg_encode_rgb8_device.argtypes = [vp, vp, ctypes.c_uint32, ctypes.c_uint32,
                                           ctypes.c_size_t, ctypes.POINTER(_Buffer)]
    lib.jxg_encode_batch_rgb8.argtypes = [vp, ctypes.POINTER(ctypes.c_void_p), ctypes.c_uint32,
                                          ctypes.c_uint32, ctypes.c_uint32, ctypes.c_size_t,
                                          ctypes.POINTER(_Buffer)]
    lib.jxg_encode_batch_rgb8_device.argtypes = lib.jxg_encode_batch_rgb8.argtypes
    lib.jxg_submit_rgb8.argtypes = [vp, vp, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_size_t]
    lib.jxg_submit_rgb8_device.argtypes = lib.jxg_submit_rgb8.argtypes
    lib.jxg_receive.argtypes = [vp, ctypes.POINTER(_Buffer)]
    lib.jxg_pending.argtypes = [vp, ctypes.POINTER(ctypes.c_uint32)]
    lib.jxg_get_stats.argtypes = [vp, ctypes.POINTER(_Stats)]
    lib.jxg_buffer_free.argtypes = [ctypes.POINTER(_Buffer)]
    lib.jxg_buffer_free.restype = None
    lib.jxg_homogeneity_map.argtypes = [vp, vp, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_float,
                                        ctypes.c_uint32, vp, vp]
    sz = ctypes.c_size_t
    lib.jxg_shard_sizes.argtypes = [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32,
                                    ctypes.POINTER(sz), ctypes.POINTER(sz)]
    lib.jxg_shard_exchange.argtypes = [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32,
                                       ctypes.c_uint32, ctypes.POINTER(sz), ctypes.POINTER(sz)]
    lib.jxg_shard_begin.argtypes = [vp, vp, ctypes.c_uint32, ctypes.c_uint32, sz, ctypes.c_uint32,
                                    ctypes.c_uint32, vp, vp]
    lib.jxg_shard_end.argtypes = [vp, vp, vp, ctypes.POINTER(sz)]
    lib.jxg_shard_payload.argtypes = [vp, vp, ctypes.c_int]
    lib.jxg_shard_assemble_device.argtypes = [vp, vp, ctypes.POINTER(sz), ctypes.POINTER(sz),
                                              ctypes.c_uint32, ctypes.POINTER(_Buffer)]
    lib.jxg_shard_assemble.argtypes = [ctypes.POINTER(ctypes.POINTER(ctypes.c_uint8)),
                                       ctypes.POINTER(sz), ctypes.c_uint32, ctypes.POINTER(_Buffer)]
    lib.jxg_shard_head.argtypes = [vp, vp, ctypes.POINTER(sz)]
    lib.jxg_shard_write_host.argtypes = [vp, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(sz),
                                         ctypes.c_uint32, vp, sz, ctypes.POINTER(sz)]
    lib.jxg_set_input_stream.argtypes = [vp, vp]
    lib.jxg_pipeline_depth.argtypes = [vp, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32,
                                       ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32)]
    lib.jxg_shard_plan.argtypes = [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, vp, vp,
                                   ctypes.POINTER(ctypes.c_int)]
    lib.jxg_shard_submit_device.argtypes = [vp, vp, ctypes.c_uint32, ctypes.c_uint32, sz,
                                            ctypes.c_uint32, ctypes.c_uint32]
    lib.jxg_shard_next_head.argtypes = [vp, vp, ctypes.POINTER(sz)]
    lib.jxg_shard_write_next.argtypes = lib.jxg_shard_write_host.argtypes
    lib.jxg_shard_write_flush.argtypes = [vp]
    lib.jxg_set_pipeline_lanes.argtypes = [vp, ctypes.c_uint32]
    u32 = ctypes.c_uint32
    lib.jxg_host_register.argtypes = [vp, sz]
    lib.jxg_host_unregister.argtypes = [vp]
    cmp_args = [vp, vp, sz, vp, sz, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_int,
                ctypes.POINTER(_Quality)]
    lib.jxg_compare_rgb8.argtypes = cmp_args
    lib.jxg_compare_rgb8_device.argtypes = cmp_args
    lib.jxg_synth_rgb8_device.argtypes = [vp, vp, ctypes.c_uint32, ctypes.c_uint32, sz,
                                          ctypes.c_uint64]
    lib.jxg_warmup.argtypes = [vp, ctypes.c_uint32, ctypes.c_uint32]
    lib.jxg_reconstruct_rgb8.argtypes = [vp, vp, sz]
    lib.jxg_reconstruct_rgb8_device.argtypes = [vp, vp, sz]
    lib.jxg_decode_info.argtypes = [vp, sz, ctypes.POINTER(_StreamInfo)]
    lib.jxg_decode_rgb8.argtypes = [vp, vp, sz, vp, sz]
    lib.jxg_decode_rgb8_device.argtypes = [vp, vp, sz, vp, sz]
    lib.jxg_decode_maps.argtypes = [vp, vp, sz, vp, vp, vp, vp, vp]
    lib.jxg_decode_timings.argtypes = [vp, ctypes.POINTER(ctypes.c_float)]
    lib.jxg_decode_batch_rgb8.argtypes = [vp, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(sz),
                                          ctypes.c_uint32, ctypes.POINTER(vp), ctypes.POINTER(sz),
                                          ctypes.POINTER(ctypes.c_int)]
    lib.jxg_decode_batch_rgb8_device.argtypes = lib.jxg_decode_batch_rgb8.argtypes
    lib.jxg_set_decode_batch_bytes.argtypes = [vp, sz]
    lib.jxg_decode_batch_timings.argtypes = [vp, ctypes.POINTER(_DecodeBatchStats)]
    lib.jxg_sweep_rgb8.argtypes = [vp, vp, ctypes.c_uint32, ctypes.c_uint32, sz,
                                   ctypes.POINTER(_SweepPoint), ctypes.c_uint32, ctypes.c_int,
                                   ctypes.POINTER(_Buffer), ctypes.POINTER(_Quality),
                                   ctypes.POINTER(ctypes.c_int)]
    lib.jxg_sweep_rgb8_device.argtypes = lib.jxg_sweep_rgb8.argtypes
    lib.jxg_sweep_timings.argtypes = [vp, ctypes.POINTER(_SweepStats)]
    ms_args = [vp, vp, sz, vp, sz, ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(_Msssim)]
    lib.jxg_msssim_rgb8.argtypes = ms_args
    lib.jxg_msssim_rgb8_device.argtypes = ms_args
    lib.jxg_set_sweep_msssim.argtypes = [vp, ctypes.c_int]
    lib.jxg_sweep_msssim.argtypes = [vp, ctypes.POINTER(_Msssim), ctypes.c_uint32]
    rep_args = [vp, vp, sz, ctypes.POINTER(_StrategyReport), vp]
    lib.jxg_strategy_report_rgb8.argtypes = rep_args
    lib.jxg_strategy_report_rgb8_device.argtypes = rep_args
    lib.jxg_set_sweep_report.argtypes = [vp, ctypes.c_int]
    lib.jxg_sweep_report.argtypes = [vp, ctypes.POINTER(_StrategyReport), ctypes.c_uint32]
    lib.jxg_rate_symbol_cost.argtypes = [ctypes.c_uint32]
    lib.jxg_rate_symbol_cost.restype = ctypes.c_uint32
    lib.jxg_rate_report.argtypes = [vp, ctypes.POINTER(_RateReport), vp]
    lib.jxg_rate_report_device.argtypes = [vp, ctypes.POINTER(_RateReport), vp]
    lib.jxg_set_sweep_rates.argtypes = [vp, ctypes.c_int]
    lib.jxg_sweep_rates.argtypes = [vp, ctypes.POINTER(_RateReport), ctypes.c_uint32]
    ab_args = [vp, vp, vp, ctypes.c_size_t, ctypes.POINTER(_AbReport), vp]
    lib.jxg_ab_report_rgb8.argtypes = ab_args
    lib.jxg_ab_report_rgb8_device.argtypes = ab_args
    lib.jxg_set_sweep_ab.argtypes = [vp, ctypes.POINTER(ctypes.c_int32), ctypes.c_uint32]
    lib.jxg_sweep_ab.argtypes = [vp, ctypes.POINTER(_AbReport), ctypes.c_uint32]
    lib.jxg_check_strategy_map.argtypes = [vp, ctypes.c_uint32, ctypes.c_uint32,
                                           ctypes.POINTER(ctypes.c_uint32)]
    forced_args = [vp, vp, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_size_t, vp, vp,
                   ctypes.POINTER(_Buffer)]
    lib.jxg_encode_forced_rgb8.argtypes = forced_args
    lib.jxg_encode_forced_rgb8_device.argtypes = forced_args
    traced_args = [vp, vp, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_size_t,
                   ctypes.POINTER(_Buffer)]
    lib.jxg_encode_traced_rgb8.argtypes = traced_args
    lib.jxg_encode_traced_rgb8_device.argtypes = traced_args
    lib.jxg_search_trace.argtypes = [vp, ctypes.POINTER(_TraceMaps),
                                     ctypes.POINTER(_TraceSummary)]
    lib.jxg_set_sweep_trace.argtypes = [vp, ctypes.c_int]
    lib.jxg_sweep_trace.argtypes = [vp, ctypes.POINTER(_TraceSummary), ctypes.c_uint32]
    _lib = lib
    return lib


def _check(st):
    if st != 0:
        raise JxgError("jxg: %s (%d)" % (load().jxg_status_str(st).decode(), st))


class Codestream:
    """Zero-copy view of a jxg_buffer; released with jxg_buffer_free."""

    def __init__(self, buf):
        self._buf = buf
        self.size = buf.size

    def memoryview(self):
        return memoryview((ctypes.c_uint8 * self.size).from_address(self._buf.data)).cast("B")

    def tobytes(self) -> bytes:
        return ctypes.string_at(self._buf.data, self.size)

    def __len__(self):
        return self.size

    def release(self):
        if self._buf is not None and self._buf.data:
            load().jxg_buffer_free(ctypes.byref(self._buf))
        self._buf = None

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass


class Encoder:
    """One encoder context (= one HIP stream + device buffers) on one GPU."""

    def __init__(self, distance=1.0, effort=7, proposals=0, device=0, flags=0, num_devices=1):
        lib = load()
        self.params = _Params(distance, effort, proposals, num_devices, flags, device)
        self._ctx = ctypes.c_void_p()
        self._last_wh = None  # size of the last one-at-a-time encode (reconstruct)
        _check(lib.jxg_create(ctypes.byref(self.params), ctypes.byref(self._ctx)))

    def close(self):
        if self._ctx:
            load().jxg_destroy(self._ctx)
            self._ctx = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @staticmethod
    def _take(buf):
        try:
            return ctypes.string_at(buf.data, buf.size)
        finally:
            load().jxg_buffer_free(ctypes.byref(buf))

    def encode(self, rgb: np.ndarray) -> bytes:
        """Host (H, W, 3) uint8 -> codestream bytes."""
        rgb = np.ascontiguousarray(rgb, dtype=np.uint8)
        h, w, c = rgb.shape
        if c != 3:
            raise ValueError("expected (H, W, 3) uint8")
        buf = _Buffer()
        _check(load().jxg_encode_rgb8(self._ctx, rgb.ctypes.data, w, h, w * 3, ctypes.byref(buf)))
        self._last_wh = (w, h)
        return self._take(buf)

    @staticmethod
    def _forced_maps(strategy, quant_field, w, h):
        """the two maps as contiguous uint8 (bys, bxs) arrays (quant_field may be None)"""
        shp = ((h + 7) // 8, (w + 7) // 8)
        maps = []
        for name, m in (("strategy", strategy), ("quant_field", quant_field)):
            if m is None:
                maps.append(None)
                continue
            m = np.ascontiguousarray(m, dtype=np.uint8)
            if m.shape != shp:
                raise ValueError("%s must be uint8 %r for a %d x %d frame, got %r"
                                 % (name, shp, w, h, m.shape))
            maps.append(m)
        return maps

    def encode_forced(self, rgb: np.ndarray, strategy: np.ndarray,
                      quant_field: "np.ndarray | None" = None) -> bytes:
        """Host (H, W, 3) uint8 -> codestream bytes with the caller's AC-strategy
        map instead of the search (jxg_encode_forced_rgb8).  `strategy` is uint8
        (ysize_blocks, xsize_blocks) in the layout of ``stats()["acs"]`` (see
        :func:`make_strategy_map`), `quant_field` (optional) the same shape,
        raw - 1 per block as ``stats()["qf"]``.  The ids of FORCED_SHAPES are
        taken, those of 128 / 256 px (21 - 26) on their own grid and on a context
        of any effort.  A map the validator refuses
        raises JxgError and leaves the context as it was (:func:`check_strategy_map`
        names the block)."""
        rgb = np.ascontiguousarray(rgb, dtype=np.uint8)
        h, w, c = rgb.shape
        if c != 3:
            raise ValueError("expected (H, W, 3) uint8")
        acs, qf = self._forced_maps(strategy, quant_field, w, h)
        buf = _Buffer()
        _check(load().jxg_encode_forced_rgb8(self._ctx, rgb.ctypes.data, w, h, w * 3,
                                             acs.ctypes.data,
                                             qf.ctypes.data if qf is not None else None,
                                             ctypes.byref(buf)))
        self._last_wh = (w, h)
        return self._take(buf)

    def encode_forced_device(self, ptr: int, width: int, height: int, strategy: np.ndarray,
                             quant_field: "np.ndarray | None" = None,
                             row_stride: "int | None" = None) -> bytes:
        """:meth:`encode_forced` of a device-resident frame (the maps stay host arrays)."""
        acs, qf = self._forced_maps(strategy, quant_field, width, height)
        buf = _Buffer()
        _check(load().jxg_encode_forced_rgb8_device(
            self._ctx, ctypes.c_void_p(ptr), width, height,
            row_stride if row_stride is not None else width * 3, acs.ctypes.data,
            qf.ctypes.data if qf is not None else None, ctypes.byref(buf)))
        self._last_wh = (width, height)
        return self._take(buf)

    def encode_traced(self, rgb: np.ndarray) -> bytes:
        """:meth:`encode` that also keeps, on the device, every estimate the
        AC-strategy search compared (jxg_encode_traced_rgb8): the same bytes,
        maps, reconstruction and reports; :meth:`search_trace` fetches the
        estimates.  Effort < 5 has no search and raises JxgError."""
        rgb = np.ascontiguousarray(rgb, dtype=np.uint8)
        h, w, c = rgb.shape
        if c != 3:
            raise ValueError("expected (H, W, 3) uint8")
        buf = _Buffer()
        _check(load().jxg_encode_traced_rgb8(self._ctx, rgb.ctypes.data, w, h, w * 3,
                                             ctypes.byref(buf)))
        self._last_wh = (w, h)
        return self._take(buf)

    def encode_traced_device(self, ptr: int, width: int, height: int,
                             row_stride: "int | None" = None) -> bytes:
        """:meth:`encode_traced` of a device-resident frame."""
        buf = _Buffer()
        _check(load().jxg_encode_traced_rgb8_device(
            self._ctx, ctypes.c_void_p(ptr), width, height,
            row_stride if row_stride is not None else width * 3, ctypes.byref(buf)))
        self._last_wh = (width, height)
        return self._take(buf)

    def search_trace(self, maps: bool = True) -> dict:
        """The trace of the last :meth:`encode_traced` (jxg_search_trace): the
        summary (``blocks``, ``max_px``, ``flip``, ``hook_p``, ``merged_over``,
        ``margin``, ``margin_skipped``) and, with `maps`, the planes over the
        block grid: ``cand8_raw`` / ``cand8`` float32 (6, bys, bxs) in
        TRACE_SCAN_IDS order, ``scan8`` / ``front8`` / ``qf8`` uint8 (bys, bxs),
        ``merged`` float32 (9, bys, bxs) in TRACE_MERGED_IDS order, ``big``
        float32 (6, bys, bxs) in TRACE_BIG_IDS order, ``chosen`` float32
        (bys, bxs).  Raises JxgError unless the context's last use was a
        traced encode."""
        w, h = self._last_wh or (1, 1)
        bxs, bys = (w + 7) // 8, (h + 7) // 8
        out, m = {}, _TraceMaps()
        if maps:
            for name, planes, dt in _TRACE_PLANES:
                out[name] = np.empty((planes, bys, bxs) if planes else (bys, bxs), dt)
                setattr(m, name, out[name].ctypes.data)
        s = _TraceSummary()
        _check(load().jxg_search_trace(self._ctx, ctypes.byref(m) if maps else None,
                                       ctypes.byref(s)))
        out.update(s.as_dict())
        return out

    def reconstruct(self) -> np.ndarray:
        """(H, W, 3) uint8: the decoded image of the frame last encoded with
        :meth:`encode` / :meth:`encode_device`, reconstructed on the GPU from
        the context's coefficients (jxg_reconstruct_rgb8; no decoder run).
        Raises JxgError when the last encode was a batch, streamed or sharded
        one, or none."""
        w, h = self._last_wh or (1, 1)
        out = np.empty((h, w, 3), dtype=np.uint8)
        _check(load().jxg_reconstruct_rgb8(self._ctx, out.ctypes.data, w * 3))
        return out

    def reconstruct_device(self, ptr: int, row_stride: int | None = None) -> None:
        """The same image written to a device pointer (rows of `row_stride`
        bytes, default 3 * width; only the first 3 * width of each are
        written); returns when it is complete."""
        w, _ = self._last_wh or (1, 1)
        _check(load().jxg_reconstruct_rgb8_device(self._ctx, ctypes.c_void_p(ptr),
                                                  row_stride or w * 3))

    def strategy_report(self, orig: np.ndarray, block_map: bool = False) -> dict:
        """Per-strategy statistics of the frame last encoded with
        :meth:`encode` / :meth:`encode_device` against ``orig``, the (H, W, 3)
        uint8 image it was encoded from (jxg_strategy_report_rgb8): a dict of
        ``[27]`` uint64 arrays indexed by raw AcStrategy id -- ``varblocks``,
        ``blocks``, ``pixels``, ``nonzeros`` (``[27, 3]``: X, Y, B), ``qf_sum``,
        ``sse`` -- and ``names``.  Exact integer sums, reduced on the GPU; the
        squared error is against exactly the pixels :meth:`reconstruct`
        returns.  ``block_map=True`` adds ``block_sse``, the ``(bys, bxs)``
        uint32 squared error of every 8x8 block.  Raises JxgError where
        :meth:`reconstruct` does."""
        orig = np.ascontiguousarray(orig, dtype=np.uint8)
        w, h = self._last_wh or (1, 1)
        if orig.shape != (h, w, 3):
            raise ValueError("orig must be the (H, W, 3) uint8 image of the last encode")
        rep = _StrategyReport()
        bmap = np.empty(((h + 7) // 8, (w + 7) // 8), dtype=np.uint32) if block_map else None
        _check(load().jxg_strategy_report_rgb8(
            self._ctx, orig.ctypes.data, w * 3, ctypes.byref(rep),
            bmap.ctypes.data if block_map else None))
        out = rep.as_dict()
        if block_map:
            out["block_sse"] = bmap
        return out

    def strategy_report_device(self, ptr: int, row_stride: int | None = None,
                               block_map_ptr: int | None = None) -> dict:
        """:meth:`strategy_report` against a device-resident original (rows of
        ``row_stride`` bytes, default 3 * width); ``block_map_ptr``: device
        memory for the ``(bys, bxs)`` uint32 block map
        (jxg_strategy_report_rgb8_device)."""
        w, _ = self._last_wh or (1, 1)
        rep = _StrategyReport()
        _check(load().jxg_strategy_report_rgb8_device(
            self._ctx, ctypes.c_void_p(ptr), row_stride or w * 3, ctypes.byref(rep),
            ctypes.c_void_p(block_map_ptr) if block_map_ptr else None))
        return rep.as_dict()

    def rate_report(self, block_map: bool = False) -> dict:
        """Coded bits of the frame last encoded with :meth:`encode` /
        :meth:`encode_device`, per AC strategy (jxg_rate_report): ``tokens`` and
        ``cost`` are ``[27, 3]`` uint64 arrays (raw AcStrategy id; X, Y, B), cost
        in 1 / ``RATE_UNIT`` bit of the pass groups' AC streams as written;
        ``ac_bits`` is the exact size of those streams, ``stream_bits`` the
        codestream's, ``ans`` the coder, ``groups`` the pass groups.  Exact
        integer sums priced on the GPU from the encode's own token records and
        final code tables; needs no image.  ``block_map=True`` adds
        ``block_cost``, ``(bys, bxs)`` uint32: a varblock's cost at its first
        block, 0 at the blocks it covers.  Raises JxgError where
        :meth:`reconstruct` does."""
        w, h = self._last_wh or (1, 1)
        rep = _RateReport()
        bmap = np.empty(((h + 7) // 8, (w + 7) // 8), dtype=np.uint32) if block_map else None
        _check(load().jxg_rate_report(self._ctx, ctypes.byref(rep),
                                      bmap.ctypes.data if block_map else None))
        out = rep.as_dict()
        if block_map:
            out["block_cost"] = bmap
        return out

    def rate_report_device(self, block_map_ptr: int | None = None) -> dict:
        """:meth:`rate_report` with the ``(bys, bxs)`` uint32 block map written
        to device memory at ``block_map_ptr`` (jxg_rate_report_device)."""
        rep = _RateReport()
        _check(load().jxg_rate_report_device(
            self._ctx, ctypes.byref(rep),
            ctypes.c_void_p(block_map_ptr) if block_map_ptr else None))
        return rep.as_dict()

    def decode(self, data: bytes) -> np.ndarray:
        """Codestream bytes -> (H, W, 3) uint8, decoded on the GPU
        (jxg_decode_rgb8): any codestream this encoder writes -- one-at-a-time,
        batch, streamed or sharded.  The context's parameters play no part;
        afterwards :meth:`reconstruct` raises until the next :meth:`encode`."""
        data = bytes(data)
        info = stream_info(data)
        w, h = info["xsize"], info["ysize"]
        out = np.empty((h, w, 3), dtype=np.uint8)
        _check(load().jxg_decode_rgb8(self._ctx, data, len(data), out.ctypes.data, w * 3))
        return out

    def decode_device(self, data: bytes, ptr: int, row_stride: int | None = None) -> None:
        """The same image written to a device pointer (rows of `row_stride`
        bytes, default 3 * width); returns when it is complete."""
        data = bytes(data)
        if row_stride is None:
            row_stride = stream_info(data)["xsize"] * 3
        _check(load().jxg_decode_rgb8_device(self._ctx, data, len(data), ctypes.c_void_p(ptr),
                                             row_stride))

    def decode_timings(self) -> dict:
        """Milliseconds of the last :meth:`decode` / :meth:`decode_device`
        (jxg_decode_timings)."""
        ms = (ctypes.c_float * 5)()
        _check(load().jxg_decode_timings(self._ctx, ms))
        return dict(zip(("ms_head", "ms_lf", "ms_groups", "ms_recon", "ms_call"), map(float, ms)))

    def _decode_batch_call(self, fn, datas, ptrs, strides):
        """one jxg_decode_batch_rgb8[_device] call -> (call status, frame statuses)"""
        n = len(datas)
        sz = ctypes.c_size_t
        c_datas = (ctypes.c_char_p * n)(*[d if d else None for d in datas])
        c_sizes = (sz * n)(*[len(d) for d in datas])
        c_ptrs = (ctypes.c_void_p * n)(*ptrs)
        c_strides = (sz * n)(*strides)
        st = (ctypes.c_int * n)()
        ret = fn(self._ctx, c_datas, c_sizes, n, c_ptrs, c_strides, st)
        return ret, [int(v) for v in st]

    @staticmethod
    def _batch_call_failed(ret, st):
        """the call itself failed (as opposed to frames of it): its arguments were
        refused with no status written, or a device / memory error filled them all"""
        return ret != 0 and (not any(st) or ret not in (-1, -5))

    def decode_batch(self, datas, strict: bool = True):
        """Codestreams -> list of (H, W, 3) uint8 arrays, decoded on the GPU in
        one call (jxg_decode_batch_rgb8): the pass groups of all frames share
        the pass-group launches.  Frames may differ in size, coder, presets and
        filters; each result equals :meth:`decode` of that stream.  Raises
        JxgError on the first frame that is refused; with ``strict=False``
        returns ``(arrays, statuses)`` instead, with None for a refused frame
        and its jxg_status (0 for a decoded one).  Afterwards
        :meth:`reconstruct` raises until the next :meth:`encode`."""
        datas = [bytes(d) for d in datas]
        if not datas:
            return [] if strict else ([], [])
        outs = []
        for d in datas:
            info = _StreamInfo()
            if d and load().jxg_decode_info(d, len(d), ctypes.byref(info)) == 0:
                outs.append(np.empty((info.ysize, info.xsize, 3), dtype=np.uint8))
            else:  # the call refuses the stream as well, with the frame's status
                outs.append(np.empty((1, 1, 3), dtype=np.uint8))
        ret, st = self._decode_batch_call(load().jxg_decode_batch_rgb8, datas,
                                          [o.ctypes.data for o in outs],
                                          [o.shape[1] * 3 for o in outs])
        if strict or self._batch_call_failed(ret, st):
            _check(ret)
        if strict:
            return outs
        return [o if s == 0 else None for o, s in zip(outs, st)], st

    def decode_batch_device(self, datas, ptrs, row_strides=None) -> list:
        """The same images written to device pointers (rows of row_strides[i]
        bytes, default 3 * width); returns the frames' statuses when the images
        are complete (jxg_decode_batch_rgb8_device)."""
        datas = [bytes(d) for d in datas]
        if row_strides is None:
            row_strides = [stream_info(d)["xsize"] * 3 for d in datas]
        ret, st = self._decode_batch_call(load().jxg_decode_batch_rgb8_device, datas, list(ptrs),
                                          list(row_strides))
        if self._batch_call_failed(ret, st):
            _check(ret)
        return st

    def decode_batch_timings(self) -> dict:
        """Counts and milliseconds of the last :meth:`decode_batch`
        (jxg_decode_batch_timings): frames, chunks, work items launched with
        their tables staged in LDS / not, host parse, pass-group launches and
        reconstruction chains (device time by events), the whole call."""
        s = _DecodeBatchStats()
        _check(load().jxg_decode_batch_timings(self._ctx, ctypes.byref(s)))
        return {k: (int if t is ctypes.c_uint32 else float)(getattr(s, k))
                for k, t in _DecodeBatchStats._fields_}

    def set_decode_batch_bytes(self, nbytes: int = 0) -> None:
        """Device-memory budget of one chunk of :meth:`decode_batch`
        (jxg_set_decode_batch_bytes); 0: the default, 2 GiB."""
        _check(load().jxg_set_decode_batch_bytes(self._ctx, nbytes))

    def encode_batch(self, frames) -> list:
        """Host frames of equal size, each (H, W, 3) uint8 -> list of codestream
        bytes (jxg_encode_batch_rgb8, BASELINE config 3)."""
        frames = [np.ascontiguousarray(f, dtype=np.uint8) for f in frames]
        if not frames:
            return []
        h, w, c = frames[0].shape
        if c != 3 or any(f.shape != frames[0].shape for f in frames):
            raise ValueError("expected equal-size (H, W, 3) uint8 frames")
        n = len(frames)
        ptrs = (ctypes.c_void_p * n)(*[f.ctypes.data for f in frames])
        outs = (_Buffer * n)()
        _check(load().jxg_encode_batch_rgb8(self._ctx, ptrs, n, w, h, w * 3, outs))
        return [self._take(outs[i]) for i in range(n)]

    def encode_batch_device(self, ptrs, width: int, height: int, row_stride: int | None = None,
                            copy: bool = True) -> list:
        """Device-resident frames of equal size (pointers) -> list of
        codestreams (jxg_encode_batch_rgb8_device); copy=False returns
        :class:`Codestream` views of the library's pinned buffers."""
        n = len(ptrs)
        if n == 0:
            return []
        arr = (ctypes.c_void_p * n)(*ptrs)
        outs = (_Buffer * n)()
        _check(load().jxg_encode_batch_rgb8_device(self._ctx, arr, n, width, height,
                                                   row_stride or width * 3, outs))
        return [self._take(outs[i]) if copy else Codestream(outs[i]) for i in range(n)]

    def encode_device(self, ptr: int, width: int, height: int, row_stride: int | None = None,
                      copy: bool = True):
        """Device-resident RGB8 (e.g. ``tensor.data_ptr()`` of a uint8 CUDA tensor).

        copy=False returns a :class:`Codestream` that owns the library's
        (pinned) output buffer instead of copying it into ``bytes``."""
        buf = _Buffer()
        _check(load().jxg_encode_rgb8_device(self._ctx, ctypes.c_void_p(ptr), width, height,
                                             row_stride or width * 3, ctypes.byref(buf)))
        self._last_wh = (width, height)
        return self._take(buf) if copy else Codestream(buf)

    # ---- sweep: one image over many settings (jxg_sweep_rgb8) ----
    # "msssim": a quality-2 sweep with jxg_set_sweep_msssim on for its duration
    _QUALITY = {None: 0, "none": 0, "psnr": 1, "ssim": 2, "msssim": 2, 0: 0, 1: 1, 2: 2}

    @staticmethod
    def _sweep_points(points):
        pts = []
        for p in points:
            if isinstance(p, dict):
                pts.append(_SweepPoint(p["distance"], p["effort"], p.get("proposals", 0),
                                       p.get("flags", 0)))
            else:
                p = tuple(p)
                pts.append(_SweepPoint(p[0], p[1], *(tuple(p[2:4]) + (0, 0))[:2]))
        return pts

    # a sweep's riders, one row each: the keyword's name, its setter (called with
    # the keyword's value to switch it on, with `off` in the end), its getter, the
    # result type, and how a point's result enters its dict
    _RIDERS = (
        ("msssim", "jxg_set_sweep_msssim", (0,), "jxg_sweep_msssim", _Msssim,
         lambda r: {"ms_ssim": float(r.ms_ssim), "cs": [float(v) for v in r.cs]}),
        ("strategies", "jxg_set_sweep_report", (0,), "jxg_sweep_report", _StrategyReport,
         lambda r: {"strategies": r.as_dict()}),
        ("ab", "jxg_set_sweep_ab", (None, 0), "jxg_sweep_ab", _AbReport,
         lambda r: {"ab": r.as_dict()}),
        ("rates", "jxg_set_sweep_rates", (0,), "jxg_sweep_rates", _RateReport,
         lambda r: {"rates": r.as_dict()}),
        ("trace", "jxg_set_sweep_trace", (0,), "jxg_sweep_trace", _TraceSummary,
         lambda r: {"trace": r.as_dict()}),
    )

    def _sweep_call(self, fn, ptr, w, h, stride, points, quality, strict, strategies=False,
                    rates=False, ab=None, trace=False):
        if quality not in self._QUALITY:
            raise ValueError("quality: 'msssim', 'ssim', 'psnr' or None")
        level = self._QUALITY[quality]
        if strategies and not level:
            raise ValueError("strategies ride on a sweep's quality chain: quality must not be None")
        pts = self._sweep_points(points)
        n = len(pts)
        if ab is not None:
            ab = [int(v) for v in ab]
            if not level:
                raise ValueError("ab rides on a sweep's quality chain: quality must not be None")
            if len(ab) != n:
                raise ValueError("ab: one base index per point")
            if any(v < -1 or v >= i for i, v in enumerate(ab)):
                raise ValueError("ab: a base index is -1 or that of an earlier point")
        if n == 0:
            return []
        # the setters' arguments of the riders that are asked for
        on = {"msssim": (1,) if quality == "msssim" else None,
              "strategies": (1,) if strategies else None,
              "rates": (1,) if rates else None,
              "trace": (1,) if trace else None,
              "ab": ((ctypes.c_int32 * n)(*ab), n) if ab is not None else None}
        riders = [r for r in self._RIDERS if on[r[0]] is not None]
        c_pts = (_SweepPoint * n)(*pts)
        outs = (_Buffer * n)()
        qs = (_Quality * n)() if level else None
        st = (ctypes.c_int * n)()
        got = {}  # by keyword: the results of a sweep that has them (a failed one has none)
        lib = load()
        try:
            for name, setter, _, _, _, _ in riders:
                _check(getattr(lib, setter)(self._ctx, *on[name]))
            ret = fn(self._ctx, ptr, w, h, stride, c_pts, n, level, outs, qs, st)
            for name, _, _, getter, ctype, _ in riders:
                r = (ctype * n)()
                if getattr(lib, getter)(self._ctx, r, n) == 0:
                    got[name] = r
        finally:
            for _, setter, off, _, _, _ in riders:
                getattr(lib, setter)(self._ctx, *off)
        st = [int(v) for v in st]
        if ret != 0 and (strict or self._batch_call_failed(ret, st)):
            for i in range(n):
                lib.jxg_buffer_free(ctypes.byref(outs[i]))
            _check(ret)
        res = []
        for i in range(n):
            if st[i] != 0:
                res.append((None, st[i]))
                continue
            q = None
            if level:
                q = {k: getattr(qs[i], k) for k in ("sse", "samples", "mse", "psnr", "ssim")}
            for name, _, _, _, _, put in riders:
                # (quality None: rates and trace alone, the others were refused above)
                if name in got and (name != "ab" or ab[i] >= 0):
                    q = dict(q or {}, **put(got[name][i]))
            res.append((self._take(outs[i]), q))
        return res

    def sweep(self, rgb: np.ndarray, points, quality="ssim", strict: bool = True,
              strategies: bool = False, rates: bool = False, ab=None,
              trace: bool = False) -> list:
        """One host (H, W, 3) uint8 image encoded at every point of ``points``
        in one call (jxg_sweep_rgb8): the image is uploaded once and the points
        run through the streaming pipeline's lanes of this context, whose own
        distance / effort / proposals / flags play no part.  A point is a dict
        with ``distance``, ``effort`` and optionally ``proposals`` / ``flags``
        (the keywords of :class:`Encoder`), or a tuple in that order.
        ``quality``: ``"ssim"`` (sse, mse, psnr and ssim of each point's
        decoded image against ``rgb``), ``"msssim"`` (the same plus ``ms_ssim``
        and the per-scale ``cs`` of :meth:`msssim`, computed on the point's
        lane), ``"psnr"`` (the decoded image is never written; ssim NaN) or
        ``None``.  Returns ``[(bytes, dict | None), ...]``
        in point order, each equal to a fresh ``Encoder(**point)``'s
        ``encode`` / ``reconstruct_device`` / ``compare_device``.  Raises
        JxgError on the first refused point; with ``strict=False`` a refused
        point comes back as ``(None, status)``.  ``strategies=True`` (not with
        ``quality=None``): each point's dict gains ``"strategies"``, the
        :meth:`strategy_report` of that point, reduced on its lane
        (jxg_set_sweep_report).  ``rates=True``: each point's dict gains
        ``"rates"``, the :meth:`rate_report` of that point, priced on its lane
        after its emission (jxg_set_sweep_rates); with ``quality=None`` the dict
        holds only that.  ``ab=[base indices]`` (one per point, -1 or the index
        of an earlier point; not with ``quality=None``): the dict of every point
        with a base >= 0 gains ``"ab"``, the :func:`ab_report` of the base point
        (side A) and this point (side B), reduced on its lane against a snapshot
        of the base point's maps (jxg_set_sweep_ab; all zero where the base
        point was refused).  ``trace=True`` (allowed with ``quality=None``):
        each point's dict gains ``"trace"``, the summary of
        :meth:`search_trace` after :meth:`encode_traced` with that point,
        reduced on its lane (jxg_set_sweep_trace); a point of effort < 5 has no
        search and gets the all-zero summary (``blocks == 0``); the planes are
        not kept.  Afterwards :meth:`reconstruct` and :meth:`search_trace`
        raise until the next :meth:`encode` / :meth:`encode_traced`."""
        rgb = np.ascontiguousarray(rgb, dtype=np.uint8)
        if rgb.ndim != 3 or rgb.shape[2] != 3:
            raise ValueError("expected (H, W, 3) uint8")
        h, w = rgb.shape[:2]
        return self._sweep_call(load().jxg_sweep_rgb8, rgb.ctypes.data, w, h, w * 3, points,
                                quality, strict, strategies, rates, ab, trace)

    def sweep_device(self, ptr: int, width: int, height: int, points, quality="ssim",
                     strict: bool = True, row_stride: int | None = None,
                     strategies: bool = False, rates: bool = False, ab=None,
                     trace: bool = False) -> list:
        """:meth:`sweep` of a device-resident RGB8 image (rows of ``row_stride``
        bytes, default 3 * width), which must stay unchanged until the call
        returns (jxg_sweep_rgb8_device)."""
        return self._sweep_call(load().jxg_sweep_rgb8_device, ctypes.c_void_p(ptr), width, height,
                                row_stride or width * 3, points, quality, strict, strategies,
                                rates, ab, trace)

    def sweep_timings(self) -> dict:
        """The last :meth:`sweep` (jxg_sweep_timings): points encoded, lanes,
        the call's host wall time, the upload, and device time by events summed
        over the points -- encode, reconstruction chain, metrics."""
        s = _SweepStats()
        _check(load().jxg_sweep_timings(self._ctx, ctypes.byref(s)))
        return {k: (int if t is ctypes.c_uint32 else float)(getattr(s, k))
                for k, t in _SweepStats._fields_}

    # streaming encode (jxg_submit_rgb8[_device] / jxg_receive): a software
    # pipeline inside the library, driven by this thread
    def submit(self, rgb: np.ndarray):
        """Queue a host (H, W, 3) uint8 frame (copied before returning)."""
        rgb = np.ascontiguousarray(rgb, dtype=np.uint8)
        h, w, c = rgb.shape
        if c != 3:
            raise ValueError("expected (H, W, 3) uint8")
        _check(load().jxg_submit_rgb8(self._ctx, rgb.ctypes.data, w, h, w * 3))

    def submit_device(self, ptr: int, width: int, height: int, row_stride: int | None = None):
        """Queue a device-resident RGB8 frame; it must stay unchanged until its
        codestream has been received."""
        _check(load().jxg_submit_rgb8_device(self._ctx, ctypes.c_void_p(ptr), width, height,
                                             row_stride or width * 3))

    def receive(self, copy: bool = True):
        """Codestream of the oldest submitted frame (blocks until complete)."""
        buf = _Buffer()
        _check(load().jxg_receive(self._ctx, ctypes.byref(buf)))
        return self._take(buf) if copy else Codestream(buf)

    def pending(self) -> int:
        n = ctypes.c_uint32()
        _check(load().jxg_pending(self._ctx, ctypes.byref(n)))
        return n.value

    def pipeline_depth(self, width: int, height: int, rank: int = 0, world: int = 1) -> int:
        """Lanes of the streaming pipeline for these frames (or this rank's shard)."""
        n = ctypes.c_uint32()
        _check(load().jxg_pipeline_depth(self._ctx, width, height, rank, world, ctypes.byref(n)))
        return n.value

    def set_pipeline_lanes(self, lanes: int) -> None:
        """Cap this context's pipeline lanes (0: default) -- several contexts
        streaming on one GPU share its hardware queues (include/jxg.h)."""
        _check(load().jxg_set_pipeline_lanes(self._ctx, lanes))

    def set_input_stream(self, stream) -> None:
        """Order every later device-input call after the work submitted so far
        to `stream` (a hipStream_t handle, e.g. ``torch.cuda.current_stream()
        .cuda_stream``; None: the caller's writes are complete before each
        call) -- include/jxg.h."""
        _check(load().jxg_set_input_stream(self._ctx, ctypes.c_void_p(stream or None)))

    # streaming sharded encode (jxg_shard_submit_device / jxg_shard_next_head /
    # jxg_shard_write_next): see jxg.dist.ShardStream
    def shard_submit_device(self, ptr: int, width: int, height: int, rank: int, world: int,
                            row_stride: int | None = None):
        _check(load().jxg_shard_submit_device(self._ctx, ctypes.c_void_p(ptr), width, height,
                                              row_stride or width * 3, rank, world))

    def shard_next_head(self) -> np.ndarray:
        """Payload head of the oldest pending shard frame (waits for its sections)."""
        n = ctypes.c_size_t(0)
        _check(load().jxg_shard_next_head(self._ctx, None, ctypes.byref(n)))
        out = np.zeros(n.value, dtype=np.uint32)
        _check(load().jxg_shard_next_head(self._ctx, out.ctypes.data, ctypes.byref(n)))
        return out

    def shard_write_next(self, heads, dst_ptr: int, dst_size: int):
        """jxg_shard_write_host for the oldest pending shard frame, which is then
        released; returns (ok, total) -- ok False when dst_size < total (the
        frame stays pending, nothing written).  The copies are enqueued: the
        PREVIOUS frame's are complete on return (:meth:`shard_write_flush`:
        the last one's)."""
        return self._write(load().jxg_shard_write_next, heads, dst_ptr, dst_size)

    def shard_write_flush(self):
        """Wait for the last shard_write_next's copies."""
        _check(load().jxg_shard_write_flush(self._ctx))

    def timings(self) -> tuple:
        """(ms_front_kernel, ms_host_call, ms_host_codes, ms_host_layout, ms_aq)
        of the last encode -- the per-frame subset of :meth:`stats` without its
        copies."""
        s = _Stats()
        _check(load().jxg_get_stats(self._ctx, ctypes.byref(s)))
        return s.ms_front_kernel, s.ms_host_call, s.ms_host_codes, s.ms_host_layout, s.ms_aq

    def stats(self) -> dict:
        s = _Stats()
        _check(load().jxg_get_stats(self._ctx, ctypes.byref(s)))
        nb = s.xsize_blocks * s.ysize_blocks
        out = {k: getattr(s, k) for k in ("xsize", "ysize", "xsize_blocks", "ysize_blocks",
                                          "num_groups", "num_lf_groups", "global_scale",
                                          "quant_dc", "bytes", "ms_front", "ms_histogram",
                                          "ms_emit", "ms_assemble", "ms_total",
                                          "ms_host_call", "ms_host_codes",
                                          "ms_host_layout", "ms_front_kernel", "ms_aq")}
        if s.ac_tokens:
            out["ac_tokens"] = np.ctypeslib.as_array(s.ac_tokens, (s.num_groups * 3,)).reshape(-1, 3).copy()
        if s.ac_strategy:
            shp = (s.ysize_blocks, s.xsize_blocks)
            out["acs"] = np.ctypeslib.as_array(s.ac_strategy, (nb,)).reshape(shp).copy()
            out["qf"] = np.ctypeslib.as_array(s.quant_field, (nb,)).reshape(shp).copy()
            out["dc"] = np.ctypeslib.as_array(s.dc, (3 * nb,)).reshape((3,) + shp).copy()
            out["ac"] = np.ctypeslib.as_array(s.ac, (nb * 192,)).reshape(shp + (3, 64)).copy()
            if s.homogeneity:
                out["homog"] = np.ctypeslib.as_array(s.homogeneity, (nb * 3,)).reshape(shp + (3,)).copy()
        return out

    # ---- sharded encode (one context per rank; see jxg.dist) ----
    def shard_begin(self, ptr: int, width: int, height: int, rank: int, world: int,
                    d_hist: int, d_xbuf: int, row_stride: int | None = None):
        """Front end + merge + AC statistics of this rank's pass groups;
        d_hist / d_xbuf are device pointers (sizes: :func:`shard_sizes`)."""
        _check(load().jxg_shard_begin(self._ctx, ctypes.c_void_p(ptr), width, height,
                                      row_stride or width * 3, rank, world,
                                      ctypes.c_void_p(d_hist), ctypes.c_void_p(d_xbuf)))

    def shard_end(self, d_hist: int, d_xbuf: int) -> int:
        """After all-reduce(d_hist) and all-gather(d_xbuf): emit this rank's
        sections; returns the payload size (kept on the device, see
        :meth:`shard_payload`)."""
        n = ctypes.c_size_t()
        _check(load().jxg_shard_end(self._ctx, ctypes.c_void_p(d_hist), ctypes.c_void_p(d_xbuf),
                                    ctypes.byref(n)))
        return n.value

    def shard_payload(self, dst: int, on_device: bool = True):
        """Copy the last payload to `dst` (device or host pointer)."""
        _check(load().jxg_shard_payload(self._ctx, ctypes.c_void_p(dst), 1 if on_device else 0))

    def shard_payload_bytes(self, size: int) -> bytes:
        buf = (ctypes.c_uint8 * size)()
        self.shard_payload(ctypes.addressof(buf), on_device=False)
        return bytes(buf)

    def shard_assemble_device(self, d_base: int, offsets, sizes, copy: bool = True):
        """Payloads gathered in device memory (d_base + offsets[i]) -> codestream."""
        n = len(sizes)
        offs = (ctypes.c_size_t * n)(*offsets)
        szs = (ctypes.c_size_t * n)(*sizes)
        buf = _Buffer()
        _check(load().jxg_shard_assemble_device(self._ctx, ctypes.c_void_p(d_base), offs, szs, n,
                                                ctypes.byref(buf)))
        return self._take(buf) if copy else Codestream(buf)

    def shard_head(self) -> np.ndarray:
        """This rank's payload head (u32 words) after shard_end."""
        n = ctypes.c_size_t(0)
        _check(load().jxg_shard_head(self._ctx, None, ctypes.byref(n)))
        out = np.zeros(n.value, dtype=np.uint32)
        _check(load().jxg_shard_head(self._ctx, out.ctypes.data, ctypes.byref(n)))
        return out

    def shard_write_host(self, heads, dst_ptr: int, dst_size: int):
        """Write this rank's sections (and, on rank 0, headers + TOC) into the
        shared host buffer at dst_ptr; returns (ok, total codestream bytes) --
        ok False when dst_size < total (nothing written)."""
        return self._write(load().jxg_shard_write_host, heads, dst_ptr, dst_size)

    def _write(self, fn, heads, dst_ptr: int, dst_size: int):
        heads = [np.ascontiguousarray(h, dtype=np.uint32) for h in heads]
        n = len(heads)
        ptrs = (ctypes.c_void_p * n)(*[h.ctypes.data for h in heads])
        words = (ctypes.c_size_t * n)(*[h.size for h in heads])
        total = ctypes.c_size_t(0)
        st = fn(self._ctx, ptrs, words, n, ctypes.c_void_p(dst_ptr), dst_size, ctypes.byref(total))
        if st == -1 and total.value > dst_size:
            return False, total.value
        _check(st)
        return True, total.value

    def homogeneity_map(self, xyb: np.ndarray, distance: float, flags: int = 0):
        """Thesis selector over a (3, H, W) float32 XYB frame (H, W multiples of 8)."""
        xyb = np.ascontiguousarray(xyb, dtype=np.float32)
        _, ys, xs = xyb.shape
        r3 = np.zeros((ys // 8, xs // 8, 3), dtype=np.float32)
        t = np.zeros((ys // 8, xs // 8), dtype=np.uint8)
        _check(load().jxg_homogeneity_map(self._ctx, xyb.ctypes.data, xs, ys, distance, flags,
                                          r3.ctypes.data, t.ctypes.data))
        return r3, t

    def warmup(self, width: int, height: int):
        """jxg_warmup: allocate this context's buffers for width x height and
        load every kernel (one synthetic frame, result discarded)."""
        _check(load().jxg_warmup(self._ctx, width, height))

    def synth_device(self, ptr: int, width: int, height: int, seed: int,
                     row_stride: int | None = None):
        """Fill device memory with the benchmark's synthetic RGB8 frame
        (jxg.synth.synth_rgb8 bytes) on this context's stream."""
        _check(load().jxg_synth_rgb8_device(self._ctx, ctypes.c_void_p(ptr), width, height,
                                            row_stride or width * 3,
                                            seed & 0xFFFFFFFFFFFFFFFF))

    def compare(self, orig: np.ndarray, comp: np.ndarray, ssim: bool = True) -> dict:
        """Decode-side quality on the GPU (jxg_compare_rgb8): orig / comp are
        (H, W, 3) uint8 (comp = the decoded image).  Returns sse, samples, mse,
        psnr (image_reader.rs:555-606) and ssim (metrics.rs:55-84 counterpart)."""
        o = np.asarray(orig)
        c = np.asarray(comp)
        if o.shape != c.shape or o.ndim != 3 or o.shape[2] != 3:
            raise ValueError("orig / comp must both be (H, W, 3) uint8")
        o = np.ascontiguousarray(o, dtype=np.uint8)
        c = np.ascontiguousarray(c, dtype=np.uint8)
        h, w = o.shape[:2]
        q = _Quality()
        _check(load().jxg_compare_rgb8(self._ctx, o.ctypes.data, w * 3, c.ctypes.data, w * 3, w, h,
                                       1 if ssim else 0, ctypes.byref(q)))
        return {"sse": q.sse, "samples": q.samples, "mse": q.mse, "psnr": q.psnr, "ssim": q.ssim}

    def compare_device(self, d_orig: int, d_comp: int, width: int, height: int,
                       orig_stride: int | None = None, comp_stride: int | None = None,
                       ssim: bool = True) -> dict:
        """Same on device-resident RGB8 (e.g. torch tensors' data_ptr())."""
        q = _Quality()
        _check(load().jxg_compare_rgb8_device(
            self._ctx, ctypes.c_void_p(d_orig), orig_stride or width * 3, ctypes.c_void_p(d_comp),
            comp_stride or width * 3, width, height, 1 if ssim else 0, ctypes.byref(q)))
        return {"sse": q.sse, "samples": q.samples, "mse": q.mse, "psnr": q.psnr, "ssim": q.ssim}

    def msssim(self, orig: np.ndarray, comp: np.ndarray) -> dict:
        """MS-SSIM on the GPU (jxg_msssim_rgb8; Wang, Simoncelli, Bovik 2003):
        orig / comp are (H, W, 3) uint8.  Returns ``ms_ssim`` and the per-scale
        means ``cs[5]`` / ``ssim[5]`` (``ssim[0]`` is :meth:`compare`'s ssim);
        every field is NaN when min(H, W) < 176."""
        o = np.asarray(orig)
        c = np.asarray(comp)
        if o.shape != c.shape or o.ndim != 3 or o.shape[2] != 3:
            raise ValueError("orig / comp must both be (H, W, 3) uint8")
        o = np.ascontiguousarray(o, dtype=np.uint8)
        c = np.ascontiguousarray(c, dtype=np.uint8)
        h, w = o.shape[:2]
        m = _Msssim()
        _check(load().jxg_msssim_rgb8(self._ctx, o.ctypes.data, w * 3, c.ctypes.data, w * 3, w, h,
                                      ctypes.byref(m)))
        return m.as_dict()

    def msssim_device(self, d_orig: int, d_comp: int, width: int, height: int,
                      orig_stride: int | None = None, comp_stride: int | None = None) -> dict:
        """Same on device-resident RGB8 (jxg_msssim_rgb8_device)."""
        m = _Msssim()
        _check(load().jxg_msssim_rgb8_device(
            self._ctx, ctypes.c_void_p(d_orig), orig_stride or width * 3, ctypes.c_void_p(d_comp),
            comp_stride or width * 3, width, height, ctypes.byref(m)))
        return m.as_dict()


# ---------------------------------------------------------------------------
# A/B report of two encodes (jxg_ab_report_rgb8)
# ---------------------------------------------------------------------------
def ab_report(enc_a: Encoder, enc_b: Encoder, orig: np.ndarray, block_delta: bool = False) -> dict:
    """Strategy transitions between two encodes of ``orig``, the (H, W, 3) uint8
    image both encoders encoded last with :meth:`Encoder.encode` /
    :meth:`Encoder.encode_device` (jxg_ab_report_rgb8): a dict of ``[27, 27]``
    uint64 arrays indexed ``[from, to]`` by the raw AcStrategy id a block's
    varblock has in A and in B -- ``blocks``, ``pixels``, ``sse_a``, ``sse_b``
    (the blocks' words of :meth:`Encoder.strategy_report`'s ``block_sse``),
    ``cost_a``, ``cost_b`` (the blocks' shares of their varblocks' coded cost,
    1 / ``RATE_UNIT`` bit: a varblock of cost C over n blocks gives block k, in
    raster order, ``C // n + (k < C % n)``) -- and ``names``.  Exact integer
    sums, reduced on the GPU.  ``block_delta=True`` adds ``block_delta``,
    ``(2, bys, bxs)`` int32: ``sse_b - sse_a`` and ``cost_b - cost_a`` per
    block.  ``enc_a is enc_b`` gives a diagonal table.  Raises JxgError where
    :meth:`Encoder.reconstruct` does on either encoder, and for encodes of
    different sizes."""
    orig = np.ascontiguousarray(orig, dtype=np.uint8)
    w, h = enc_a._last_wh or (1, 1)
    if orig.shape != (h, w, 3):
        raise ValueError("orig must be the (H, W, 3) uint8 image of the last encodes")
    rep = _AbReport()
    dmap = np.empty((2, (h + 7) // 8, (w + 7) // 8), dtype=np.int32) if block_delta else None
    _check(load().jxg_ab_report_rgb8(enc_a._ctx, enc_b._ctx, orig.ctypes.data, w * 3,
                                     ctypes.byref(rep), dmap.ctypes.data if block_delta else None))
    out = rep.as_dict()
    if block_delta:
        out["block_delta"] = dmap
    return out


def ab_report_device(enc_a: Encoder, enc_b: Encoder, ptr: int, row_stride: int | None = None,
                     block_delta_ptr: int | None = None) -> dict:
    """:func:`ab_report` against a device-resident original (rows of
    ``row_stride`` bytes, default 3 * width); ``block_delta_ptr``: device memory
    for the ``(2, bys, bxs)`` int32 planes (jxg_ab_report_rgb8_device)."""
    w, _ = enc_a._last_wh or (1, 1)
    rep = _AbReport()
    _check(load().jxg_ab_report_rgb8_device(
        enc_a._ctx, enc_b._ctx, ctypes.c_void_p(ptr), row_stride or w * 3, ctypes.byref(rep),
        ctypes.c_void_p(block_delta_ptr) if block_delta_ptr else None))
    return rep.as_dict()


# ---------------------------------------------------------------------------
# forced encode (Encoder.encode_forced): maps and their validator (host side)
# ---------------------------------------------------------------------------
# the ids a strategy map may hold at a varblock's first block -> (blocks down,
# blocks across)
FORCED_SHAPES = {0: (1, 1), 1: (1, 1), 2: (1, 1), 3: (1, 1), 12: (1, 1), 13: (1, 1),
                 6: (2, 1), 7: (1, 2), 4: (2, 2), 10: (4, 2), 11: (2, 4), 5: (4, 4),
                 19: (8, 4), 20: (4, 8), 18: (8, 8),
                 # the kinds of 128 / 256 px: accepted on their own grid alone (block row a
                 # multiple of the blocks down, block column of the blocks across)
                 22: (16, 8), 23: (8, 16), 21: (16, 16), 25: (32, 16), 26: (16, 32), 24: (32, 32)}


def check_strategy_map(strategy: np.ndarray, xsize: int, ysize: int):
    """jxg_check_strategy_map (host only): (status, bad_block) -- status 0 when
    :meth:`Encoder.encode_forced` accepts the map for an xsize x ysize frame,
    else the jxg_status it would return and the raster index of the first
    offending block.  A map of another shape than (ysize_blocks, xsize_blocks)
    raises ValueError."""
    acs = np.ascontiguousarray(strategy, dtype=np.uint8)
    if xsize > 0 and ysize > 0 and acs.shape != ((ysize + 7) // 8, (xsize + 7) // 8):
        raise ValueError("strategy must be uint8 (%d, %d), got %r"
                         % ((ysize + 7) // 8, (xsize + 7) // 8, acs.shape))
    bad = ctypes.c_uint32(0)
    st = load().jxg_check_strategy_map(acs.ctypes.data, xsize, ysize, ctypes.byref(bad))
    return int(st), int(bad.value)


def make_strategy_map(bys: int, bxs: int, varblocks=(), fill: int = 0) -> np.ndarray:
    """uint8 (bys, bxs) strategy map for :meth:`Encoder.encode_forced`: every
    (id, block row, block column) of `varblocks` gets its first block's id and
    0x80 | id on the other blocks it covers, every block left over is the
    8x8-class id `fill`.  Raises ValueError for an id outside FORCED_SHAPES, a
    varblock reaching past the map, or overlap (the tile rule of the shapes up
    to 64 px and the own-grid rule of ids 21 - 26 are
    :func:`check_strategy_map`'s to judge: a big id placed off its grid is made
    here and refused there)."""
    if fill not in FORCED_SHAPES or FORCED_SHAPES[fill] != (1, 1):
        raise ValueError("fill must be an 8x8-class id, got %r" % (fill,))
    acs = np.full((bys, bxs), fill, np.uint8)
    used = np.zeros((bys, bxs), bool)
    for t, by, bx in varblocks:
        if t not in FORCED_SHAPES:
            raise ValueError("id %r is not one a forced encode accepts" % (t,))
        cy, cx = FORCED_SHAPES[t]
        if by < 0 or bx < 0 or by + cy > bys or bx + cx > bxs:
            raise ValueError("varblock %r reaches past the map" % ((t, by, bx),))
        if used[by:by + cy, bx:bx + cx].any():
            raise ValueError("varblock %r overlaps another" % ((t, by, bx),))
        used[by:by + cy, bx:bx + cx] = True
        acs[by:by + cy, bx:bx + cx] = t | 0x80
        acs[by, bx] = t
    return acs


# ---------------------------------------------------------------------------
# decoder (host side: no device needed without an encoder)
# ---------------------------------------------------------------------------
def stream_info(data: bytes) -> dict:
    """jxg_decode_info: size, group counts, scales, HF presets, coder (ans 1 /
    prefix codes 0) and loop filters of a codestream; host only."""
    data = bytes(data)
    info = _StreamInfo()
    _check(load().jxg_decode_info(data, len(data), ctypes.byref(info)))
    return {k: int(getattr(info, k)) for k, _ in _StreamInfo._fields_}


def decode_maps(data: bytes, encoder: "Encoder | None" = None) -> dict:
    """jxg_decode_maps: the decoded maps shaped like :meth:`Encoder.stats` --
    acs and qf (H/8, W/8), dc (3, H/8, W/8), ac (H/8, W/8, 3, 64), cmap
    (2, tiles down, tiles across).  Without an encoder everything is decoded
    on the host; with one, the pass groups are decoded on its GPU."""
    data = bytes(data)
    info = stream_info(data)
    bxs, bys = (info["xsize"] + 7) // 8, (info["ysize"] + 7) // 8
    out = {"acs": np.zeros((bys, bxs), np.uint8), "qf": np.zeros((bys, bxs), np.uint8),
           "dc": np.zeros((3, bys, bxs), np.int32), "ac": np.zeros((bys, bxs, 3, 64), np.int32),
           "cmap": np.zeros((2, (bys + 7) // 8, (bxs + 7) // 8), np.int8)}
    ctx = encoder._ctx if encoder is not None else None
    _check(load().jxg_decode_maps(ctx, data, len(data), *[out[k].ctypes.data for k in
                                                        ("acs", "qf", "dc", "ac", "cmap")]))
    return out


# ---------------------------------------------------------------------------
# sharding helpers (host side; no device needed)
# ---------------------------------------------------------------------------
def shard_sizes(width: int, height: int, world: int):
    """(AC histogram words, record buffer bytes) of a sharded encode: the
    capacity of the send and of the receive buffer (largest of any rank)."""
    hw, sb = ctypes.c_size_t(), ctypes.c_size_t()
    _check(load().jxg_shard_sizes(width, height, world, ctypes.byref(hw), ctypes.byref(sb)))
    return hw.value, sb.value


def shard_exchange(width: int, height: int, world: int, rank: int):
    """(send bytes per peer, receive bytes per peer) of this rank's record
    exchange (an all_to_all with these splits)."""
    snd = (ctypes.c_size_t * world)()
    rcv = (ctypes.c_size_t * world)()
    _check(load().jxg_shard_exchange(width, height, world, rank, snd, rcv))
    return [int(x) for x in snd], [int(x) for x in rcv]


def shard_assemble(payloads) -> bytes:
    """Payloads of ranks 0..world-1 -> codestream (host only)."""
    n = len(payloads)
    keep = [np.frombuffer(bytes(p), dtype=np.uint8) for p in payloads]
    ptrs = (ctypes.POINTER(ctypes.c_uint8) * n)(
        *[k.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)) for k in keep])
    sizes = (ctypes.c_size_t * n)(*[k.size for k in keep])
    buf = _Buffer()
    _check(load().jxg_shard_assemble(ptrs, sizes, n, ctypes.byref(buf)))
    return Encoder._take(buf)


def group_count(width: int, height: int) -> int:
    return ((width + 255) // 256) * ((height + 255) // 256)


def lf_group_count(width: int, height: int) -> int:
    return ((width + 2047) // 2048) * ((height + 2047) // 2048)


def shard_plan(width: int, height: int, world: int):
    """The partition of a sharded encode (jxg_shard_plan; include/jxg.h):
    (owner rank of every pass group, owner rank of every LF group, kind) --
    kind 0 contiguous ranges, 1 whole LF groups per rank, 2 ranges with the
    per-block record exchange."""
    ng, nlf = group_count(width, height), lf_group_count(width, height)
    go = np.zeros(ng, dtype=np.uint32)
    lo = np.zeros(nlf, dtype=np.uint32)
    kind = ctypes.c_int(0)
    _check(load().jxg_shard_plan(width, height, world, go.ctypes.data, lo.ctypes.data,
                                 ctypes.byref(kind)))
    return go.tolist(), lo.tolist(), kind.value


def lf_owners(width: int, height: int, world: int) -> list:
    """Owner rank of every LF group in a sharded encode (jxg_shard_plan)."""
    return shard_plan(width, height, world)[1]


def shard_sections(width: int, height: int, rank: int, world: int, ans: bool = False):
    """TOC indices of the sections rank `rank` of `world` produces: LfGlobal on
    rank 0, the LF groups it owns, its pass groups (jxg_shard_plan), and on
    rank 0 HfGlobal -- except with ANS over several ranks, where HfGlobal is
    written at assembly from the ranks' HF presets (version-2 payload heads)."""
    go, lo, _ = shard_plan(width, height, world)
    nlf = len(lo)
    ids = [0] if rank == 0 else []
    ids += [1 + lg for lg in range(nlf) if lo[lg] == rank]
    if rank == 0 and not (ans and world > 1):
        ids.append(1 + nlf)
    ids += [2 + nlf + g for g in range(len(go)) if go[g] == rank]
    return ids


def make_payload(rank: int, world: int, width: int, height: int, sections) -> bytes:
    """The shard payload format of jxg_shard_host.cpp / jxg_payload.h (``JXGS`` v1) for a list of
    (TOC index, bytes) -- used by tests to feed jxg_shard_assemble."""
    head = np.array([0x5347584A, 1, rank, world, width, height, len(sections)] +
                    [v for i, b in sections for v in (i, len(b))], dtype="<u4").tobytes()
    return head + b"".join(b for _, b in sections)


# ---------------------------------------------------------------------------
# harness mirror (benchmark-jpegxl)
# ---------------------------------------------------------------------------
def _rust_plain(digits_repr: str) -> str:
    """Shortest round-trip digits (Python repr) -> Rust's exponent-free form."""
    s = digits_repr
    neg = s.startswith("-")
    if neg:
        s = s[1:]
    if "e" in s or "E" in s:
        mant, exp = s.lower().split("e")
        e = int(exp)
        if "." in mant:
            ip, fp = mant.split(".")
        else:
            ip, fp = mant, ""
        point = len(ip) + e  # position of the decimal point within ip + fp
        allds = ip + fp
        if point <= 0:
            s = "0." + "0" * (-point) + allds.lstrip("0")
        elif point >= len(allds):
            s = allds + "0" * (point - len(allds))
        else:
            s = allds[:point] + "." + allds[point:]
    if s.endswith(".0"):
        s = s[:-2]
    return ("-" if neg else "") + s


def rust_f64(v: float) -> str:
    """Rust ``format!("{}", f64)`` / ``f64::to_string``: shortest round-trip
    digits, never an exponent (1.0 -> "1", 1e-7 -> "0.0000001", 1e20 ->
    "100000000000000000000"), "NaN", "inf", "-inf"."""
    v = float(v)
    if math.isnan(v):
        return "NaN"
    if math.isinf(v):
        return "inf" if v > 0 else "-inf"
    if v == 0.0:
        return "-0" if math.copysign(1.0, v) < 0 else "0"
    return _rust_plain(repr(v))


def rust_f32(v: float) -> str:
    """Rust ``f32::to_string`` (the CSV's Distance column, csv_writer.rs:27):
    the shortest digits that round-trip through f32."""
    f = np.float32(v)
    if np.isnan(f):
        return "NaN"
    if np.isinf(f):
        return "inf" if f > 0 else "-inf"
    if f == 0:
        return "-0" if np.signbit(f) else "0"
    return _rust_plain(np.format_float_positional(f, unique=True, trim="-"))


def comp_image_name(stem: str, distance: float, effort: int) -> str:
    """benchmark.rs:644-650: ``{stem}-{distance}-{effort}.jxl``."""
    return "%s-%s-%d.jxl" % (stem, rust_f64(distance), effort)


def execute_cjxl(input_file: str, output_file: str, distance: float, effort: int,
                 proposals: str = "none", device: int = 0):
    """DockerManager::execute_cjxl (docker_manager.rs:100-137) with the GPU
    encoder in place of ``/libjxl/build/tools/cjxl``."""
    d = os.path.dirname(output_file)
    if d:
        os.makedirs(d, exist_ok=True)
    if not os.path.exists(CLI_PATH):
        raise JxgError("jxg_cjxl not built at %s" % CLI_PATH)
    args = [CLI_PATH, input_file, output_file, "--distance=%s" % rust_f64(distance),
            "--effort=%d" % effort, "--proposals=%s" % proposals, "--device=%d" % device]
    p = subprocess.run(args, capture_output=True, text=True)
    if p.returncode == 0:
        return True, p.stdout
    return False, p.stderr or p.stdout


def calculate_mse(orig: np.ndarray, comp: np.ndarray) -> float:
    """image_reader.rs:569-593: f64 sum of squared sample differences / count."""
    o = np.asarray(orig, dtype=np.float64).ravel()
    c = np.asarray(comp, dtype=np.float64).ravel()
    if o.size != c.size:
        raise ValueError("sample count mismatch")
    return float(np.sum((o - c) ** 2) / o.size)


def calculate_psnr(mse: float, max_value: float = 255.0) -> float:
    """image_reader.rs:604-606."""
    return 10.0 * math.log10((max_value * max_value) / mse) if mse > 0 else float("inf")
