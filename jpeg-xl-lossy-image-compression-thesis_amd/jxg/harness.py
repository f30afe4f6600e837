"""Harness counterpart: the benchmark-jpegxl comparison
records, their CSV files and the A/B comparison, with the GPU encoder behind
``execute_cjxl`` and the GPU quality kernels (jxg_compare_rgb8) behind the
metrics.

Mirrors pscoro/JPEG-XL-Lossy-Image-Compression-Thesis benchmark-jpegxl:

* ``ComparisonResult`` / ``ComparisonResultDiff`` -- csv_writer.rs:23-63
  (17 columns each, same order and header text, csv_writer.rs:113-142 and
  :178-196); values formatted as Rust's ``to_string`` (f32 distance, f64
  metrics, integer sizes).
* ``write_csv_header`` writes the header only to a missing or empty file
  (csv_writer.rs:113-121); ``write_csv`` appends (csv_writer.rs:82-86).
* ``compare_results`` -- JXLCompressionBenchmark::compare_results
  (benchmark.rs:727-864): sort both runs by original image name, assert the
  rows pair up, diff = run 2 - run 1 per column, summary = mean of the diffs,
  written to ``comparison_diffs.csv`` and ``summary.csv`` next to results_1.
* ``compare_to_orig`` -- JXLCompressionBenchmark::compare_to_orig
  (benchmark.rs:895-972): file-size ratios (metrics.rs:15-26), MSE / PSNR /
  SSIM on the GPU; MS-SSIM is 0.0 by default as in the reference
  (benchmark.rs:932-933 never fills it) and, with ``ms_ssim=True``, the GPU's
  jxg_msssim_rgb8 (Wang, Simoncelli, Bovik 2003; NaN under 176 pixels);
  Butteraugli and SSIMULACRA2 need libjxl's tools (Docker) and are 0.0 here.
* ``file_size_ratio`` -- metrics.rs:15-26.
* ``sweep_and_compare`` -- the per-image loop of benchmark.rs:637-677 (every
  distance x effort: encode, decode, compare) as one Encoder.sweep call.

The project's own extension (no counterpart in the reference): ``StrategyStat``
rows -- one per (image, point, non-empty AC strategy) from the GPU's strategy
report (Encoder.strategy_report) -- in ``strategy_stats.csv``,
and ``compare_strategy_stats``, their A/B difference; ``RateStat`` rows -- one
per (image, point, strategy that holds tokens) from the GPU's rate report
(Encoder.rate_report): tokens and coded bits per channel;
``AbStat`` rows -- one per (image, pair of points, non-empty cell) from the
GPU's A/B report (jxg.ab_report): the blocks that moved from
one strategy to another between two encodes, with bits and error of both.
"""
import csv
import os
from dataclasses import dataclass, fields

import numpy as np

from . import STRATEGY_NAMES, TRACE_SCAN_IDS, comp_image_name, rust_f32, rust_f64

RESULT_HEADER = [
    "Original Image Name", "Compressed Image Name", "Distance", "Effort",
    "Original File Size", "Compressed File Size", "Original Raw Size", "Compressed Raw Size",
    "File Size Ratio", "Raw Size Ratio", "MSE", "PSNR", "SSIM", "MS-SSIM", "Butteraugli",
    "Butteraugli 3-Norm", "SSIMULACRA2",
]
DIFF_HEADER = [
    "Original Image Name", "Compressed Image Name", "Distance", "Effort",
    "Diff Original File Size", "Diff Compressed File Size", "Diff Original Raw Size",
    "Diff Compressed Raw Size", "Diff File Size Ratio", "Diff Raw Size Ratio", "Diff MSE",
    "Diff PSNR", "Diff SSIM", "Diff MS-SSIM", "Diff Butteraugli", "Diff Butteraugli 3-Norm",
    "Diff SSIMULACRA2",
]


@dataclass
class ComparisonResult:
    orig_image_name: str
    comp_image_name: str
    distance: float  # f32
    effort: int
    orig_file_size: int
    comp_file_size: int
    orig_raw_size: int
    comp_raw_size: int
    comp_file_size_ratio: float
    raw_file_size_ratio: float
    mse: float
    psnr: float
    ssim: float
    ms_ssim: float
    butteraugli: float
    butteraugli_pnorm: float
    ssimulacra2: float

    def row(self):
        return [self.orig_image_name, self.comp_image_name, rust_f32(self.distance),
                str(self.effort), str(self.orig_file_size), str(self.comp_file_size),
                str(self.orig_raw_size), str(self.comp_raw_size)] + [
                    rust_f64(getattr(self, f.name)) for f in fields(self)[8:]]

    @classmethod
    def parse(cls, rec):
        """csv_writer.rs:200-226 (read_csv): f32 distance, u32 effort, u64 sizes."""
        return cls(rec[0], rec[1], float(np.float32(rec[2])), int(rec[3]), int(rec[4]),
                   int(rec[5]), int(rec[6]), int(rec[7]), *[float(v) for v in rec[8:17]])


@dataclass
class ComparisonResultDiff:
    orig_image_name: str
    comp_image_name: str
    distance: float
    effort: int
    diff_orig_file_size: float
    diff_comp_file_size: float
    diff_orig_raw_size: float
    diff_comp_raw_size: float
    diff_comp_file_size_ratio: float
    diff_raw_file_size_ratio: float
    diff_mse: float
    diff_psnr: float
    diff_ssim: float
    diff_ms_ssim: float
    diff_butteraugli: float
    diff_butteraugli_pnorm: float
    diff_ssimulacra2: float

    def row(self):
        return [self.orig_image_name, self.comp_image_name, rust_f32(self.distance),
                str(self.effort)] + [rust_f64(getattr(self, f.name)) for f in fields(self)[4:]]


def write_csv_header(file_name: str, header) -> None:
    if os.path.exists(file_name) and os.path.getsize(file_name) > 0:
        return
    parent = os.path.dirname(file_name)
    if parent:
        os.makedirs(parent, exist_ok=True)
    with open(file_name, "w", newline="") as f:
        csv.writer(f, lineterminator="\n").writerow(header)


def write_csv(records, file_name: str) -> None:
    with open(file_name, "a", newline="") as f:
        w = csv.writer(f, lineterminator="\n")
        for r in records:
            w.writerow(r.row())


def read_csv(file_name: str):
    with open(file_name, newline="") as f:
        rows = list(csv.reader(f))
    return [ComparisonResult.parse(r) for r in rows[1:] if r]


def file_size_ratio(orig: int, comp: int, denom: str) -> float:
    if (orig == 0 and denom == "orig") or (comp == 0 and denom == "comp"):
        return 0.0
    if denom == "orig":
        return float(comp) / float(orig)
    if denom == "comp":
        return float(orig) / float(comp)
    raise ValueError("Invalid denominator for file size ratio")


class _StatRow:
    """row() and parse() of a per-strategy CSV record from its dataclass fields:
    names as they are, ``distance`` as f32, the fields of ``_FLOATS`` as f64,
    every other one an integer."""
    _FLOATS = ()

    @classmethod
    def _kind(cls, f):
        if f.name == "distance":
            return rust_f32, lambda v: float(np.float32(v))
        if f.type in (str, "str"):
            return str, str
        return (rust_f64, float) if f.name in cls._FLOATS else (str, int)

    def row(self):
        return [self._kind(f)[0](getattr(self, f.name)) for f in fields(self)]

    @classmethod
    def parse(cls, rec):
        return cls(*[cls._kind(f)[1](v) for f, v in zip(fields(cls), rec)])


def _append_stats(rows, file_name: str, header) -> None:
    write_csv_header(file_name, header)
    write_csv(rows, file_name)


def _read_stats(cls, file_name: str):
    with open(file_name, newline="") as f:
        rows = list(csv.reader(f))
    return [cls.parse(r) for r in rows[1:] if r]


STRATEGY_HEADER = [
    "Original Image Name", "Compressed Image Name", "Distance", "Effort", "Strategy", "Name",
    "Varblocks", "Blocks", "Pixels", "Area Share", "Nonzeros X", "Nonzeros Y", "Nonzeros B",
    "Mean Quant Field", "SSE", "MSE",
]
STRATEGY_DIFF_HEADER = STRATEGY_HEADER[:6] + ["Diff " + h for h in STRATEGY_HEADER[6:]]


@dataclass
class StrategyStat(_StatRow):
    """One strategy of one encode: the report's row and what follows from it
    (area share = pixels / image pixels, mean quant field = qf_sum / blocks,
    MSE = SSE / (3 * pixels))."""
    orig_image_name: str
    comp_image_name: str
    distance: float  # f32
    effort: int
    strategy: int
    name: str
    varblocks: int
    blocks: int
    pixels: int
    area_share: float
    nonzeros_x: int
    nonzeros_y: int
    nonzeros_b: int
    mean_quant_field: float
    sse: int
    mse: float

    _FLOATS = ("area_share", "mean_quant_field", "mse")


@dataclass
class StrategyStatDiff:
    orig_image_name: str
    comp_image_name: str
    distance: float
    effort: int
    strategy: int
    name: str
    diffs: list  # run 2 - run 1 of the ten value columns, f64

    def row(self):
        return [self.orig_image_name, self.comp_image_name, rust_f32(self.distance),
                str(self.effort), str(self.strategy), self.name] + [rust_f64(v) for v in self.diffs]


def strategy_stats(orig_name: str, comp_name: str, distance: float, effort: int, report: dict,
                   width: int, height: int):
    """The StrategyStat rows of one report (Encoder.strategy_report / a
    sweep point's ``"strategies"``): its non-empty strategies in id order."""
    rows = []
    for i in range(len(report["blocks"])):
        blocks, pixels = int(report["blocks"][i]), int(report["pixels"][i])
        if blocks == 0:
            continue
        sse = int(report["sse"][i])
        nz = [int(v) for v in report["nonzeros"][i]]
        rows.append(StrategyStat(
            orig_name, comp_name, float(np.float32(distance)), int(effort), i,
            report["names"][i], int(report["varblocks"][i]), blocks, pixels,
            float(pixels) / (float(width) * float(height)), nz[0], nz[1], nz[2],
            float(int(report["qf_sum"][i])) / float(blocks), sse,
            float(sse) / (3.0 * float(pixels))))
    return rows


def write_strategy_stats(rows, strategy_file: str) -> None:
    _append_stats(rows, strategy_file, STRATEGY_HEADER)


def read_strategy_stats(file_name: str):
    return _read_stats(StrategyStat, file_name)


def compare_strategy_stats(file_1: str, file_2: str):
    """Run 2 - run 1 per (image, compressed name, distance, effort, strategy):
    a strategy that only one run uses counts as zeros in the other.  Writes
    ``strategy_diffs.csv`` next to file_1 and returns the rows, sorted by key."""
    value_fields = [f.name for f in fields(StrategyStat)[6:]]

    def keyed(path):
        return {(r.orig_image_name, r.comp_image_name, r.distance, r.effort, r.strategy): r
                for r in read_strategy_stats(path)}

    a, b = keyed(file_1), keyed(file_2)
    diffs = []
    for k in sorted(set(a) | set(b)):
        ra, rb = a.get(k), b.get(k)
        vals = [float(getattr(rb, n) if rb else 0) - float(getattr(ra, n) if ra else 0)
                for n in value_fields]
        diffs.append(StrategyStatDiff(k[0], k[1], k[2], k[3], k[4], (ra or rb).name, vals))
    diff_file = os.path.join(os.path.dirname(os.path.abspath(file_1)), "strategy_diffs.csv")
    write_csv_header(diff_file, STRATEGY_DIFF_HEADER)
    write_csv(diffs, diff_file)
    return diffs


RATE_HEADER = [
    "Original Image Name", "Compressed Image Name", "Distance", "Effort", "Strategy", "Name",
    "Tokens X", "Tokens Y", "Tokens B", "Bits X", "Bits Y", "Bits B", "AC Bits", "Stream Bits",
]


@dataclass
class RateStat(_StatRow):
    """One strategy of one encode in the rate report (Encoder.rate_report,
    DESIGN.md 3.17): the tokens of its varblocks per channel and what they cost
    in the written AC streams, in bits (the report's cost / 256); beside them
    the point's ``ac_bits`` and ``stream_bits``, the same on every row of it."""
    orig_image_name: str
    comp_image_name: str
    distance: float  # f32
    effort: int
    strategy: int
    name: str
    tokens_x: int
    tokens_y: int
    tokens_b: int
    bits_x: float
    bits_y: float
    bits_b: float
    ac_bits: int
    stream_bits: int

    _FLOATS = ("bits_x", "bits_y", "bits_b")


def rate_stats(orig_name: str, comp_name: str, distance: float, effort: int, report: dict):
    """The RateStat rows of one report (Encoder.rate_report / a sweep point's
    ``"rates"``): the strategies that hold tokens, in id order."""
    rows = []
    for i in range(len(report["tokens"])):
        tok = [int(v) for v in report["tokens"][i]]
        if sum(tok) == 0:
            continue
        bits = [float(int(v)) / 256.0 for v in report["cost"][i]]
        rows.append(RateStat(orig_name, comp_name, float(np.float32(distance)), int(effort), i,
                             report["names"][i], tok[0], tok[1], tok[2], bits[0], bits[1], bits[2],
                             int(report["ac_bits"]), int(report["stream_bits"])))
    return rows


def write_rate_stats(rows, rate_file: str) -> None:
    _append_stats(rows, rate_file, RATE_HEADER)


def read_rate_stats(file_name: str):
    return _read_stats(RateStat, file_name)


AB_HEADER = [
    "Original Image Name", "Compressed Image Name A", "Compressed Image Name B", "Distance",
    "Effort", "From", "From Name", "To", "To Name", "Blocks", "Pixels", "Area Share", "SSE A",
    "SSE B", "Bits A", "Bits B", "Diff SSE", "Diff Bits",
]


@dataclass
class AbStat(_StatRow):
    """One non-empty cell of an A/B report (jxg.ab_report / a sweep point's
    ``"ab"``): the 8x8 blocks whose varblock has strategy
    ``from`` in encode A and ``to`` in encode B, their squared error and their
    shares of the coded bits (the report's cost / 256) on both sides, and B - A
    of the two.  Distance and effort are B's."""
    orig_image_name: str
    comp_image_name_a: str
    comp_image_name_b: str
    distance: float  # f32
    effort: int
    from_strategy: int
    from_name: str
    to_strategy: int
    to_name: str
    blocks: int
    pixels: int
    area_share: float
    sse_a: int
    sse_b: int
    bits_a: float
    bits_b: float
    diff_sse: int
    diff_bits: float

    _FLOATS = ("area_share", "bits_a", "bits_b", "diff_bits")


def ab_stats(orig_name: str, comp_name_a: str, comp_name_b: str, distance: float, effort: int,
             report: dict, width: int, height: int):
    """The AbStat rows of one report: its non-empty cells, by from id, then to id."""
    rows = []
    names = report["names"]
    for f, t in np.argwhere(np.asarray(report["blocks"]) != 0):
        f, t = int(f), int(t)
        pixels = int(report["pixels"][f, t])
        sse_a, sse_b = int(report["sse_a"][f, t]), int(report["sse_b"][f, t])
        cost_a, cost_b = int(report["cost_a"][f, t]), int(report["cost_b"][f, t])
        rows.append(AbStat(orig_name, comp_name_a, comp_name_b, float(np.float32(distance)),
                           int(effort), f, names[f], t, names[t], int(report["blocks"][f, t]),
                           pixels, float(pixels) / (float(width) * float(height)), sse_a, sse_b,
                           float(cost_a) / 256.0, float(cost_b) / 256.0, sse_b - sse_a,
                           float(cost_b - cost_a) / 256.0))
    return rows


def write_ab_stats(rows, ab_file: str) -> None:
    _append_stats(rows, ab_file, AB_HEADER)


def read_ab_stats(file_name: str):
    return _read_stats(AbStat, file_name)


TRACE_HEADER = [
    "Original Image Name", "Compressed Image Name", "Distance", "Effort", "Scan Index", "Strategy",
    "Name", "Blocks", "Max Px", "Scan Wins", "Raw DCT8", "Raw DCT4X4", "Raw DCT2X2", "Raw DCT4X8",
    "Raw DCT8X4", "Raw IDENTITY", "Hook P", "Merged Over", "Margin 0", "Margin 1", "Margin 2",
    "Margin 3", "Margin 4", "Margin 5", "Margin 6", "Margin 7", "Margin Skipped",
]


@dataclass
class TraceStat(_StatRow):
    """One scan index s of one encode's search-trace summary
    (Encoder.search_trace / a sweep point's ``"trace"``): the
    blocks the 8x8 scan gave to s (``scan_wins``, the column sum of ``flip``), of
    them by the winner of the scan without hook F (``raw_*`` = ``flip[r][s]``),
    the hook-P overrides with target s, the blocks merged over, the margin
    histogram and the blocks it skipped; beside them the point's ``blocks`` and
    ``max_px``, the same on every row of it.  Every value is an integer."""
    orig_image_name: str
    comp_image_name: str
    distance: float  # f32
    effort: int
    scan_index: int
    strategy: int
    name: str
    blocks: int
    max_px: int
    scan_wins: int
    raw_dct8: int
    raw_dct4x4: int
    raw_dct2x2: int
    raw_dct4x8: int
    raw_dct8x4: int
    raw_identity: int
    hook_p: int
    merged_over: int
    margin_0: int
    margin_1: int
    margin_2: int
    margin_3: int
    margin_4: int
    margin_5: int
    margin_6: int
    margin_7: int
    margin_skipped: int


def trace_stats(orig_name: str, comp_name: str, distance: float, effort: int, summary: dict):
    """The six TraceStat rows of one summary (Encoder.search_trace / a sweep
    point's ``"trace"``), one per scan index, with the values ``jxg_cjxl
    --jxg_trace`` writes."""
    flip = np.asarray(summary["flip"]).astype(np.int64).reshape(6, 6)
    margin = np.asarray(summary["margin"]).astype(np.int64).reshape(6, 8)
    rows = []
    for s, sid in enumerate(TRACE_SCAN_IDS):
        rows.append(TraceStat(
            orig_name, comp_name, float(np.float32(distance)), int(effort), s, sid,
            STRATEGY_NAMES[sid], int(summary["blocks"]), int(summary["max_px"]),
            int(flip[:, s].sum()), *[int(flip[r, s]) for r in range(6)],
            int(summary["hook_p"][s]), int(summary["merged_over"][s]),
            *[int(margin[s, k]) for k in range(8)], int(summary["margin_skipped"][s])))
    return rows


def write_trace_stats(rows, trace_file: str) -> None:
    _append_stats(rows, trace_file, TRACE_HEADER)


def read_trace_stats(file_name: str):
    return _read_stats(TraceStat, file_name)


_DIFF_FIELDS = [f.name for f in fields(ComparisonResult)[4:]]


def compare_results(results_1: str, results_2: str):
    """benchmark.rs:727-864; returns (diffs, summary) and writes the CSVs."""
    r1 = sorted(read_csv(results_1), key=lambda r: r.orig_image_name)
    r2 = sorted(read_csv(results_2), key=lambda r: r.orig_image_name)
    assert len(r1) == len(r2)
    diffs = []
    for a, b in zip(r1, r2):
        assert a.orig_image_name == b.orig_image_name
        assert a.comp_image_name == b.comp_image_name
        assert a.distance == b.distance
        assert a.effort == b.effort
        vals = [float(getattr(b, n)) - float(getattr(a, n)) for n in _DIFF_FIELDS]
        diffs.append(ComparisonResultDiff(a.orig_image_name, a.comp_image_name, a.distance,
                                          a.effort, *vals))
    acc = [0.0] * len(_DIFF_FIELDS)
    for d in diffs:
        for i, f in enumerate(fields(ComparisonResultDiff)[4:]):
            acc[i] += getattr(d, f.name)
    n = float(len(diffs))
    summary = ComparisonResultDiff("Summary", "Summary", 0.0, 0, *[v / n for v in acc])
    out_dir = os.path.dirname(os.path.abspath(results_1))
    diff_file = os.path.join(out_dir, "comparison_diffs.csv")
    write_csv_header(diff_file, DIFF_HEADER)
    write_csv(diffs, diff_file)
    summary_file = os.path.join(out_dir, "summary.csv")
    write_csv_header(summary_file, DIFF_HEADER)
    write_csv([summary], summary_file)
    return diffs, summary


def compare_to_orig(encoder, orig_name: str, orig_rgb: np.ndarray, orig_file_size: int,
                    comp_name: str, comp_rgb, comp_file_size: int,
                    distance: float, effort: int, result_file: str | None = None,
                    ssim: bool = True, decode_with=None,
                    ms_ssim: bool = False) -> ComparisonResult:
    """benchmark.rs:895-972 with the metrics on the GPU.  ``encoder`` is a
    jxg.Encoder (its context runs jxg_compare_rgb8); ``comp_rgb`` is the
    decoded image (stock djxl where present, any decoder otherwise) -- or,
    with ``decode_with`` (a jxg.Encoder, which may be ``encoder``), the
    codestream bytes of the compressed file, which that context decodes on the
    GPU (Encoder.decode, jxg_decode_rgb8): the reference harnesses' step of
    decoding the file that was written (image_reader.rs:555-606 through
    jpegxl-rs; ``djxl IN.jxl OUT.png``).  Raw sizes are width * height * 3
    (image_reader.rs:523-540, Rgb8).  ``ms_ssim``: fill the MS-SSIM column
    (Encoder.msssim) instead of the reference's 0.0."""
    if decode_with is not None:
        comp_rgb = decode_with.decode(comp_rgb)
    h, w = orig_rgb.shape[:2]
    raw = w * h * 3
    q = encoder.compare(orig_rgb, comp_rgb, ssim=ssim)
    if ms_ssim:
        q["ms_ssim"] = encoder.msssim(orig_rgb, comp_rgb)["ms_ssim"]
    return _record(orig_name, comp_name, distance, effort, orig_file_size, comp_file_size, raw, q,
                   ssim, result_file)


def compare_batch_to_orig(encoder, items, decode_with, result_file: str | None = None,
                          ssim: bool = True, ms_ssim: bool = False):
    """compare_to_orig(..., decode_with=) of many files with one decode: the
    harness decodes every compressed file it wrote (benchmark.rs:637-660), and
    one frame's pass-group kernel leaves the GPU almost idle, so all items'
    codestreams go through ``decode_with.decode_batch`` (jxg_decode_batch_rgb8)
    and each decoded image is then compared as compare_to_orig does.  ``items``:
    tuples ``(orig_name, orig_rgb, orig_file_size, comp_name, codestream,
    comp_file_size, distance, effort)``.  Returns the records in order, equal
    to per-item compare_to_orig; the CSV rows are written in that order."""
    items = list(items)
    decoded = decode_with.decode_batch([it[4] for it in items])
    return [compare_to_orig(encoder, it[0], it[1], it[2], it[3], rgb, it[5], it[6], it[7],
                            result_file=result_file, ssim=ssim, ms_ssim=ms_ssim)
            for it, rgb in zip(items, decoded)]


def _record(orig_name, comp_name, distance, effort, orig_file_size, comp_file_size, raw, q, ssim,
            result_file) -> ComparisonResult:
    res = ComparisonResult(
        orig_name, comp_name, float(np.float32(distance)), int(effort), int(orig_file_size),
        int(comp_file_size), raw, raw,
        file_size_ratio(orig_file_size, comp_file_size, "comp"),
        file_size_ratio(raw, comp_file_size, "comp"),
        q["mse"], q["psnr"], q["ssim"] if ssim else 0.0, q.get("ms_ssim", 0.0), 0.0, 0.0, 0.0)
    if result_file:
        write_csv_header(result_file, RESULT_HEADER)
        write_csv([res], result_file)
    return res


def encode_and_compare(encoder, orig_name: str, orig_rgb: np.ndarray, orig_file_size: int,
                       comp_name: str, distance: float, effort: int,
                       result_file: str | None = None, ssim: bool = True,
                       ms_ssim: bool = False):
    """Encode + compare_to_orig in one process with no decoder: the image is
    encoded from device memory, its decoded pixels are reconstructed on the
    device (Encoder.reconstruct_device, jxg_reconstruct_rgb8_device) and the
    metrics run on the two device images.  ``encoder`` carries the distance and
    effort it was created with; ``distance`` / ``effort`` fill the record.
    Returns (codestream bytes, ComparisonResult)."""
    import torch

    o = np.ascontiguousarray(orig_rgb, dtype=np.uint8)
    if o.ndim != 3 or o.shape[2] != 3:
        raise ValueError("orig_rgb must be (H, W, 3) uint8")
    h, w = o.shape[:2]
    dev = "cuda:%d" % encoder.params.device
    d_orig = torch.from_numpy(o).to(dev)
    d_comp = torch.empty_like(d_orig)
    torch.cuda.synchronize(dev)
    data = encoder.encode_device(d_orig.data_ptr(), w, h)
    encoder.reconstruct_device(d_comp.data_ptr())
    q = encoder.compare_device(d_orig.data_ptr(), d_comp.data_ptr(), w, h, ssim=ssim)
    if ms_ssim:
        q["ms_ssim"] = encoder.msssim_device(d_orig.data_ptr(), d_comp.data_ptr(), w, h)["ms_ssim"]
    raw = w * h * 3
    return data, _record(orig_name, comp_name, distance, effort, orig_file_size, len(data), raw, q,
                         ssim, result_file)


def sweep_and_compare(encoder, orig_name: str, orig_rgb: np.ndarray, orig_file_size: int, points,
                      result_file: str | None = None, ssim: bool = True, ms_ssim: bool = False,
                      strategy_file: str | None = None, rate_file: str | None = None,
                      ab_file: str | None = None, ab_base=None, trace_file: str | None = None):
    """The harness's per-image loop (benchmark.rs:637-677) in one call: the
    image is encoded at every point (dicts with ``distance`` / ``effort`` and
    optionally ``proposals`` / ``flags``) by ``encoder.sweep`` -- one upload,
    the points overlapped over the pipeline's lanes, each point's decoded
    quality computed on its lane -- and one record per point is built, named
    ``comp_image_name(stem of orig_name, distance, effort)`` (benchmark.rs:
    644-650).  ``encoder``'s own parameters play no part.  Returns
    (codestreams, records); the records, and the CSV rows in point order, equal
    per-point :func:`encode_and_compare` on an encoder of those parameters.
    ``ms_ssim`` (needs ``ssim``): the MS-SSIM column from the points' lanes
    (``quality="msssim"``).  ``strategy_file``: every point's strategy report
    is reduced on its lane as well (``strategies=True``) and one StrategyStat
    row per non-empty strategy is appended to that file (strategy_stats.csv).
    ``rate_file``: every point's rate report is priced on its lane
    (``rates=True``) and one RateStat row per strategy that holds tokens is
    appended to that file.  ``ab_file`` with ``ab_base`` (one base index per
    point: -1, or the index of an earlier point): every point with a base is
    compared with it on its lane (``ab=ab_base``) and one AbStat row per
    non-empty cell of that A/B report is appended to that file.
    ``trace_file``: every point of effort >= 5 runs traced on its lane
    (``trace=True``, the same codestreams) and the six TraceStat rows of its
    search-trace summary are appended to that file; a point without a search
    (``blocks == 0``) writes none."""
    if (ab_file is None) != (ab_base is None):
        raise ValueError("ab_file and ab_base go together")
    if ms_ssim and not ssim:
        raise ValueError("ms_ssim rides on the quality-2 sweep: it needs ssim=True")
    o = np.ascontiguousarray(orig_rgb, dtype=np.uint8)
    if o.ndim != 3 or o.shape[2] != 3:
        raise ValueError("orig_rgb must be (H, W, 3) uint8")
    h, w = o.shape[:2]
    points = list(points)
    res = encoder.sweep(o, points, quality=("msssim" if ms_ssim else "ssim") if ssim else "psnr",
                        strategies=strategy_file is not None, rates=rate_file is not None,
                        trace=trace_file is not None,
                        **({} if ab_base is None else {"ab": list(ab_base)}))
    stem = os.path.splitext(orig_name)[0]
    raw = w * h * 3
    datas, records = [], []

    def d_e(p):
        return (p["distance"], p["effort"]) if isinstance(p, dict) else (p[0], p[1])

    names = [comp_image_name(stem, *d_e(p)) for p in points]
    for i, (p, (data, q)) in enumerate(zip(points, res)):
        d, e = d_e(p)
        datas.append(data)
        records.append(_record(orig_name, names[i], d, e, orig_file_size, len(data), raw, q, ssim,
                               result_file))
        if strategy_file is not None:
            write_strategy_stats(strategy_stats(orig_name, names[i], d, e, q["strategies"], w, h),
                                 strategy_file)
        if rate_file is not None:
            write_rate_stats(rate_stats(orig_name, names[i], d, e, q["rates"]), rate_file)
        if ab_file is not None and ab_base[i] >= 0:
            write_ab_stats(ab_stats(orig_name, names[ab_base[i]], names[i], d, e, q["ab"], w, h),
                           ab_file)
        if trace_file is not None and int(q["trace"]["blocks"]) != 0:
            write_trace_stats(trace_stats(orig_name, names[i], d, e, q["trace"]), trace_file)
    return datas, records
