"""The format's AC context model (csrc/jxg_acmodel.h), the token record
(csrc/jxg_acrec.h) and the merged shapes (csrc/jxg_shapes.h), run as themselves
(no GPU, nothing loaded into Python): tests/native/ac_model.cpp is built by g++
-- under ASan + UBSan where the compiler has them -- linked with the oracle's
tables (oracle/entropy.c), and prints every table exhaustively.  The encoder's
kernels, the decoder and the host's map validator all read these functions."""
import hashlib
import json
import os

import pytest

import ac_model_native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# raw strategy id -> (blocks down, blocks across) of the strategies the encoder writes
SHAPES = {0: (1, 1), 1: (1, 1), 2: (1, 1), 3: (1, 1), 12: (1, 1), 13: (1, 1), 6: (2, 1), 7: (1, 2),
          4: (2, 2), 10: (4, 2), 11: (2, 4), 5: (4, 4), 19: (8, 4), 20: (4, 8), 18: (8, 8),
          22: (16, 8), 23: (8, 16), 21: (16, 16), 25: (32, 16), 26: (16, 32), 24: (32, 32)}


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return ac_model_native.build(tmp_path_factory)


@pytest.fixture(scope="module")
def tables(exe):
    out = {}
    for ln in ac_model_native.run(exe):
        name, *vals = ln.split()
        out[name] = vals
    return out


def _ints(tables, name):
    return [int(v) for v in tables[name]]


@pytest.mark.parametrize("name,n", [("strategy_order", 27), ("block_ctx", 39), ("freq_ctx", 64),
                                    ("nnz_ctx", 64)])
def test_context_tables_equal_the_oracles(tables, name, n):
    got, want = _ints(tables, name), _ints(tables, "oracle_" + name)
    assert len(got) == n and len(want) == n
    assert got == want


def test_sizes(tables):
    assert _ints(tables, "sizes") == [15, 37, 458, 7425, 132, 64, 1024 * 3 * 64, 256 * 3 * 64,
                                      1024 * 3]


def test_strategy_shape_and_varblock_dims(tables):
    shape = _ints(tables, "strategy_shape")
    dims = [tuple(int(x) for x in v.split(":")) for v in tables["varblock_dims"]]
    assert len(shape) == 27 and len(dims) == 27
    for t in range(27):
        cy, cx = SHAPES.get(t, (0, 0))
        assert shape[t] == (cy | cx << 8), t
        cy, cx = SHAPES.get(t, (1, 1))  # an id without a shape counts as the 8x8 class
        assert dims[t] == ((cy * cx).bit_length() - 1, cx, cy), t


def test_merged_shapes_are_strategy_shapes(tables):
    shape = _ints(tables, "strategy_shape")
    got = [tuple(int(x) for x in v.split(":")) for v in tables["shapes"]]
    assert [t for t, _, _ in got] == [6, 7, 4, 10, 11, 5, 19, 20, 18]
    for t, lcy, lcx in got:
        assert shape[t] == (1 << lcy | (1 << lcx) << 8), t


def test_nz_bucket(tables):
    """oracle/encode.c nz_bucket, restated (the decoder's walk writes the same
    expression in unsigned arithmetic, csrc/jxg_decode_core.h)"""
    def want(n):
        n = min(n, 64)
        return n if n < 8 else 4 + n // 2

    def decoder(pred):
        pp = pred if pred < 64 else 64
        return pp if pp < 8 else 4 + pp // 2

    got = _ints(tables, "nz_bucket")
    assert len(got) == 1025
    assert got == [want(n) for n in range(1025)] == [decoder(n) for n in range(1025)]
    assert max(got) == 36


def test_ac_cluster_is_the_recorded_map(tables):
    with open(os.path.join(ROOT, "tests", "golden", "ac_model.json")) as f:
        want = json.load(f)
    clu = bytes.fromhex(tables["ac_cluster"][0])
    assert len(clu) == 7425
    assert max(clu) == 131
    assert hashlib.sha256(clu).hexdigest() == want["sha256"]["ac_cluster"]


# (cluster, token, raw-bit count, raw bits): the field edges of tests/highrate_cases.py, then
# every field alone and all together at the top of its bit field
EDGES = [(0, 0, 0, 0), (131, 0, 0, 0), (0, 63, 0, 0), (0, 0, 13, 0), (0, 0, 0, (1 << 13) - 1),
         (131, 63, 13, (1 << 13) - 1),
         (255, 0, 0, 0), (0, 63, 0, 0), (0, 0, 15, 0), (0, 0, 0, (1 << 14) - 1),
         (255, 63, 15, (1 << 14) - 1)]


@pytest.fixture(scope="module")
def records(exe):
    lines = ac_model_native.run(exe, "record", "".join("%d %d %d %d\n" % e for e in EDGES))
    return [tuple(int(v) for v in ln.split()) for ln in lines]


def test_record_round_trip_at_the_field_edges(records):
    assert [r[:4] for r in records] == EDGES
    for c, t, n, b, packed, rc, rt, rn, rb in records:
        assert (rc, rt, rn, rb) == (c, t, n, b)  # no bleed into a neighbour
        assert 0 <= packed < 1 << 32


def test_record_bytes_are_the_formats(records):
    """the layout tests/test_highrate_cases.py and the recorded records rely on"""
    for c, t, n, b, packed, *_ in records:
        assert packed == c | t << 8 | n << 14 | b << 18
