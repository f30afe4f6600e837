"""A sweep's riders without a device: each switch and getter pair is exported,
listed, and refuses a null context."""
import ctypes

import pytest

INVALID_ARG = -1
RIDERS = [
    ("jxg_set_sweep_msssim", "jxg_sweep_msssim", "_Msssim"),
    ("jxg_set_sweep_report", "jxg_sweep_report", "_StrategyReport"),
    ("jxg_set_sweep_rates", "jxg_sweep_rates", "_RateReport"),
    ("jxg_set_sweep_ab", "jxg_sweep_ab", "_AbReport"),
]


@pytest.mark.parametrize("setter,getter,ctype", RIDERS, ids=[r[1] for r in RIDERS])
def test_null_context_is_refused(jxg_mod, setter, getter, ctype):
    lib = jxg_mod.load()
    for name in (setter, getter):
        assert hasattr(lib, name), name
        assert name in jxg_mod.EXPORTS
    if setter == "jxg_set_sweep_ab":
        base = (ctypes.c_int32 * 2)(-1, 0)
        assert lib.jxg_set_sweep_ab(None, base, 2) == INVALID_ARG
        assert lib.jxg_set_sweep_ab(None, None, 0) == INVALID_ARG
    else:
        for on in (0, 1):
            assert getattr(lib, setter)(None, on) == INVALID_ARG
    out = (getattr(jxg_mod, ctype) * 2)()
    ctypes.memset(out, 0xA5, ctypes.sizeof(out))
    assert getattr(lib, getter)(None, out, 2) == INVALID_ARG
    assert bytes(out) == b"\xa5" * ctypes.sizeof(out), "nothing written"
