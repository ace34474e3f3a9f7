"""Host arithmetic of the PixelCNN chain's code tables (csrc/code_tables.hip), no GPU: table sizes, the cap, which launches
of a code row become lookups (slot V0 from row 1 on, hg_0 of column 1 only), which riders a V0 lookup writes, and the pass rule behind
TS_PIX_TABLES — through `ts_debug_code_tables_plan`, the same functions the model code calls.
"""
import ctypes as C

import pytest


@pytest.fixture(scope="module")
def lib():
    from talkshow_amd import _lib
    return _lib.load()


FIELDS = ("fits", "takes", "waves_v0", "sets_v0", "bytes_v0", "waves_hg", "bytes_hg", "v0", "q1", "q0", "hg", "cap")


def plan(lib, V=2048, D=256, B=256, r=5, j=1, last_row=1 << 30, knobs=None):
    o = (C.c_int64 * 12)()
    assert lib.ts_debug_code_tables_plan(V, D, B, r, j, last_row, knobs.encode() if knobs else None, o) == 0
    return dict(zip(FIELDS, (int(x) for x in o)))


def waves(K):
    """plan_skinny's K split of the 16-column chain kernels: 8 waves from K = 256 on, else 4"""
    return 8 if K // 8 >= 32 else 4


@pytest.mark.parametrize("V,D", [(2048, 256), (64, 32), (64, 64), (256, 64), (2048, 128), (1000, 96), (2048, 512)])
def test_table_sizes(lib, V, D):
    p = plan(lib, V, D)
    wv, wh = waves(2 * D), waves(D)
    assert (p["waves_v0"], p["waves_hg"]) == (wv, wh)
    # V0: K = 2D in wv slices, the first half column 0's (one prefix row), the second half column 1's (one row each)
    assert p["sets_v0"] == 1 + wv // 2
    assert p["bytes_v0"] == 3 * p["sets_v0"] * V * 4 * D * 4
    assert p["bytes_hg"] == V * 2 * D * 4          # one prefix row of 2D floats per code


def test_shipped_sizes_are_the_documented_ones(lib):
    p = plan(lib)
    assert p["sets_v0"] == 5 and p["bytes_v0"] == 3 * 5 * 2048 * 1024 * 4 == 125829120   # 120 MiB
    assert p["bytes_hg"] == 4 << 20
    assert p["fits"] == 1 and p["takes"] == 1


def test_cap(lib):
    cap = plan(lib)["cap"]
    assert cap == 192 << 20
    for V, D in [(2048, 256), (64, 32), (3276, 256), (3277, 256), (2048, 512), (4096, 256), (1024, 512)]:
        assert plan(lib, V, D)["fits"] == int(V * 4 * D * 4 * 15 <= cap), (V, D)
    big = plan(lib, 4096, 512)
    assert big["fits"] == 0 and big["takes"] == 0 and (big["v0"], big["q1"], big["q0"], big["hg"]) == (0, 0, 0, 0)


def test_rows_and_columns(lib):
    for r in range(0, 12):
        for j in (0, 1):
            p = plan(lib, r=r, j=j)
            assert p["v0"] == int(r >= 1), r           # row 0 has no code above it: its launch stays
            assert p["hg"] == int(j == 1), (r, j)      # column 0 has no code to its left, in any row


def test_riders_follow_last_row(lib):
    """The Q1 rider serves row r+1, the Q0 rider row r+2: written iff that row is generated — the GEMM riders' rule."""
    for last_row in (1, 2, 3, 5, 8):
        for r in range(0, last_row):
            p = plan(lib, r=r, last_row=last_row)
            assert p["q1"] == int(r >= 1 and r + 1 < last_row), (r, last_row)
            assert p["q0"] == int(r >= 1 and r + 2 < last_row), (r, last_row)
    p = plan(lib, r=7)                                   # chunked and streaming runs: no last row
    assert (p["q1"], p["q0"]) == (1, 1)


def test_pass_rule_and_knob(lib):
    for B in (1, 32, 33, 63, 64, 65, 128, 256):
        assert plan(lib, B=B)["takes"] == int(B >= 64), B                       # default: the passes whose V0 is a wide launch
        assert plan(lib, B=B, knobs="TS_PIX_TABLES=1")["takes"] == 1
        off = plan(lib, B=B, knobs="TS_PIX_TABLES=0")
        assert off["takes"] == 0 and (off["v0"], off["q1"], off["q0"], off["hg"]) == (0, 0, 0, 0)
        assert off["fits"] == 1                                                     # the knob is not the cap
    # the 32-column generic kernel groups its products differently: no tables under it
    nt32 = plan(lib, knobs="TS_SKINNY_NT=32")
    assert nt32["fits"] == 0 and nt32["takes"] == 0
    for knobs in ("TS_SKINNY_V=0", "TS_SKINNY_TILED=0", "TS_SKINNY_WIDE_MIN=0", "TS_NO_GRAPH=1"):   # same K split: the tables stay
        assert plan(lib, knobs=knobs)["takes"] == 1, knobs
