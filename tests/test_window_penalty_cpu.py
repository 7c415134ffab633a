"""Host-only geometry of the common-penalty window path: the size of the per-tick, per-wave
penalty partial rows ([32][tiles_padded][2] doubles) and the check every such launch runs first."""
from mdr_amd import _lib as L

SIZES = (1, 63, 64, 128, 129, 512, 513, 2049, 65536, 131071, 1 << 20, (1 << 20) + 7)


def _want(n):
    tiles = -(-n // 128)          # a 128-house tile per wave
    blocks = -(-tiles // 4)       # four waves per step-window block
    return blocks * 4 * 32 * 2 * 8


def test_window_pen_bytes():
    lib = L.load()
    for n in SIZES:
        assert lib.mdr_window_pen_bytes(n) == _want(n), n
    assert lib.mdr_window_pen_bytes(-1) == 0


def test_window_pen_check():
    lib = L.load()
    for n in SIZES:
        need = _want(n)
        assert lib.mdr_window_pen_check(n, need) == 0, n
        assert lib.mdr_window_pen_check(n, need - 1) == -1, n
        assert b"penalty partial" in lib.mdr_last_error()
    assert lib.mdr_window_pen_check(0, 1 << 20) == -1
    assert b"penalty partial" in lib.mdr_last_error()
