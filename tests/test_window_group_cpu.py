"""The host-side check every k_step_group launch makes (mdr_window_group_check, no GPU calls): group
mask rows one byte short of `windows` x the 4-wave grid's rows, or an end-word buffer one word short
of the shard, are refused with MDR_EARG before anything launches; the exact sizes pass."""
import golden_util as gu  # noqa: F401  (sys.path set by conftest)


def test_window_group_guard():
    from mdr_amd import _lib

    lib = _lib.load()
    hpt, kmax, group = 2, 32, 4  # kWinHpt, kWindowMax, kWinGroup (mdr_kernels.h)
    for n in (1, 63, 64, 128, 129, 257, 2049, 65536, 131071, 1 << 20, (1 << 20) + 7):
        tiles = (n + 64 * hpt - 1) // (64 * hpt)
        rows = (tiles + 3) // 4 * 4 * hpt * kmax * 8  # every wave of the grid, ragged last block included
        assert lib.mdr_window_onb_bytes(n, 4) == rows
        for g in range(1, group + 1):
            assert lib.mdr_window_group_check(n, g, g * rows, n * 4) == 0, lib.mdr_last_error()
            assert lib.mdr_window_group_check(n, g, g * rows - 1, n * 4) == -1
            assert b"ON-mask" in lib.mdr_last_error()
            assert lib.mdr_window_group_check(n, g, g * rows, n * 4 - 4) == -1
            assert b"end-word" in lib.mdr_last_error()
            assert lib.mdr_window_group_check(n, g, g * rows, n * 4 - 1) == -1
        # the allocation of mdr_create behind the first window's rows: kWinGroup x (whole count blocks + one row)
        alloc = group * ((tiles + 16) // 16 * 16 * hpt + 1) * kmax * 8
        assert lib.mdr_window_group_check(n, group, alloc, (n + 1) * 4) == 0, lib.mdr_last_error()
    assert lib.mdr_window_group_check(0, 1, 1 << 20, 1 << 20) == -1
    assert lib.mdr_window_group_check(128, 0, 1 << 20, 1 << 20) == -1
    assert lib.mdr_window_group_check(128, group + 1, 1 << 30, 1 << 20) == -1
