"""The host side of MDR_OPT_GROUP_LA_ORDER without a GPU: the two halves of group mask
rows every k_step_group launch checks (mdr_window_group_halves_check), and the half that travels with
the carried count (csrc/mdr_validity.h group_half / CarriedCount::half): tests/la_half_check.cpp, a
stand-alone program over the real Validity, built plain and with AddressSanitizer + UBSan (runtimes
linked statically: nothing is preloaded) and run."""
import os
import shutil
import subprocess

import pytest

import golden_util as gu  # noqa: F401  (sys.path set by conftest)

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "marl-demandresponse_amd", "csrc")
SRC = os.path.join(HERE, "la_half_check.cpp")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]


def _gxx():
    gxx = os.environ.get("CXX") or shutil.which("g++")
    if not gxx:
        pytest.skip("no g++ on this machine")
    return gxx


def _build(out, extra=()):
    cmd = [_gxx(), "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-I" + CSRC, *extra, SRC, "-o", str(out)]
    return subprocess.run(cmd, capture_output=True, text=True)


def _run(exe):
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "la_half_check: ok" in r.stdout


def test_la_half_check_plain(tmp_path):
    b = _build(tmp_path / "la_half_check")
    assert b.returncode == 0, b.stderr
    _run(tmp_path / "la_half_check")


def test_la_half_check_sanitized(tmp_path):
    plain = _build(tmp_path / "la_half_check")
    assert plain.returncode == 0, plain.stderr  # (so a failure below is the sanitizer runtime's)
    b = _build(tmp_path / "la_half_check_san", SAN + ["-fno-omit-frame-pointer"])
    # (only the sanitizer runtimes' absence skips: any other build error of the sanitized program fails)
    if b.returncode != 0 and any(w in b.stderr for w in ("libasan", "libubsan", "-static-libasan", "-static-libubsan")):
        pytest.skip("no static sanitizer runtime for g++ here: " + b.stderr.strip().splitlines()[-1])
    assert b.returncode == 0, b.stderr
    _run(tmp_path / "la_half_check_san")


@pytest.mark.parametrize("n", [1, 1500, 4396, 131700, (1 << 20) + 7])
def test_two_halves_geometry_guard(n):
    """A launch reads four windows of mask rows per tile from one half and writes four to the other,
    the second half starting mdr_window_group_half_bytes behind the first: the check refuses group rows
    one byte short of the second half's end, and an end-word buffer one word short of the shard."""
    from mdr_amd import _lib

    lib = _lib.load()
    hpt, kmax, group = 2, 32, 4  # kWinHpt, kWindowMax, kWinGroup (mdr_kernels.h)
    tiles = (n + 64 * hpt - 1) // (64 * hpt)
    half = group * ((tiles + 3) // 4 * 4 * hpt * kmax * 8)
    assert lib.mdr_window_group_half_bytes(n) == half == group * lib.mdr_window_onb_bytes(n, 4)
    assert lib.mdr_window_group_halves_check(n, 2 * half, n * 4) == 0, lib.mdr_last_error()
    assert lib.mdr_window_group_halves_check(n, 2 * half - 1, n * 4) == -1
    assert b"two halves" in lib.mdr_last_error()
    assert lib.mdr_window_group_halves_check(n, half, n * 4) == -1  # (one half alone: the old reserve)
    assert lib.mdr_window_group_halves_check(n, 2 * half, n * 4 - 4) == -1
    assert b"end-word" in lib.mdr_last_error()
    assert lib.mdr_window_group_halves_check(0, 1 << 30, 1 << 20) == -1
    # what mdr_create reserves behind the first window's rows covers both halves
    tiles64 = ((tiles + 1 + 15) // 16 * 16) * hpt + 1
    assert 2 * group * tiles64 * kmax * 8 >= 2 * half


def test_la_order_option_exported():
    from mdr_amd import _lib

    lib = _lib.load()
    assert _lib.OPTIONS["group_la_order"] == 20
    assert (_lib.LA_AFTER, _lib.LA_ALT1, _lib.LA_ALT8, _lib.LA_ALT256, _lib.LA_BEFORE, _lib.LA_TAIL_BEFORE) == (0, 1, 2, 3, 4, 16)
    assert lib.mdr_set_option(None, _lib.OPTIONS["group_la_order"], 1) == -1
