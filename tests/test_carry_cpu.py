"""The carried count of csrc/mdr_validity.h (CarriedCount: the next direct rollout's first group of
windows, counted by the previous call's last step launch) on the CPU: tests/carry_check.cpp,
a stand-alone program that raises the transitions in the order the entry points of the host library
raise them (a model of mdr_rollout / mdr_rollout_begin over the real Validity, not mdr_capi.hip's own
code: tests/test_rollout_carry_gpu.py runs that) — arm, consume, and a drop under every transition that can invalidate the count; the slots
running on across 20 call boundaries — built plain and with AddressSanitizer + UBSan (runtimes linked
statically: nothing is preloaded) and run.  And the host-side check every group launch makes, for the
groups a carried call steps and counts."""
import os
import shutil
import subprocess

import pytest

import golden_util as gu  # noqa: F401  (sys.path set by conftest)

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "marl-demandresponse_amd", "csrc")
SRC = os.path.join(HERE, "carry_check.cpp")
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
    assert "carry_check: ok" in r.stdout


def test_carry_check_plain(tmp_path):
    b = _build(tmp_path / "carry_check")
    assert b.returncode == 0, b.stderr
    _run(tmp_path / "carry_check")


def test_carry_check_sanitized(tmp_path):
    plain = _build(tmp_path / "carry_check")
    assert plain.returncode == 0, plain.stderr  # (so a failure below is the sanitizer runtime's)
    b = _build(tmp_path / "carry_check_san", SAN + ["-fno-omit-frame-pointer"])
    # (only the sanitizer runtimes' absence skips: any other build error of the sanitized program fails)
    if b.returncode != 0 and any(w in b.stderr for w in ("libasan", "libubsan", "-static-libasan", "-static-libubsan")):
        pytest.skip("no static sanitizer runtime for g++ here: " + b.stderr.strip().splitlines()[-1])
    assert b.returncode == 0, b.stderr
    _run(tmp_path / "carry_check_san")


def test_carried_group_geometry_guard():
    """A launch of a carried call reads the rows of the windows it steps and replaces them with the
    rows of the windows it counts — the next group's, or the first min(G, nw) of the next call: rows
    for the larger of the two, and an end word per house.  mdr_window_group_check (no GPU calls)
    refuses mask rows one byte short or an end-word buffer one word short of that."""
    from mdr_amd import _lib

    lib = _lib.load()
    hpt, kmax = 2, 32  # kWinHpt, kWindowMax (mdr_kernels.h)
    for n in (1, 129, 257, 2049, (1 << 20) + 7):
        tiles = (n + 64 * hpt - 1) // (64 * hpt)
        rows = (tiles + 3) // 4 * 4 * hpt * kmax * 8
        for nw in (1, 3, 4, 6):
            for group in (1, 2, 3, 4):
                stepped = min(group, nw - (nw - 1) // group * group)  # the call's last group
                counted = min(group, nw)                              # the next call's first
                w = max(stepped, counted)
                assert lib.mdr_window_group_check(n, w, w * rows, n * 4) == 0, lib.mdr_last_error()
                assert lib.mdr_window_group_check(n, w, w * rows - 1, n * 4) == -1
                assert b"ON-mask" in lib.mdr_last_error()
                assert lib.mdr_window_group_check(n, w, w * rows, n * 4 - 4) == -1
                assert b"end-word" in lib.mdr_last_error()


def test_carry_option_and_info_exported():
    from mdr_amd import _lib

    lib = _lib.load()
    assert _lib.OPTIONS["rollout_carry"] == 19
    assert lib.mdr_rollout_carry_info(None, None, 0) == -1
