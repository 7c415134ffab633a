"""csrc/mdr_devbuf.h (the owner of the context's device buffers) on the CPU: tests/devbuf_check.cpp, a
stand-alone program over a counting allocator that fails the k-th allocation on request, built
plain and with AddressSanitizer + UBSan (runtimes linked statically: nothing is preloaded) and run.
The allocation-failure paths of the host library cannot be exercised on a GPU; this is where the
rules they rely on are checked: release before allocate, empty after a failed grow, units that
grow all or nothing, one release per block."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "marl-demandresponse_amd", "csrc")
SRC = os.path.join(HERE, "devbuf_check.cpp")
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
    assert "devbuf_check: ok" in r.stdout


def test_header_is_host_only():
    """The header names no HIP type or function (plain g++ compiles it: the builds below) and no
    HIP header."""
    with open(os.path.join(CSRC, "mdr_devbuf.h")) as f:
        text = f.read()
    assert "#include <hip" not in text and "hipMalloc" not in text and "hipFree" not in text


def test_devbuf_check_plain(tmp_path):
    b = _build(tmp_path / "devbuf_check")
    assert b.returncode == 0, b.stderr
    _run(tmp_path / "devbuf_check")


def test_devbuf_check_sanitized(tmp_path):
    plain = _build(tmp_path / "devbuf_check")
    assert plain.returncode == 0, plain.stderr  # (so a failure below is the sanitizer runtime's)
    b = _build(tmp_path / "devbuf_check_san", SAN + ["-fno-omit-frame-pointer"])
    if b.returncode != 0 and any(w in b.stderr for w in ("libasan", "libubsan", "cannot find", "unrecognized")):
        pytest.skip("no static sanitizer runtime for g++ here: " + b.stderr.strip().splitlines()[-1])
    assert b.returncode == 0, b.stderr
    _run(tmp_path / "devbuf_check_san")
