"""csrc/mdr_validity.h (the owner of the context's beliefs about derived device state) on
the CPU: tests/validity_check.cpp, a stand-alone program that raises the transitions in the order
each entry point of the host library raises them and checks the fields after each script, built
plain and with AddressSanitizer + UBSan (runtimes linked statically: nothing is preloaded) and run.
The failure paths of a launch sequence cannot be exercised on a GPU; this is where their rule is
checked: behind a failed sequence nothing derived is vouched for."""
import os
import re
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "marl-demandresponse_amd", "csrc")
SRC = os.path.join(HERE, "validity_check.cpp")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]
FIELDS = ("ring", "counts_ready", "gq_keys_ready", "gq_hist_dirty", "gq_slab_zeroed", "gq_map_stale", "fz_ready",
          "fz_par", "gq_nparts", "coef_dirty", "wslab_dirty", "begun", "gq_s1", "gq_s2")


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
    assert "validity_check: ok" in r.stdout


def test_header_is_host_only():
    """The header names no HIP type or function (plain g++ compiles it: the builds below) and no
    HIP header."""
    with open(os.path.join(CSRC, "mdr_validity.h")) as f:
        text = f.read()
    assert "#include <hip" not in text and "hipStream" not in text and "hipError" not in text


def test_capi_assigns_no_validity_field():
    """mdr_capi.hip says what happened; it never sets a field of DESIGN §7.2's table itself, directly
    or through the context (the fields live in mdr::Validity, private)."""
    with open(os.path.join(CSRC, "mdr_capi.hip")) as f:
        text = f.read()
    # (a field by its bare name, or through the context; another struct's field of the same name is not meant)
    pat = re.compile(r"(?<![\w.>])(?:c->(?:v\.)?)?(?:" + "|".join(FIELDS) + r")_?(?:\.\w+)?\s*(?:=(?!=)|\+=|-=|\+\+|--)")
    hits = [(text.count("\n", 0, m.start()) + 1, m.group(0)) for m in pat.finditer(text)]
    assert not hits, hits


def test_validity_check_plain(tmp_path):
    b = _build(tmp_path / "validity_check")
    assert b.returncode == 0, b.stderr
    _run(tmp_path / "validity_check")


def test_validity_check_sanitized(tmp_path):
    plain = _build(tmp_path / "validity_check")
    assert plain.returncode == 0, plain.stderr  # (so a failure below is the sanitizer runtime's)
    b = _build(tmp_path / "validity_check_san", SAN + ["-fno-omit-frame-pointer"])
    if b.returncode != 0 and any(w in b.stderr for w in ("libasan", "libubsan", "cannot find", "unrecognized")):
        pytest.skip("no static sanitizer runtime for g++ here: " + b.stderr.strip().splitlines()[-1])
    assert b.returncode == 0, b.stderr
    _run(tmp_path / "validity_check_san")
