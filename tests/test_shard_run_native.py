"""The shard-run tracker (mi355x_ddp/ops/csrc/shard_run.h) as a stand-alone
host program under AddressSanitizer and UBSan: tests/native/
shard_run_check.cpp includes only that header, runs the documented
schedules and 300 randomized step/bind/flush sequences against a naive
model, and is run here as a child process. Nothing sanitized is loaded
into Python."""

import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "shard_run_check.cpp")
INC = os.path.join(ROOT, "mi355x_ddp", "ops", "csrc")
# the runtimes linked INTO the program: it then starts the same way
# whatever else the environment loads into every process
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all",
       "-static-libasan", "-static-libubsan"]


def _compile(cxx, src, out, extra=()):
    return subprocess.run(
        [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", *SAN, *extra,
         src, "-o", out], capture_output=True, text=True, timeout=300)


def test_shard_run_header_under_sanitizers(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++ on this host")
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    got = _compile(cxx, str(probe), str(tmp_path / "probe"))
    if got.returncode != 0:
        pytest.skip("g++ lacks the sanitizer runtimes: "
                    + got.stderr.strip()[-200:])

    exe = str(tmp_path / "shard_run_check")
    got = _compile(cxx, SRC, exe, extra=["-I", INC])
    assert got.returncode == 0, got.stderr[-4000:]
    assert "warning" not in got.stderr, got.stderr[-4000:]

    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, (run.stdout + run.stderr)[-4000:]
    assert "shard_run_check: ok" in run.stdout
