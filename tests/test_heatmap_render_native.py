"""CPU: the render kernel's own source (csrc/heatmap_render.hip) compiled for the host and run thread by thread on exact-size heap
buffers under AddressSanitizer + UndefinedBehaviorSanitizer -- tests/native/heatmap_render_check.cpp, a program of its own, run as a
child process.  Sides 1, 2, 3, 5, 33, 64 with count, level start, rows behind the level, image stride and the outputs varied: an
index past an end, a store across a frame's end or a misaligned dword store is a sanitizer error; every value is compared with a
scalar evaluation of the arithmetic, bit for bit."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
SAN = ["-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-g", "-O1"]


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    exe = tmp_path_factory.mktemp("heatmap_render") / "heatmap_render_check"
    subprocess.run([CLANG, *SAN, "-std=c++17", "-ffp-contract=off", "-Wno-unknown-pragmas", "-I", ROOT,
                    os.path.join(ROOT, "tests", "native", "heatmap_render_check.cpp"), "-o", str(exe)], check=True, capture_output=True, text=True)
    env = dict(os.environ, ASAN_OPTIONS="abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    return subprocess.run([str(exe)], capture_output=True, env=env, timeout=300)


def test_kernel_source_on_the_host_is_clean_and_exact(run):
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-3000:]
    assert b"runtime error" not in run.stderr and b"AddressSanitizer" not in run.stderr, run.stderr[-2000:]
    last = run.stdout.decode().splitlines()[-1]
    assert last == "heatmap_render_check: 480 runs, 0 values wrong, 64 misaligned frames, 128 partial groups, 3 of 3 refusals", last
