"""CPU: split3 (csrc/tile.h), the exact fp32 -> three bf16 pieces split under the plain eval layer's matrix product, as a host
program of its own (tests/native/split3_check.cpp; host compilation of the header only, nothing is launched): over 2^24 random
bit patterns and every exponent with all-zero, all-ones and single-bit significands the pieces sum to the input bit for bit,
each is one bf16 value with the input's sign, and a non-finite input gives a non-finite piece."""
import os
import re
import subprocess

from echoglad_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_split3_pieces_sum_to_the_input_bit_for_bit(tmp_path):
    exe = tmp_path / "split3_check"
    # -ffp-contract=off: the sums under test are two separate fp32 additions
    cmd = [build.hipcc(), "-x", "hip", "--cuda-host-only", f"--offload-arch={build.ARCH}", "-O2", "-std=c++17", "-ffp-contract=off",
           "-Wno-unused-function", os.path.join(ROOT, "tests", "native", "split3_check.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    m = re.search(r"split3_check: 0 failure\(s\) over (\d+) values", r.stdout)
    assert m and int(m.group(1)) >= (1 << 24) + 2 * 256 * 25, r.stdout[-3000:]
