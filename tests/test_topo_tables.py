"""CPU: the host tables of a closed-form topology handle (csrc/topo_tables.h: build_topo_tables) under AddressSanitizer +
UndefinedBehaviorSanitizer.  tests/native/topo_tables_check.cpp (a program of its own) is linked against the host-sanitized build
of the library that tests/test_abi_sanitized.py uses and run as a child process; nothing is loaded into python under a sanitizer.
It prints a digest of every table per configuration, compared here with tests/golden/topo_tables.json (recorded from the last
commit that built the tables inside eg_topo_create), and checks the invariants the layer kernels rely on: patches cover the frame
once, run bases stay inside the frame, child-sum runs inside the side buffer, pattern indices inside the table, and (deg + 1)^-1/2
against the degrees of echoglad_amd/topology.py's edge list."""
import json
import os
import subprocess

import pytest

from echoglad_amd.topology import HierTopology, TopologySpec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
SAN = ["-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-g"]
TABLES = ("dis", "tiles", "segs", "pats", "patsq", "conn_table", "h_rowptr", "h_colidx")
SCALARS = ("n_pats", "kid_rows", "flat", "hybrid", "conn_chunks")


def _spec(args):
    frame, naux, main_only, coord, conn, diag_main, diag_aux = args
    return TopologySpec(frame, naux, bool(main_only), bool(coord), bool(conn),
                        "grid-diagonal" if diag_main else "grid", "grid-diagonal" if diag_aux and not main_only else "grid")


def _parse(line):
    t = line.split()
    assert t[0] == "cfg" and "REJECTED" not in t, line
    got, i = {"args": [int(x) for x in t[1:8]]}, 8
    for name in TABLES:
        assert t[i] == name, line
        got[name] = [int(t[i + 1]), t[i + 2]]
        i += 3
    for name in SCALARS:
        assert t[i] == name, line
        got[name] = int(t[i + 1])
        i += 2
    return got


@pytest.fixture(scope="module")
def check_run(tmp_path_factory, golden_dir):
    from echoglad_amd import build
    with open(os.path.join(golden_dir, "topo_tables.json")) as f:
        gold = json.load(f)["configs"]
    tmp = tmp_path_factory.mktemp("topo_tables")
    cfg_file = tmp / "configs.txt"
    with open(cfg_file, "w") as f:
        for g in gold:
            deg = HierTopology(_spec(g["args"])).degree()
            f.write(" ".join(map(str, [*g["args"], len(deg), *deg.tolist()])) + "\n")
    lib = build.build(extra_flags=SAN + ["-fno-gpu-sanitize"], variant="asan")          # device code unsanitized (not offered here)
    exe = tmp / "topo_tables_check"
    cmd = [CLANG, *SAN, "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-Wno-unknown-attributes", "-Wno-unknown-pragmas",
           os.path.join(ROOT, "tests", "native", "topo_tables_check.cpp"), "-o", str(exe),
           str(lib), f"-Wl,-rpath,{os.path.dirname(lib)}", "-Wl,-rpath,/opt/rocm/lib"]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1:protect_shadow_gap=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([str(exe), str(cfg_file)], capture_output=True, text=True, env=env, timeout=300)
    return gold, r


def test_tables_are_clean_under_asan_and_ubsan_and_keep_their_invariants(check_run):
    gold, r = check_run
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert f"topo_tables_check: 0 failure(s) over {len(gold)} configurations" in r.stdout, r.stdout[-3000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-2000:]


def test_tables_equal_the_recorded_ones(check_run):
    gold, r = check_run
    got = [_parse(ln) for ln in r.stdout.splitlines() if ln.startswith("cfg ")]
    assert [g["args"] for g in got] == [g["args"] for g in gold]
    for want, have in zip(gold, got):
        assert have == want, (want["args"], [k for k in want if want[k] != have[k]])
