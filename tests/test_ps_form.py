"""CPU: which form of the producer/consumer layer kernel a call gets (csrc/ps_form.h: ps_choose_form), over EVERY combination of
the function's inputs.  tests/native/ps_form_check.cpp (a program of its own, AddressSanitizer + UndefinedBehaviorSanitizer, no
library) prints one result per combination; they are compared with tests/golden/ps_forms.json, recorded from the line-for-line
extraction of the conditions eg_launch_layer_ps had until then.  The program itself checks that every form chosen is one of
PS_FORMS and that each of the 18 is chosen somewhere; the rows of the routing table are spelled out below."""
import json
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
SAN = ["-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-g", "-O1"]
NONE, X_ITSELF, OWN = 0, 1, 2              # residual
HEADS, FOLDED = 1, 2                       # heads
INCOMPLETE, COMPLETE = 1, 2                # lower


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    exe = tmp_path_factory.mktemp("ps_form") / "ps_form_check"
    subprocess.run([CLANG, *SAN, "-std=c++17", os.path.join(ROOT, "tests", "native", "ps_form_check.cpp"), "-o", str(exe)],
                   check=True, capture_output=True, text=True)
    env = dict(os.environ, ASAN_OPTIONS="abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    return subprocess.run([str(exe)], capture_output=True, env=env, timeout=300)


def parse(stdout):
    """-> (fields [(name, radix)], results [text], codes: one per combination, the last field running fastest)"""
    head, _, body = stdout.partition(b"\n")
    assert head.startswith(b"fields "), head[:200]
    fields = [(f.split(":")[0], int(f.split(":")[1])) for f in head.decode().split()[1:]]
    n = int(np.prod([r for _, r in fields]))
    lines = np.frombuffer(body, dtype=np.uint8, count=3 * n).reshape(n, 3)
    assert (lines[:, 2] == 10).all() and (lines[:, :2] >= 48).all() and (lines[:, :2] <= 57).all()
    codes = (lines[:, 0] - 48) * 10 + (lines[:, 1] - 48)
    tail = body[3 * n:].decode().splitlines()
    results = [ln.split(" ", 2)[2] for ln in tail if ln.startswith("result ")]
    assert [int(ln.split()[1]) for ln in tail if ln.startswith("result ")] == list(range(len(results)))
    assert int(codes.max()) == len(results) - 1
    return fields, results, codes, tail[-1]


@pytest.fixture(scope="module")
def table(run):
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-3000:]
    return parse(run.stdout)


def test_clean_under_asan_and_ubsan_every_form_listed_and_reached(run, table):
    assert b"runtime error" not in run.stderr and b"AddressSanitizer" not in run.stderr, run.stderr[-2000:]
    fields, results, codes, last = table
    assert last == f"ps_form_check: {len(codes)} combinations, 0 with a form PS_FORMS does not list, 0 of 18 forms never chosen"
    assert len({tuple(r.split()[1:7]) for r in results if r.startswith("F ")}) == 18


def test_results_equal_the_recorded_ones(table, golden_dir):
    fields, results, codes, _ = table
    with open(os.path.join(golden_dir, "ps_forms.json")) as f:
        gold = json.load(f)
    assert [list(f) for f in fields] == gold["fields"]
    runs = np.array(gold["runs"]).reshape(-1, 2)                     # (index into gold["results"], count)
    want = np.repeat(runs[:, 0], runs[:, 1])
    assert len(want) == len(codes)
    # (the program numbers the results in the order of their first appearance; compare texts, not numbers)
    have_text, want_text = np.array(results, dtype=object)[codes], np.array(gold["results"], dtype=object)[want]
    bad = np.flatnonzero(have_text != want_text)
    assert len(bad) == 0, (len(bad), int(bad[0]), have_text[bad[0]], want_text[bad[0]])


def test_the_routing_table(table):
    """The rows of eg_launch_layer_ps's if / else chain as it stood, form = (CLS, JK, MODE, DIAG, FOLD, SPLIT)."""
    fields, results, codes, _ = table
    names = [n for n, _ in fields]
    grid = codes.reshape([r for _, r in fields])
    is_form = np.array([r.startswith("F ") for r in results])
    form_of = [tuple(int(v) for v in r.split()[1:7]) if r.startswith("F ") else None for r in results]

    def chosen(**fixed):
        """the distinct results of the combinations with these inputs, on a topology handle"""
        idx = tuple(fixed.get(n, slice(None)) for n in names)
        return {results[k] for k in np.unique(grid[idx])}

    def forms(**fixed):
        """the forms launched with these inputs (on the handles that take the call at all)"""
        idx = tuple(fixed.get(n, slice(None)) for n in names)
        got = np.unique(grid[idx])
        assert is_form[got].any(), fixed
        return {form_of[k] for k in got if is_form[k]}

    impl = names.index("layer_impl")
    assert fields[impl][1] == 3                                       # -1, 0, 1 in this order
    for d in (0, 1):
        plain = dict(topo=1, hybrid=d, lower=NONE, agg_out=0, stats_partial=0, kin=0, kout=0, heads=NONE, jk_in=0, jk_out=0)
        assert forms(**{**plain, "stats_partial": 1, "residual": NONE}) == {(0, 0, 1, d, 0, 0)}                # train
        assert forms(**{**plain, "stats_partial": 1, "agg_out": 1, "kin": 1, "residual": X_ITSELF}) == {(0, 0, 1, d, 0, 0)}
        assert forms(**{**plain, "residual": OWN, "lower": COMPLETE}) == {(0, 0, 3, d, 0, 0)}                  # own residual + lower
        assert forms(**{**plain, "residual": OWN}) == {(0, 0, 2, d, 0, 0)}                                     # own residual
        for res, fold in ((X_ITSELF, 1), (NONE, 2)):                                                         # fold
            for kin in (0, 1):
                assert forms(**{**plain, "heads": FOLDED, "residual": res, "kin": kin}) == {(1, 0, 0, d, fold, 0)}
        for res in (NONE, X_ITSELF):
            for kin in (0, 1):
                assert forms(**{**plain, "heads": HEADS, "residual": res, "kin": kin}) == {(1, 0, 0, d, 0, 0)}     # heads
                for kout in (0, 1):                                                                          # plain, also chained
                    for split in (0, 1):
                        assert forms(**{**plain, "residual": res, "kin": kin, "kout": kout, "layer_split": split}) == {(0, 0, 0, d, 0, split)}
    for res in (NONE, X_ITSELF):
        for kin in (0, 1):
            jk = dict(topo=1, hybrid=0, lower=NONE, agg_out=0, stats_partial=0, kin=kin, residual=res, jk_in=1)
            assert forms(**jk, heads=HEADS, kout=0, jk_out=0) == {(1, 1, 0, 0, 0, 0)}                          # heads on the running maximum
            for kout in (0, 1):
                assert forms(**jk, heads=NONE, kout=kout, jk_out=1) == {(0, 1, 0, 0, 0, 0)}                    # plain with jk_in
    # diag && jk: unsupported, whatever else is asked for (argument errors come first)
    got = chosen(topo=1, hybrid=1, jk_in=1)
    assert "U" in got and not any(r.startswith(("F ", "OK")) for r in got)
    assert chosen(topo=1, hybrid=1, jk_in=1, jk_out=1, heads=NONE, lower=NONE, agg_out=0, stats_partial=0) == {"U"}
    assert chosen(topo=1, hybrid=1, jk_in=1, jk_out=0, heads=HEADS, lower=NONE, agg_out=0, stats_partial=0, residual=NONE) == {"U"}
    # lower without an own residual: EG_ERR_ARG
    for res in (NONE, X_ITSELF):
        for lower in (INCOMPLETE, COMPLETE):
            assert chosen(topo=1, residual=res, lower=lower) == {"A the lower layer's sums go with the dX launch (a residual tensor of its own)"}
    assert chosen(topo=1, residual=OWN, lower=INCOMPLETE) == {"A incomplete LowerSums"}
    # fold with relu, scale, shift or jk: EG_ERR_ARG (on the handles that take the heads, with tiles to run)
    takes = dict(topo=1, kids=1, hybrid=0, no_tiles=0, lower=NONE, agg_out=0, stats_partial=0, kout=0, heads=FOLDED, jk_out=0)
    msg = "A the folded heads take no running maximum, ReLU, scale or shift"
    for res in (NONE, X_ITSELF):
        for extra in ("relu", "scale", "shift", "jk_in"):
            assert chosen(**takes, residual=res, **{extra: 1}) == {msg}
        assert msg not in chosen(**takes, residual=res, relu=0, scale=0, shift=0, jk_in=0)
    # not a topology handle: the other kernel, always
    assert chosen(topo=0) == {"U"}
    # no tiles: EG_OK without a launch wherever a form would have been chosen or the later checks would have refused
    assert chosen(topo=1, no_tiles=1, kids=1, hybrid=0, residual=NONE, lower=NONE, agg_out=0, stats_partial=0, kin=0, kout=0,
                  heads=NONE, jk_in=0, jk_out=0, layer_impl=0) == {"OK"}
