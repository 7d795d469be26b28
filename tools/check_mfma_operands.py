"""Lint over a kernel's assembly (hipcc -S --cuda-device-only): the operand-register rule of DESIGN_NOTES 5.14 for the bf16 chain of
the split layer kernel (tile.h mfma_rowblock_bf16x6) and of the folded last layer's bf16 body (v_mfma_f32_16x16x32_bf16, tile.h
fs_step; gcn_layer_ps_fold_split.hip).  Walks one function straight through and reports every vector-ALU, LDS-return or
vector-memory-return write (global_load / buffer_load / scratch_load destinations: the streamed lo fragments land in operand
registers) to a register that an earlier bf16 v_mfma read as its A / B operand with no guard (`s_nop 15`, which in these kernels
only the guard emits, behind its accumulator read) in between.  Straight-line only: the tile loop's back edge is covered by the
guard that ends every chain.
usage: hipcc --offload-arch=gfx950 -O3 -std=c++17 -mllvm -amdgpu-atomic-optimizer-strategy=None --cuda-device-only -S \\
           echoglad_amd/csrc/gcn_layer_ps_split.hip -o /tmp/split.s && python tools/check_mfma_operands.py /tmp/split.s [function substring]
Exit code 1 if anything is found.  (Shipped form: 96 MFMAs, 16 guards, 0 findings per split instantiation; 384 MFMAs and 32 guards for the folded body with the
residual, 192 and 16 without.)"""
import re
import sys


def regs(tok):
    m = re.match(r"v\[(\d+):(\d+)\]", tok)
    if m:
        return set(range(int(m.group(1)), int(m.group(2)) + 1))
    m = re.match(r"v(\d+)$", tok)
    return {int(m.group(1))} if m else set()


def functions(text, want):
    out, cur = {}, None
    for line in text.splitlines():
        m = re.match(r"^(\w+):", line)
        if m and not line.startswith(".L"):
            cur = m.group(1) if want in m.group(1) else None
            if cur:
                out[cur] = []
        elif cur is not None:
            out[cur].append(line)
            if line.strip().startswith("s_endpgm"):
                cur = None
    return out


def check(lines):
    last_read, guards, mfmas, found = {}, 0, 0, []
    for i, line in enumerate(lines):
        s = line.split(";")[0].strip()
        m = re.match(r"(\S+)\s+(.*)", s)
        if s.startswith("s_nop 15"):
            guards += 1
        if not m:
            continue
        op, toks = m.group(1), [t.strip() for t in m.group(2).split(",")]
        if op.startswith(("v_mfma_f32_32x32x16_bf16", "v_mfma_f32_16x16x32_bf16")):
            mfmas += 1
            for t in toks[1:3]:
                for r in regs(t):
                    last_read[r] = (i, guards)
        elif (op.startswith("v_") and not op.startswith(("v_cmp", "v_readfirstlane", "v_readlane", "v_nop", "v_mfma"))) or op.startswith(("ds_read", "global_load", "buffer_load", "scratch_load")):
            for r in regs(toks[0]):
                if r in last_read:
                    j, g = last_read.pop(r)
                    if guards == g:
                        found.append(f"line {i}: {s[:80]}  rewrites v{r}, read by the MFMA {i - j} lines before, no guard between")
    return mfmas, guards, found


if __name__ == "__main__":
    want = sys.argv[2] if len(sys.argv) > 2 else "k_gcn_layer_ps"
    bad = 0
    for name, lines in functions(open(sys.argv[1]).read(), want).items():
        mfmas, guards, found = check(lines)
        if mfmas:
            print(f"{name[:60]}: {mfmas} bf16 MFMAs, {guards} guards, {len(found)} finding(s)")
            print("\n".join(found))
            bad += len(found)
    sys.exit(1 if bad else 0)
