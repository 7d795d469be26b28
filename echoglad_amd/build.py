"""Build the gfx950 C-ABI library in-tree with hipcc (no torch headers, no cmake).

    python -m echoglad_amd.build [--force] [--verbose]

The shared object lands in echoglad_amd/lib/libechoglad_hip.so so it travels with
the repository snapshot to the GPU box."""
from __future__ import annotations

import os
import shutil
import subprocess
import sys
from pathlib import Path

PKG = Path(__file__).resolve().parent
CSRC = PKG / "csrc"
LIBDIR = PKG / "lib"
LIBNAME = "libechoglad_hip.so"
SOURCES = ["graph.hip", "topo_tables.hip", "gcn_layer.hip", "gcn_layer_ps.hip", "gcn_layer_ps_split.hip", "gcn_layer_ps_fold_split.hip", "conn.hip", "classifier.hip", "tail_heads.hip", "train.hip", "bn_act_tiles.hip", "cls_train.hip", "coord.hip", "coord_mlp.hip", "heatmap.hip", "heatmap_render.hip", "pack.hip", "pack_train.hip", "conn_rows.hip", "pool.hip", "adam.hip", "optim.hip", "metrics.hip", "labels.hip", "frame_prep.hip", "frontend.hip", "frontend_train.hip", "embedder.hip", "pyramid_conv.hip", "pyramid_train.hip"]
ARCH = "gfx950"
# per-file flags and extra dependencies, and objects whose device code must hold no packed fp32 vector instruction.
# gcn_layer_ps_split.hip (the bf16-path instantiations of the layer kernel, gcn_layer_ps.hip included) is compiled without them:
# beside bf16 MFMAs they return wrong results now and then (see there).  The feature goes through -Xclang, which the driver cannot
# scope to the device side (-Xarch_device refuses it, and there is no -m option for it); the host compilation ignores it.  A flag
# that stopped taking effect must not go unnoticed: the object is disassembled and checked below.
# gcn_layer_ps_fold_split.hip (the bf16 bodies of the folded last layer + heads, v_mfma_f32_16x16x32_bf16) likewise.
_NO_PACKED = ["-Xclang", "-target-feature", "-Xclang", "-packed-fp32-ops"]
FILE_FLAGS = {"gcn_layer_ps_split.hip": _NO_PACKED, "gcn_layer_ps_fold_split.hip": _NO_PACKED}
FILE_DEPS = {"gcn_layer_ps_split.hip": ["gcn_layer_ps.hip"], "gcn_layer_ps_fold_split.hip": ["gcn_layer_ps.hip"]}
NO_PACKED_FP32 = ("gcn_layer_ps_split.hip",)
NO_PACKED_FP32_16X16 = ("gcn_layer_ps_fold_split.hip",)
LLVM_BIN = Path("/opt/rocm/lib/llvm/bin")


def device_disassembly(binary: Path) -> str:
    """llvm-objdump -d of every gfx950 code object in `binary` (an object file or the library): section .hip_fatbin holds one
    clang offload bundle per translation unit."""
    import re
    import tempfile
    with tempfile.TemporaryDirectory(prefix="eg_build_") as tmp:
        fat = Path(tmp) / "fatbin"
        subprocess.run(["objcopy", "-O", "binary", "--only-section=.hip_fatbin", str(binary), str(fat)], check=True)
        blob = fat.read_bytes()
        starts = [m.start() for m in re.finditer(re.escape(b"__CLANG_OFFLOAD_BUNDLE__"), blob)]
        text = []
        for i, a in enumerate(starts):
            piece, out = Path(tmp) / f"bundle{i}", Path(tmp) / f"{ARCH}_{i}.co"
            piece.write_bytes(blob[a:starts[i + 1] if i + 1 < len(starts) else len(blob)])
            r = subprocess.run([str(LLVM_BIN / "clang-offload-bundler"), "--unbundle", "--type=o", f"--input={piece}",
                                f"--targets=hipv4-amdgcn-amd-amdhsa--{ARCH}", f"--output={out}"], capture_output=True)
            if r.returncode == 0 and out.exists() and out.stat().st_size > 0:
                text.append(subprocess.run([str(LLVM_BIN / "llvm-objdump"), "-d", str(out)], check=True, capture_output=True, text=True).stdout)
    return "\n".join(text)


def packed_fp32_census(binary: Path):
    """(bf16 MFMAs, packed fp32 vector instructions) in the device code of `binary`."""
    import re
    text = device_disassembly(binary)
    return len(re.findall(r"\bv_mfma_f32_32x32x16_bf16\b", text)), len(re.findall(r"\bv_pk_\w+_f32\b", text))


def fold_split_census(binary: Path):
    """(v_mfma_f32_16x16x32_bf16, packed fp32 vector instructions, kernels with scratch) in the device code of `binary`."""
    import re
    text = device_disassembly(binary)
    return (len(re.findall(r"\bv_mfma_f32_16x16x32_bf16\b", text)), len(re.findall(r"\bv_pk_\w+_f32\b", text)),
            len(re.findall(r"\bscratch_(?:load|store)\w*\b", text)))


def hipcc() -> str:
    for cand in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found; the HIP extension cannot be built")


def lib_path() -> Path:
    return LIBDIR / LIBNAME


def _stale(target: Path, deps) -> bool:
    if not target.exists():
        return True
    t = target.stat().st_mtime
    return any(Path(d).stat().st_mtime > t for d in deps)


def build(force: bool = False, verbose: bool = False, extra_flags=(), variant: str = "") -> Path:
    """variant != "": an experiment build (extra -D flags) written to lib/libechoglad_hip.<variant>.so;
    select it at run time with ECHOGLAD_LIB=<path>."""
    LIBDIR.mkdir(exist_ok=True)
    objdir = LIBDIR / ("obj" + ("_" + variant if variant else ""))
    objdir.mkdir(exist_ok=True)
    headers = list(CSRC.glob("*.h")) + [PKG.parent / "include" / "echoglad_hip.h"]
    cc = hipcc()
    # atomic optimizer off: it turns the single-lane queue claims into "atomic + wait + readfirstlane", which makes
    # every claim a synchronous memory round trip in front of the tile's loads
    flags = [f"--offload-arch={ARCH}", "-O3", "-fPIC", "-std=c++17", "-Wall", "-Wno-unused-function",
             "-mllvm", "-amdgpu-atomic-optimizer-strategy=None", *extra_flags]
    if verbose:
        flags.append("-Rpass-analysis=kernel-resource-usage")
    objs = []
    procs = []
    for src in SOURCES:
        s = CSRC / src
        if not s.exists():
            continue
        o = objdir / (s.stem + ".o")
        objs.append(o)
        if force or _stale(o, [s] + [CSRC / d for d in FILE_DEPS.get(src, [])] + headers):
            cmd = [cc, *flags, *FILE_FLAGS.get(src, []), "-c", str(s), "-o", str(o)]
            if verbose:
                print(" ".join(cmd), flush=True)
            procs.append((src, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)))
    for src, p in procs:
        out, _ = p.communicate()
        if verbose or p.returncode != 0:
            print(out, flush=True)
        if p.returncode != 0:
            raise RuntimeError(f"hipcc failed on {src}")
        if src in NO_PACKED_FP32:
            o = objdir / (Path(src).stem + ".o")
            n_mfma, n_packed = packed_fp32_census(o)
            if n_mfma == 0 or n_packed != 0:
                o.unlink()
                raise RuntimeError(f"{src}: {n_mfma} bf16 MFMAs and {n_packed} packed fp32 instructions in the device code; "
                                   "expected some and none (packed fp32 instructions beside bf16 MFMAs return wrong results)")
        if src in NO_PACKED_FP32_16X16:
            o = objdir / (Path(src).stem + ".o")
            n_mfma, n_packed, _ = fold_split_census(o)
            if n_mfma == 0 or n_packed != 0:
                o.unlink()
                raise RuntimeError(f"{src}: {n_mfma} 16x16x32 bf16 MFMAs and {n_packed} packed fp32 instructions in the device code; "
                                   "expected some and none (packed fp32 instructions beside bf16 MFMAs return wrong results)")
    target = lib_path() if not variant else LIBDIR / f"libechoglad_hip.{variant}.so"
    if force or _stale(target, objs):
        cmd = [cc, f"--offload-arch={ARCH}", "-shared", "-fPIC", "-o", str(target), *map(str, objs)]
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.run(cmd, check=True)
    return target


if __name__ == "__main__":
    extra = [a for a in sys.argv[1:] if a.startswith("-D")]
    if "--" in sys.argv:                                   # everything after "--" goes to hipcc verbatim (experiments)
        extra += sys.argv[sys.argv.index("--") + 1:]
    var = [a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--variant=")]
    p = build(force="--force" in sys.argv, verbose="--verbose" in sys.argv, extra_flags=extra,
              variant=var[0] if var else "")
    print(p)
