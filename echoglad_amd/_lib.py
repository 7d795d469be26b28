"""ctypes binding of the C-ABI library (include/echoglad_hip.h).

The ctypes signature of every entry point is read from the header when this module is imported: the header is the
ABI contract, and a table written out a second time by hand can disagree with it in a type or in the order of two
arguments without anything noticing.

There is no CPU fallback: if the shared object is missing or does not load,
``load()`` raises and every op that needs it fails loudly."""
from __future__ import annotations

import ctypes as ct
import os
import re
from pathlib import Path
from typing import Dict, List, Optional, Tuple

_PKG = Path(__file__).resolve().parent
LIB_PATH = Path(os.environ.get("ECHOGLAD_LIB", _PKG / "lib" / "libechoglad_hip.so"))
HEADER_PATH = _PKG.parent / "include" / "echoglad_hip.h"

EG_OK, EG_ERR_ARG, EG_ERR_UNSUPPORTED, EG_ERR_HIP = 0, -1, -2, -3
# EG_ABI_VERSION of the include/echoglad_hip.h that the structures below and the wrappers' argument order were written for
# (the header's version history says what each number added; 155: eg_sgd_step, eg_rmsprop_step; 156: eg_heatmap_render;
# 157: eg_conn_rows_plan / _workspace_bytes / _fwd / _bwd)
ABI_VERSION = 157

_lib: Optional[ct.CDLL] = None

_p = ct.c_void_p


class ClsTrainParams(ct.Structure):
    """eg_cls_train_params of include/echoglad_hip.h (stacked parameters of the 4 classifier heads, train mode)."""
    _fields_ = [(n, _p) for n in ("w1", "b1", "gamma1", "beta1", "w2", "b2", "gamma2", "beta2", "w3", "b3",
                                  "running_mean1", "running_var1", "running_mean2", "running_var2")] + \
               [(n, ct.c_float) for n in ("eps1", "eps2", "momentum1", "momentum2", "p1", "p2")] + \
               [("seed1", ct.c_uint64), ("seed2", ct.c_uint64)]


class LowerSums(ct.Structure):
    """eg_lower_sums: the layer below the one whose dX launch takes its BatchNorm-backward sums (eg_gcn_layer_bwd_lower)."""
    _fields_ = [("z", _p), ("bn", _p), ("relu", ct.c_int), ("dropout_p", ct.c_float), ("seed", ct.c_uint64),
                ("row_hi", ct.c_int64), ("tile_scratch", _p), ("sums_out", _p)]


class GivenSums(ct.Structure):
    """eg_given_sums: sums of THIS layer that somebody else has taken already (+ the bilinear backward's later additions)."""
    _fields_ = [("sums", _p), ("frames", ct.c_int), ("row_lo", ct.c_int64), ("n_valid", ct.c_int64), ("taps", _p)]


# ---------------------------------------------------------------------------
# the header -> name -> (restype, argtypes)
# ---------------------------------------------------------------------------
_SCALARS = {"int": ct.c_int, "int64_t": ct.c_int64, "uint64_t": ct.c_uint64, "float": ct.c_float, "size_t": ct.c_size_t,
            "unsigned": ct.c_uint}
_STRUCTS = {"eg_cls_train_params": ClsTrainParams, "eg_lower_sums": LowerSums, "eg_given_sums": GivenSums}
# what a pointer that is passed as an address (c_void_p takes tensors' addresses, ctypes arrays and byref(...)) may point to
_POINTEES = set(_SCALARS) | {"void", "char", "unsigned char", "uint8_t", "double", "eg_graph", "eg_adam_tensor", "eg_sgd_tensor", "eg_rmsprop_tensor"}
_DECLARATION = re.compile(r"([A-Za-z_][\w \t\n\*]*?)\b(eg_[a-z0-9_]+)\s*\(([^()]*)\)\s*;")


def _ctype(text: str, entry: str, is_param: bool):
    """The ctypes type of one C type as the header spells it (a parameter together with its name, or a return type)."""
    if "[" in text or "]" in text:
        raise RuntimeError(f"{entry}: array parameter '{' '.join(text.split())}' has no ctypes mapping: declare it as a pointer")
    words = [w for w in text.replace("*", " * ").split() if w != "const"]
    stars = words.count("*")
    words = [w for w in words if w != "*"]
    if is_param and len(words) > 1:
        words = words[:-1]                                  # the parameter's name
    base = " ".join(words)
    if stars == 0 and base in _SCALARS:
        return _SCALARS[base]
    if stars == 0 and base == "eg_stream_t":
        return ct.c_void_p
    if stars == 1 and base in _STRUCTS:
        return ct.POINTER(_STRUCTS[base])
    if stars == 1 and base == "char" and not is_param:
        return ct.c_char_p
    if stars >= 1 and base in _POINTEES and is_param:
        return ct.c_void_p
    raise RuntimeError(f"{entry}: no ctypes mapping for '{' '.join(text.split())}' (echoglad_amd/_lib.py reads its signatures "
                       f"from {HEADER_PATH.name})")


def parse_header(text: str) -> Dict[str, Tuple[object, list, bool]]:
    """name -> (restype, argtypes, last parameter is the stream) of every function a C header in the style of
    include/echoglad_hip.h declares.  A type with no ctypes mapping raises with the entry point's name."""
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    text = re.sub(r"^[ \t]*#[^\n]*", "", text, flags=re.M)                       # preprocessor lines
    text = text.replace('extern "C" {', "")
    text = re.sub(r"typedef\s+struct\s+\w+\s*\{[^{}]*\}\s*\w+\s*;", "", text)   # field layouts: the ct.Structure classes
    table = {}
    for m in _DECLARATION.finditer(text):
        ret, name, params = m.group(1), m.group(2), m.group(3).strip()
        params = [] if params in ("", "void") else [p.strip() for p in params.split(",")]
        if name in table:
            raise RuntimeError(f"{name} is declared twice")
        table[name] = (_ctype(ret, name, False), [_ctype(p, name, True) for p in params],
                       bool(params) and params[-1].split()[0] == "eg_stream_t")
    return table


def _read_header() -> str:
    try:
        return HEADER_PATH.read_text()
    except OSError as e:
        raise RuntimeError(f"{HEADER_PATH} cannot be read ({e}): the binding takes every entry point's signature from it") from e


_PARSED = parse_header(_read_header())
# name -> (restype, argtypes) of every symbol the header declares
SIGNATURES: Dict[str, tuple] = {name: (res, args) for name, (res, args, _) in _PARSED.items()}
TAKES_STREAM = frozenset(name for name, d in _PARSED.items() if d[2])        # ... and those whose last argument is the stream


def header_symbols() -> List[str]:
    """Every function name declared in include/echoglad_hip.h."""
    return sorted(SIGNATURES)


def load() -> ct.CDLL:
    """Load the library (after torch, so both share one HIP runtime instance)."""
    global _lib
    if _lib is not None:
        return _lib
    import torch  # noqa: F401  — must come first: libamdhip64.so.7 resolves to the copy torch loaded
    if not LIB_PATH.exists():
        raise RuntimeError(
            f"{LIB_PATH} is missing: build the HIP extension first "
            "(python -m echoglad_amd.build, or __graft_entry__.build()). There is no CPU fallback.")
    lib = ct.CDLL(str(LIB_PATH), mode=ct.RTLD_GLOBAL if hasattr(ct, "RTLD_GLOBAL") else 0)
    # a library built from other sources than this binding would take the calls below with shifted arguments: refuse it
    try:
        lib.eg_version.restype, lib.eg_version.argtypes = SIGNATURES["eg_version"]
        got = int(lib.eg_version())
    except AttributeError:
        got = None
    if got != ABI_VERSION:
        raise RuntimeError(f"{LIB_PATH} reports eg_version() = {got}, this binding is written for ABI {ABI_VERSION}: rebuild the "
                           "library (python -m echoglad_amd.build --force) or point ECHOGLAD_LIB at a matching build")
    for name, (res, args) in SIGNATURES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError:
            continue          # checked by check_exports(); ops fail on use
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check_exports() -> List[str]:
    """Names declared in the header that the library does not export."""
    lib = load()
    return [n for n in header_symbols() if not hasattr(lib, n)]


def last_error() -> str:
    msg = load().eg_last_error()
    return msg.decode() if msg else ""


def check(rc: int, what: str) -> None:
    if rc != EG_OK:
        kind = {EG_ERR_ARG: "bad argument", EG_ERR_UNSUPPORTED: "unsupported", EG_ERR_HIP: "HIP error"}.get(rc, str(rc))
        raise RuntimeError(f"{what} failed ({kind}): {last_error()}")
