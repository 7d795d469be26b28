"""What every wrapper of this package shares: the call into the C-ABI library, the argument checker and the scratch cache."""
from __future__ import annotations

import ctypes as ct
import functools
from typing import Optional

import torch

from .. import _lib

C = 128
_Tensor = torch.Tensor


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else ct.c_void_p(t.data_ptr())


def _stream():
    """The caller's current stream on the current device, as a raw ABI call passes it (`raw` appends it by itself)."""
    return ct.c_void_p(torch.cuda.current_stream().cuda_stream)


def _seed(value) -> int:
    """A dropout seed as the uint64_t the kernels hash with."""
    return int(value) & 0xFFFFFFFFFFFFFFFF


# ---------------------------------------------------------------------------
# the call: entry point by name, tensors as addresses, the current stream last
# ---------------------------------------------------------------------------
_entries = {}           # name -> (ctypes function, which of the caller's arguments are addresses, the stream is appended)


def _resolve(name: str):
    try:
        fn = getattr(_lib.load(), name)
    except AttributeError:
        raise RuntimeError(f"{_lib.LIB_PATH} does not export {name}: rebuild the library (there is no fallback path)") from None
    takes_stream = name in _lib.TAKES_STREAM
    argtypes = _lib.SIGNATURES[name][1]
    pointers = tuple(t is ct.c_void_p for t in (argtypes[:-1] if takes_stream else argtypes))
    entry = _entries[name] = (fn, pointers, takes_stream)
    return entry


def _invoke(name: str, args: tuple):
    fn, pointers, takes_stream = _entries.get(name) or _resolve(name)
    if len(args) != len(pointers):
        raise RuntimeError(f"{name} takes {len(pointers)} arguments{' and the stream' if takes_stream else ''}, got {len(args)}")
    argv = [a.data_ptr() if (p and isinstance(a, _Tensor)) else a for a, p in zip(args, pointers)]
    if takes_stream:
        argv.append(torch.cuda.current_stream().cuda_stream)
    try:
        return fn(*argv)
    except ct.ArgumentError as e:           # "argument N: ...": a value the declared C type does not take (numpy scalars, tensors as scalars)
        raise RuntimeError(f"{name}: {e} (pointer slots take tensors, None, ctypes arrays and byref(); scalar slots take Python "
                           "bool, int and float)") from None


def raw(name: str, *args):
    """``name(*args)`` of the library -> its return value.  In a pointer slot a tensor goes as its address (None: a null pointer;
    ctypes arrays and byref(...) pass as they are); Python bool, int and float are converted by the signature _lib read from the
    header, anything else in a scalar slot is a RuntimeError that names the entry point and the argument's position.  Where the
    declaration ends in ``eg_stream_t`` the caller's current stream is appended.  The entry point is looked up once per name; the
    conversion is one flat loop.  Nothing is checked here but the number of arguments: shapes, dtypes and devices are the
    wrappers' business (`_check`, `_check_rows`)."""
    return _invoke(name, args)


def call(name: str, *args) -> None:
    """`raw` for an entry point that returns a status: anything but EG_OK raises with the entry point's name and eg_last_error()."""
    rc = _invoke(name, args)
    if rc != _lib.EG_OK:
        _lib.check(rc, name)


# ---------------------------------------------------------------------------
# the argument checker
# ---------------------------------------------------------------------------
def _shape_is(got, want) -> bool:
    return got == want or (len(got) == len(want) and all(w is None or w == g for w, g in zip(want, got)))


def _check(t: torch.Tensor, name: str, shape=None, dtype=torch.float32, numel: Optional[int] = None, device=None) -> None:
    """``t`` is a CUDA tensor of `dtype`, contiguous, of `shape` (None in it: any extent) and / or with `numel` elements, on
    `device` if one is given; a RuntimeError that names the argument otherwise."""
    if not t.is_cuda:
        raise RuntimeError(f"{name} must be a CUDA (ROCm) tensor: the HIP path has no CPU fallback")
    if t.dtype != dtype or not t.is_contiguous() or (numel is not None and t.numel() != numel) or \
            (shape is not None and not _shape_is(t.shape, shape)):
        want = "" if shape is None else " [" + ", ".join("*" if w is None else str(w) for w in shape) + "]"
        want += "" if numel is None else f" with {numel} elements"
        raise RuntimeError(f"{name} must be a contiguous CUDA {str(dtype).replace('torch.', '')} tensor{want}, "
                           f"got {tuple(t.shape)} {t.dtype}")
    if device is not None and t.device != device:
        raise RuntimeError(f"{name} is on {t.device}, expected {device}")


def _on_current_device(t: torch.Tensor, name: str) -> None:
    """The kernels launch on the device that is current for the calling thread: a tensor on another one is an error, not a
    cross-device launch."""
    if t.get_device() != torch.cuda.current_device():
        raise RuntimeError(f"{name} is on {t.device} but the current device is cuda:{torch.cuda.current_device()} "
                           "(kernels launch on the current device: use torch.cuda.device(tensor.device))")


def _check_rows(t: Optional[torch.Tensor], name: str, rows: Optional[int] = None, cols: int = C, optional: bool = False) -> None:
    """float32 [rows, cols] (rows None: any) on the current device; optional: None passes.  Every node array goes through here,
    also where it reaches the library as an offset row pointer (_frame_rows_ptr) or inside a struct (_lower_sums).  Vectors and
    parameters (`_check_vec`, plain `_check`) are not tested for their device, and never were."""
    if t is not None or not optional:
        _check(t, name, (rows, cols))
        if t.get_device() != torch.cuda.current_device():
            _on_current_device(t, name)


def _check_vec(t: Optional[torch.Tensor], name: str, n: int) -> None:
    """float32 with n elements in any shape; None passes (an optional argument)."""
    if t is not None:
        _check(t, name, numel=n)


# ---------------------------------------------------------------------------
# the scratch cache: the C side never allocates
# ---------------------------------------------------------------------------
_SCRATCH_MIN = {"heatmap": 1 << 16}     # bytes a buffer of that kind is never smaller than
_scratch_buffers = {}


def _scratch(kind: str, device, nbytes: int) -> torch.Tensor:
    """The uint8 buffer of one kind (a kind's buffer is never another kind's: captured graphs hold the addresses) for this device
    and the current stream, `nbytes` or more; grown, never shrunk."""
    key = (kind, torch.device(device), torch.cuda.current_stream().cuda_stream)
    buf = _scratch_buffers.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = _scratch_buffers[key] = torch.empty(max(nbytes, _SCRATCH_MIN.get(kind, 0)), dtype=torch.uint8, device=device)
    return buf


@functools.lru_cache(maxsize=None)
def _fixed_bytes(name: str) -> int:
    return int(raw(name))


def _workspace(device) -> torch.Tensor:
    """The reduction workspace (eg_workspace_bytes)."""
    return _scratch("reduce", device, _fixed_bytes("eg_workspace_bytes"))


def _cls_workspace(device) -> torch.Tensor:
    """The classifier heads' train-mode workspace (eg_classifier_train_workspace_bytes)."""
    return _scratch("heads", device, _fixed_bytes("eg_classifier_train_workspace_bytes"))


def _level_arrays(levels):
    n = len(levels)
    if not 1 <= n <= 16:
        raise RuntimeError("1..16 levels supported")
    start = (ct.c_int * n)(*[int(s) for s, _ in levels])
    side = (ct.c_int * n)(*[int(p) for _, p in levels])
    return start, side, n


def _hm_workspace(device, entry: str, batch: int, side, n: int) -> torch.Tensor:
    """The losses' workspace, sized by eg_heatmap_workspace_bytes or eg_criteria_workspace_bytes (`entry`) for these levels."""
    return _scratch("heatmap", device, int(raw(entry, batch, side, n)))
