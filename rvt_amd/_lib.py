"""ctypes binding of librvt_hip.so — the only compute path of this package.  Every type in it is derived from
include/rvt_hip.h (rvt_amd/_header.py); nothing here restates a prototype, a struct, a table row or an enumerator.

There is no PyTorch / CPU fallback: if the gfx950 library or a GPU is missing, every op raises.
The unit tests may install the CPU SIMT-emulator build of the same kernel sources through
``_install_test_library`` (tests/emu); that hook is never used by the package itself.
"""
from __future__ import annotations

import ctypes
import os
from typing import Optional

import numpy as np
import torch

from ._header import ENUMS, RECORDS as _RECORDS, SIGS as _SIGS, STRUCTS as _STRUCTS, bind as _bind     # enumerators; name -> argument types; structs; types onto a loaded library

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('RVT_HIP_LIB') or os.path.join(_HERE, 'librvt_hip.so')   # env: another BUILD of the same library

RVT_F32, RVT_BF16 = ENUMS['RVT_F32'], ENUMS['RVT_BF16']
_DT = {torch.float32: RVT_F32, torch.bfloat16: RVT_BF16}

_lib: Optional[ctypes.CDLL] = None
_is_emu = False

EXPORTS = sorted(_SIGS)


def load_library(path: str = LIB_PATH) -> ctypes.CDLL:
    """dlopen + bind every symbol of include/rvt_hip.h (no GPU needed to *load*)."""
    if not os.path.exists(path):
        raise RuntimeError(f'{path} not found: build it with `python -c "import __graft_entry__ as g; g.build()"` '
                           f'(rvt_amd/csrc/build.sh).  rvt_amd has no fallback compute path.')
    return _bind(ctypes.CDLL(path))


def get_lib() -> ctypes.CDLL:
    global _lib
    if _lib is None:
        lib = load_library()
        if not torch.cuda.is_available():
            raise RuntimeError('rvt_amd needs an AMD GPU (gfx950): torch.cuda.is_available() is False '
                               'and there is no CPU fallback.')
        _lib = lib
        from . import tuning
        tuning.push(lib)        # the caller's overrides (none = the production route) into the freshly loaded library
    return _lib


def _install_test_library(lib: Optional[ctypes.CDLL]) -> None:
    """TEST HOOK ONLY (tests/emu): route calls to the CPU SIMT-emulator build of the kernel sources."""
    global _lib, _is_emu
    _lib = lib
    _is_emu = bool(lib is not None and lib.rvt_is_emulator())
    if lib is not None:
        from . import tuning
        tuning.push(lib)


def is_emulator() -> bool:
    return _is_emu


def dtype_code(dt: torch.dtype) -> int:
    try:
        return _DT[dt]
    except KeyError:
        raise TypeError(f'rvt_amd kernels support float32 and bfloat16 activations, got {dt}') from None


def ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    if t is None:
        return None
    if not t.is_contiguous():
        raise ValueError('rvt_amd kernels need contiguous tensors')
    if not (t.is_cuda or _is_emu):
        raise RuntimeError('rvt_amd kernels need CUDA (ROCm) tensors; there is no CPU path')
    return t.data_ptr()


class _Stream(int):
    """hipStream_t handle (as an int for ctypes) that remembers the device it belongs to."""
    dev = -1


_raw_stream = getattr(torch._C, '_cuda_getCurrentRawStream', None)


def stream_of(t: torch.Tensor) -> Optional[int]:
    """Current HIP stream of the tensor's device.  Every entry point takes it as its LAST argument; call() uses the
    device it carries to make that device current for the launch (the C ABI has no device parameter: a kernel launched
    on stream S runs on S's device, but occupancy queries and the null stream follow the thread's current device)."""
    if not t.is_cuda:
        return None
    idx = t.device.index
    s = _Stream(_raw_stream(idx) if _raw_stream is not None else torch.cuda.current_stream(t.device).cuda_stream)
    s.dev = idx
    return s


def call(name: str, *args) -> None:
    lib = get_lib()
    st = args[-1] if args else None
    if isinstance(st, _Stream) and st.dev != torch.cuda.current_device():
        with torch.cuda.device(st.dev):
            rc = getattr(lib, name)(*args)
    else:
        rc = getattr(lib, name)(*args)
    if rc != 0:
        check(name, rc, lib)


def check(name: str, rc: int, lib: Optional[ctypes.CDLL] = None) -> None:
    """The one status check: a non-zero return of entry point `name` raises with the library's message.  For the calls that do not
    go through call() (stage drivers, route planner, tuning record: bench.py and the launch-trace recorder price / record what call() sees)."""
    if rc != 0:
        raise RuntimeError(f'{name} failed: {(lib or get_lib()).rvt_last_error().decode()}')


_WS = {}


def workspace(kind: str, like: torch.Tensor, n: int, dtype: torch.dtype, floor: int = 0):
    """(stream handle of `like`, the workspace of `kind` on that stream with at least n elements of `dtype`).  One buffer per
    (kind, device, stream): kernels on one stream serialise, so consecutive launches of a kind share it, launches on different
    streams never do.  Grow-only: a buffer that fits is never shrunk, dropped or replaced - captured graphs hold these addresses."""
    st, dev = stream_of(like), like.device
    key = (kind, dev.type, dev.index, 0 if st is None else int(st))
    ws = _WS.get(key)
    if ws is None or ws.numel() < n:
        ws = _WS[key] = torch.empty(max(n, floor), dtype=dtype, device=dev)
    return st, ws


def row_dtype(struct: str) -> np.dtype:
    """numpy dtype of one of the header's table rows or device-written records: the C struct's field names, offsets and size."""
    return np.dtype(_STRUCTS[struct] if struct in _STRUCTS else _RECORDS[struct])


class DeviceTable:
    """Host-built array of one of the header's row structs -> device bytes (one launch walks it).  Filled row by row (`add`) or
    from a whole array of the struct's dtype (`upload(device, arr)`)."""

    def __init__(self, struct: str):
        self.dtype = row_dtype(struct)
        self.rows = []                              # {field: value} per row; the array itself after upload(device, arr)
        self.blocks = 0                             # blocks owned by the rows so far = block0 of the next one
        self.dev: Optional[torch.Tensor] = None

    def add(self, nblocks: int = 0, **fields) -> None:
        """One row by field name.  A struct with a block0 field: the row owns nblocks blocks of the launch behind those before it."""
        if 'block0' in self.dtype.names:
            fields['block0'] = self.blocks
        self.rows.append(fields)
        self.blocks += nblocks

    def upload(self, device, arr: Optional[np.ndarray] = None) -> 'DeviceTable':
        if arr is None:
            arr = np.zeros(len(self.rows), dtype=self.dtype)
            for i, r in enumerate(self.rows):
                for k, v in r.items():
                    arr[i][k] = v                   # (a field the struct does not have raises)
        elif arr.dtype != self.dtype:
            raise TypeError(f'table rows of dtype {arr.dtype}, the header says {self.dtype}')
        else:
            self.rows = arr
        self.dev = torch.from_numpy(arr.view(np.uint8).reshape(-1).copy()).to(device)
        return self

    def __len__(self):
        return len(self.rows)
