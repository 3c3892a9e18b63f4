"""ctypes binding of the entry points of a Linear's backward in libisg_hip.so (include/isg_linear_train.h), derived from the header like _lib's.

The header has an ABI version of its own (ISG_LINEAR_TRAIN_ABI_VERSION): no other header moves when the backward's kernels do.  The
symbols live in the same shared library (csrc/isg_linear_bwd.hip).

One of the headers of _lib.HEADERS: parsed, bound and version-checked there, on the one handle of the package, so
`load() is _lib.load()`, always -- a library swapped in through `_lib._lib` is the library here too.
"""
from __future__ import annotations

from . import _lib

# name -> (restype, argtypes) of every symbol include/isg_linear_train.h declares; ISG_LINEAR_TRAIN_ABI_VERSION
HEADER_PATH, SIGNATURES, ABI_VERSION = _lib.header("isg_linear_train.h")


def load():
    """The package's handle (_lib.load(), looked up when called), where the Linear-backward symbols are bound beside all others."""
    return _lib.load()
