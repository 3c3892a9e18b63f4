"""ctypes binding of the step-tail entry points of libisg_hip.so (include/isg_optim.h), derived from the header like _lib's.

The third device header has an ABI version of its own (ISG_OPTIM_ABI_VERSION): include/isg.h and include/isg_train.h do not move
when an entry point of the loss, the gradient norm or Adam does.  The symbols live in the same shared library (csrc/isg_optim.hip).

One of the headers of _lib.HEADERS: parsed, bound and version-checked there, on the one handle of the package, so
`load() is _lib.load()`, always -- a library swapped in through `_lib._lib` is the library here too.
"""
from __future__ import annotations

from . import _lib

# name -> (restype, argtypes) of every symbol include/isg_optim.h declares; ISG_OPTIM_ABI_VERSION
HEADER_PATH, SIGNATURES, ABI_VERSION = _lib.header("isg_optim.h")


def load():
    """The package's handle (_lib.load(), looked up when called), where the step-tail symbols are bound beside all others."""
    return _lib.load()
