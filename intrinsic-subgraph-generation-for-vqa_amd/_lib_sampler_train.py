"""ctypes binding of the sampler-training entry points of libisg_hip.so (include/isg_sampler_train.h), derived from the header
like _lib's.

The ninth device header has an ABI version of its own (ISG_SAMPLER_TRAIN_ABI_VERSION): none of the other headers moves when an entry
point here does.  The symbols live in the same shared library.

One of the headers of _lib.HEADERS: parsed, bound and version-checked there, on the one handle of the package, so
`load() is _lib.load()`, always -- a library swapped in through `_lib._lib` is the library here too.
"""
from __future__ import annotations

from . import _lib

# name -> (restype, argtypes) of every symbol include/isg_sampler_train.h declares; ISG_SAMPLER_TRAIN_ABI_VERSION
HEADER_PATH, SIGNATURES, ABI_VERSION = _lib.header("isg_sampler_train.h")


def load():
    """The package's handle (_lib.load(), looked up when called), where the sampler-training symbols are bound beside all others."""
    return _lib.load()
