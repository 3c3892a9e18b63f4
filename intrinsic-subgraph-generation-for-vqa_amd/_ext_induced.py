"""ctypes binding of the induced-subgraph instances of libisg_hip.so (include/ext/isg_induced.h), derived from the header like _lib's.

The second extension header has an ABI version of its own (ISG_INDUCED_ABI_VERSION).  The symbols live in the same shared library.

One of the headers of _lib.EXTENSIONS: parsed there once and held against every other header; outside _lib.HEADERS, so it is
bound and version-checked by _lib.load_extension, on whatever handle _lib.load() returns, the first time that handle is seen --
`load() is _lib.load()`, always, and a library swapped in through `_lib._lib` is the library here too.
"""
from __future__ import annotations

from . import _lib

# name -> (restype, argtypes) of every symbol include/ext/isg_induced.h declares; ISG_INDUCED_ABI_VERSION
HEADER_PATH, SIGNATURES, ABI_VERSION = _lib.extension("isg_induced.h")
VERSION_SYMBOL = _lib.EXTENSIONS["isg_induced.h"][0]


def load():
    """The package's handle (_lib.load(), looked up when called) with this header's symbols bound and its version checked."""
    return _lib.load_extension("isg_induced.h")


def refuse_redeclared(signatures, declared_in) -> None:
    """_lib.refuse_redeclared for this header.  declared_in: symbol -> the file under include/ that declares it."""
    _lib.refuse_redeclared("isg_induced.h", signatures, declared_in)


def declared_elsewhere() -> dict:
    """symbol -> file under include/ of every device header and of every other extension header."""
    return _lib.declared_elsewhere("isg_induced.h")
