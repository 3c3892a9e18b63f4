"""ctypes binding of the evaluation by question type of libisg_hip.so (include/isg_eval.h), derived from the header like _lib's.

The sixteenth device header has an ABI version of its own (ISG_EVAL_ABI_VERSION): none of the other headers moves when an
entry point here does.  The symbols live in the same shared library.
"""
from __future__ import annotations

import ctypes
import os

from . import _lib

HEADER_PATH = os.path.join(os.path.dirname(_lib._HERE), "include", "isg_eval.h")
# name -> (restype, argtypes) of every symbol include/isg_eval.h declares; ISG_EVAL_ABI_VERSION
SIGNATURES, ABI_VERSION = _lib.read_header(HEADER_PATH)

_bound = None


def load():
    """The product library with the evaluation symbols bound; raises (never falls back) when one is missing."""
    global _bound
    if _bound is not None:
        return _bound
    _lib.load()                                   # existence, the inference ABI
    lib = ctypes.CDLL(_lib.LIB_PATH)
    try:
        _lib.bind(lib, SIGNATURES)
    except AttributeError as e:
        raise _lib.IsgError(f"{_lib.LIB_PATH} lacks a symbol of include/isg_eval.h ({e}): rebuild it (build())") from None
    v = lib.isg_eval_abi_version()
    if v != ABI_VERSION:
        raise _lib.IsgError(f"libisg_hip.so eval ABI version {v}, binding expects {ABI_VERSION}")
    _bound = lib
    return lib
