"""ctypes binding of the training entry points of libisg_hip.so (include/isg_train.h), derived from the header like _lib's.

The second device header has an ABI version of its own (ISG_TRAIN_ABI_VERSION): include/isg.h, the inference ABI, does not move
when a training entry point does.  The symbols live in the same shared library (csrc/isg_text_bwd.hip).
"""
from __future__ import annotations

import ctypes
import os

from . import _lib

HEADER_PATH = os.path.join(os.path.dirname(_lib._HERE), "include", "isg_train.h")
# name -> (restype, argtypes) of every symbol include/isg_train.h declares; ISG_TRAIN_ABI_VERSION
SIGNATURES, ABI_VERSION = _lib.read_header(HEADER_PATH)

_bound = None


def load():
    """The product library with the training symbols bound; raises (never falls back) when one is missing."""
    global _bound
    if _bound is not None:
        return _bound
    _lib.load()                                   # existence, the inference ABI
    lib = ctypes.CDLL(_lib.LIB_PATH)
    try:
        _lib.bind(lib, SIGNATURES)
    except AttributeError as e:
        raise _lib.IsgError(f"{_lib.LIB_PATH} lacks a symbol of include/isg_train.h ({e}): rebuild it (build())") from None
    v = lib.isg_train_abi_version()
    if v != ABI_VERSION:
        raise _lib.IsgError(f"libisg_hip.so training ABI version {v}, binding expects {ABI_VERSION}")
    _bound = lib
    return lib
