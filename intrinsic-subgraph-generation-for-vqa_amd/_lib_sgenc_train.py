"""ctypes binding of the scene-graph encoder's training entry points of libisg_hip.so (include/isg_sgenc_train.h), derived from the header like _lib's.

The fifth device header has an ABI version of its own (ISG_SGENC_TRAIN_ABI_VERSION): include/isg.h and the other three headers do
not move when one of these entry points does.  The symbols live in the same shared library (csrc/isg_sgenc_bwd.hip).
"""
from __future__ import annotations

import ctypes
import os

from . import _lib

HEADER_PATH = os.path.join(os.path.dirname(_lib._HERE), "include", "isg_sgenc_train.h")
# name -> (restype, argtypes) of every symbol include/isg_sgenc_train.h declares; ISG_SGENC_TRAIN_ABI_VERSION
SIGNATURES, ABI_VERSION = _lib.read_header(HEADER_PATH)

_bound = None


def load():
    """The product library with the scene-graph training symbols bound; raises (never falls back) when one is missing."""
    global _bound
    if _bound is not None:
        return _bound
    _lib.load()                                   # existence, the inference ABI
    lib = ctypes.CDLL(_lib.LIB_PATH)
    try:
        _lib.bind(lib, SIGNATURES)
    except AttributeError as e:
        raise _lib.IsgError(f"{_lib.LIB_PATH} lacks a symbol of include/isg_sgenc_train.h ({e}): rebuild it (build())") from None
    v = lib.isg_sgenc_train_abi_version()
    if v != ABI_VERSION:
        raise _lib.IsgError(f"libisg_hip.so scene-graph training ABI version {v}, binding expects {ABI_VERSION}")
    _bound = lib
    return lib
