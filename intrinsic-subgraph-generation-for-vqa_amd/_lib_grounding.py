"""ctypes binding of the grounding score of libisg_hip.so (include/isg_grounding.h), derived from the header like _lib's.

The seventeenth device header has an ABI version of its own (ISG_GROUNDING_ABI_VERSION): none of the other headers moves when
the entry point here does.  The symbols live in the same shared library.  The layout constants (ISG_GROUND_*) are read from the
header too: the header is the contract, and nothing in Python restates a number of it.
"""
from __future__ import annotations

import ctypes
import os
import re

from . import _lib

HEADER_PATH = os.path.join(os.path.dirname(_lib._HERE), "include", "isg_grounding.h")
# name -> (restype, argtypes) of every symbol include/isg_grounding.h declares; ISG_GROUNDING_ABI_VERSION
SIGNATURES, ABI_VERSION = _lib.read_header(HEADER_PATH)


def read_constants(path: str = HEADER_PATH) -> dict:
    """{name: int} of the header's `#define ISG_GROUND_<name> <integer expression of earlier ones>` lines, in file order."""
    text = re.sub(r"/\*.*?\*/", " ", open(path).read(), flags=re.S)
    out: dict = {}
    for name, expr in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(ISG_GROUND_\w+)[ \t]+(\S.*?)[ \t]*$", text, flags=re.M):
        if not re.fullmatch(r"[\w\s()+*\-]+", expr):
            raise _lib.IsgError(f"{path}: cannot read `#define {name} {expr}`")
        out[name] = int(eval(expr, {"__builtins__": {}}, dict(out)))      # integers, + - * and names defined above: checked
    return out


CONSTANTS = read_constants()

_bound = None


def load():
    """The product library with the grounding symbols bound; raises (never falls back) when one is missing."""
    global _bound
    if _bound is not None:
        return _bound
    _lib.load()                                   # existence, the inference ABI
    lib = ctypes.CDLL(_lib.LIB_PATH)
    try:
        _lib.bind(lib, SIGNATURES)
    except AttributeError as e:
        raise _lib.IsgError(f"{_lib.LIB_PATH} lacks a symbol of include/isg_grounding.h ({e}): rebuild it (build())") from None
    v = lib.isg_grounding_abi_version()
    if v != ABI_VERSION:
        raise _lib.IsgError(f"libisg_hip.so grounding ABI version {v}, binding expects {ABI_VERSION}")
    _bound = lib
    return lib
