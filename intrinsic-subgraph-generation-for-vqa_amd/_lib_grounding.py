"""ctypes binding of the grounding score of libisg_hip.so (include/isg_grounding.h), derived from the header like _lib's.

The seventeenth device header has an ABI version of its own (ISG_GROUNDING_ABI_VERSION): none of the other headers moves when
the entry point here does.  The symbols live in the same shared library.  The layout constants (ISG_GROUND_*) are read from the
header too: the header is the contract, and nothing in Python restates a number of it.

One of the headers of _lib.HEADERS: parsed, bound and version-checked there, on the one handle of the package, so
`load() is _lib.load()`, always -- a library swapped in through `_lib._lib` is the library here too.
"""
from __future__ import annotations

import re

from . import _lib

# name -> (restype, argtypes) of every symbol include/isg_grounding.h declares; ISG_GROUNDING_ABI_VERSION
HEADER_PATH, SIGNATURES, ABI_VERSION = _lib.header("isg_grounding.h")


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


def load():
    """The package's handle (_lib.load(), looked up when called), where the grounding symbols are bound beside all others."""
    return _lib.load()
