"""ctypes binding of the Shapley-sampling entry points of libisg_hip.so (include/ext/isg_shapley.h), derived from the header like
_lib's.

An EXTENSION header: it lies under include/ext/, outside _lib.HEADERS, so _lib.load() / _lib.checked() neither bind nor check
it.  load() here does both on whatever handle _lib.load() returns, the first time it sees that handle -- the product library, the
strict twin or a variant build swapped in through `_lib._lib` / _lib.using() alike -- and `load() is _lib.load()` holds as for the
_lib_<name> modules.  The header has an ABI version of its own (ISG_SHAPLEY_ABI_VERSION).
"""
from __future__ import annotations

import os

from . import _ext_curves, _ext_ig, _ext_induced, _ext_instances_train, _ext_maskopt, _ext_rollout, _lib

HEADER_PATH = os.path.join(_lib.INCLUDE, "ext", "isg_shapley.h")
# name -> (restype, argtypes) of every symbol the header declares; ISG_SHAPLEY_ABI_VERSION
SIGNATURES, ABI_VERSION = _lib.read_header(HEADER_PATH)
VERSION_SYMBOL = "isg_shapley_abi_version"


def refuse_redeclared(signatures, declared_in) -> None:
    """A symbol of this header that another header declares as well is refused, by name.  declared_in: symbol -> the file under
    include/ that declares it."""
    for name in signatures:
        if name in declared_in:
            raise _lib.IsgError(f"`{name}` is declared in include/{declared_in[name]} and in include/ext/isg_shapley.h")


def declared_elsewhere() -> dict:
    """symbol -> file under include/ of every device header of the table and of the six other extension headers."""
    where = dict(_lib._declared_in)
    for mod in (_ext_instances_train, _ext_induced, _ext_rollout, _ext_ig, _ext_maskopt, _ext_curves):
        file = "ext/" + os.path.basename(mod.HEADER_PATH)
        for name in mod.SIGNATURES:
            where.setdefault(name, file)
    return where


refuse_redeclared(SIGNATURES, declared_elsewhere())

_checked = {}       # id(handle) -> the handle (kept, so that an id is never handed to another object): bound and version-checked


def load():
    """The package's handle (_lib.load(), looked up when called) with this header's symbols bound and its version checked: once
    per handle; raises IsgError (never falls back) when the handle lacks a symbol or answers another version."""
    lib = _lib.load()
    if _checked.get(id(lib)) is not lib:
        try:
            _lib.bind(lib, SIGNATURES)
        except AttributeError as e:
            raise _lib.IsgError(f"{_lib.LIB_PATH} lacks a symbol of include/ext/isg_shapley.h ({e}): rebuild it (build())") from None
        v = getattr(lib, VERSION_SYMBOL)()
        if v != ABI_VERSION:
            raise _lib.IsgError(f"libisg_hip.so Shapley-sampling ABI version {v}, binding expects {ABI_VERSION}")
        _checked[id(lib)] = lib
    return lib
