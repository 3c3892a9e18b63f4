"""ctypes binding of libisg_hip.so (C ABI declared in include/isg.h).

The product path has no CPU fallback: if the shared library is missing or a tensor is not on
an MI355X, the ops raise.  Build the library with ``python -c "import __graft_entry__ as g; g.build()"``.
"""
from __future__ import annotations

import ctypes
import os
import re
from ctypes import c_char_p, c_double, c_float, c_int, c_int32, c_int64, c_size_t, c_uint64, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libisg_hip.so")

ISG_OK = 0
_SCALARS = {"int": c_int, "int32_t": c_int32, "int64_t": c_int64, "uint64_t": c_uint64, "size_t": c_size_t, "float": c_float,
            "double": c_double}


class IsgError(RuntimeError):
    pass


def _ctype(text: str, decl: str):
    """The ctypes type of one C type as the two headers spell them.  Any data pointer is c_void_p (callers pass data_ptr()
    integers), `const char *` is c_char_p, `void` is None; an unknown word raises with the declaration it stands in."""
    words = [w for w in text.replace("*", " * ").split() if w != "const"]
    base = [w for w in words if w != "*"]
    stars = len(words) - len(base)
    if len(base) != 1 or words[0] == "*" or (stars == 0 and base[0] != "void" and base[0] not in _SCALARS):
        raise ValueError(f"cannot bind `{decl}`: type `{' '.join(text.split())}`")
    if stars:
        return c_char_p if (base[0], stars) == ("char", 1) else c_void_p
    return None if base[0] == "void" else _SCALARS[base[0]]


def parse_header(text: str, prefix: str = "isg_"):
    """({name: (restype, argtypes)}, ABI version) of a C header's `<prefix>*` function declarations.  Strict: a declaration that
    is skipped or half-understood would bind a symbol with the wrong registers, silently -- so an unknown type word, an array,
    function-pointer, variadic or unnamed parameter raises with the declaration's text, and every `<prefix>name(` of the
    comment-stripped header has to be one of the declarations that were understood."""
    body = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    body = re.sub(r"//[^\n]*", " ", body)
    body = re.sub(r"^[ \t]*#.*$", " ", body, flags=re.M)
    body = re.sub(r'extern\s+"C"\s*\{', " ", body)
    called = re.compile(r"\b(%s\w+)\s*\(" % prefix)
    named = re.compile(r"(.*[\s\*])(\w+)", flags=re.S)
    sigs, types = {}, {}                            # types: the ~1000 parameters of isg.h spell some twenty types
    for stmt in body.split(";")[:-1]:                # what follows the last `;` is no declaration
        m = called.search(stmt)
        if m is None:
            continue                                # a typedef
        decl, name, params = " ".join(stmt.split()), m.group(1), stmt[m.end():].strip()
        if not params.endswith(")"):
            raise ValueError(f"cannot bind `{decl}`: not a plain function declaration")
        if re.search(r"[()\[\]{}]|\.\.\.", params[:-1]):
            raise ValueError(f"cannot bind `{decl}`: array, function-pointer or variadic parameter")
        args = []
        if params[:-1].split() != ["void"]:
            for p in params[:-1].split(","):
                pm = named.fullmatch(p.strip())
                if pm is None:
                    raise ValueError(f"cannot bind `{decl}`: parameter `{p.strip()}` has no name")
                if pm.group(1) not in types:
                    types[pm.group(1)] = _ctype(pm.group(1), decl)
                if types[pm.group(1)] is None:
                    raise ValueError(f"cannot bind `{decl}`: parameter `{p.strip()}`")
                args.append(types[pm.group(1)])
        sig = (_ctype(stmt[:m.start()], decl), args)
        if sigs.setdefault(name, sig) != sig:
            raise ValueError(f"cannot bind `{decl}`: `{name}` is declared twice, differently")
    declared = set(called.findall(body))
    if len(declared) != len(sigs):
        raise ValueError(f"declarations not understood: {sorted(declared ^ set(sigs))}")
    abi = re.findall(r"^[ \t]*#[ \t]*define[ \t]+\w*ABI_VERSION[ \t]+(\d+)", text, flags=re.M)
    if len(abi) != 1:
        raise ValueError(f"expected one `#define ...ABI_VERSION <n>`, found {len(abi)}")
    return sigs, int(abi[0])


def read_header(path: str, error=IsgError):
    """parse_header() of the header that lies beside the package in the tree."""
    if not os.path.exists(path):
        raise error(f"{path} not found: the binding is derived from the C header, which travels with the package")
    with open(path) as f:
        return parse_header(f.read())


HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "isg.h")
# name -> (restype, argtypes), one entry per symbol declared in include/isg.h; ISG_ABI_VERSION
SIGNATURES, ABI_VERSION = read_header(HEADER_PATH)

_lib = None


def bind(lib, signatures=None):
    """Set restype / argtypes of every declared symbol on a CDLL (the product library, or a variant build of it)."""
    for name, (res, args) in (SIGNATURES if signatures is None else signatures).items():
        fn = getattr(lib, name)   # AttributeError here = header and library disagree
        fn.restype = res
        fn.argtypes = args
    return lib


def load():
    """Load libisg_hip.so once; raise (never fall back) when it is absent or has the wrong ABI."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise IsgError(
            f"{LIB_PATH} not found: the HIP extension is not built. Run `python -c \"import __graft_entry__ as g; "
            "g.build()\"` (hipcc --offload-arch=gfx950). There is no CPU fallback for this path.")
    lib = bind(ctypes.CDLL(LIB_PATH))
    v = lib.isg_abi_version()
    if v != ABI_VERSION:
        raise IsgError(f"libisg_hip.so ABI version {v}, binding expects {ABI_VERSION}")
    _lib = lib
    return lib


def check(status: int, what: str) -> None:
    if status != ISG_OK:
        lib = load()
        msg = lib.isg_status_string(status).decode()
        hip = lib.isg_last_hip_error().decode()
        raise IsgError(f"{what}: {msg} (status {status})" + (f"; HIP: {hip}" if hip else ""))
