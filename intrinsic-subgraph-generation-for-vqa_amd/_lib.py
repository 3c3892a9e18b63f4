"""ctypes binding of libisg_hip.so (C ABI declared in include/isg.h, the include/isg_*.h of HEADERS and the include/ext/isg_*.h of
EXTENSIONS).

The product path has no CPU fallback: if the shared library is missing or a tensor is not on
an MI355X, the ops raise.  Build the library with ``python -c "import __graft_entry__ as g; g.build()"``.
"""
from __future__ import annotations

import contextlib
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


INCLUDE = os.path.join(os.path.dirname(_HERE), "include")
# Every device header of libisg_hip.so, in the order they were added: file -> (its version symbol, the noun its messages use).
# Each has an ABI version of its own, so none of the others moves when an entry point of one does; the symbols live in the one
# shared library, and load() binds and checks them all on the one handle.  (The loader's two headers declare another library:
# loader.py.)
HEADERS = {
    "isg.h": ("isg_abi_version", ""),
    "isg_train.h": ("isg_train_abi_version", "training "),
    "isg_optim.h": ("isg_optim_abi_version", "optimizer "),
    "isg_fused.h": ("isg_fused_abi_version", "fused-launch "),
    "isg_sgenc_train.h": ("isg_sgenc_train_abi_version", "scene-graph training "),
    "isg_dist.h": ("isg_dist_abi_version", "data-parallel "),
    "isg_linear_train.h": ("isg_linear_train_abi_version", "Linear-backward "),
    "isg_masked.h": ("isg_masked_abi_version", "masked-layer "),
    "isg_sampler_train.h": ("isg_sampler_train_abi_version", "sampler-training "),
    "isg_topk_rows.h": ("isg_topk_rows_abi_version", "per-row top-k "),
    "isg_mp_train.h": ("isg_mp_train_abi_version", "attention-dropout "),
    "isg_sparse_out.h": ("isg_sparse_out_abi_version", "sparse-output "),
    "isg_mp_f16_train.h": ("isg_mp_f16_train_abi_version", "half-row training "),
    "isg_concat.h": ("isg_concat_abi_version", "concat_instr "),
    "isg_instances.h": ("isg_instances_abi_version", "instances "),
    "isg_eval.h": ("isg_eval_abi_version", "eval "),
    "isg_grounding.h": ("isg_grounding_abi_version", "grounding "),
}
_parsed, _declared_in = {}, {}                      # file -> header(file); symbol -> the file that declares it


def header(file: str):
    """(path, {name: (restype, argtypes)}, ABI version) of one header of HEADERS, read once.  The headers share one library and
    one handle, so a symbol that two of them declare raises, naming both."""
    if file not in _parsed:
        path = os.path.join(INCLUDE, file)
        signatures, abi = read_header(path)
        for name in signatures:
            if _declared_in.setdefault(name, file) != file:
                raise IsgError(f"`{name}` is declared in include/{_declared_in[name]} and in include/{file}")
        _parsed[file] = (path, signatures, abi)
    return _parsed[file]


# name -> (restype, argtypes), one entry per symbol declared in include/isg.h; ISG_ABI_VERSION
HEADER_PATH, SIGNATURES, ABI_VERSION = header("isg.h")
for _file in HEADERS:
    header(_file)

# Every extension header (include/ext/) of the same library, in the order they were added: file -> (its version symbol, the
# noun its messages use).  Outside HEADERS: bind() without signatures, checked() and load() neither bind nor check them, so a
# variant build that lacks one extension's symbols still serves everything else; load_extension() does both, per header, on
# whatever handle load() returns.
EXTENSIONS = {
    "isg_instances_train.h": ("isg_instances_train_abi_version", "instance-training "),
    "isg_induced.h": ("isg_induced_abi_version", "induced-instance "),
    "isg_rollout.h": ("isg_rollout_abi_version", "attention-rollout "),
    "isg_ig.h": ("isg_ig_abi_version", "integrated-gradients "),
    "isg_maskopt.h": ("isg_maskopt_abi_version", "mask-optimisation "),
    "isg_curves.h": ("isg_curve_abi_version", "fidelity-curve "),
    "isg_shapley.h": ("isg_shapley_abi_version", "Shapley-sampling "),
}
_extensions = {}                                    # file -> extension(file)
_bound = {}         # (id(handle), file) -> the handle (kept, so that an id is never handed to another object): bound and checked


def refuse_redeclared(file: str, signatures, declared_in) -> None:
    """A symbol of the extension header `file` that another header declares as well is refused, by name.  declared_in: symbol ->
    the file under include/ that declares it."""
    for name in signatures:
        if name in declared_in:
            raise IsgError(f"`{name}` is declared in include/{declared_in[name]} and in include/ext/{file}")


def declared_elsewhere(file: str) -> dict:
    """symbol -> file under include/ of every device header and of every extension header read so far but `file` (all of
    EXTENSIONS, once this module is imported)."""
    where = dict(_declared_in)
    for other, (_, signatures, _) in _extensions.items():
        if other != file:
            for name in signatures:
                where.setdefault(name, "ext/" + other)
    return where


def extension(file: str):
    """(path, {name: (restype, argtypes)}, ABI version) of one header of EXTENSIONS, read once and held against every device header
    and every extension read before it: between them, each pair of headers is compared."""
    if file not in _extensions:
        path = os.path.join(INCLUDE, "ext", file)
        signatures, abi = read_header(path)
        refuse_redeclared(file, signatures, declared_elsewhere(file))
        _extensions[file] = (path, signatures, abi)
    return _extensions[file]


for _file in EXTENSIONS:
    extension(_file)

_lib = None


def bind(lib, signatures=None):
    """Set restype / argtypes of the given symbols -- without `signatures`, of every symbol of every header -- on a CDLL (the
    product library, or a variant build of it)."""
    for sigs in ([header(f)[1] for f in HEADERS] if signatures is None else [signatures]):
        for name, (res, args) in sigs.items():
            fn = getattr(lib, name)   # AttributeError here = header and library disagree
            fn.restype = res
            fn.argtypes = args
    return lib


def _check_one(lib, where: str, parsed, version: str, noun: str) -> None:
    """bind() one header's symbols (where: its file under include/), then its version check."""
    _, signatures, abi = parsed
    try:
        bind(lib, signatures)
    except AttributeError as e:
        raise IsgError(f"{LIB_PATH} lacks a symbol of include/{where} ({e}): rebuild it (build())") from None
    v = getattr(lib, version)()
    if v != abi:
        raise IsgError(f"libisg_hip.so {noun}ABI version {v}, binding expects {abi}")


def checked(lib):
    """bind() header by header, each followed by its version check: the handle, or the IsgError that names the header at fault."""
    for file, (version, noun) in HEADERS.items():
        _check_one(lib, file, header(file), version, noun)
    return lib


def load():
    """Load libisg_hip.so once, with every header bound and checked; raise (never fall back) when it is absent, lacks a symbol or
    has the wrong ABI.  The one handle of the package: every _lib_<name>.load() returns it, so assigning `_lib._lib` (or using())
    swaps the library under every entry point."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise IsgError(
            f"{LIB_PATH} not found: the HIP extension is not built. Run `python -c \"import __graft_entry__ as g; "
            "g.build()\"` (hipcc --offload-arch=gfx950). There is no CPU fallback for this path.")
    _lib = checked(ctypes.CDLL(LIB_PATH))
    return _lib


def load_extension(file: str):
    """The package's handle (load(), looked up when called) with the symbols of one header of EXTENSIONS bound and its version
    checked: once per handle and header -- the product library, the strict twin or a variant build swapped in through `_lib` /
    using() alike; raises IsgError (never falls back) when the handle lacks a symbol or answers another version.  Every
    _ext_<name>.load() is this."""
    lib = load()
    if _bound.get((id(lib), file)) is not lib:
        _check_one(lib, "ext/" + file, extension(file), *EXTENSIONS[file])
        _bound[id(lib), file] = lib
    return lib


@contextlib.contextmanager
def using(handle):
    """Run the block on another handle -- a variant build from bind(ctypes.CDLL(path)), or a proxy around one -- and put back
    what was there."""
    global _lib
    keep, _lib = load(), handle
    try:
        yield handle
    finally:
        _lib = keep


def check(status: int, what: str) -> None:
    if status != ISG_OK:
        lib = load()
        msg = lib.isg_status_string(status).decode()
        hip = lib.isg_last_hip_error().decode()
        raise IsgError(f"{what}: {msg} (status {status})" + (f"; HIP: {hip}" if hip else ""))
