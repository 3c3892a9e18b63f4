"""What each header's CPU test asks of the build (__graft_entry__.py), asked of its behaviour: build_checks(file) finds the header
among header_dependencies() and in exactly one of the binding's two tables, then runs check_binding() -- what build() runs after
linking -- on stubs that stand in for a freshly linked library: one answers this header's version call with n + 1, one lacks
the header's last symbol.  Each has to raise the IsgError that names the header, word for word.  Nothing is launched."""
import os
import types

import pytest

from conftest import ROOT

LOADER_HEADERS = {"isg_loader.h", "isg_loader_objects.h"}            # another library: isubgvqa_amd/loader.py


class Stub:
    """A handle that passes every name on to `real`, but for those replaced: by a callable, or by None for a missing symbol."""

    def __init__(self, real, **replaced):
        self.real, self.replaced = real, replaced

    def __getattr__(self, name):
        if name in self.replaced:
            if self.replaced[name] is None:
                raise AttributeError(f"undefined symbol: {name}")
            return self.replaced[name]
        return getattr(self.real, name)


def post_link_check(stub) -> None:
    """check_binding() as build() runs it after linking, `stub` being the library: the package holds no handle yet, and the CDLL
    that _lib.load() opens is the stub.  What was there is put back."""
    import __graft_entry__ as ge
    from isubgvqa_amd import _lib
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(_lib, "_lib", None)
        mp.setattr(_lib, "ctypes", types.SimpleNamespace(CDLL=lambda path: stub))
        ge.check_binding()
        assert _lib.load() is stub


def build_checks(file: str) -> None:
    import __graft_entry__ as ge
    from isubgvqa_amd import _lib
    if file in LOADER_HEADERS:
        return loader_checks(file)
    ext = file in _lib.EXTENSIONS
    assert (file in _lib.HEADERS) != ext, f"{file} has to be in exactly one of _lib.HEADERS and _lib.EXTENSIONS"
    where = "ext/" + file if ext else file
    path, signatures, abi = _lib.extension(file) if ext else _lib.header(file)
    assert path == os.path.join(ROOT, "include", *where.split("/")) and os.path.exists(path)
    assert path in ge.header_dependencies(), f"include/{where} is not among build()'s header dependencies"
    version, noun = (_lib.EXTENSIONS if ext else _lib.HEADERS)[file]
    assert version in signatures, (file, version)
    real = _lib.load()
    post_link_check(Stub(real))                                      # a stub that lacks nothing passes
    with pytest.raises(_lib.IsgError) as err:
        post_link_check(Stub(real, **{version: lambda n=abi + 1: n}))
    assert str(err.value) == f"libisg_hip.so {noun}ABI version {abi + 1}, binding expects {abi}"
    gone = list(signatures)[-1]
    with pytest.raises(_lib.IsgError) as err:
        post_link_check(Stub(real, **{gone: None}))
    assert str(err.value) == f"{_lib.LIB_PATH} lacks a symbol of include/{where} (undefined symbol: {gone}): rebuild it (build())"
    assert _lib.load() is real                                       # a handle that fails its checks is never the package's


def loader_checks(file: str) -> None:
    """The loader's headers make libisg_loader.so stale, not libisg_hip.so; check_binding() still asserts the object ABI."""
    import __graft_entry__ as ge
    from isubgvqa_amd import _lib, loader
    path = os.path.join(ROOT, "include", file)
    assert path in ge.loader_dependencies() and path not in ge.header_dependencies() and os.path.exists(path)
    assert file not in _lib.HEADERS and file not in _lib.EXTENSIONS
    real = loader.load()
    assert real.isg_loader_objects_abi_version() == loader.OBJECT_ABI_VERSION
    stale = Stub(real, isg_loader_objects_abi_version=lambda: loader.OBJECT_ABI_VERSION + 1)
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(loader, "load", lambda: stale)
        with pytest.raises(AssertionError):
            ge.check_binding()
    ge.check_binding()
