"""The binding of libisg_hip.so as a whole (isubgvqa_amd/_lib.py) without a GPU: one table of device headers, one
handle that every _lib_<name>.load() returns, a swap of `_lib._lib` that reaches every header's entry points -- the strict twin,
a proxy that is no CDLL -- and the three ways a load fails, header by header; then the same for the table of extension headers,
which bind lazily, each on its own, and the eighth header that needs a table row and no edit to build().  The entry points
called here refuse or return before any launch."""
import ctypes
import glob
import importlib
import os

import pytest

from binding_checks import Stub
from conftest import ROOT

# header -> the noun of its version message, as the messages have always read ("" for include/isg.h)
NOUNS = {"isg.h": "", "isg_train.h": "training ", "isg_optim.h": "optimizer ", "isg_fused.h": "fused-launch ",
         "isg_sgenc_train.h": "scene-graph training ", "isg_dist.h": "data-parallel ", "isg_linear_train.h": "Linear-backward ",
         "isg_masked.h": "masked-layer ", "isg_sampler_train.h": "sampler-training ", "isg_topk_rows.h": "per-row top-k ",
         "isg_mp_train.h": "attention-dropout ", "isg_sparse_out.h": "sparse-output ", "isg_mp_f16_train.h": "half-row training ",
         "isg_concat.h": "concat_instr ", "isg_instances.h": "instances ", "isg_eval.h": "eval ", "isg_grounding.h": "grounding "}
# extension header -> the noun of its version message
EXT_NOUNS = {"isg_instances_train.h": "instance-training ", "isg_induced.h": "induced-instance ", "isg_rollout.h": "attention-rollout ",
             "isg_ig.h": "integrated-gradients ", "isg_maskopt.h": "mask-optimisation ", "isg_curves.h": "fidelity-curve ",
             "isg_shapley.h": "Shapley-sampling "}
LOADER_HEADERS = {"isg_loader.h", "isg_loader_objects.h"}            # another library: isubgvqa_amd/loader.py
TILE_BYTES = 4176                                                    # isg_layer_conv_live_tables_bytes(1), include/isg_masked.h


@pytest.fixture(scope="module")
def binding():
    """(_lib, {header: its _lib_<name> module}) after a build."""
    import __graft_entry__ as ge
    ge.build()
    from isubgvqa_amd import _lib
    names = sorted(os.path.basename(p)[:-3] for p in glob.glob(os.path.join(os.path.dirname(_lib.__file__), "_lib_*.py")))
    mods = {"isg" + n[len("_lib"):] + ".h": importlib.import_module("isubgvqa_amd." + n) for n in names}
    return _lib, mods


@pytest.fixture(scope="module")
def extensions(binding):
    """(_lib, {extension header: its _ext_<name> module})."""
    _lib, _ = binding
    names = sorted(os.path.basename(p)[:-3] for p in glob.glob(os.path.join(os.path.dirname(_lib.__file__), "_ext_*.py")))
    return _lib, {"isg" + n[len("_ext"):] + ".h": importlib.import_module("isubgvqa_amd." + n) for n in names}


class Recorder:
    """Not a CDLL, only __getattr__: the calls that reach it, by name, passed on to a handle."""

    def __init__(self, lib):
        self.lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self.lib, name)

        def wrapped(*a):
            self.calls.append(name)
            return fn(*a)
        return wrapped


def test_the_table_covers_every_device_header_and_module(binding):
    _lib, mods = binding
    on_disk = {os.path.basename(p) for p in glob.glob(os.path.join(ROOT, "include", "isg*.h"))}
    assert set(_lib.HEADERS) == on_disk - LOADER_HEADERS == set(NOUNS) and LOADER_HEADERS <= on_disk
    assert list(_lib.HEADERS)[0] == "isg.h" and set(mods) == set(_lib.HEADERS) - {"isg.h"}
    assert {f: noun for f, (_, noun) in _lib.HEADERS.items()} == NOUNS
    assert (_lib.HEADER_PATH, _lib.SIGNATURES, _lib.ABI_VERSION) == _lib.header("isg.h")
    assert _lib.ABI_VERSION == 23 and len(_lib.SIGNATURES) == 74            # include/isg.h alone, as before
    for file, mod in mods.items():
        assert mod.HEADER_PATH == os.path.join(ROOT, "include", file)
        assert (mod.SIGNATURES, mod.ABI_VERSION) == _lib.read_header(mod.HEADER_PATH), file
        assert _lib.header(file) == (mod.HEADER_PATH, mod.SIGNATURES, mod.ABI_VERSION)
        assert _lib.header(file)[1] is mod.SIGNATURES, "header() parses a header once"
    sets = [set(_lib.header(f)[1]) for f in _lib.HEADERS]
    assert sum(map(len, sets)) == len(set().union(*sets)), "a symbol is declared in two headers"
    for file, (version, _) in _lib.HEADERS.items():
        assert version in _lib.header(file)[1], (file, version)


def test_a_symbol_declared_in_two_headers_raises_naming_both(binding, monkeypatch):
    _lib, _ = binding
    monkeypatch.setattr(_lib, "_parsed", dict(_lib._parsed))
    monkeypatch.setattr(_lib, "_declared_in", dict(_lib._declared_in))
    monkeypatch.setattr(_lib, "read_header", lambda path: ({"isg_new": (None, []), "isg_small_mlps": (ctypes.c_int, [])}, 1))
    with pytest.raises(_lib.IsgError, match=r"`isg_small_mlps` is declared in include/isg_fused\.h and in include/isg_twice\.h"):
        _lib.header("isg_twice.h")


def test_every_module_loads_the_one_handle_with_every_header_bound(binding):
    _lib, mods = binding
    lib = _lib.load()
    assert isinstance(lib, ctypes.CDLL) and _lib.load() is lib
    for file, (version, _) in _lib.HEADERS.items():
        if file != "isg.h":
            assert mods[file].load() is lib, file
        _, signatures, abi = _lib.header(file)
        for name, (res, args) in signatures.items():
            fn = getattr(lib, name)
            assert fn.restype == res and list(fn.argtypes or []) == args, (file, name)
        assert getattr(lib, version)() == abi, file


def test_a_swap_to_the_strict_twin_reaches_every_header(binding):
    import __graft_entry__ as ge
    _lib, mods = binding
    fast = _lib.load()
    strict = _lib.bind(ctypes.CDLL(ge.STRICT_LIB))                   # what every variant tool and tests/test_gpu_strict.py write
    assert strict is not fast and strict._name == ge.STRICT_LIB
    try:
        _lib._lib = strict
        assert _lib.load() is strict
        for file, mod in mods.items():
            assert mod.load() is strict, file
            for name, (res, args) in mod.SIGNATURES.items():
                fn = getattr(strict, name)
                assert fn.restype == res and list(fn.argtypes or []) == args, (file, name)
            assert getattr(mod.load(), _lib.HEADERS[file][0])() == mod.ABI_VERSION
        masked = mods["isg_masked.h"].load()
        assert masked.isg_layer_conv_live_tables_bytes(1) == TILE_BYTES and masked.isg_layer_conv_live_tables_bytes(-3) == 0
        assert mods["isg_instances.h"].load().isg_instances_workspace_bytes(3) == 16
    finally:
        _lib._lib = fast
    assert mods["isg_masked.h"].load() is fast


def test_a_swap_to_a_proxy_sees_the_calls_of_every_header(binding):
    _lib, mods = binding
    real = _lib.load()
    rec = Recorder(real)
    try:
        _lib._lib = rec
        on = mods["isg_masked.h"].load().isg_layer_conv_live_tables_enabled()
        assert mods["isg_instances.h"].load().isg_instances_workspace_bytes(3) == 16
        assert mods["isg_eval.h"].load().isg_eval_abi_version() == mods["isg_eval.h"].ABI_VERSION
        assert _lib.load().isg_abi_version() == _lib.ABI_VERSION
    finally:
        _lib._lib = real
    assert on == real.isg_layer_conv_live_tables_enabled()
    assert rec.calls == ["isg_layer_conv_live_tables_enabled", "isg_instances_workspace_bytes", "isg_eval_abi_version",
                         "isg_abi_version"]
    with _lib.using(rec) as handle:                                  # the same swap as a block
        assert handle is rec and mods["isg_fused.h"].load() is rec
        with pytest.raises(ZeroDivisionError):
            with _lib.using(real):
                assert mods["isg_fused.h"].load() is real
                1 / 0
        assert _lib.load() is rec                                    # put back when the block raises, too
    assert _lib.load() is real and mods["isg_fused.h"].load() is real


def test_each_header_keeps_its_three_ways_to_fail(binding, monkeypatch):
    """Stubs stand in for libraries: one lacks a symbol of a header, one answers that header's version call with n + 1."""
    _lib, _ = binding
    real = _lib.load()

    class Stub:
        def __init__(self, **replaced):
            self.replaced = replaced

        def __getattr__(self, name):
            if name in self.replaced:
                if self.replaced[name] is None:
                    raise AttributeError(f"undefined symbol: {name}")
                return self.replaced[name]
            return getattr(real, name)

    assert _lib.checked(Stub()) is not None                          # a stub that lacks nothing passes
    for file, (version, _) in _lib.HEADERS.items():
        _, signatures, abi = _lib.header(file)
        gone = list(signatures)[-1]
        with pytest.raises(_lib.IsgError) as err:
            _lib.checked(Stub(**{gone: None}))
        assert str(err.value) == f"{_lib.LIB_PATH} lacks a symbol of include/{file} (undefined symbol: {gone}): rebuild it (build())"
        with pytest.raises(_lib.IsgError) as err:
            _lib.checked(Stub(**{version: lambda n=abi + 1: n}))
        assert str(err.value) == f"libisg_hip.so {NOUNS[file]}ABI version {abi + 1}, binding expects {abi}"
        with pytest.raises(AttributeError, match=gone):              # bind() alone: the header and the handle disagree
            _lib.bind(Stub(**{gone: None}))
    assert _lib.load() is real                                       # a handle that fails its checks is never the package's
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", os.path.join(ROOT, "no_such_dir", "libisg_hip.so"))
    with pytest.raises(_lib.IsgError, match=r"no_such_dir/libisg_hip\.so not found: the HIP extension is not built"):
        _lib.load()


def test_patching_the_one_load_reaches_every_module(binding, monkeypatch):
    _lib, mods = binding
    other = object()
    monkeypatch.setattr(_lib, "load", lambda: other)
    assert all(mod.load() is other for mod in mods.values())
    monkeypatch.undo()
    assert all(mod.load() is _lib.load() for mod in mods.values())
    fused = mods["isg_fused.h"]                                      # and one module's own load can still be replaced alone
    monkeypatch.setattr(fused, "load", lambda: other)
    assert fused.load() is other and mods["isg_masked.h"].load() is _lib.load()


# ---------------------------------------------------------------------------------------------------------------------
# the extension headers (include/ext/, _lib.EXTENSIONS)
# ---------------------------------------------------------------------------------------------------------------------
def test_the_extension_table_covers_every_extension_header_and_module(extensions):
    _lib, mods = extensions
    on_disk = {os.path.basename(p) for p in glob.glob(os.path.join(ROOT, "include", "ext", "*.h"))}
    assert set(_lib.EXTENSIONS) == on_disk == set(mods) == set(EXT_NOUNS) and not set(_lib.EXTENSIONS) & set(_lib.HEADERS)
    assert list(_lib.EXTENSIONS) == list(EXT_NOUNS), "the order the headers were added in"
    assert {f: noun for f, (_, noun) in _lib.EXTENSIONS.items()} == EXT_NOUNS
    for file, mod in mods.items():
        assert mod.HEADER_PATH == os.path.join(ROOT, "include", "ext", file)
        assert (mod.SIGNATURES, mod.ABI_VERSION) == _lib.read_header(mod.HEADER_PATH), file
        assert _lib.extension(file) == (mod.HEADER_PATH, mod.SIGNATURES, mod.ABI_VERSION)
        assert _lib.extension(file)[1] is mod.SIGNATURES, "extension() parses a header once"
        assert mod.VERSION_SYMBOL == _lib.EXTENSIONS[file][0] and mod.VERSION_SYMBOL in mod.SIGNATURES, file
        others = mod.declared_elsewhere()                            # every device header and the six other extensions
        assert others == _lib.declared_elsewhere(file) and not set(mod.SIGNATURES) & set(others)
        assert set(others) == set(_lib._declared_in) | {n for f in mods if f != file for n in mods[f].SIGNATURES}
        assert all(others[n] == "ext/" + f for f in mods if f != file for n in mods[f].SIGNATURES)
        assert all(others[n] == f for f in _lib.HEADERS for n in _lib.header(f)[1])
    sets = [set(_lib.header(f)[1]) for f in _lib.HEADERS] + [set(_lib.extension(f)[1]) for f in _lib.EXTENSIONS]
    assert len(sets) == 24 and sum(map(len, sets)) == len(set().union(*sets)), "a symbol is declared in two of the 24 headers"


def test_extensions_bind_lazily_each_only_its_own_header(extensions):
    import __graft_entry__ as ge
    _lib, mods = extensions
    fast = _lib.load()
    strict = _lib.bind(ctypes.CDLL(ge.STRICT_LIB))                   # every device header, no extension
    for file in _lib.EXTENSIONS:
        for name in _lib.extension(file)[1]:
            assert getattr(strict, name).argtypes is None, (file, name)
    with _lib.using(strict):
        files = list(_lib.EXTENSIONS)
        for i, file in enumerate(files):
            assert mods[file].load() is strict and _lib.load_extension(file) is strict
            for name, (res, args) in mods[file].SIGNATURES.items():
                fn = getattr(strict, name)
                assert fn.restype == res and list(fn.argtypes or []) == args, (file, name)
            assert getattr(strict, _lib.EXTENSIONS[file][0])() == mods[file].ABI_VERSION
            for later in files[i + 1:]:
                for name in mods[later].SIGNATURES:
                    assert getattr(strict, name).argtypes is None, (file, later, name)
    assert all(mod.load() is fast for mod in mods.values())


def test_a_swap_to_a_proxy_sees_an_extension_s_calls(extensions):
    _lib, mods = extensions
    real = _lib.load()
    assert all(mod.load() is real for mod in mods.values())          # the real handle's extension symbols are bound
    rec = Recorder(real)
    with _lib.using(rec):
        lib = mods["isg_shapley.h"].load()
        assert lib is rec and mods["isg_shapley.h"].load() is rec    # bound and checked once per handle
        # N = -1: refused before any launch (tests/test_shapley_cpu.py)
        assert lib.isg_shapley_keep_bits(4096, 4096, 4096, -1, 2, 2, 4, 12, 1, 5, 1, 4096, 4096, 4096, 4096, None) == -1
        assert mods["isg_curves.h"].load().isg_curve_abi_version() == mods["isg_curves.h"].ABI_VERSION
    assert rec.calls == ["isg_shapley_abi_version", "isg_shapley_keep_bits", "isg_curve_abi_version", "isg_curve_abi_version"]
    assert mods["isg_shapley.h"].load() is real


def test_each_extension_keeps_its_three_ways_to_fail(extensions, monkeypatch):
    _lib, mods = extensions
    real = _lib.load()
    with _lib.using(Stub(real)):
        assert all(_lib.load_extension(file) is _lib.load() for file in _lib.EXTENSIONS)       # a stub that lacks nothing passes
    for file, (version, _) in _lib.EXTENSIONS.items():
        _, signatures, abi = _lib.extension(file)
        gone = list(signatures)[-1]
        for load in (mods[file].load, lambda: _lib.load_extension(file)):
            with _lib.using(Stub(real, **{gone: None})), pytest.raises(_lib.IsgError) as err:
                load()
            assert str(err.value) == \
                f"{_lib.LIB_PATH} lacks a symbol of include/ext/{file} (undefined symbol: {gone}): rebuild it (build())"
            with _lib.using(Stub(real, **{version: lambda n=abi + 1: n})), pytest.raises(_lib.IsgError) as err:
                load()
            assert str(err.value) == f"libisg_hip.so {EXT_NOUNS[file]}ABI version {abi + 1}, binding expects {abi}"
        # a handle that lacks this extension's symbols still serves every other one, and the device headers
        with _lib.using(_lib.checked(Stub(real, **{gone: None}))):
            assert all(_lib.load_extension(f) is _lib.load() for f in _lib.EXTENSIONS if f != file)
    assert _lib.load() is real
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", os.path.join(ROOT, "no_such_dir", "libisg_hip.so"))
    for mod in mods.values():
        with pytest.raises(_lib.IsgError, match=r"no_such_dir/libisg_hip\.so not found: the HIP extension is not built"):
            mod.load()


def test_patching_the_one_load_reaches_every_extension(extensions, monkeypatch):
    _lib, mods = extensions
    other = Stub(_lib.load())
    monkeypatch.setattr(_lib, "load", lambda: other)
    assert all(mod.load() is other for mod in mods.values())
    monkeypatch.undo()
    assert all(mod.load() is _lib.load() for mod in mods.values())


@pytest.mark.parametrize("second, message", [
    ("int isg_curve_sums(int n);", "`isg_curve_sums` is declared in include/ext/isg_curves.h and in include/ext/isg_eighth.h"),
    ("int isg_small_mlps(int n);", "`isg_small_mlps` is declared in include/isg_fused.h and in include/ext/isg_eighth.h"),
    ("int isg_eighth_run(const float *x, int64_t n);", None)],
    ids=["redeclares-an-extension", "redeclares-a-device-header", "not-exported"])
def test_an_eighth_header_needs_a_table_row_and_no_edit_to_build(extensions, monkeypatch, tmp_path, second, message):
    """A made-up header under a made-up include/ext/, entered in the table: what it redeclares is refused by name as soon as it
    is read; what the library does not export fails check_binding(), which build() runs after linking."""
    import __graft_entry__ as ge
    _lib, _ = extensions
    os.makedirs(tmp_path / "ext")
    (tmp_path / "ext" / "isg_eighth.h").write_text(
        "#include <stdint.h>\n#define ISG_EIGHTH_ABI_VERSION 1\nint isg_eighth_abi_version(void);\n" + second + "\n")
    before = ge.header_dependencies()
    monkeypatch.setattr(_lib, "INCLUDE", str(tmp_path))
    monkeypatch.setattr(_lib, "_extensions", dict(_lib._extensions))
    monkeypatch.setattr(_lib, "EXTENSIONS", {**_lib.EXTENSIONS, "isg_eighth.h": ("isg_eighth_abi_version", "eighth ")})
    if message is not None:
        for reads in (lambda: _lib.extension("isg_eighth.h"), ge.header_dependencies, ge.check_binding):
            with pytest.raises(_lib.IsgError) as err:
                reads()
            assert str(err.value) == message
        return
    path, signatures, abi = _lib.extension("isg_eighth.h")
    assert path == str(tmp_path / "ext" / "isg_eighth.h") and list(signatures) == ["isg_eighth_abi_version", "isg_eighth_run"] and abi == 1
    assert signatures["isg_eighth_run"] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64])
    assert ge.header_dependencies() == before + [path]
    with pytest.raises(_lib.IsgError) as err:
        ge.check_binding()
    text = str(err.value)
    assert text.startswith(f"{_lib.LIB_PATH} lacks a symbol of include/ext/isg_eighth.h (") and text.endswith("): rebuild it (build())")
    assert "undefined symbol: isg_eighth_abi_version" in text
    # with a library that has the symbols (a stub answers them), the same table row is all build() needs
    stub = Stub(_lib.load(), isg_eighth_abi_version=lambda: 1, isg_eighth_run=lambda x, n: 0)
    with _lib.using(stub):
        ge.check_binding()
        assert _lib.load_extension("isg_eighth.h") is stub
