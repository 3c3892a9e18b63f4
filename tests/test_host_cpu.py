"""Host-side checks that need no GPU: the C-ABI library loads and exports every declared symbol,
the modules keep the reference's state_dict layout, the product path refuses to run on the CPU."""
import argparse
import glob
import os
import re

import pytest
import torch

from conftest import GOLDEN, ROOT, load_golden


def test_library_exports_every_symbol_in_header():
    import __graft_entry__ as ge
    ge.build()
    from isubgvqa_amd import _lib
    header = open(os.path.join(ROOT, "include", "isg.h")).read()
    declared = set(re.findall(r"\b(isg_[a-z0-9_]+)\s*\(", header))
    assert declared == set(_lib.SIGNATURES), declared ^ set(_lib.SIGNATURES)
    lib = _lib.load()
    for name in declared:
        assert hasattr(lib, name)
    assert lib.isg_abi_version() == _lib.ABI_VERSION == int(re.search(r"#define ISG_ABI_VERSION (\d+)", header).group(1))
    assert lib.isg_status_string(-2) == b"unsupported shape"
    assert lib.isg_csr_workspace_bytes(10, 7) == (2 * 11 + 7 + 2) * 4


def test_binding_is_derived_from_the_header_rule_by_rule():
    """_lib.parse_header on small headers: every mapping rule of the two real headers, and nothing a comment says."""
    import ctypes as ct
    from isubgvqa_amd import _lib
    sigs, abi = _lib.parse_header("""
        #include <stdint.h>
        #define ISG_ABI_VERSION 7
        /* not a declaration: int isg_in_comment(int64_t n);  nor this call: isg_called( x ) */
        // nor this one: float isg_line_comment(void);
        typedef struct isg_thing isg_thing;
        int isg_a(void);
        const char *isg_b(int status);
        void isg_c(isg_thing *t);
        size_t isg_d(int64_t n, int32_t c, uint64_t seed, size_t bytes, float slope, double eps);
        int64_t isg_e(const float *x, int32_t *const out, void *stream, const char *path,
                      const char *const *names, isg_thing **made);
        """)
    assert abi == 7
    assert list(sigs) == ["isg_a", "isg_b", "isg_c", "isg_d", "isg_e"]
    assert sigs["isg_a"] == (ct.c_int, [])
    assert sigs["isg_b"] == (ct.c_char_p, [ct.c_int])
    assert sigs["isg_c"] == (None, [ct.c_void_p])
    assert sigs["isg_d"] == (ct.c_size_t, [ct.c_int64, ct.c_int32, ct.c_uint64, ct.c_size_t, ct.c_float, ct.c_double])
    assert sigs["isg_e"] == (ct.c_int64, [ct.c_void_p, ct.c_void_p, ct.c_void_p, ct.c_char_p, ct.c_void_p, ct.c_void_p])
    # the real headers: the library's own answers are bound as the header types them
    assert _lib.SIGNATURES["isg_csr_workspace_bytes"] == (ct.c_size_t, [ct.c_int64, ct.c_int64])
    assert _lib.SIGNATURES["isg_status_string"] == (ct.c_char_p, [ct.c_int])
    from isubgvqa_amd import loader
    assert loader.SIGNATURES["isg_sg_vocab_free"] == (None, [ct.c_void_p])
    assert loader.SIGNATURES["isg_sg_vocab_lookup"] == (ct.c_int64, [ct.c_void_p, ct.c_char_p])


@pytest.mark.parametrize("decl, says", [
    ("int isg_x(long n);", "type `long`"),                                   # a type word the headers do not use
    ("int isg_x(unsigned int n);", "type `unsigned int`"),
    ("bool isg_x(int n);", "type `bool`"),                                   # ... as a return type
    ("ISG_API int isg_x(int n);", "type `ISG_API int`"),
    ("int isg_x(const float x[4], int n);", "array, function-pointer or variadic"),
    ("int isg_x(void (*done)(int), int n);", "array, function-pointer or variadic"),
    ("int isg_x(const char *fmt, ...);", "array, function-pointer or variadic"),
    ("int isg_x(int64_t, int32_t c);", "has no name"),
    ("int isg_x(const float *, int32_t c);", "has no name"),
    ("int isg_x(void v);", "parameter `void v`"),
    ("static inline int isg_x(int n) { return n; } int isg_y(void);", "not a plain function declaration"),
    ("int isg_x(int n), isg_y(int n);", "array, function-pointer or variadic"),
    ("*isg_x(int n);", "type `*`"),
    ("const isg_x(int n);", "type `const`"),
    ("int isg_x(int * n, float *const *p, const *q);", "type `const *`"),
    ("int isg_x(int n); int isg_x(int64_t n);", "declared twice"),
])
def test_binding_refuses_a_declaration_it_does_not_understand(decl, says):
    """A declaration that was skipped or half-understood would be a symbol bound with the wrong registers: each raises, with
    the declaration's text."""
    from isubgvqa_amd import _lib
    with pytest.raises(ValueError, match="isg_x") as err:
        _lib.parse_header("#define ISG_ABI_VERSION 1\nint isg_ok(void);\n" + decl)
    assert says in str(err.value), str(err.value)


def test_binding_counts_the_declarations_it_skipped():
    """Every `isg_name(` of the comment-stripped header has to be a declaration that was parsed: one that was passed over (no `;`
    behind it) is named instead of silently left unbound."""
    from isubgvqa_amd import _lib
    with pytest.raises(ValueError, match=r"not understood: \['isg_skipped'\]"):
        _lib.parse_header("#define ISG_ABI_VERSION 1\nint isg_ok(void);\nint isg_skipped(int n)\n")
    for text in ("int isg_ok(void);", "#define ISG_ABI_VERSION 1\n#define ISG_LOADER_ABI_VERSION 2\nint isg_ok(void);"):
        with pytest.raises(ValueError, match="ABI_VERSION"):
            _lib.parse_header(text)
    with pytest.raises(_lib.IsgError, match="no_such_dir/isg.h"):
        _lib.read_header(os.path.join(ROOT, "no_such_dir/isg.h"))


def test_cache_entry_made_from_a_tensor_holds_for_that_tensor_only():
    """The plan's edge planes and the oversize graphs' edge rows are kept "for this very edge_attr": the same object (held
    weakly -- a freed tensor's id and address can be handed to the next one), version, storage and shape."""
    import gc
    from isubgvqa_amd import ops
    t = torch.zeros(6, 4)
    entry = ops._from_tensor(t, "made")
    assert ops._if_from_tensor(entry, t) == "made" and ops._if_from_tensor(None, t) is None
    assert ops._if_from_tensor(entry, t.view(6, 4)) is None          # same storage, version and shape: another object
    assert ops._if_from_tensor(entry, t.clone()) is None
    t.add_(1.0)
    assert ops._if_from_tensor(entry, t) is None                     # written in place since
    entry = ops._from_tensor(t, "made")
    ref = entry[0]
    del t
    gc.collect()
    assert ref() is None                                             # the entry does not keep the tensor alive ...
    assert ops._if_from_tensor(entry, torch.zeros(6, 4)) is None     # ... and no later tensor is taken for it


def test_product_path_fails_loudly_on_cpu_tensors():
    from isubgvqa_amd import _lib, ops
    with pytest.raises(_lib.IsgError):
        ops.instr_gate(torch.zeros(4, 8), torch.zeros(2, 8), torch.zeros(4, dtype=torch.long))
    with pytest.raises(_lib.IsgError):
        ops.GraphPlan.build(torch.zeros(4, dtype=torch.long), num_graphs=1, max_nodes=4)


def test_product_package_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "intrinsic-subgraph-generation-for-vqa_amd")
    for path in glob.glob(os.path.join(pkg, "**", "*.py"), recursive=True):
        src = open(path).read()
        assert not re.search(r"^\s*(from|import)\s+oracle\b", src, re.M), path
        assert "/root/reference" not in src, path


G5 = sorted(glob.glob(os.path.join(GOLDEN, "g5_mgat_*.pt")))


@pytest.mark.parametrize("path", G5, ids=[os.path.basename(p) for p in G5])
def test_mgat_and_pooling_accept_reference_state_dict(path):
    from isubgvqa_amd.models import MGAT, GlobalAttention
    g = torch.load(path, map_location="cpu", weights_only=False)
    c = g["cfg"]
    m = MGAT(channels=c["C"], num_ins=c["L"], heads=4, use_instr=True, masking_thresholds=c["masks"], use_topk=True,
             interpretable_mode=c["interp"], sampler_type=c["sampler"], sample_k=c["k"])
    sd = {k[len("gat_seq."):]: v for k, v in g["sd"].items() if k.startswith("gat_seq.")}
    res = m.load_state_dict(sd, strict=False)
    assert not res.unexpected_keys, res.unexpected_keys
    assert all(k.startswith("node_logits.") for k in res.missing_keys), res.missing_keys   # dropped from the fixture
    p = GlobalAttention(c["C"], c["C"])
    p.load_state_dict({k[len("graph_global_attention_pooling."):]: v for k, v in g["sd"].items()
                       if k.startswith("graph_global_attention_pooling.")}, strict=True)


def test_question_modules_accept_reference_state_dict():
    from isubgvqa_amd.models import CLIPTextEmbeddings, QuestionDecoder, QuestionEncoder
    g = load_golden("g4_question.pt")
    enc = QuestionEncoder(CLIPTextEmbeddings(50, 32, 77), 32, 32, g["nhead"], 64, 2, 0.1)
    res = enc.load_state_dict({k[len("question_encoder."):]: v for k, v in g["sd"].items()
                               if k.startswith("question_encoder.")}, strict=False)
    assert not res.unexpected_keys and res.missing_keys == ["pos_encoder.pe"], res
    dec = QuestionDecoder(4, 32, g["nhead"], 64, 2, 0.1)
    dec.load_state_dict({k[len("program_decoder."):]: v for k, v in g["sd"].items()
                         if k.startswith("program_decoder.")}, strict=True)


def _args(**kw):
    d = dict(text_sampling=False, general_hidden_dim=300, distributed=False, mgat_layers=4, use_all_instrs=False,
             use_global_mask=False, node_classification=False, sampler_type="imle", sample_k=5, nb_samples=1,
             alpha=1.0, beta=10.0, tau=1.0, use_masking=True, use_instruction=1, use_mgat=True,
             mgat_masks=[1.0, 1.0, 1.0, 0.15], use_topk=True, interpretable_mode=False, concat_instr=0, embed_cat=0,
             device="cpu", text_vocab_size=64, sg_vocab_size=40)
    d.update(kw)
    return argparse.Namespace(**d)


def test_isubgvqa_state_dict_layout_matches_appendix_c():
    from isubgvqa_amd.models import build_model
    m = build_model(_args(), None)
    sd = m.state_dict()
    C, H = 300, 4
    expect = {
        "scene_graph_encoder.sg_vocab_embedding.weight": (40, 300),
        "scene_graph_encoder.scene_graph_encoding_layer.edge_model.edge_mlp.0.weight": (C, 900),
        "scene_graph_encoder.scene_graph_encoding_layer.node_model.node_mlp_1.0.weight": (C, 600),
        "scene_graph_encoder.scene_graph_encoding_layer.node_model.node_mlp_2.2.weight": (C, C),
        "scene_graph_encoder.graph_layer_norm.mean_scale": (300,),
        "scene_graph_encoder.bbox_encoding.0.running_mean": (4,),
        "scene_graph_encoder.bbox_encoding.4.weight": (32, 16),
        "scene_graph_encoder.feat_reduc.1.weight": (300, 332),
        "text_vocab_embedding.token_embedding.weight": (64, 512),
        "question_encoder.text_vocab_embedding.position_embedding.weight": (77, 512),
        "question_encoder.emb_proj.weight": (512, 512),
        "question_encoder.pos_encoder.pe": (5000, 1, 512),
        "question_encoder.transformer_encoder.layers.3.self_attn.in_proj_weight": (1536, 512),
        "question_encoder.transformer_encoder.layers.0.linear1.weight": (2048, 512),
        "question_encoder.transformer_encoder.norm.weight": (512,),
        "program_decoder.query_embed.weight": (4, 512),
        "program_decoder.coarse_decoder.layers.2.multihead_attn.out_proj.weight": (512, 512),
        "program_decoder.coarse_decoder.layers.0.norm3.bias": (512,),
        "gat_seq.convs.3.att": (1, H, C),
        "gat_seq.convs.0.bias": (H * C,),
        "gat_seq.convs.0.lin_l.weight": (H * C, C),
        "gat_seq.convs.0.lin_r.bias": (H * C,),
        "gat_seq.convs.0.lin_edge.weight": (H * C, C),
        "gat_seq.convs.0.mask.gate_nn.2.weight": (1, C),
        "gat_seq.convs.0.mask.node_nn.0.weight": (C, C),
        "gat_seq.convs.0.mask.ques_nn.0.bias": (C,),
        "gat_seq.convs.0.mask.gate_top.select.weight": (1, C),
        "gat_seq.x_proj.1.0.weight": (H * C // 2, H * C),
        "gat_seq.x_proj.1.2.weight": (C, H * C // 2),
        "gat_seq.bns.2.mean_scale": (C,),
        "gat_seq.node_logits.2.weight": (2577, 512),
        "graph_global_attention_pooling.gate_nn.2.weight": (1, C),
        "graph_global_attention_pooling.node_nn.2.weight": (C, C),
        "graph_global_attention_pooling.ques_nn.0.weight": (C, C),
        "qsts_reduction.0.weight": (C, 2048),
        "instr_reduction.0.weight": (C, 512),
        "embedding.0.weight": (512, 3 * C),
        "logit_fc.weight": (1842, 512),
    }
    for k, shp in expect.items():
        assert k in sd, k
        assert tuple(sd[k].shape) == shp, (k, tuple(sd[k].shape))
    assert "gat_seq.convs.0.lin_edge.bias" not in sd
    # the CLIP embedding module is shared, so its tensors appear under both prefixes (isubgvqa.py:120,126-127)
    assert sd["text_vocab_embedding.token_embedding.weight"].data_ptr() == \
        sd["question_encoder.text_vocab_embedding.token_embedding.weight"].data_ptr()
    # a DDP checkpoint carries a "module." prefix (train_loop.py:89): stripping it must load strictly
    ddp = {"module." + k: v for k, v in sd.items()}
    m2 = build_model(_args(), None)
    m2.load_state_dict({k[len("module."):]: v for k, v in ddp.items()}, strict=True)


def test_forward_requires_return_masks_like_the_reference():
    from isubgvqa_amd.models import build_model
    m = build_model(_args(), None).eval()
    with pytest.raises(ValueError):
        m(None, None, None, None, None, None, return_masks=False)


def test_synthetic_cfg2_shapes():
    from isubgvqa_amd import synthetic
    cfg = synthetic.WorkloadConfig(num_graphs=512)
    wl = synthetic.make_workload(cfg)
    N, E = wl.x.size(0), wl.edge_index.size(1)
    assert 18.0 < N / 512 < 22.0 and 45.0 < E / 512 < 55.0
    assert torch.equal(wl.batch, wl.batch.sort().values)
    b = wl.batch
    assert torch.equal(b[wl.edge_index[0]], b[wl.edge_index[1]])          # edges stay inside their graph
    assert wl.edge_index.min() >= 0 and wl.edge_index.max() < N
    n = torch.bincount(b)
    assert n.min() >= 4 and n.max() <= 48 and wl.max_nodes == int(n.max())
    # every node has its self-loop
    loops = wl.edge_index[0] == wl.edge_index[1]
    assert torch.unique(wl.edge_index[0][loops]).numel() == N
    wl5 = synthetic.make_workload(synthetic.WorkloadConfig(num_graphs=256, nodes_dist="pareto", nodes_min=8,
                                                           nodes_max=200, edges_per_graph=0.0, degree="powerlaw"))
    deg = torch.bincount(wl5.edge_index[1], minlength=wl5.x.size(0))
    assert deg.max() > 8 * deg.float().mean()                            # hubs exist


def test_reference_checkpoint_reader_roundtrip(tmp_path):
    """A checkpoint in the reference's layout (train_loop.py:84-130: DDP 'module.' prefix, pickled Namespace) loads
    strictly into the drop-in model."""
    from isubgvqa_amd.checkpoint import load_model, read_checkpoint
    from isubgvqa_amd.models import build_model
    torch.manual_seed(3)
    src = build_model(_args(sampler_type="gumbel"), None)
    args = _args(sampler_type="gumbel")
    del args.nb_samples                                   # an older Namespace without this flag
    path = os.path.join(tmp_path, "checkpoint.pth")
    torch.save({"model": {"module." + k: v for k, v in src.state_dict().items()}, "optimizer": {"state": {}},
                "lr_scheduler": {}, "epoch": 7, "args": args}, path)
    sd, got_args, rest = read_checkpoint(path)
    assert rest["epoch"] == 7 and got_args.nb_samples == 1 and not any(k.startswith("module.") for k in sd)
    model, _, _ = load_model(path, device="cpu")
    assert not model.training
    for k, v in src.state_dict().items():
        assert torch.equal(model.state_dict()[k], v), k


def test_docs_quote_the_headers_symbol_count_and_abi_version():
    """README.md / DESIGN.md / INTEGRATION.md quote the number of C-ABI symbols and the ABI version; both drifted more than
    once while entry points were added.  They are checked against include/isg.h."""
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "isg.h")).read()
    body = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    n_sym = len(set(re.findall(r"\b(isg_[a-z0-9_]+)\s*\(", body)))
    abi = int(re.search(r"#define ISG_ABI_VERSION (\d+)", hdr).group(1))
    readme = open(os.path.join(root, "README.md")).read()
    m = re.search(r"\((\d+) symbols, ABI v(\d+)\)", readme)
    assert m, "README.md no longer states '(N symbols, ABI vM)'"
    assert (int(m.group(1)), int(m.group(2))) == (n_sym, abi), f"README says {m.groups()}, header has {n_sym} symbols, ABI v{abi}"
    for name in ("DESIGN.md", "INTEGRATION.md"):
        text = open(os.path.join(root, name)).read()
        for q in re.findall(r"(\d+) (?:`extern \"C\"` )?symbols", text) + re.findall(r"for all (\d+)\b", text):
            if 30 <= int(q) <= 200:      # counts of the device library (the loader's 15 are quoted too)
                assert int(q) == n_sym, f"{name} quotes {q} symbols, include/isg.h declares {n_sym}"
    # INTEGRATION.md's binding stubs: the argtypes / restype lines a maintainer would copy are hand-written and reviewed; the
    # binding derived from the header has to agree with each of them
    import ctypes
    from isubgvqa_amd import _lib
    names = dict(zip(("P", "I64", "I32", "F32"), (ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_float)), ctypes=ctypes)
    text = open(os.path.join(root, "INTEGRATION.md")).read()
    assert "P, I64, I32, F32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_float" in text
    quoted = re.findall(r"^_lib\.(isg_\w+)\.(restype|argtypes) = ([^#\n]+)", text, flags=re.M)
    assert {(n, k) for n, k, _ in quoted} == {
        ("isg_graph_ptr", "argtypes"), ("isg_csr_workspace_bytes", "restype"), ("isg_csr_workspace_bytes", "argtypes"),
        ("isg_csr_build", "argtypes"), ("isg_gatv2_mp_fwd", "argtypes"), ("isg_planes32_elems", "restype"),
        ("isg_planes32_elems", "argtypes"), ("isg_split_planes32", "argtypes"), ("isg_linear_h3p", "argtypes")}, quoted
    for sym, kind, value in quoted:
        restype, argtypes = _lib.SIGNATURES[sym]
        got = eval(value, dict(names))
        assert got == (argtypes if kind == "argtypes" else restype), f"INTEGRATION.md: {sym}.{kind} = {value.strip()}, header: {(restype, argtypes)}"


def test_library_holds_no_cross_selecting_packed_fp32_operation():
    """on gfx950 a v_pk_fma_f32 / v_pk_mul_f32 / v_pk_add_f32 that takes a LOW-half operand from the HIGH dword of
    a register pair (op_sel:[..1..]) intermittently lost its low-half result in isg_gatv2_tile_conv (tools/flake/: 48-417 wrong
    launches of 1600 in every variant with the form, 0 of 1600 without).  The form is the compiler's choice, so the guard reads the
    BUILT library: every gfx950 code object is disassembled and must hold none (round 4 had 31 in five kernels)."""
    import importlib.util
    import __graft_entry__ as ge
    ge.build()
    spec = importlib.util.spec_from_file_location("scan_pk_cross", os.path.join(ROOT, "tools", "scan_pk_cross.py"))
    scan = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(scan)
    # the scanner sees the form where it is (a line of round 4's failing loop) and only there
    sample = ["0000 <_Zkernel>:", "\tv_pk_fma_f32 v[34:35], v[44:45], v[52:53], v[34:35] op_sel_hi:[1,0,1] // 0001: AA",
              "\tv_pk_fma_f32 v[34:35], v[48:49], v[52:53], v[34:35] op_sel:[0,1,0] // 0002: BB",
              "\tv_pk_mul_f32 v[20:21], v[228:229], v[20:21] op_sel:[1,0]", "\tv_pk_add_f32 v[2:3], v[4:5], v[6:7]",
              "\tv_pk_fma_f16 v1, v2, v3, v4 op_sel:[0,1,0]"]
    total, hits = scan.scan_text(sample, re.compile(r"^[0-9a-f]+ <(\S+)>:"))
    assert total == 4 and [h[1].split()[0] for h in hits] == ["v_pk_fma_f32", "v_pk_mul_f32"] and hits[0][0] == "_Zkernel"
    if not os.path.exists(scan.OBJDUMP):
        pytest.skip(f"{scan.OBJDUMP} is not installed: the built libraries cannot be disassembled here")
    # both shipped libraries: tests/test_gpu_strict.py demands equal bits from the strict build, so a cross-selecting operation that
    # exists only there would show up as a "schedule bug" of the fast one
    for lib in (scan.LIB, scan.STRICT_LIB):
        objects, total, hits = scan.scan_library(lib)
        assert objects >= 18 and total > 10000, (lib, objects, total)    # the whole library was read, not an empty extraction
        assert not hits, os.path.basename(lib) + ":\n" + "\n".join(f"{scan.demangle(k)}: {t}" for k, t in hits[:10])


def test_kernel_argument_structs_are_built_by_one_complete_initialiser():
    """Round 5's GPU fault was a kernel-argument struct filled field by field with one assignment lost; the
    in-process suite passed because the stack slot still held the previous call's pointers.  Since round 6 every `*Args` struct
    that is passed to a kernel is built by ONE braced initialiser and the build refuses a field left out
    (-Werror=missing-field-initializers in HIP_FLAGS).  This test holds the three parts of that together:
      (1) the flag is in the flags every source is compiled with, and it does refuse an incomplete initialiser (hipcc, syntax only);
      (2) no source declares an argument struct without an initialiser, or with the empty one, and fills it afterwards;
      (3) every designated initialiser names every field of its struct (what the compiler enforces, read from the text), and every
          pointer the struct hands to a kernel is either null-checked on the STRUCT (`!a.field`) before the launch or documented
          as optional (`NULL` / `optional` / `may be` in the field's comment)."""
    import subprocess
    import tempfile
    import __graft_entry__ as ge
    assert "-Werror=missing-field-initializers" in ge.HIP_FLAGS
    probe = ("struct PArgs { const float *p; const int *q; int n; };\n__global__ void k(PArgs a) { if (a.q) *(float *)a.p = a.n; }\n"
             "void f(const float *p) { PArgs a = {.p = p, .n = 1}; k<<<1, 1>>>(a); }\n"
             "void g(const float *p) { PArgs a{p}; k<<<1, 1>>>(a); }\n")
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, "probe.hip")
        open(src, "w").write("#include <hip/hip_runtime.h>\n" + probe)
        r = subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), *ge.HIP_FLAGS, "--cuda-host-only", "-fsyntax-only", src],
                           capture_output=True, text=True)
    assert r.returncode != 0 and r.stderr.count("missing field 'q' initializer") >= 2, r.stderr[-2000:]
    csrc = os.path.join(ROOT, "intrinsic-subgraph-generation-for-vqa_amd", "csrc")
    structs, texts = {}, {}
    for f in sorted(os.listdir(csrc)):
        if not f.endswith((".hip", ".hpp")):
            continue
        text = open(os.path.join(csrc, f)).read()
        texts[f] = text
        for m in re.finditer(r"struct (\w+Args) \{(.*?)\n\};", text, flags=re.S):
            fields = []          # (name, is_pointer, optional)
            for line in m.group(2).split("\n"):
                code, _, comment = line.partition("//")
                code = code.strip().rstrip(";")
                if not code:
                    if fields and comment:          # a comment line continues the previous field's description
                        fields[-1][2] = fields[-1][2] or bool(re.search(r"NULL|optional|may be", comment))
                    continue
                names = re.findall(r"(\*?)\s*(\w+)\s*(?:,|$)", code.split(None, 1)[1] if " " in code else code)
                first_ptr = "*" in code.split(",")[0]
                for i, (star, name) in enumerate(names):
                    fields.append([name, bool(star) or (i == 0 and first_ptr), bool(re.search(r"NULL|optional|may be", comment))])
            structs[m.group(1)] = fields
    assert len(structs) >= 13, sorted(structs)
    for f, text in texts.items():
        body = re.sub(r"struct \w+ \{.*?\n\};", "", text, flags=re.S)          # a member `P3Args p;` of another struct is not a fill site
        for name in structs:
            bad = re.findall(rf"\b(?:isg::)?{name} \w+(?: = \{{\}})?;", body)
            assert not bad, f"{f}: `{bad[0]}` -- build the struct with one initialiser that names every field"
        for m in re.finditer(r"\b(?:isg::)?(\w+Args) (\w+) = \{\s*\.(.*?)\};", body, flags=re.S):
            name, var, init = m.group(1), m.group(2), "." + m.group(3)
            named = re.findall(r"\.(\w+) =", init)
            want = [fl[0] for fl in structs[name]]
            assert named == want, f"{f}: {name} initialiser names {named}, the struct declares {want}"
            after = body[m.end():m.end() + 1500]
            for fname, is_ptr, optional in structs[name]:
                if is_ptr and not optional and name != "Q3Args":
                    assert re.search(rf"!{var}\.{fname}\b", after), f"{f}: {name}.{fname} is handed to a kernel without `!{var}.{fname}` behind the initialiser"


def test_switches_are_one_frozen_object_swapped_atomically():
    """ops' A/B switches live in ONE frozen dataclass (ops.CFG): the historical spelling `ops.NAME = value` (tests, tools, bench.py)
    replaces the whole object, `ops.NAME` reads the field, `with ops.configured(...)` restores; a field cannot be written in place."""
    import dataclasses
    from isubgvqa_amd import ops
    before = ops.CFG
    assert dataclasses.is_dataclass(before) and ops.SPLIT_FORWARD is before.split_forward
    with pytest.raises(dataclasses.FrozenInstanceError):
        before.split_forward = False
    try:
        ops.SPLIT_FORWARD = not before.split_forward
        assert ops.CFG is not before and ops.CFG.split_forward == (not before.split_forward) and before.split_forward != ops.SPLIT_FORWARD
        assert ops.CFG.mixed_min_nodes == before.mixed_min_nodes            # every other field carried over
        with ops.configured(mixed_min_nodes=7, gemm_kernel="panel") as cfg:
            assert ops.MIXED_MIN_NODES == 7 and ops.GEMM_KERNEL == "panel" and cfg is ops.CFG
        assert ops.MIXED_MIN_NODES == before.mixed_min_nodes and ops.GEMM_KERNEL == before.gemm_kernel
        with pytest.raises(TypeError):
            with ops.configured(no_such_switch=1):
                pass
        assert not hasattr(ops, "NO_SUCH_SWITCH")
    finally:
        ops.CFG = before
    assert ops.CFG is before


F16 = torch.float16
# (M, N, K, linear_route keywords, switch overrides, the kernel ops.linear launched for it before the routing was one function)
ROUTES = [
    # thresholds under the default switches, each side
    (1024, 512, 512, {}, {}, "skinny"), (1025, 512, 512, {}, {}, "bf16x6"),                              # skinny_max_m
    (1024, 1024, 1024, {}, {}, "skinny"), (1024, 1024, 1028, {}, {}, "bf16x6"),                          # skinny_max_work
    (2047, 512, 512, {"carries_planes": True}, {}, "bf16x6"), (2048, 512, 512, {"carries_planes": True}, {}, "h3p"),   # h3p_min_m
    (8191, 512, 512, {}, {}, "f16x3_tile"), (8192, 512, 512, {}, {}, "h3p"),                             # h3p_min_m_unsplit
    (8191, 512, 512, {"carries_planes": True}, {}, "h3p"), (8192, 512, 512, {"aligned": False}, {}, "f16x3_tile"),
    (8192, 512, 252, {}, {}, "f16x3_tile"), (8192, 512, 256, {}, {}, "h3p"), (8192, 510, 256, {}, {}, "f16x3_tile"),  # h3p_min_k, 4 | N
    (32767, 256, 128, {}, {}, "bf16x6"), (32768, 256, 128, {}, {}, "f16x3"),                             # the panel rule: M
    (32768, 256, 132, {}, {}, "f16x3_tile"), (32768, 255, 128, {}, {}, "bf16x6"),                        # K, N
    (4095, 256, 300, {}, {}, "bf16x6"), (4096, 256, 300, {}, {}, "f16x3_tile"), (4096, 255, 300, {}, {}, "bf16x6"),   # f16x3_tile
    (1025, 96, 300, {"rowmax_slices": True}, {}, "f16x3_tile"), (4095, 256, 128, {"rowmax_slices": True}, {}, "bf16x6"),
    (1 << 23, 256, 300, {"aligned": False}, {}, "bf16x6"),
    # fp16 rows in / out, ReLU, autograd, no rows, K % 4, a Planes32, isg_linear_skinny refusing the layout
    (32768, 256, 128, {"x_dtype": F16}, {}, "panel"), (32768, 256, 128, {"out_dtype": F16}, {}, "f16x3_f16"),
    (12, 512, 512, {"out_dtype": F16}, {}, "bf16x6_f16"), (8192, 512, 512, {"x_dtype": F16}, {}, "bf16x6_f16"),
    (12, 512, 512, {"relu": True}, {}, "skinny"), (32768, 256, 128, {"relu": True}, {}, "bf16x6"),
    (12, 512, 512, {"recording": True}, {}, "autograd"), (12, 512, 512, {"recording": True, "relu": True}, {}, "torch"),
    (0, 512, 512, {}, {}, "empty"), (0, 512, 512, {"relu": True}, {}, "torch"), (0, 512, 512, {"recording": True}, {}, "empty"),
    (12, 512, 37, {}, {}, "torch"), (12, 512, 37, {"recording": True}, {}, "torch"),
    (12, 512, 512, {"planes32": True}, {}, "h3p"), (12, 512, 512, {"skinny_layout": False}, {}, "bf16x6"),
    # the overrides tests and tools use
    (12, 512, 512, {}, {"gemm_kernel": "panel"}, "panel"), (12, 512, 128, {}, {"gemm_kernel": "panel"}, "f16x3"),
    (12, 512, 512, {"relu": True}, {"gemm_kernel": "panel"}, "bf16x6"),
    (32768, 256, 128, {}, {"gemm_kernel": "tile"}, "bf16x6"), (8192, 512, 512, {}, {"gemm_kernel": "tile"}, "bf16x6"),
    (32768, 256, 128, {}, {"gemm_f16x3": False}, "panel"), (8192, 512, 512, {}, {"gemm_f16x3": False}, "bf16x6"),
    (32768, 256, 128, {"out_dtype": F16}, {"f16x3_f16_out": False}, "panel"),
    (12, 512, 512, {}, {"gemm_backend": "torch"}, "torch"), (0, 512, 512, {}, {"gemm_backend": "torch"}, "empty"),
    (12, 512, 512, {}, {"skinny": False}, "bf16x6"),
    (12, 512, 512, {"carries_planes": True}, {"h3p_min_m": 1}, "skinny"),
    (1025, 512, 512, {"carries_planes": True}, {"h3p_min_m": 1}, "h3p"), (1025, 512, 512, {}, {"h3p_min_m": 1}, "bf16x6"),
    # real shapes.  One question of the full model (C = 300): every Linear on isg_linear_skinny, the [V, C] table aside
    (1, 1842, 512, {}, {}, "skinny"), (12, 1536, 512, {"rowmax_slices": True}, {}, "skinny"),
    (12, 2048, 512, {"relu": True, "rowmax_slices": True}, {}, "skinny"), (21, 600, 1200, {}, {}, "skinny"),
    (45, 1200, 300, {}, {}, "skinny"), (2578, 300, 300, {}, {}, "bf16x6"),
    # configs[1] (4096 graphs, C = 128)
    (4096, 128, 128, {}, {}, "bf16x6"), (4096, 1842, 512, {"rowmax_slices": True}, {}, "f16x3_tile"),
    (4096, 512, 384, {"rowmax_slices": True}, {}, "f16x3_tile"),
    # the full model at C = 300 over 4096 graphs
    (16384, 1536, 512, {}, {}, "h3p"), (4096, 300, 2048, {}, {}, "f16x3_tile"), (4096, 300, 300, {}, {}, "f16x3_tile"),
    (82189, 2400, 300, {"carries_planes": True}, {}, "h3p"), (82189, 32, 16, {}, {}, "bf16x6"), (82189, 300, 332, {}, {}, "h3p"),
    (204753, 300, 300, {}, {}, "h3p"),
    # configs[4] (2048 skewed graphs, fp16 rows)
    (43633, 1024, 128, {"out_dtype": F16}, {}, "f16x3_f16"), (43633, 128, 256, {}, {}, "h3p"),
    (43633, 256, 512, {"x_dtype": F16}, {}, "bf16x6_f16"), (43633, 128, 128, {}, {}, "bf16x6"),
]


@pytest.mark.parametrize("M,N,K,kw,switches,kernel", ROUTES)
def test_linear_route_names_the_kernel_a_linear_runs_on(M, N, K, kw, switches, kernel):
    """ops.linear_route is the whole decision of which kernel runs a Linear (which kernel a row meets depends on the batch's size):
    each side of every threshold, the switches' overrides, and the Linears of real forwards."""
    from isubgvqa_amd import ops
    with ops.configured(**switches):
        assert ops.linear_route(M, N, K, **kw) == kernel
    assert ops.linear_route(M, N, K, cfg=ops.Switches(**switches), **kw) == kernel


def test_linear_route_memo_follows_the_switches_and_what_the_input_carries():
    """ops.linear memoises the route per shape and switch object; a changed switch or attachment is seen on the next call."""
    from isubgvqa_amd import ops
    x = torch.zeros(2048, 512)
    assert ops._route(x, 2048, 512, 512, torch.float32, False, False) == "bf16x6"
    ops._attach(x, "_isg_planes32", object())
    assert ops._route(x, 2048, 512, 512, torch.float32, False, False) == "h3p"
    with ops.configured(h3p=False):
        assert ops._route(x, 2048, 512, 512, torch.float32, False, False) == "bf16x6"
    x.add_(1.0)                                      # an in-place write invalidates the planes
    assert ops._route(x, 2048, 512, 512, torch.float32, False, False) == "bf16x6"


# facts of BASELINE configs[1]'s batch (4096 graphs) and layer (C = 128, H = 4, every width 128): what CONV_ROUTES' rows override
_CONV = dict(heads=4, channels=128, in_channels=128, edge_dim=128, N=82189, B=4096, E=204753, nmax=40, has_csr=True, tile_mode="tiles")
_C300 = dict(channels=300, in_channels=300, edge_dim=300)
_SMALL = dict(N=5000, B=200, E=16383)
UNFUSED = ("unfused", "rows", True, True)
# (conv_route keywords over _CONV, switch overrides, (conv, gate, gate_rows, e_proj))
CONV_ROUTES = [
    ({}, {}, ("layer_conv", "planes", False, False)),
    # the layer kernel: a 128-wide input, lin_l and lin_r distinct, H <= 16 (H x ceil32(C) <= 2048 ends the fused logits at C = 128)
    ({"in_channels": 300}, {}, ("tile_conv", "planes32", True, False)), ({"in_channels": 64}, {}, ("tile_conv", "rows", True, False)),
    ({"share_weights": True}, {}, ("tile_conv", "rows", True, False)),
    ({"heads": 16}, {}, ("layer_conv", "planes", False, False)), ({"heads": 17}, {}, UNFUSED),
    ({"heads": 64, "channels": 32}, {}, ("pair", "rows", True, False)), ({"heads": 65, "channels": 32}, {}, UNFUSED),
    # edge widths: the tile kernels to 128, the rows kernel to 304, multiples of 4
    ({"edge_dim": 64}, {}, ("layer_conv", "planes", False, False)), ({"edge_dim": 132}, {}, ("pair", "rows", True, False)),
    ({"edge_dim": 304}, {}, ("pair", "rows", True, False)), ({"edge_dim": 308}, {}, UNFUSED), ({"edge_dim": 130}, {}, UNFUSED),
    ({"edge_dim": None}, {}, UNFUSED),
    # head dimensions: C = 128 on tiles, 32 | C or not (wide) on the per-graph pair, 4 !| C nowhere
    ({"channels": 96}, {}, ("pair", "rows", True, False)), (_C300, {}, ("pair", "planes32", True, False)),
    ({"channels": 130}, {}, UNFUSED),
    # a wide layer on each side of rows_kernel_min_edges; a narrow one does not care
    ({**_C300, **_SMALL}, {}, ("unfused", "planes32", True, True)), ({**_C300, **_SMALL, "E": 16384}, {}, ("pair", "planes32", True, False)),
    ({**_SMALL, "edge_dim": 132}, {}, UNFUSED), (_SMALL, {}, ("layer_conv", "planes", False, False)),
    ({**_C300, **_SMALL}, {"rows_kernel_min_edges": 1000}, ("pair", "planes32", True, False)),
    # nothing to do, no CSR
    ({"N": 100, "B": 5, "E": 0}, {}, UNFUSED), ({"N": 0, "B": 0, "E": 0, "nmax": 0}, {}, UNFUSED), ({"has_csr": False}, {}, UNFUSED),
    # half rows (configs[4]): the pair on the rows kernel from K = 128; an oversize batch keeps fp32 rows and is beyond the tiles too
    ({"rows_dtype": F16, "edge_dim": 64}, {}, UNFUSED), ({"rows_dtype": F16}, {}, ("pair", "rows", True, False)),
    ({"rows_dtype": torch.bfloat16}, {}, UNFUSED),
    ({"rows_dtype": torch.float32, "nmax": 300, "tile_mode": "none"}, {}, ("pair", "rows", True, False)),
    # autograd, an e_proj handed in, no lin_edge
    ({"grad": True}, {}, UNFUSED), ({"grad": True, "in_channels": 300}, {}, UNFUSED), ({"e_proj_given": True}, {}, UNFUSED),
    ({"has_edge_lin": False}, {}, UNFUSED),
    # graphs beyond a tile
    ({"tile_mode": "tiles"}, {}, ("layer_conv", "planes", False, False)), ({"tile_mode": "mixed"}, {}, ("layer_conv", "planes", False, False)),
    ({"tile_mode": "none"}, {}, ("pair", "rows", True, False)), ({"tile_mode": "mixed", "in_channels": 300}, {}, ("tile_conv", "planes32", True, False)),
    ({"tile_mode": "none", "in_channels": 300}, {}, ("pair", "planes32", True, False)),
    # the gate: planes with and without rows (a node gate that cannot run on the planes reads rows), planes32 from h3p_min_m rows
    ({"masked": True, "gate_on_planes": True}, {}, ("layer_conv", "planes", False, False)),
    ({"masked": True, "gate_on_planes": False}, {}, ("layer_conv", "planes", True, False)),
    ({"masked": True, "gate_on_planes": True, "share_weights": True}, {}, ("tile_conv", "rows", True, False)),
    ({"in_channels": 300, "N": 2047, "B": 90, "E": 5000}, {}, ("tile_conv", "rows", True, False)),
    ({"in_channels": 300, "N": 2048, "B": 90, "E": 5000}, {}, ("tile_conv", "planes32", True, False)),
    ({"in_channels": 300, "N": 2048, "B": 90, "E": 5000, "masked": True}, {}, ("tile_conv", "planes32", True, False)),
    ({"in_channels": 300, "rows_dtype": F16}, {}, ("pair", "rows", True, False)),
    ({"use_instr": False}, {}, ("layer_conv", "none", False, False)), ({"use_instr": False, "in_channels": 300}, {}, ("tile_conv", "none", True, False)),
    # the overrides tests and tools use
    ({}, {"fuse_layer_conv": False}, ("tile_conv", "rows", True, False)), ({}, {"fuse_tile_conv": False}, ("pair", "rows", True, False)),
    ({}, {"fuse_logits": False}, UNFUSED), ({}, {"fuse_logits_wide": False}, ("layer_conv", "planes", False, False)),
    (_C300, {"fuse_logits_wide": False}, ("unfused", "planes32", True, True)),
    ({}, {"gemm_backend": "torch"}, UNFUSED), (_C300, {"gemm_backend": "torch"}, UNFUSED), ({}, {"gemm_f16x3": False}, UNFUSED),
    ({}, {"mp_kernel": "chunk"}, UNFUSED), ({"in_channels": 300}, {"h3p": False}, ("tile_conv", "rows", True, False)),
    ({}, {"h3p_min_k": 128, "fuse_layer_conv": False}, ("tile_conv", "planes32", True, False)),
    # real forwards.  configs[1]: two plain layers and the masked last one; with a few graphs beyond a tile
    ({}, {}, ("layer_conv", "planes", False, False)), ({"masked": True, "gate_on_planes": True}, {}, ("layer_conv", "planes", False, False)),
    ({"nmax": 100, "tile_mode": "mixed", "masked": True, "gate_on_planes": True}, {}, ("layer_conv", "planes", False, False)),
    # the full model at C = 300 over 4096 graphs, and over one question
    ({**_C300, "masked": True}, {}, ("pair", "planes32", True, False)),
    ({**_C300, "N": 17, "B": 1, "E": 40, "nmax": 17}, {}, UNFUSED), ({"N": 17, "B": 1, "E": 40, "nmax": 17}, {}, ("layer_conv", "planes", False, False)),
    # configs[4] (2048 skewed graphs, fp16 rows)
    ({"rows_dtype": F16, "N": 43633, "B": 2048, "E": 110000, "nmax": 180, "tile_mode": "none", "masked": True}, {}, ("pair", "rows", True, False)),
]


@pytest.mark.parametrize("facts,switches,route", CONV_ROUTES)
def test_conv_route_names_how_a_gatv2_layer_runs(facts, switches, route):
    """ops.conv_route is the whole decision of how a MaskingGATv2Conv layer runs -- its message-passing kernels, what its
    instruction gate writes, whether fp32 rows of the gated input are read, whether e_proj exists in memory: each side of every
    rule, the switches' overrides, and the layers of real forwards."""
    from isubgvqa_amd import ops
    with ops.configured(**switches):
        assert ops.conv_route(**{**_CONV, **facts}) == route
    assert ops.conv_route(cfg=ops.Switches(**switches), **{**_CONV, **facts}) == route


class _StubPlan:
    """What MaskingGATv2Conv.route reads of an ops.GraphPlan (which only a GPU can build); counts the calls of tile_mode."""
    def __init__(self, N=82189, B=4096, E=204753, nmax=40, emax=100, mode="tiles"):
        self.N, self.B, self.E, self.nmax, self.emax, self.rowptr = N, B, E, nmax, emax, object()
        self.mode, self.asked, self._memo = mode, 0, {}

    def memo(self):
        return self._memo

    def tile_mode(self, node_cap=64, edge_cap=256):
        self.asked += 1
        return self.mode


def _conv_layer(in_channels=128, channels=128, **kw):
    from isubgvqa_amd.models.mgat_v2_conv import MaskingGATv2Conv
    return MaskingGATv2Conv(in_channels, channels, heads=4, edge_dim=channels, add_self_loops=False, masking_threshold=1.0,
                            use_instr=True, **kw)


def test_conv_route_asks_the_plans_tile_mode_only_when_the_route_depends_on_it():
    """GraphPlan.tile_mode can cost a device-to-host sync (a big batch with a graph beyond a tile): a layer that cannot run on the
    tile kernels whatever it says -- the C = 300 full model, fuse_tile_conv off -- never asks; one that can asks once per plan."""
    from isubgvqa_amd import ops
    with torch.no_grad():
        wide, plan = _conv_layer(300, 300), _StubPlan(nmax=100, mode="none")
        assert wide.route(plan, 300, torch.empty(0, 300)) == ("pair", "planes32", True, False) and plan.asked == 0
        assert not ops.layer_conv_supported(plan, 4, 300, 128, 300) and not ops.tile_conv_supported(plan, 4, 300, 300) and plan.asked == 0
        conv, ea = _conv_layer(), torch.empty(0, 128)
        with ops.configured(fuse_tile_conv=False):
            assert conv.route(plan, 128, ea) == ("pair", "rows", True, False) and conv.dispatch(plan, 128, ea) == "pair"
            assert not ops.layer_conv_supported(plan, 4, 128, 128, 128) and plan.asked == 0
        for mode, route in (("none", ("pair", "rows", True, False)), ("mixed", ("layer_conv", "planes", False, False)),
                            ("tiles", ("layer_conv", "planes", False, False))):
            plan = _StubPlan(nmax=100, mode=mode)
            assert conv.route(plan, 128, ea) == route and conv.dispatch(plan, 128, ea) == route[0] and plan.asked == 1, mode
            assert ops.layer_conv_supported(plan, 4, 128, 128, 128) == (mode != "none") and plan.asked == 2
    assert conv.route(plan, 128, ea) == UNFUSED and conv.route(None, 128, ea, None) == UNFUSED and plan.asked == 2      # autograd; no plan


def test_conv_route_memo_is_per_plan_and_follows_the_switches():
    """MaskingGATv2Conv.route keeps its answer on the plan, per layer, facts and switch object; a changed switch is seen on the next call."""
    from isubgvqa_amd import ops
    conv, other, plan, ea = _conv_layer(), _conv_layer(share_weights=True), _StubPlan(), torch.empty(0, 128)
    with torch.no_grad():
        first = conv.route(plan, 128, ea)
        assert first == ("layer_conv", "planes", False, False) and conv.route(plan, 128, ea) is first and plan.asked == 1
        assert other.route(plan, 128, ea).conv == "tile_conv" and conv.route(plan, 300, ea).conv == "tile_conv"
        assert conv.route(plan, 128, ea, e_proj=ea) == UNFUSED and conv.route(plan, 128, ea) is first
        with ops.configured(fuse_layer_conv=False):
            assert conv.route(plan, 128, ea).conv == "tile_conv" and conv.dispatch(plan, 128, ea) == "tile_conv"
        again = conv.route(plan, 128, ea)                      # the switches are a new object again: decided again
        assert again == first and again is not first
        assert conv.route(_StubPlan(mode="none"), 128, ea).conv == "pair" and conv.route(plan, 128, ea) is again


def _hand_plan():
    """A GraphPlan of two graphs (3 and 4 nodes) from CPU tensors: nothing here touches the library."""
    from isubgvqa_amd import ops
    batch = torch.tensor([0, 0, 0, 1, 1, 1, 1])
    ei = torch.tensor([[0, 1, 3, 4, 5], [1, 2, 4, 5, 6]])
    return ops.GraphPlan(N=7, E=5, B=2, ptr=torch.tensor([0, 3, 7], dtype=torch.int32), nmax_dev=torch.zeros(1, dtype=torch.int32),
                         nmax=4, emax=3, batch=batch, edge_index=ei)


def test_graph_plan_takes_no_attribute_it_does_not_declare():
    """A lazily built member goes into the plan's cache object, a new fact into a declared field: a misspelt or forgotten name
    raises instead of riding along unseen.  The cache object is closed in the same way."""
    p = _hand_plan()
    for name in ("_bound_dev", "_tiles", "_parent_edge_rows", "anything"):
        with pytest.raises(AttributeError):
            setattr(p, name, None)
    with pytest.raises(AttributeError):
        p._cache.tile = {}
    assert p._bounds_dev is None and p._bounds_host is None and p._hints is None       # declared, unset outside a capture
    p._hints = (4, 3)
    p.verify_hints()                                                                   # no bounds on the device: nothing to compare


def test_graph_plan_with_holes_is_a_view_that_shares_the_cache():
    """GraphPlan.with_holes(sub) -- the plan run_split hands its tile pass: a new plan, equal field for field, with `holes` = sub,
    an empty memo of its own and the SAME cache object, so that what the pass builds lazily the caller's plan finds again; the
    caller's plan is not written to."""
    import dataclasses
    from isubgvqa_amd import ops
    p = _hand_plan()
    p.memo()["asked"] = 1
    sub = ops.OversizeGraphs(torch.tensor([1]), torch.arange(3, 7), None, torch.zeros(4, dtype=torch.long), None, _hand_plan())
    v = p.with_holes(sub)
    assert v is not p and type(v) is ops.GraphPlan
    assert v.holes is sub and p.holes is None
    assert v._cache is p._cache and isinstance(p._cache, ops._PlanCache)
    assert v.memo() == {} and v.memo() is not p.memo() and p.memo() == {"asked": 1}
    names = [f.name for f in dataclasses.fields(ops.GraphPlan)]
    assert "holes" in names and "_memo" in names and "_cache" in names
    for name in names:
        if name not in ("holes", "_memo"):
            assert getattr(v, name) is getattr(p, name), name
    # a tile plan in the cache answers both, without the library (these CPU tensors could not be handed to it)
    t = ops.TilePlan(torch.tensor([0, 1, 2], dtype=torch.int32), torch.tensor([2], dtype=torch.int32), 2,
                     torch.zeros(2, 4, dtype=torch.int32), torch.ones(2, 4, dtype=torch.int32))
    p._cache.tiles[(64, 256)] = t
    for plan in (p, v):
        got = plan.tiles(64, 256)
        assert type(got) is tuple and len(got) == 4 and all(a is b for a, b in zip(got, t[:4]))
        assert plan.tiles_heavy_first(64, 256) is t.heavy
        with ops.configured(tile_heavy_first=False):
            assert plan.tiles_heavy_first(64, 256) is t.info
    # what the view adds, the caller's plan sees -- and a view of the view too
    t2 = t._replace(cap=3)
    v._cache.tiles[(64, 0)] = t2
    slots = v.dense_slots()
    assert p.tiles(64, 0)[2] == 3 and p.dense_slots() is slots and slots.tolist() == [0, 1, 2, 4, 5, 6, 7]
    assert v.with_holes(sub)._cache is p._cache and p.holes is None and p.memo() == {"asked": 1}
    assert _hand_plan()._cache is not p._cache and _hand_plan().memo() is not p.memo()      # per plan, not per class


def test_linear_relu_and_gelu_are_exclusive_at_every_size():
    from isubgvqa_amd import ops
    for M in (0, 12, 1024, 5000):
        with pytest.raises(ValueError):
            ops.linear(torch.zeros(M, 512), torch.zeros(512, 512), relu=True, gelu=True)


def _watched_module():
    torch.manual_seed(0)
    return torch.nn.Sequential(torch.nn.Linear(8, 8), torch.nn.BatchNorm1d(8), torch.nn.Sequential(torch.nn.Linear(8, 4, bias=False)))


def test_weights_watch_stamp_is_stable_while_nothing_is_written():
    """ops.WeightsWatch.stamp() -- what a StepCapture entry is stamped with: equal between two calls with nothing in between, a
    forward in eval mode included, and equal for two watches' own repeated stamps; one tree walk serves them all."""
    from isubgvqa_amd import ops
    m = _watched_module().eval()
    w = ops.WeightsWatch(m)
    s0, walks = w.stamp(), ops.WeightsWatch._WALKS
    with torch.no_grad():
        m(torch.zeros(3, 8))
    assert w.stamp() == s0 and w.stamp() == s0
    assert ops.WeightsWatch._WALKS == walks, "the module tree was walked again although nothing changed"
    # the walk number; versions of five parameters (the absent bias has none) and BatchNorm's three buffers; their eight addresses
    assert len(s0) == 1 + (5 + 3) + (5 + 3)


@pytest.mark.parametrize("write", ["parameter_in_place", "optimizer_step", "buffer_in_place", "batchnorm_in_training", "load_state_dict",
                                   "parameter_replaced", "buffer_replaced", "bias_added", "data_assigned", "invalidate_weight_cache"])
def test_weights_watch_stamp_changes_with_every_write_it_promises_to_see(write):
    """Each way the weights of a module change between two captured calls changes the stamp -- and the stamp is stable again
    afterwards.  Documented blind spots, stated rather than asserted away: a WRITE through `.data` moves neither a version, an address
    nor an identity (the derived-weight cache cannot see it either), a submodule exchanged for another and a tensor
    registered on a module that had none are not looked for per call; all three are answered by ops.invalidate_weight_cache(),
    the last case here."""
    from isubgvqa_amd import ops
    m = _watched_module().eval()
    w = ops.WeightsWatch(m)
    s0 = w.stamp()
    if write == "parameter_in_place":
        with torch.no_grad():
            m[2][0].weight.add_(1.0)
    elif write == "optimizer_step":
        m[0].bias.grad = torch.ones(8)
        torch.optim.SGD([m[0].bias], lr=0.1).step()
    elif write == "buffer_in_place":
        m[1].running_var.mul_(2.0)
    elif write == "batchnorm_in_training":
        m.train()(torch.randn(5, 8))
    elif write == "load_state_dict":
        m.load_state_dict({k: v + 1 for k, v in m.state_dict().items()})
    elif write == "parameter_replaced":
        m[0].weight = torch.nn.Parameter(m[0].weight.detach().clone())
    elif write == "buffer_replaced":
        m[1].running_mean = torch.ones(8)
    elif write == "data_assigned":
        m[0].weight.data = m[0].weight.data.clone()                 # what Module.to(dtype) does: same object, same version, new address
    elif write == "bias_added":
        m[2][0].bias = torch.nn.Parameter(torch.zeros(4))           # (the slot existed, holding None)
    else:
        m[0].weight.data.mul_(2.0)
        assert w.stamp() == s0, "a write through .data is the documented blind spot; if it is seen now, say so in the docstrings"
        ops.invalidate_weight_cache()
    s1 = w.stamp()
    assert s1 != s0
    assert w.stamp() == s1


def test_weights_watch_over_inference_tensors_and_several_modules():
    """Tensors made under torch.inference_mode() have no version counter (ops._ver answers -1; reading `._version` raises): the stamp
    must not raise, and identity still stands for them.  A watch over several modules (the question side of ISubGVQA) sees each."""
    from isubgvqa_amd import ops
    with torch.inference_mode():
        a = torch.nn.Linear(4, 4)
    b = torch.nn.Linear(4, 4)
    w = ops.WeightsWatch(a, b)
    s0 = w.stamp()
    assert w.stamp() == s0 and len(s0) == 1 + 2 + 4        # the walk number, b's two versions, four addresses
    with torch.inference_mode():
        a.weight.add_(1.0)                                 # invisible (no version), as for the derived-weight cache
    assert w.stamp() == s0
    a.weight = torch.nn.Parameter(torch.zeros(4, 4))
    s1 = w.stamp()
    assert s1 != s0
    with torch.no_grad():
        b.bias.add_(1.0)
    assert w.stamp() != s1
