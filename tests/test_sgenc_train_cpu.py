"""Training of the scene-graph encoder without its concatenations, the parts that need no GPU: the fifth header and its binding,
ops.token_csr on CPU tensors, and THE ALGEBRA -- the split training walk restated in float64 (tests/sgenc_bwd_restated.py) against
the oracle's form with the [E, 900] / [E, 600] concatenations, outputs and every parameter gradient."""
import os
import re

import torch

import sgenc_bwd_restated as R
from binding_checks import build_checks
from conftest import ROOT

ENTRY_POINTS = {"isg_sgenc_train_abi_version", "isg_segment_rows_sum", "isg_segment_rows_chunk", "isg_segment_rows_ws_bytes",
                "isg_gather_add_bwd", "isg_gather_add_bwd_parts", "isg_scatter_mean_bwd", "isg_graph_norm_bwd"}


def test_fifth_header_declares_the_entry_points_and_the_binding_follows_it():
    import __graft_entry__ as ge
    ge.build()
    from isubgvqa_amd import _lib, _lib_fused, _lib_optim, _lib_sgenc_train, _lib_train
    header = open(os.path.join(ROOT, "include", "isg_sgenc_train.h")).read()
    body = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(isg_[a-z0-9_]+)\s*\(", body))
    assert declared == ENTRY_POINTS == set(_lib_sgenc_train.SIGNATURES), declared ^ ENTRY_POINTS
    assert int(re.search(r"#define ISG_SGENC_TRAIN_ABI_VERSION (\d+)", header).group(1)) == 1 == _lib_sgenc_train.ABI_VERSION
    lib = _lib_sgenc_train.load()
    for name in ENTRY_POINTS:
        assert hasattr(lib, name), name
    assert lib.isg_sgenc_train_abi_version() == 1
    # the other four headers did not move
    assert (_lib.ABI_VERSION, _lib_train.ABI_VERSION, _lib_optim.ABI_VERSION, _lib_fused.ABI_VERSION) == (23, 1, 1, 1)
    assert len(_lib.SIGNATURES) == 74
    # the pure host functions of the header
    L = lib.isg_segment_rows_chunk()
    assert L >= 16 and lib.isg_segment_rows_ws_bytes(0, 300) == 0
    assert lib.isg_segment_rows_ws_bytes(L, 300) == 2 * 300 * 4 and lib.isg_segment_rows_ws_bytes(L + 1, 300) == 2 * 2 * 300 * 4
    assert lib.isg_gather_add_bwd_parts(0) == 0 and lib.isg_gather_add_bwd_parts(1) == 1
    assert 1 <= lib.isg_gather_add_bwd_parts(1 << 20) <= 4096
    # every source that is compiled is listed for staleness with the header
    build_checks("isg_sgenc_train.h")


def test_token_csr_on_cpu_tensors():
    from isubgvqa_amd import ops
    gen = torch.Generator().manual_seed(2)
    V, M = 11, 400
    idx = torch.randint(2, V - 1, (M,), generator=gen)                 # tokens 0, 1 and V - 1 unused
    idx[torch.randperm(M, generator=gen)[:260]] = 5                    # one token owns more than half the entries
    rowptr, eid = ops.token_csr(idx.view(100, 4), V)
    assert rowptr.dtype == torch.int32 and eid.dtype == torch.int32 and tuple(rowptr.shape) == (V + 1,) and tuple(eid.shape) == (M,)
    want_ptr, want_eid = R.token_csr(idx, V)
    assert torch.equal(rowptr, want_ptr) and torch.equal(eid, want_eid)
    assert int(rowptr[0]) == 0 and int(rowptr[-1]) == M
    counts = (rowptr[1:] - rowptr[:-1]).long()
    assert counts[0] == counts[1] == counts[V - 1] == 0 and int(counts[5]) > M // 2
    for v in range(V):
        seg = eid[int(rowptr[v]):int(rowptr[v + 1])].long()
        assert bool((idx[seg] == v).all()) and bool((seg[1:] > seg[:-1]).all()), v        # stable: ascending position
    r0, e0 = ops.token_csr(torch.zeros(0, dtype=torch.int64), V)
    assert tuple(r0.shape) == (V + 1,) and int(r0.abs().sum()) == 0 and e0.numel() == 0


def test_segment_sum_restatement_on_a_case_written_out_by_hand():
    rowptr = torch.tensor([0, 0, 2, 3, 3, 5], dtype=torch.int32)
    eid = torch.tensor([1, 4, 0, 2, 3], dtype=torch.int32)
    G = torch.tensor([[1.0, 10.0], [2.0, 20.0], [3.0, 30.0]])
    w = torch.tensor([1.0, -1.0, 1.0, 1.0, -1.0])
    out = R.segment_rows_sum(rowptr, eid, G, w=w, gdiv=2)               # entry e reads row e // 2
    want = torch.tensor([[0.0, 0.0], [-1.0 - 3.0, -10.0 - 30.0], [1.0, 10.0], [0.0, 0.0], [2.0 + 2.0, 20.0 + 20.0]]).double()
    assert torch.equal(out, want)
    assert torch.equal(R.segment_rows_sum(rowptr, eid, G, w=w, gdiv=2, skip=1)[1], torch.zeros(2).double())


def test_split_training_walk_is_the_oracles_function_in_float64():
    """Outputs and every parameter gradient of the split walk against oracle.model.scene_graph_encoder_forward in train mode
    (batch-statistics BatchNorm), to 1e-10 of the tensor's largest entry; the pad row's gradient exactly zero; no parameter left
    out (mean_scale is drawn from U(0.5, 1.5), so none has a vanishing gradient)."""
    enc = R.make_encoder()
    inputs = R.make_batch()
    assert len(R.SIZES) == 6 and 1 in R.SIZES and max(R.SIZES) == 12
    assert 0.3 < float((inputs["x"][:, 1:] == R.PAD).float().mean()) < 0.7
    assert abs(float((inputs["edge_attr"] == 7).float().mean()) - 0.4) < 0.05
    sym = inputs["added_sym_edge"]
    assert sym.unique().numel() < sym.numel()
    p = "scene_graph_encoder"
    x_ref, e_ref, g_ref = R.oracle_grads(enc, inputs, p)
    sd = R.state_dict64(enc, p)
    x_enc, e_enc = R.split_walk(sd, p, **inputs)
    wx, we = R.loss_weights(x_enc.size(0), e_enc.size(0), x_enc.size(1))
    ((x_enc * wx).sum() + (e_enc * we).sum()).backward()

    def rel(a, b):
        return float((a.detach().double() - b.detach().double()).abs().max()) / max(float(b.abs().max()), 1e-300)

    assert rel(x_enc, x_ref) <= 1e-10 and rel(e_enc, e_ref) <= 1e-10, (rel(x_enc, x_ref), rel(e_enc, e_ref))
    names = [k for k, _ in enc.named_parameters()]
    assert len(names) == 28, names
    for k in names:
        ref, got = g_ref[k], sd[f"{p}.{k}"].grad
        assert ref is not None and got is not None, k
        assert float(ref.abs().max()) > 1e-6, f"{k}: the oracle's gradient vanishes ({float(ref.abs().max()):.1e}); nothing would be checked"
        assert rel(got, ref) <= 1e-10, f"{k}: {rel(got, ref):.2e}"
    pad = sd[f"{p}.sg_vocab_embedding.weight"].grad[R.PAD]
    assert torch.equal(pad, torch.zeros_like(pad)) and torch.equal(g_ref["sg_vocab_embedding.weight"][R.PAD], torch.zeros_like(pad))


def test_encoder_module_has_the_switch_and_the_counter():
    from isubgvqa_amd import ops
    from isubgvqa_amd.models import scene_graph_encoder as M
    assert isinstance(M.SPLIT_TRAIN, bool) and M.SPLIT_LINEARS is True
    assert "sgenc_train_kernels" in ops.COUNTERS
    assert hasattr(M._MetaLayer, "forward_split_train")
