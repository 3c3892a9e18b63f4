"""isg_small_mlps: the question-side MLPs of a step as one launch on 32-row blocks must leave the BITS that
ops.mlp / ops.linear leave chain by chain on isg_linear_bf16x6 (int32 views compared: NaNs and signed zeros count).

Rows 1025, 1056, 1057 and 2079: the smallest sizes at which the fused route is taken at all (1024 rows and fewer are
isg_linear_skinny's), a whole number of 32-row blocks, one row more, and a last block of 31 rows.  Widths 128 -> 128 and
96 -> 128 -> 64 (one, two and three active waves; k loops of 6 and 8 steps); one, three and four chains, the four with inputs of
their own; a trailing GELU or none; rows scaled by exp(U(0, 6)) as bench.dense_err_vs_fp32 scales them; a zero row.

Model level: synthetic.AnswerModel on 1100 graphs of the configs[1] distribution -- the masked third layer, the read-out and the
head all on the path -- gives the same logits, mask and read-out gate with the switch on and off, eager and captured, and so does a
batch that goes through ops.run_split."""
import pytest
import torch

pytestmark = pytest.mark.gpu

ROWS = (1025, 1056, 1057, 2048 + 31)


def bits(t):
    return t.contiguous().view(torch.int32)


def seq_of(widths, tail_gelu, gen, dev):
    """Linear(+GELU) over widths (k, n) or Linear, GELU, Linear(+GELU) over (k, n1, n2), weights from `gen`."""
    mods = []
    for i, (k, n) in enumerate(zip(widths[:-1], widths[1:])):
        lin = torch.nn.Linear(k, n)
        with torch.no_grad():
            lin.weight.copy_(torch.randn(n, k, generator=gen) / k ** 0.5)
            lin.bias.copy_(torch.randn(n, generator=gen))
        mods.append(lin)
        if i + 2 < len(widths) or tail_gelu:
            mods.append(torch.nn.GELU())
    return torch.nn.Sequential(*mods).to(dev).eval()


def rows_of(M, K, gen, dev, zero_row=None):
    x = torch.randn(M, K, generator=gen) * torch.rand(M, 1, generator=gen).mul(6).exp()
    if zero_row is not None:
        x[zero_row] = 0.0
    return x.to(dev)


def check(chains):
    from isubgvqa_amd import ops
    with torch.no_grad():
        assert ops._small_mlps_plan(chains) is not None
        ref = [ops.mlp(seq, x) for seq, x in chains]
        got = ops.small_mlps(chains)
        torch.cuda.synchronize()
    assert len(got) == len(ref)
    for i, (g, r) in enumerate(zip(got, ref)):
        assert g.shape == r.shape and g.dtype == torch.float32
        assert torch.isfinite(r).all()
        diff = (bits(g) != bits(r))
        assert not diff.any(), f"chain {i}: {int(diff.sum())} of {r.numel()} elements differ, first at {diff.nonzero()[0].tolist()}"


@pytest.mark.parametrize("M", ROWS)
@pytest.mark.parametrize("tail_gelu", [False, True])
def test_one_chain(M, tail_gelu):
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(M + tail_gelu)
    check([(seq_of((128, 128), tail_gelu, gen, dev), rows_of(M, 128, gen, dev))])
    check([(seq_of((96, 128, 64), tail_gelu, gen, dev), rows_of(M, 96, gen, dev, zero_row=M - 1))])


@pytest.mark.parametrize("M", ROWS)
def test_three_chains_share_their_rows(M):
    """The step's own list: two gates (Linear + GELU) and the read-out's Linear, GELU, Linear over the same question rows."""
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(3 * M)
    x = rows_of(M, 128, gen, dev, zero_row=M // 2)
    check([(seq_of((128, 128), True, gen, dev), x), (seq_of((128, 128), True, gen, dev), x),
           (seq_of((128, 128, 128), False, gen, dev), x)])


@pytest.mark.parametrize("M", ROWS)
def test_four_chains_with_inputs_of_their_own(M):
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(4 * M)
    check([(seq_of((128, 128), True, gen, dev), rows_of(M, 128, gen, dev)),
           (seq_of((96, 128, 64), True, gen, dev), rows_of(M, 96, gen, dev, zero_row=0)),
           (seq_of((32, 64), False, gen, dev), rows_of(M, 32, gen, dev)),
           (seq_of((64, 32, 96), False, gen, dev), rows_of(M, 64, gen, dev, zero_row=M - 1))])


def test_rows_a_view_of_wider_rows():
    """A column slice (row stride 256) is made contiguous by the wrapper, as ops.mlp makes it."""
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(9)
    wide = rows_of(1057, 256, gen, dev)
    check([(seq_of((128, 128), True, gen, dev), wide[:, 128:])])


# ---------------------------------------------------------------------------------------------------------------------------
def _model_and_batch(dev, big=0):
    from isubgvqa_amd import synthetic
    graphs = 1100
    base = {**synthetic.CFG2.__dict__, "num_graphs": graphs}
    if big:
        gen = torch.Generator().manual_seed(3)
        sizes = synthetic.graph_sizes(synthetic.WorkloadConfig(**base), gen).tolist()
        for i in range(big):      # bench.mixed_leg's graphs beyond a tile
            sizes[(i * 977 + 13) % graphs] = 100 + (i * 37) % 90
        base["sizes"] = tuple(sizes)
    cfg = synthetic.WorkloadConfig(**base)
    return synthetic.build_answer_model(cfg).to(dev).eval(), synthetic.make_workload(cfg).to(dev)


def _same(a, b, what):
    for name, x, y in zip(("logits", "mask", "gate"), a, b):
        assert x.shape == y.shape
        assert torch.equal(bits(x.float()), bits(y.float())), f"{what}: {name} differs with fuse_question_mlps off"


def test_answer_model_is_bit_identical_with_the_switch_off():
    from isubgvqa_amd import ops, synthetic
    dev = torch.device("cuda:0")
    model, wl = _model_and_batch(dev)
    B, nmax = wl.glf.size(0), wl.max_nodes
    noises = {2: synthetic.gumbel_noise((B, nmax), dev)}
    with torch.no_grad():
        calls = []
        keep = ops.small_mlps
        try:
            ops.small_mlps = lambda chains, strict=True: (calls.append(len(chains)), keep(chains, strict))[1]
            on = [t.clone() for t in model(wl, noises=noises)]
        finally:
            ops.small_mlps = keep
        assert calls == [2], f"the masked layer's gate and the read-out as ONE launch of two chains, got {calls}"
        with ops.configured(fuse_question_mlps=False):
            off = [t.clone() for t in model(wl, noises=noises)]
        _same(on, off, "eager")
        cap_on = [t.clone() for t in model(wl, noises=noises, capture=True)]
        _same(cap_on, off, "captured")
        with ops.configured(fuse_question_mlps=False):
            model.__dict__.pop("_step_capture", None)
            cap_off = [t.clone() for t in model(wl, noises=noises, capture=True)]
        _same(cap_on, cap_off, "captured, both")
        torch.cuda.synchronize()


def test_answer_model_through_run_split():
    """Three graphs beyond a tile: the whole batch's pass takes the launch (1100 rows), the sub-batch of three -- whose gate rows
    are not its glf rows -- stays on isg_linear_skinny; the merged result does not depend on the switch."""
    from isubgvqa_amd import ops
    dev = torch.device("cuda:0")
    model, wl = _model_and_batch(dev, big=3)
    with torch.no_grad(), ops.configured(mixed_min_nodes=0, mixed_max_fraction=0.5):
        ops.reset_counters()
        on = [t.clone() for t in model(wl, seed=5)]
        assert ops.counters()["oversize_nodes"] > 0, "the batch did not go through ops.run_split"
        with ops.configured(fuse_question_mlps=False):
            off = [t.clone() for t in model(wl, seed=5)]
        torch.cuda.synchronize()
    _same(on, off, "run_split")


def test_gate_rows_that_are_not_glf_reach_the_gate_through_the_launch():
    """AnswerModel._answer with gate_feats (what ops.run_split hands a sub-batch) over 1100 rows: the masked layer's ques_nn
    runs in the launch on rows that are NOT glf (a permutation of it), the read-out's on glf, two input pointers.  The results
    equal the switch-off path bit for bit, and differ from the run without gate_feats (the rows do reach the gate)."""
    from isubgvqa_amd import ops
    dev = torch.device("cuda:0")
    model, wl = _model_and_batch(dev)
    B = wl.glf.size(0)
    perm = torch.randperm(B, generator=torch.Generator().manual_seed(1)).to(dev)
    gate_feats = wl.glf[perm].contiguous()
    run = lambda gf: [t.clone() for t in model._answer(wl.x, wl.edge_index, wl.edge_attr, wl.batch, wl.instr, wl.glf,
                                                       ops.GraphPlan.build(wl.batch, wl.edge_index, num_graphs=B), None, 5, gf)]
    with torch.no_grad():
        seen = []
        keep = ops.small_mlps
        try:
            ops.small_mlps = lambda chains, strict=True: (seen.append([x.data_ptr() for _, x in chains]), keep(chains, strict))[1]
            on = run(gate_feats)
        finally:
            ops.small_mlps = keep
        assert len(seen) == 1 and len(seen[0]) == 2 and seen[0][0] != seen[0][1], seen
        with ops.configured(fuse_question_mlps=False):
            off = run(gate_feats)
        plain = run(None)
        torch.cuda.synchronize()
    _same(on, off, "gate_feats")
    assert not torch.equal(on[2], plain[2]) or not torch.equal(on[1], plain[1]), "gate_feats did not reach the node gate"


def test_a_declined_launch_means_not_taken():
    """Where the library declines (ISG_GEMM_KROT / ISG_GEMM_DUAL_K give isg_linear_bf16x6 another order: ISG_EUNSUPPORTED),
    strict=False answers None and the modules run their own MLPs; here the status is produced by a stand-in entry point."""
    from isubgvqa_amd import ops, _lib_fused
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(2)
    chains = [(seq_of((128, 128), True, gen, dev), rows_of(1057, 128, gen, dev))]

    class Declines:
        def isg_small_mlps(self, *a):
            return ops.ISG_EUNSUPPORTED
    keep = _lib_fused.load
    try:
        _lib_fused.load = lambda: Declines()
        with torch.no_grad():
            assert ops.small_mlps(chains, strict=False) is None
            with pytest.raises(Exception):
                ops.small_mlps(chains)
    finally:
        _lib_fused.load = keep
