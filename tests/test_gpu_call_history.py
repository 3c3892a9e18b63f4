"""For given weights, switches and inputs, a forward's outputs are the same bits WHATEVER WAS CALLED BEFORE.

The kernels are held to fp64 and to each other elsewhere; this module holds the state that lives BETWEEN calls: replayed hipGraphs
(ops.StepCapture), the derived-weight cache (ops._DERIVED) and module attributes one call leaves for the next (last_mask_text).

The oracle is a TWIN: a second model built from the model-under-test's state_dict() at that moment (own parameter objects, no
history), run eagerly on the same inputs and explicit noise; every returned tensor must be torch.equal.  The eager forward of a
freshly built model is itself pinned to the reference implementation's forward and, kernel by kernel, to fp64 (test_gpu_models.py,
test_gpu_ops.py); the first test here checks the premise that two such models agree bit for bit.  The model under test is never
run eagerly inside a scenario unless the scenario says so -- an eager call refreshes exactly the state in question.

No test here runs a kernel under an understated hint: the bounds scenarios lower `plan._hints` of an honestly captured entry,
which is host-side bookkeeping (the kernels were sized by the honest hints at capture time)."""
import gc

import pytest
import torch

pytestmark = pytest.mark.gpu

TEXT_VOCAB = 2048


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X (run with -m gpu on the GPU box)"
    return torch.device("cuda:0")


# ---------------------------------------------------------------------------------------------------------------------
# helpers: models, twins, workloads, comparisons
# ---------------------------------------------------------------------------------------------------------------------
def _args(**over):
    from isubgvqa_amd import synthetic
    return synthetic.full_model_args(text_vocab_size=TEXT_VOCAB, **over)


def _full_model(dev, seed=0, **over):
    from isubgvqa_amd.models import build_model
    torch.manual_seed(seed)
    return build_model(_args(**over), None).to(dev).eval()


def _full_twin(model, dev):
    """A model of its own (never a deepcopy: a capture entry holds a CUDAGraph) with the model's state at this moment."""
    from isubgvqa_amd.models import build_model
    twin = build_model(model.args, None)
    twin.load_state_dict({k: v.detach().cpu().clone() for k, v in model.state_dict().items()}, strict=True)
    return twin.to(dev).eval()


def _full_wl(dev, graphs, tokens, seed):
    from isubgvqa_amd import synthetic
    return synthetic.make_full_workload(graphs, tokens=tokens, seed=seed, text_vocab=TEXT_VOCAB).to(dev)


def _uniform(wl, dev, seed):
    """text_uniform [B, n], n a power of two >= T (the SIMPLE sampler's noise, as test_full_model_with_text_sampling passes it)."""
    B, T = wl.questions.shape
    n = 1 << max(1, (T - 1).bit_length())
    return torch.rand(B, n, generator=torch.Generator().manual_seed(seed)).to(dev)


def _full_fwd(model, wl, capture=False, text_uniform=None):
    return model(wl.x, wl.edge_index, wl.edge_attr, wl.batch, wl.questions, wl.att_mask, return_masks=True,
                 scene_graphs=wl.scene_graphs(), text_uniform=text_uniform, capture=capture)


ANSWER_GRAPHS = 300


def _answer_cfg():
    from isubgvqa_amd import synthetic
    return synthetic.WorkloadConfig(**{**synthetic.CFG2.__dict__, "num_graphs": ANSWER_GRAPHS})


def _answer_model(dev, seed=0):
    from isubgvqa_amd import synthetic
    return synthetic.build_answer_model(_answer_cfg(), weight_seed=seed).to(dev).eval()


def _answer_twin(model, dev):
    from isubgvqa_amd import synthetic
    twin = synthetic.build_answer_model(_answer_cfg(), weight_seed=12345)
    twin.load_state_dict({k: v.detach().cpu().clone() for k, v in model.state_dict().items()}, strict=True)
    return twin.to(dev).eval()


def _answer_wl(dev, seed=0):
    """(workload, explicit Gumbel noise for the masked layers): the 300-graph configs[1]-shaped batch of the capture tests."""
    from isubgvqa_amd import synthetic
    cfg = _answer_cfg()
    wl = synthetic.make_workload(cfg).to(dev)
    if seed:       # the same topology (same shapes), other features
        g = torch.Generator(device=dev).manual_seed(seed)
        wl = synthetic.Workload(torch.randn(wl.x.shape, device=dev, generator=g), wl.edge_index, torch.randn(wl.edge_attr.shape, device=dev, generator=g),
                                wl.batch, torch.randn(wl.instr.shape, device=dev, generator=g), torch.randn(wl.glf.shape, device=dev, generator=g),
                                wl.num_graphs, wl.max_nodes, wl.max_edges, wl.graph_sizes)
    g = torch.Generator().manual_seed(1000 + seed)
    tiny, eps = torch.finfo(torch.float32).tiny, torch.finfo(torch.float32).eps
    noise = {}
    for i, t in enumerate(cfg.masks):
        if t != 1.0:
            u = tiny + torch.rand(cfg.num_graphs, wl.max_nodes, generator=g) * ((1.0 - eps) - tiny)
            noise[i] = (-torch.log(-torch.log(u))).to(dev)
    return wl, noise


def _leaves(out):
    """The tensors (and Nones) of a forward's result, flattened in order."""
    if out is None or torch.is_tensor(out):
        return [out]
    assert isinstance(out, (tuple, list)), type(out)
    return [leaf for o in out for leaf in _leaves(o)]


def _keep(out):
    """A captured call's outputs are the graph's static tensors: copies, for comparisons after later calls."""
    return [None if t is None else t.clone() for t in _leaves(out)]


def _assert_same(got, ref, what):
    got, ref = _leaves(got), _leaves(ref)
    assert len(got) == len(ref), (what, len(got), len(ref))
    assert any(t is not None for t in ref)
    for i, (a, b) in enumerate(zip(got, ref)):
        assert (a is None) == (b is None), f"{what}: output {i}: {'None' if a is None else 'tensor'} vs {'None' if b is None else 'tensor'}"
        if a is not None:
            assert a.shape == b.shape and a.dtype == b.dtype, f"{what}: output {i}: {tuple(a.shape)} {a.dtype} vs {tuple(b.shape)} {b.dtype}"
            assert torch.equal(a, b), (f"{what}: output {i} differs from the twin's eager forward "
                                       f"(max |diff| {(a.double() - b.double()).abs().max().item():.3e})")


# ---------------------------------------------------------------------------------------------------------------------
# the ways weights change between two calls
# ---------------------------------------------------------------------------------------------------------------------
def _floating(tensors):
    return [t for t in tensors if t is not None and t.is_floating_point()]


def _change_add(model, dev, seed):
    """(a) p.add_(d) on every floating parameter under no_grad (what a hand-written update or an EMA does)."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in _floating(model.parameters()):
            p.add_((0.01 * torch.randn(p.shape, generator=g)).to(dev))


def _change_sgd(model, dev, seed):
    """(b) a real torch.optim.SGD.step() with hand-set gradients."""
    g = torch.Generator().manual_seed(seed)
    params = _floating(model.parameters())
    for p in params:
        p.grad = torch.randn(p.shape, generator=g).to(dev)
    torch.optim.SGD(params, lr=0.01).step()
    for p in params:
        p.grad = None


def _change_buffers(model, dev, seed):
    """(d) buffers only, in place: the BatchNorm statistics of the scene-graph encoder (bbox_encoding / feat_reduc)."""
    g = torch.Generator().manual_seed(seed)
    hit = 0
    with torch.no_grad():
        for name, b in model.named_buffers():
            if name.endswith("running_mean"):
                b.add_((0.2 * torch.randn(b.shape, generator=g)).to(dev)); hit += 1
            elif name.endswith("running_var"):
                b.mul_((1.0 + 0.5 * torch.rand(b.shape, generator=g)).to(dev)); hit += 1
    assert hit >= 2, "the model was meant to have BatchNorm statistics"


def _change_data(model, dev, seed):
    """(e) a write through `.data` (no version moves, no identity changes) followed by ops.invalidate_weight_cache(), as the
    cache's documentation demands of such code."""
    from isubgvqa_amd import ops
    g = torch.Generator().manual_seed(seed)
    for p in _floating(model.parameters()):
        p.data.add_((0.01 * torch.randn(p.shape, generator=g)).to(dev))
    ops.invalidate_weight_cache()


def _change_everything(model, dev, seed):
    """Every parameter AND buffer in place (H6)."""
    _change_add(model, dev, seed)
    if any(True for _ in model.buffers()):
        _change_buffers(model, dev, seed + 1)


# ---------------------------------------------------------------------------------------------------------------------
# the three captured modes behind one face: call(model, i) -> outputs of the i-th input, twin(model) -> oracle
# ---------------------------------------------------------------------------------------------------------------------
class _Mode:
    """mode: "answer" (AnswerModel, capture=True), "full" (ISubGVQA, capture=True), "language" (ISubGVQA, capture="language");
    every call(i) of one _Mode has the same shapes and other values."""

    def __init__(self, mode, graphs, dev):
        self.mode, self.graphs, self.dev = mode, graphs, dev
        self._inputs = {}

    def build(self, seed=0):
        return _answer_model(self.dev, seed) if self.mode == "answer" else _full_model(self.dev, seed)

    def twin(self, model):
        return _answer_twin(model, self.dev) if self.mode == "answer" else _full_twin(model, self.dev)

    def inputs(self, i):
        if i not in self._inputs:
            if self.mode == "answer":
                self._inputs[i] = _answer_wl(self.dev, seed=i)
            else:
                # one topology (the whole-forward capture repeats its shapes).  4 questions x 9 tokens: every Linear of the
                # question side runs on isg_linear_skinny, which reads the live weight; 96 x 13 = 1248 rows are beyond it
                # (ops.Switches.skinny_max_m): the Linears' derived planes are on the replayed path
                wl = _full_wl(self.dev, self.graphs, 9 if self.graphs <= 4 else 13, seed=3)
                g = torch.Generator(device=self.dev).manual_seed(50 + i)
                wl.x = torch.randint(0, 2578, wl.x.shape, device=self.dev, generator=g)
                wl.questions = torch.randint(0, TEXT_VOCAB, wl.questions.shape, device=self.dev, generator=g)
                self._inputs[i] = wl
        return self._inputs[i]

    def call(self, model, i, captured=True):
        inp = self.inputs(i)
        if self.mode == "answer":
            wl, noise = inp
            return model(wl, noises=noise, capture=captured)
        return _full_fwd(model, inp, capture=(True if self.mode == "full" else "language") if captured else False)

    def forget_captures(self, model):
        """A scenario of its own starts without captures (the model keeps its weights' history and the derived-weight cache)."""
        for name in ("_step_capture", "_language_capture"):
            model.__dict__.pop(name, None)

    def capture_of(self, model):
        return model._language_capture if self.mode == "language" else model._step_capture

    def check(self, model, i, what):
        """The captured call on input i against a twin built now; returns copies of the captured outputs."""
        got = self.call(model, i)
        twin = self.twin(model)
        _assert_same(got, self.call(twin, i, captured=False), f"{self.mode}, {self.graphs} graphs: {what}")
        kept = _keep(got)
        del twin
        return kept


# 4 questions: most Linears run on isg_linear_skinny, which reads the live weight; 96: derived planes are on the path (_Mode.inputs)
MODES = [("answer", ANSWER_GRAPHS), ("full", 4), ("full", 96), ("language", 4), ("language", 96)]
MODE_IDS = [f"{m}-{g}" for m, g in MODES]


@pytest.fixture(scope="module")
def shared(dev):
    """One model under test per (mode, size) for the weight-update scenarios: each full-model build plus capture costs seconds, and
    a model that has lived through the earlier cases is the better subject here anyway.  The price: on a tree where replays go
    stale, a case that fails leaves the model's weights updated all the same, so its failure says nothing about the next case's
    starting point -- each case therefore drops the model's captures first (forget_captures) and checks its own capturing call
    against a twin before it changes anything; a failure there, and not after the update, points at an earlier case or a `-k`
    selection, not at this one."""
    cache = {}

    def get(mode, graphs):
        if (mode, graphs) not in cache:
            m = _Mode(mode, graphs, dev)
            cache[(mode, graphs)] = (m, m.build())
        return cache[(mode, graphs)]

    yield get
    cache.clear()
    gc.collect()


# ---------------------------------------------------------------------------------------------------------------------
# the premise
# ---------------------------------------------------------------------------------------------------------------------
def test_a_twin_built_from_the_state_dict_computes_the_same_bits_eagerly(dev):
    """The harness's premise, before anything is captured: on every workload used below, a second model built from the first one's
    state_dict gives the first one's eager outputs bit for bit (dispatch depends on switches and shapes only, and every kernel is
    deterministic: test_tile_kernels_give_the_same_bits_on_every_launch rests on the same).  If THIS fails, the twin is no oracle
    and nothing below means anything."""
    with torch.no_grad():
        model = _answer_model(dev)
        wl, noise = _answer_wl(dev)
        _assert_same(model(wl, noises=noise), _answer_twin(model, dev)(wl, noises=noise), "AnswerModel, 300 graphs")
        for sampling in (False, True):
            model = _full_model(dev, text_sampling=sampling)
            twin = _full_twin(model, dev)
            for graphs, tokens in ((4, 9), (4, 13), (96, 9), (96, 13)):
                wl = _full_wl(dev, graphs, tokens, seed=3)
                u = _uniform(wl, dev, 7) if sampling else None
                got, ref = _full_fwd(model, wl, text_uniform=u), _full_fwd(twin, wl, text_uniform=u)
                _assert_same(got, ref, f"ISubGVQA (text_sampling={sampling}), {graphs} graphs x {tokens} tokens")
                assert (got[4] is not None) == sampling
                if sampling:
                    assert got[4].shape == (1, graphs, tokens, 1)


# ---------------------------------------------------------------------------------------------------------------------
# H1-H3: --text_sampling under capture="language": mask_text belongs to THIS call
# ---------------------------------------------------------------------------------------------------------------------
LEN_A, LEN_B = 9, 13


def _language_sequence(dev, model, twin, lengths, eager_at=()):
    """One forward per entry of `lengths` (4 questions, other questions / scene graphs / noise each time) through
    capture="language" -- eagerly on the same model at the positions in eager_at -- each compared with the twin (the weights never
    change here, so one twin serves the sequence)."""
    for i, T in enumerate(lengths):
        wl = _full_wl(dev, 4, T, seed=10 + i)
        u = _uniform(wl, dev, 20 + i)
        got = _full_fwd(model, wl, capture=False if i in eager_at else "language", text_uniform=u)
        assert got[4] is not None and got[4].shape == (1, 4, T, 1), \
            f"call {i + 1} (length {T}): mask_text {None if got[4] is None else tuple(got[4].shape)} is not this call's"
        _assert_same(got, _full_fwd(twin, wl, text_uniform=u), f"call {i + 1} of lengths {lengths} (length {T})")


def test_language_capture_hands_back_this_calls_mask_text(dev):
    """H1.  capture="language" with --text_sampling over question lengths A, B, A, B, A: all five outputs of every call are the
    twin's, mask_text included -- it is an output of the replayed graph, not whatever language_features() last left on the module
    (which a replay never calls)."""
    with torch.no_grad():
        model = _full_model(dev, text_sampling=True)
        _language_sequence(dev, model, _full_twin(model, dev), [LEN_A, LEN_B, LEN_A, LEN_B, LEN_A])
        cap = model._language_capture
        assert (cap.captures, cap.replays, len(cap.entries)) == (2, 5, 2)


def test_language_capture_after_an_eager_forward_of_another_length(dev):
    """H2.  Capture length A, an EAGER forward of length B on the same model, replay A: the eager call's mask_text must not
    come back from the replay."""
    with torch.no_grad():
        model = _full_model(dev, text_sampling=True)
        _language_sequence(dev, model, _full_twin(model, dev), [LEN_A, LEN_B, LEN_A], eager_at=(1,))
        cap = model._language_capture
        assert (cap.captures, cap.replays) == (1, 2)


def test_language_capture_that_evicts_and_recaptures_on_every_call(dev):
    """H3.  The same sequence with room for ONE entry: every call evicts the other length's capture and captures again."""
    from isubgvqa_amd import ops
    with torch.no_grad():
        model = _full_model(dev, text_sampling=True)
        model.__dict__["_language_capture"] = cap = ops.StepCapture(max_entries=1)
        _language_sequence(dev, model, _full_twin(model, dev), [LEN_A, LEN_B, LEN_A, LEN_B, LEN_A])
        assert model._language_capture is cap
        assert (cap.captures, cap.replays, len(cap.entries)) == (5, 5, 1)


# ---------------------------------------------------------------------------------------------------------------------
# H4, H5: a captured call after the weights changed
# ---------------------------------------------------------------------------------------------------------------------
def _load_second_seed(mode):
    def change(model, dev, seed):
        other = mode.build(seed=seed)
        model.load_state_dict(other.state_dict())
    return change


# ("buffers" first: on a tree without the fix it is the one case that passes, and it must meet the model before a stale replay does)
CHANGES = {"buffers": lambda mode: _change_buffers, "add_": lambda mode: _change_add, "sgd_step": lambda mode: _change_sgd,
           "load_state_dict": _load_second_seed, "data_write_then_invalidate": lambda mode: _change_data}
H4_CASES = [(m, g, c) for m, g in MODES for c in CHANGES if not (m == "answer" and c == "buffers")]      # (AnswerModel has no buffers)


@pytest.mark.parametrize("mode,graphs,change", H4_CASES, ids=[f"{m}-{g}-{c}" for m, g, c in H4_CASES])
def test_a_captured_call_after_the_weights_changed_runs_on_the_new_weights(dev, shared, mode, graphs, change):
    """H4.  Capture + one replay, change the weights, a captured call: its outputs are those of a twin built from the NEW state
    (and not the pre-update ones: the change was no no-op).  A capture bakes in the tensors derived_weight() made at capture time
    (split planes, fused and concatenated weights, the scene-graph encoder's table) while biases, norms and the skinny Linears'
    weights are read live: a replay after an update would mix the two.  "buffers": the BatchNorm statistics run as the torch
    module today and are read live -- the case is here so that a later fold of the statistics into a derived weight cannot go
    stale unseen."""
    m, model = shared(mode, graphs)
    m.forget_captures(model)
    with torch.no_grad():
        m.check(model, 0, "the capturing call")
        before = m.check(model, 1, "a replay, before the update")
    CHANGES[change](m)(model, dev, 700 + len(change))
    with torch.no_grad():
        after = m.check(model, 1, f"the captured call after {change}")
    assert not torch.equal(after[0], before[0]), "the update was meant to change the logits"
    m.capture_of(model).verify()


@pytest.mark.parametrize("mode,graphs", [("answer", ANSWER_GRAPHS), ("full", 4)], ids=["answer-300", "full-4"])
def test_ten_updates_on_one_shape_leave_one_capture_and_no_derived_weights_behind(dev, shared, mode, graphs):
    """H5.  Ten in-place updates, a captured call after each: right every time, ONE entry for the shape at the end (a stale entry
    is replaced, not kept beside its successor: each holds a private allocator pool), one new capture per update, and the
    derived-weight cache does not pile up.  len(ops._DERIVED) itself cannot be held constant here: every twin leaves its own
    entries behind, dead until the cache's sweep (on an insert beyond 256 entries) drops them, and the other scenarios' models
    are alive beside this one.  What is asserted is that the entries made from the MODEL's tensors stay as many as after the first
    update: a key is (tag, ids of the sources), so an in-place update must rewrite its entry, never add a second one under
    another key (a tag that took a version or an address into its key would)."""
    from isubgvqa_amd import ops
    m, model = shared(mode, graphs)

    def owned():
        """Entries of the derived-weight cache made from one of the model's own parameters or buffers."""
        ids = {id(t) for t in list(model.parameters()) + list(model.buffers())}
        return sum(1 for k in ops._DERIVED if any(i in ids for i in k[1:]))

    m.forget_captures(model)
    with torch.no_grad():
        m.check(model, 2, "before the updates")
        cap = m.capture_of(model)
        assert (len(cap.entries), cap.captures) == (1, 1)
        first = None
        for step in range(10):
            _change_add(model, dev, 900 + step)
            m.check(model, 2, f"after update {step + 1} of 10")
            gc.collect()
            first = owned() if first is None else first
        assert len(cap.entries) == 1, "a stale capture was kept beside its successor"
        assert cap.captures == 1 + 10
        assert owned() == first > 0, f"the model's derived weights grew from {first} to {owned()} entries over ten updates"
        cap.verify()


# ---------------------------------------------------------------------------------------------------------------------
# H6: the eager path after an in-place update of everything
# ---------------------------------------------------------------------------------------------------------------------
def _engine():
    """The switches of test_gpu_models.py's `engine_dispatch` (G10): every K >= 256 Linear on isg_linear_h3p and its planes32
    producers / consumers, whatever the row count."""
    from isubgvqa_amd import ops
    return ops.configured(h3p_min_m=1, skinny=False, rows_kernel_min_edges=0)


@pytest.mark.parametrize("dispatch", ["shipped_thresholds", "engine_dispatch"])
def test_eager_forward_follows_an_in_place_update_of_every_weight(dev, dispatch):
    """H6.  Eager only: forward, every parameter and buffer updated in place, forward -- the second equals the twin's: every
    derived_weight() tag of the model followed the update (the op tests check this for ONE Linear's planes)."""
    import contextlib
    with torch.no_grad(), (_engine() if dispatch == "engine_dispatch" else contextlib.nullcontext()):
        model = _full_model(dev)
        wl = _full_wl(dev, 96, 13, seed=3)
        first = _keep(_full_fwd(model, wl))
        _change_everything(model, dev, 41)
        second = _full_fwd(model, wl)
        _assert_same(second, _full_fwd(_full_twin(model, dev), wl), f"ISubGVQA eager ({dispatch}), after the update")
        assert not torch.equal(second[0], first[0])
        if dispatch == "shipped_thresholds":
            model = _answer_model(dev)
            awl, noise = _answer_wl(dev)
            first = _keep(model(awl, noises=noise))
            _change_everything(model, dev, 43)
            second = model(awl, noises=noise)
            _assert_same(second, _answer_twin(model, dev)(awl, noises=noise), "AnswerModel eager, after the update")
            assert not torch.equal(second[0], first[0])


def test_one_scene_graph_table_per_route_not_per_switch_set(dev):
    """The scene-graph encoder's [vocabulary, C] table is cached per (weights, kernel its Linear runs on): two forwards under two
    switch sets that route that Linear identically share ONE entry of the derived-weight cache (it was one per switch set, kept for
    the model's life)."""
    from isubgvqa_amd import ops
    with torch.no_grad():
        model = _full_model(dev)
        wl = _full_wl(dev, 4, 9, seed=3)
        mine = {id(p) for p in model.scene_graph_encoder.parameters()}
        tables = lambda: {k for k in ops._DERIVED if isinstance(k[0], tuple) and k[0][0] == "sg_table" and mine & set(k[1:])}
        _full_fwd(model, wl)
        one = tables()
        assert len(one) == 1, one            # (one MetaLayer, one table)
        with ops.configured(rows_kernel_min_edges=0) as other:       # another Switches object, the same route for the table's Linear
            V, C = model.args.sg_vocab_size, model.general_hidden_dim
            assert ops.linear_route(V, C, C, cfg=other) == ops.linear_route(V, C, C)
            _full_fwd(model, wl)
        assert tables() == one, f"a second table per switch set: {tables()}"


# ---------------------------------------------------------------------------------------------------------------------
# H7: no replay's bounds are lost before they were compared
# ---------------------------------------------------------------------------------------------------------------------
def _self_loop_batch(sizes, dev):
    """Graphs of the given node counts with self-loops only: E = N, and a graph's edge count is its node count."""
    batch = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes)).to(dev)
    loops = torch.arange(batch.numel(), device=dev)
    return batch, torch.stack([loops, loops]).contiguous()


class _HostRunsAhead:
    """An entry's event as a host that runs ahead of the device sees it -- made deterministic: record() and synchronize() are the
    real event's, query() answers False while `ahead` (the polls StepCapture.run makes) and the real event's answer afterwards."""

    def __init__(self, event):
        self.event, self.ahead = event, True

    def record(self, *a):
        return self.event.record(*a)

    def synchronize(self):
        return self.event.synchronize()

    def query(self):
        return False if self.ahead else self.event.query()


@pytest.mark.parametrize("host", ["in_step", "runs_ahead"])
def test_bounds_of_every_replay_are_compared_with_the_hints(dev, host):
    """H7.  An entry captured with honest hints (30 nodes / 30 edges per graph) on a batch whose largest graph has 20; then what a
    lying collate would have captured: `_hints` lowered to (25, 25) on the host (the kernels stay sized for 30).  Replay a batch of
    the same shapes with a 30-node graph, then the 20-node batch again, then verify().
    in_step: the host waits for every replay -- the error comes at the call after the bad replay.
    runs_ahead: every poll inside run() finds the last replay unfinished (in the launch-bound regime the option exists for, that
    is the rule) -- the bad replay's bounds must survive the good replay that follows: verify() raises and names 30."""
    from isubgvqa_amd import _lib, ops
    small, big = _self_loop_batch([20, 20, 20], dev), _self_loop_batch([30, 10, 20], dev)
    assert small[0].shape == big[0].shape and small[1].shape == big[1].shape

    def fn(batch, edge_index):
        plan = ops.GraphPlan.build(batch, edge_index, num_graphs=3, max_nodes=30, max_edges=30)
        return (plan.ptr.clone(),), plan

    cap = ops.StepCapture()
    with torch.no_grad():
        out = cap.run(fn, list(small))
        assert out[0].tolist() == [0, 20, 40, 60]
        cap.verify()
        (ent,) = cap.entries.values()
        assert ent["host"] is not None, "the plan was meant to report its bounds through pinned host memory"
        honest = ent["plan"]._hints
        assert honest == (30, 30)
        try:
            ent["plan"]._hints = (25, 25)
            if host == "in_step":
                assert cap.run(fn, list(big))[0].tolist() == [0, 30, 40, 60]
                torch.cuda.synchronize()
                with pytest.raises(_lib.IsgError, match="understate") as err:
                    cap.run(fn, list(small))
                assert "30 nodes" in str(err.value)
            else:
                stub = ent["event"] = _HostRunsAhead(ent["event"])
                assert cap.run(fn, list(big))[0].tolist() == [0, 30, 40, 60]
                assert cap.run(fn, list(small))[0].tolist() == [0, 20, 40, 60]
                stub.ahead = False
                with pytest.raises(_lib.IsgError, match="understate") as err:
                    cap.verify()
                assert "30 nodes" in str(err.value), str(err.value)
            assert cap.captures == 1
        finally:
            ent["plan"]._hints = honest
        torch.cuda.synchronize()
