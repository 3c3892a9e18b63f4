"""Top-level ISubGVQA module: the drop-in boundary.

Reference behaviour: ISubGVQA.__init__/forward, ISubGVQA/models/isubgvqa.py:86-297 -- same constructor
arguments (an ``args`` namespace plus the keyword flags), same forward signature, same 5-tuple result
and the same state_dict key layout, so a reference checkpoint loads with
strict=True.  Differences that do not change results: no CLIP download (weights arrive through the
state_dict), no GQA/GloVe files, one GraphPlan per batch instead of per-layer index work, and an
optional ``noises``/``seed`` pair to make the stochastic samplers reproducible across devices.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, Optional

import math

import torch
from torch import Tensor

from .. import ops
from .att_pooling import GlobalAttention
from .mgat import MGAT
from .scene_graph_encoder import SceneGraphEncoder
from .text_encoder import DECODER_SEED_OFFSET, CLIPTextEmbeddings, QuestionDecoder, QuestionEncoder

NUM_ANSWERS = 1842   # isubgvqa.py:207


@dataclass
class SceneState:
    """What ISubGVQA.encode_scene leaves for any number of ISubGVQA.ask calls: the encoder's rows of a batch of G distinct scene
    graphs -- nothing in them depends on a question."""
    x_enc: Tensor                       # fp32 [N, C]
    e_enc: Tensor                       # fp32 [E, C]
    edge_index: Tensor                  # int64 [2, E]
    plan: "ops.GraphPlan"               # of the G graphs
    sizes: Optional[Tensor] = None      # HOST int64 [2, G] (nodes, edges per graph) when the collate handed them over


class ISubGVQA(torch.nn.Module):
    def __init__(self, args, use_imle=False, use_masking=True, use_instruction=True, use_mgat=False, mgat_masks=None,
                 use_topk=False, interpretable_mode=True, concat_instr=False, embed_cat=True):
        super().__init__()
        self.args = args
        self.n_train_steps = 0
        self.n_valid_steps = 0
        self.use_imle, self.use_instruction, self.use_masking = use_imle, use_instruction, use_masking
        self.use_mgat, self.interpretable_mode = use_mgat, interpretable_mode
        self.concat_instr, self.embed_cat = concat_instr, embed_cat
        self.text_sampling = getattr(args, "text_sampling", False)

        self.general_hidden_dim = args.general_hidden_dim
        self.scene_graph_encoder = SceneGraphEncoder(hidden_dim=self.general_hidden_dim,
                                                     dist=getattr(args, "distributed", False),
                                                     vocab_size=getattr(args, "sg_vocab_size", 2578))
        self.text_emb_dim = 512
        self.text_vocab_embedding = CLIPTextEmbeddings(getattr(args, "text_vocab_size", 49408), self.text_emb_dim, 77)
        self.question_hidden_dim = self.general_hidden_dim
        hidden_dim = 512
        self.question_encoder = QuestionEncoder(text_vocab_embedding=self.text_vocab_embedding,
                                                text_emb_dim=self.text_emb_dim, ninp=self.text_emb_dim, nhead=8,
                                                nhid=4 * hidden_dim, nlayers=4, dropout=0.1)
        if self.text_sampling:                                                           # :135-148
            from ..sampling.methods.simple_scheme import EdgeSIMPLEBatched
            self.text_sampler = EdgeSIMPLEBatched(k=args.mgat_layers, device="cuda", policy="edge_candid")
            self.qsts_att_keys = torch.nn.Sequential(torch.nn.Linear(hidden_dim, hidden_dim), torch.nn.GELU())
            self.qsts_att_query = torch.nn.Sequential(torch.nn.Linear(hidden_dim, hidden_dim), torch.nn.GELU())
        self.program_decoder = QuestionDecoder(n_instructions=args.mgat_layers, ninp=self.text_emb_dim, nhead=8,
                                               nhid=4 * hidden_dim, nlayers=3, dropout=0.1)
        self.gat_seq = MGAT(channels=self.general_hidden_dim, num_ins=args.mgat_layers, use_instr=use_instruction,
                            masking_thresholds=mgat_masks, use_topk=use_topk, interpretable_mode=interpretable_mode,
                            concat_instr=concat_instr, use_all_instrs=getattr(args, "use_all_instrs", False),
                            use_global_mask=getattr(args, "use_global_mask", False),
                            node_classification=getattr(args, "node_classification", False),
                            sampler_type=args.sampler_type, sample_k=args.sample_k,
                            nb_samples=getattr(args, "nb_samples", 1), alpha=getattr(args, "alpha", 1.0),
                            beta=getattr(args, "beta", 10.0), tau=getattr(args, "tau", 1.0),
                            # a node budget per graph; a reference checkpoint's Namespace has neither field
                            sample_ratio=getattr(args, "sample_ratio", None), sample_k_min=getattr(args, "sample_k_min", 1),
                            # dropout on the layers' attention weights in train(); absent from a reference Namespace
                            attn_dropout=getattr(args, "attn_dropout", 0.0))
        self.graph_global_attention_pooling = GlobalAttention(num_node_features=self.question_hidden_dim,
                                                              num_out_features=self.question_hidden_dim)
        self.qsts_reduction = torch.nn.Sequential(
            torch.nn.Linear(self.text_emb_dim * args.mgat_layers, self.question_hidden_dim), torch.nn.GELU())
        self.instr_reduction = torch.nn.Sequential(
            torch.nn.Linear(self.text_emb_dim, self.question_hidden_dim), torch.nn.GELU())
        self.embedding = torch.nn.Sequential(torch.nn.Linear(self.question_hidden_dim * 3, 512), torch.nn.GELU(),
                                             torch.nn.Dropout(p=0.2))
        self.logit_fc = torch.nn.Linear(512, NUM_ANSWERS)

    # -- pieces of forward that the benchmark also drives on their own -------------------------------
    def language_features(self, questions: Tensor, qsts_att_mask: Tensor, text_uniform: Optional[Tensor] = None,
                          seed: Optional[int] = None):
        # `seed` also names the dropout masks of a training step on the kernels (text_encoder.py: base + site number per dropout)
        enc = self.question_encoder(questions, mask=qsts_att_mask, seed=seed)            # :228
        self.last_mask_text = None
        if self.text_sampling:                                                           # :229-241: SIMPLE over the tokens
            T, B, D = enc.shape
            keys = ops.mlp(self.qsts_att_keys, enc.reshape(T * B, D).contiguous()).view(T, B, D)
            queries = ops.mlp(self.qsts_att_query, enc.reshape(T * B, D).contiguous()).view(T, B, D)
            logits = torch.bmm(keys.permute(1, 0, 2), queries.permute(1, 2, 0)).sum(-1) / math.sqrt(D)
            mask_text, _ = self.text_sampler(logits.unsqueeze(-1), train=self.training, uniform=text_uniform, seed=seed)
            enc = (enc.permute(1, 0, 2) * mask_text.squeeze(0)).permute(1, 0, 2)
            self.last_mask_text = mask_text
        qst_feats = self.program_decoder(memory=enc, seed=None if seed is None else seed + DECODER_SEED_OFFSET)      # :243
        # :244-246 -- a .view, not a permute: rows 4b..4b+3 of the flattened [n_ins*B, 512] (quirk Q4)
        flat = qst_feats.contiguous().view(qst_feats.size(1), int(qst_feats.size(0)), qst_feats.size(2)).flatten(1)
        # Linear + GELU on this library's kernels (ops.mlp; autograd-aware), not the torch modules' hipBLASLt + GELU launches
        glf = ops.mlp(self.qsts_reduction, flat)                                         # :247
        n_ins, B, D = qst_feats.shape
        instr = ops.mlp(self.instr_reduction, qst_feats.reshape(n_ins * B, D)).view(n_ins, B, -1)      # :265
        return glf, instr

    def answer_graphs(self, x_encoded, edge_index, edge_attr_encoded, batch, instr_vectors, glf, plan,
                      return_masks=True, noises=None, seed=None, explainer=False, explainer_stage=False,
                      expl_bypass_x=False, trace=None):
        """MGAT -> pooling -> classifier (isubgvqa.py:267-292).  trace: an explain.AttentionTrace, which receives the layers'
        attention weights and node masks, the mask and the gate; the results are the bits of the call without it."""
        gate_q, pool_q = self.gat_seq.question_side(glf, None, self.graph_global_attention_pooling)
        x_mgat, imle_mask, node_logits_layers, _ = self.gat_seq(
            x=x_encoded, edge_index=edge_index, edge_attr=edge_attr_encoded, instr_vectors=instr_vectors[:4],
            global_language_feats=glf, batch=batch, return_masks=return_masks, explainer=explainer,
            explainer_stage=explainer_stage, expl_bypass_x=expl_bypass_x, plan=plan, noises=noises, seed=seed, gate_q=gate_q,
            trace=trace)
        embed, gate = self.graph_global_attention_pooling(x=x_mgat, u=glf, batch=batch, size=None,
                                                          return_mask=True, node_mask=imle_mask, plan=plan, q=pool_q)
        if trace is not None:
            trace.mask, trace.gate = imle_mask, gate
        feats = ops.cat_mul_mlp(self.embedding, embed, glf, want_rowmax=True)           # :288-291 (row maxima: for logit_fc)
        return ops.linear(feats, self.logit_fc.weight, self.logit_fc.bias), imle_mask, gate, node_logits_layers   # :292

    # -- many questions per scene graph: encode once, ask often ------------------------
    def encode_scene(self, node_embeddings, edge_index, edge_embeddings, batch, scene_graphs, plan: Optional[ops.GraphPlan] = None
                     ) -> SceneState:
        """The scene-graph encoder on a batch of G DISTINCT graphs (loader.SceneGraphStore.collate(distinct=True)), for ask().
        The number of graphs comes from `plan`, else from scene_graphs.num_graphs or .graph_sizes, else from the batch vector (a
        device-to-host sync, and trailing graphs without nodes are then not counted)."""
        if self.training:
            raise ValueError("encode_scene / ask are inference forms: in train() the encoder's BatchNorm layers use the statistics of "
                             "the batch, in which a graph asked five times would weigh once -- call eval(), or train through forward()")
        if plan is None:
            sizes = getattr(scene_graphs, "graph_sizes", None)
            G = getattr(scene_graphs, "num_graphs", None)
            if G is None and sizes is not None:
                G = sizes.size(1)
            plan = ops.GraphPlan.build(batch, edge_index, num_graphs=G, max_nodes=getattr(scene_graphs, "max_nodes", None),
                                       max_edges=getattr(scene_graphs, "max_edges", None), graph_sizes=sizes)
        x_enc, e_enc = self.scene_graph_encoder(node_embeddings, edge_index=edge_index, edge_attr=edge_embeddings, batch=batch,
                                                gt_scene_graphs=scene_graphs, plan=plan)
        return SceneState(x_enc, e_enc, edge_index, plan, plan.sizes_host)

    def ask(self, state: SceneState, questions, qsts_att_mask, graph_index, noises: Optional[Dict[int, Tensor]] = None,
            seed: Optional[int] = None, text_uniform: Optional[Tensor] = None, capture=False, explainer=False,
            explainer_stage=False, expl_bypass_x=False):
        """Q questions about the graphs graph_index[q] of an encoded batch: (forward's 5-tuple, ops.GraphInstances).  The question
        side runs as in forward (same seed offset); the graph side of answer_graphs runs on the batch of Q graph INSTANCES that
        ops.graph_instances expands on the device -- only answer_graphs' inputs are expanded, the encoder ran on the G graphs.
        imle_mask and gate have one row per instance node: the returned GraphInstances maps them back (.node_src, .ptr).
        added_sym_edge flipped edges of the DISTINCT batch's global edge list (quirk Q6); every instance inherits its graph's."""
        if self.training:
            raise ValueError("ask() is an inference form: the shared encoding was made without batch statistics of the questions' "
                             "batch (encode_scene) -- call eval(), or train through forward()")
        if capture:
            raise ValueError("ask(): capture is not supported (the instance batch's sizes are read between two launches)")
        if explainer or explainer_stage or expl_bypass_x is not False:
            raise ValueError("ask(): the explainer arguments are not supported (they replace the encoder's input per question, "
                             "which a shared encoding does not have); use forward()")
        if questions.size(0) != graph_index.numel():
            raise ValueError(f"ask(): {questions.size(0)} questions, {graph_index.numel()} entries of graph_index")
        glf, instr_vectors = self.language_features(questions, qsts_att_mask, text_uniform, None if seed is None else seed + 7919)
        mask_text = self.last_mask_text
        inst = ops.graph_instances(state.plan, state.edge_index, graph_index, sizes=state.sizes)
        x, e = inst.gather_rows(state.x_enc, state.e_enc)
        logits, imle_mask, gate, node_logits_layers = self.answer_graphs(x, inst.edge_index, e, inst.batch, instr_vectors, glf,
                                                                         inst.plan(), True, noises, seed)
        return (logits, imle_mask, gate, node_logits_layers, mask_text), inst

    def forward_shared(self, node_embeddings, edge_index, edge_embeddings, batch, questions, qsts_att_mask, graph_index,
                       scene_graphs=None, noises: Optional[Dict[int, Tensor]] = None, seed: Optional[int] = None,
                       plan: Optional[ops.GraphPlan] = None, text_uniform: Optional[Tensor] = None):
        """Q questions about the graphs graph_index[q] of a batch of G DISTINCT graphs, in either mode: (forward's 5-tuple,
        ops.GraphInstances).
        eval(): exactly encode_scene + ask, the same bits.
        train(): the encoder runs ONCE per distinct graph with multiplicity = the number of questions per graph, so that its
        BatchNorm layers see the statistics of the batch with every graph copied out; its rows are expanded into the instance
        batch by autograd.instance_rows, whose backward sums a row's copies without atomics, and answer_graphs runs on the
        instances as in ask().  A graph that no question names takes no part in the statistics and receives zero gradient from
        the expansion.  `plan`: the distinct batch's GraphPlan (built here when None, as in encode_scene)."""
        if not self.training:
            state = self.encode_scene(node_embeddings, edge_index, edge_embeddings, batch, scene_graphs, plan)
            return self.ask(state, questions, qsts_att_mask, graph_index, noises=noises, seed=seed, text_uniform=text_uniform)
        if questions.size(0) != graph_index.numel():
            raise ValueError(f"forward_shared(): {questions.size(0)} questions, {graph_index.numel()} entries of graph_index")
        from .. import autograd
        glf, instr_vectors = self.language_features(questions, qsts_att_mask, text_uniform, None if seed is None else seed + 7919)
        mask_text = self.last_mask_text
        if plan is None:
            sizes = getattr(scene_graphs, "graph_sizes", None)
            G = getattr(scene_graphs, "num_graphs", None)
            if G is None and sizes is not None:
                G = sizes.size(1)
            plan = ops.GraphPlan.build(batch, edge_index, num_graphs=G, max_nodes=getattr(scene_graphs, "max_nodes", None),
                                       max_edges=getattr(scene_graphs, "max_edges", None), graph_sizes=sizes)
        inst = ops.graph_instances(plan, edge_index, graph_index, sizes=plan.sizes_host)
        x_enc, e_enc = self.scene_graph_encoder(node_embeddings, edge_index=edge_index, edge_attr=edge_embeddings, batch=batch,
                                                gt_scene_graphs=scene_graphs, plan=plan, multiplicity=inst.counts())
        x, e = autograd.instance_rows(inst, x_enc, e_enc)
        logits, imle_mask, gate, node_logits_layers = self.answer_graphs(x, inst.edge_index, e, inst.batch, instr_vectors, glf,
                                                                         inst.plan(), True, noises, seed)
        return (logits, imle_mask, gate, node_logits_layers, mask_text), inst

    def _captured(self, node_embeddings, edge_index, edge_embeddings, batch, questions, qsts_att_mask, explainer, explainer_stage,
                  scene_graphs, noises, seed, plan, text_uniform):
        """forward() as a replayed hipGraph (ops.StepCapture), one capture per batch SHAPE -- the opt-in for evaluation loops whose
        batches are launch-bound (run_token_coo.py:49-79 evaluates one question at a time; datasets/build.py:59-62 four times the
        training batch).  Needs the collate's per-graph bounds on `scene_graphs` (max_nodes / max_edges: loader.SceneGraphBatch
        carries them); sampler noise from `noises` or from torch's generator inside the graph; a `seed` is refused (it would be
        frozen into the graph).  Returns the graph's static output tensors: valid until the next call with the same shapes.  The
        capture is stamped with the module's weights (ops.WeightsWatch): after an update it is captured again, not replayed."""
        if seed is not None:
            raise ValueError("capture=True: a seed is a kernel argument and would repeat in every replay; pass `noises` or neither")
        if plan is not None or explainer or explainer_stage:
            raise ValueError("capture=True: the plain inference forward only (no caller-built plan, no explainer)")
        mn, me = getattr(scene_graphs, "max_nodes", None), getattr(scene_graphs, "max_edges", None)
        if not mn or not me:
            raise ValueError("capture=True needs scene_graphs.max_nodes / .max_edges (the collate's per-graph bounds): a captured "
                             "step cannot read them back from the device")
        import argparse
        cap = self.__dict__.get("_step_capture")
        if cap is None:
            cap = self.__dict__["_step_capture"] = ops.StepCapture()
        watch = self.__dict__.get("_weights_watch")
        if watch is None:
            watch = self.__dict__["_weights_watch"] = ops.WeightsWatch(self)
        keys = sorted(noises) if noises else []
        x_bbox, sym = scene_graphs.x_bbox, scene_graphs.added_sym_edge

        def fn(ne, ei, ee, b, q, qm, bbox, s, tu, *nz):
            sg = argparse.Namespace(x_bbox=bbox, added_sym_edge=s)
            p = ops.GraphPlan.build(b, ei, num_graphs=q.size(0), max_nodes=int(mn), max_edges=int(me))
            out = self.forward(ne, ei, ee, b, q, qm, return_masks=True, scene_graphs=sg, noises=dict(zip(keys, nz)) if keys else None,
                               plan=p, text_uniform=tu)
            return out, p

        tensors = [node_embeddings, edge_index, edge_embeddings, batch, questions, qsts_att_mask, x_bbox, sym, text_uniform] + \
                  [noises[k] for k in keys]
        return cap.run(fn, tensors, key_extra=("isubgvqa", int(mn), int(me), tuple(keys), self.training), stamp=watch.stamp())

    def _captured_language(self, questions, qsts_att_mask, text_uniform, seed):
        """language_features() -- question encoder, program decoder, the two reductions: ~65 of a forward's ~110 launches -- as a
        replayed hipGraph keyed by the questions' SHAPE alone (`capture="language"`).  The whole-forward capture needs every batch
        shape to repeat; an evaluation loop over single questions (run_token_coo.py:49-79) never repeats a scene graph's (N, E) but
        has only a couple of dozen question lengths: the question side is replayed, the graph side issued eagerly behind it on the
        same stream (which is what orders the reads of the graph's static outputs before the next replay writes them).  Below ~32
        questions the forward is bound by the host's issue time: this removes more than half of it."""
        if self.text_sampling and seed is not None:
            raise ValueError("capture='language' with --text_sampling: a seed would be frozen into the graph; pass text_uniform or neither")
        cap = self.__dict__.get("_language_capture")
        if cap is None:
            cap = self.__dict__["_language_capture"] = ops.StepCapture(max_entries=64)
        watch = self.__dict__.get("_language_watch")
        if watch is None:      # the modules language_features() runs: the scene-graph side's weights are read eagerly behind the replay
            mods = [self.question_encoder, self.program_decoder, self.qsts_reduction, self.instr_reduction]
            if self.text_sampling:
                mods += [self.qsts_att_keys, self.qsts_att_query]
            watch = self.__dict__["_language_watch"] = ops.WeightsWatch(*mods)

        def fn(q, m, tu):       # mask_text is an OUTPUT of the graph: module state belongs to whichever call wrote it last
            glf, instr = self.language_features(q, m, tu, None)
            return (glf, instr, self.last_mask_text), None

        glf, instr, mask_text = cap.run(fn, [questions, qsts_att_mask, text_uniform], key_extra=("language", self.training),
                                        stamp=watch.stamp())
        # (static tensors of the replayed graph: the graph side reads glf / instr behind it on the same stream; mask_text leaves
        # forward(), so the caller gets a copy of its own)
        self.last_mask_text = mask_text = None if mask_text is None else mask_text.clone()
        return glf, instr, mask_text

    def forward(self, node_embeddings, edge_index, edge_embeddings, batch, questions, qsts_att_mask,
                return_masks=False, explainer=False, explainer_stage=False, expl_bypass_x=False, scene_graphs=None,
                noises: Optional[Dict[int, Tensor]] = None, seed: Optional[int] = None,
                plan: Optional[ops.GraphPlan] = None, text_uniform: Optional[Tensor] = None, capture=False):
        return self._forward(None, node_embeddings, edge_index, edge_embeddings, batch, questions, qsts_att_mask, return_masks,
                             explainer, explainer_stage, expl_bypass_x, scene_graphs, noises, seed, plan, text_uniform, capture)

    def forward_traced(self, trace, *args, **kwargs):
        """forward(*args, **kwargs) with an explain.AttentionTrace, which receives the layers' attention weights and node masks,
        the mask and the gate (see answer_graphs).  The return tuple and its bits are forward()'s; forward()'s own signature stays
        as it is.  Together with capture= it raises ValueError: a replayed step keeps no attention weights."""
        if trace is None:
            raise ValueError("forward_traced needs a trace (an explain.AttentionTrace); without one, call forward()")
        return self._forward(trace, *args, **kwargs)

    def _forward(self, trace, node_embeddings, edge_index, edge_embeddings, batch, questions, qsts_att_mask,
                 return_masks=False, explainer=False, explainer_stage=False, expl_bypass_x=False, scene_graphs=None,
                 noises: Optional[Dict[int, Tensor]] = None, seed: Optional[int] = None,
                 plan: Optional[ops.GraphPlan] = None, text_uniform: Optional[Tensor] = None, capture=False):
        if trace is not None and capture:
            raise ValueError("trace together with capture: a replayed step keeps no attention weights; run it eagerly")
        if not return_masks:
            # the reference unpacks two values from GlobalAttention.forward, which returns a bare tensor when
            # return_mask=False (isubgvqa.py:280, att_pooling.py:75-77): return_masks=True is mandatory there
            raise ValueError("return_masks=True is required (isubgvqa.py:280 unpacks (embed, gate))")
        if capture is True:
            return self._captured(node_embeddings, edge_index, edge_embeddings, batch, questions, qsts_att_mask, explainer,
                                  explainer_stage, scene_graphs, noises, seed, plan, text_uniform)
        if capture == "language":
            glf, instr_vectors, mask_text = self._captured_language(questions, qsts_att_mask, text_uniform, seed)
        elif capture:
            raise ValueError(f"capture = {capture!r}: True (the whole forward), 'language' (the question side only) or False")
        else:
            glf, instr_vectors = self.language_features(questions, qsts_att_mask, text_uniform,
                                                        None if seed is None else seed + 7919)
            mask_text = self.last_mask_text
        if explainer and explainer_stage > 0:                                            # :249-253
            node_embeddings, expl_bypass_x = expl_bypass_x, node_embeddings.clone()
        if plan is None:   # a loader.SceneGraphBatch carries the per-graph bounds: the plan is then built without a sync
            plan = ops.GraphPlan.build(batch, edge_index, num_graphs=questions.size(0),
                                       max_nodes=getattr(scene_graphs, "max_nodes", None),
                                       max_edges=getattr(scene_graphs, "max_edges", None),
                                       graph_sizes=getattr(scene_graphs, "graph_sizes", None))
        x_enc, e_enc = self.scene_graph_encoder(node_embeddings, edge_index=edge_index, edge_attr=edge_embeddings,
                                                batch=batch, explainer=explainer, explainer_stage=explainer_stage,
                                                gt_scene_graphs=scene_graphs, plan=plan)  # :255
        logits, imle_mask, gate, node_logits_layers = self.answer_graphs(
            x_enc, edge_index, e_enc, batch, instr_vectors, glf, plan, return_masks, noises, seed, explainer,
            explainer_stage, expl_bypass_x, trace)
        if explainer:
            return logits                                                                # :294-295
        return logits, imle_mask, gate, node_logits_layers, mask_text                    # :297
