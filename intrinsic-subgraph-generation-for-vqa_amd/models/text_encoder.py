"""Dense language side of ISubGVQA: CLIP token embeddings, question encoder, program decoder.

Reference behaviour:
  * CLIPTextEmbeddings copied out of a CLIP model at ISubGVQA/models/isubgvqa.py:119-120
    (token_embedding [49408,512] + position_embedding [77,512]); here a same-key module with random
    init (no network: weights come from a checkpoint's state_dict).
  * QuestionEncoder, ISubGVQA/models/question_encoder.py:6-38: 4 post-norm TransformerEncoder layers
    (d=512, 8 heads, ReLU FFN 2048) + final LayerNorm; the HF attention_mask is cast to float and
    handed over as src_key_padding_mask, i.e. it is ADDED to the attention scores (+1 on real tokens,
    pads are attended: SURVEY App. B Q5).  emb_proj and the sinusoidal pos_encoder are constructed but
    not applied (:33-34).
  * QuestionDecoder, ISubGVQA/models/question_decoder.py:4-71: n_instructions learned queries through a
    3-layer post-norm TransformerDecoder over the encoder memory, no masks.
Device work (inference): the torch modules only HOLD the parameters (so the state_dict keys are the reference's); the
forward pass below walks their layers itself: every projection and FFN layer is one launch of this library's bf16x6
matrix-core kernel with bias (+ReLU) fused (ops.linear: in_proj 512->1536 as ONE GEMM, out_proj, linear1+ReLU, linear2),
attention is isg_mha_small (csrc/isg_attn.hip: a question's K / V live in LDS, the float key-padding mask is the additive
bias it is in the reference), residual + LayerNorm are one launch of isg_add_layernorm.  Every producer leaves the row
maxima of what it wrote (ops.attach_row_maxima) so the fp16 three-product Linears downstream need no pass for their scales.
Device work (training: autograd records through the module, or train() mode with a dropout): the same walk on the autograd-aware
operators of autograd.py -- linear (forward, dX, dW on this library's GEMMs; ReLU fused), mha_small (isg_mha_small_train /
isg_mha_small_bwd), add_layernorm (isg_dropout_add_layernorm / isg_add_layernorm_bwd), dropout (isg_dropout) -- with the dropouts
where nn.TransformerEncoderLayer / DecoderLayer have them.  No mask is stored: each dropout SITE of a forward has a seed,
base + site number, and its backward kernel draws the mask again (keep rule: include/isg_train.h).  Site numbers, in call order:
    encoder layer l:  4 l + 0  attention probabilities      4 l + 1  dropout1 (before norm1's residual add)
                      4 l + 2  the FFN's dropout (after ReLU) 4 l + 3  dropout2 (before norm2's residual add)
    decoder layer l:  6 l + 0  self-attention probabilities  6 l + 1  dropout1      6 l + 2  cross-attention probabilities
                      6 l + 3  dropout2                      6 l + 4  the FFN's dropout      6 l + 5  dropout3
A site keeps its number when its p is 0 (nothing is drawn there).  The base is the forward's `seed` argument, or, without one, a
draw from torch's CPU generator (no device sync; torch.manual_seed reproduces a run).  Every p is read from the torch modules at
call time and is 0 in eval() mode.  Switch off (FUSED_TEXT_TRAIN), CPU tensors or shapes beyond the kernels: the torch modules.
"""
from __future__ import annotations

import math

import torch
from torch import Tensor

from .. import ops

FUSED_TEXT = True     # inference path on this library's kernels (A/B switch: False = torch's nn.Transformer* forward)
FUSED_TEXT_TRAIN = True     # the same under autograd / in train() mode (False = torch's modules: hipBLASLt, torch's attention)
DECODER_SEED_OFFSET = 4096  # ISubGVQA.language_features: the decoder's base seed = the encoder's + this (sites never collide)


def _recording(module: torch.nn.Module, *inputs) -> bool:
    """True when the raw inference kernels (no autograd, no dropout) cannot serve and the training walk runs (or, where that does
    not fit or FUSED_TEXT_TRAIN is off, the torch modules): autograd is
    recording through a parameter OR an input (a frozen decoder over a trainable encoder's memory), or the module is in
    train() mode with a non-zero dropout somewhere in it."""
    if torch.is_grad_enabled() and (any(p.requires_grad for p in module.parameters()) or
                                    any(t is not None and t.requires_grad for t in inputs)):
        return True
    return module.training and any(isinstance(m, torch.nn.Dropout) and m.p > 0 for m in module.modules())


def _kernels_fit(T_kv: int, head_dim: int) -> bool:
    return ops.mha_small_supported(T_kv, head_dim)


def _attention(mha: torch.nn.MultiheadAttention, x_q: Tensor, x_kv: Tensor, B: int, key_bias=None, self_attn=True) -> Tensor:
    """nn.MultiheadAttention (batch_first=False) on flattened [T*B, D] rows: fused in_proj, isg_mha_small, out_proj."""
    D = x_q.size(1)
    w, b = mha.in_proj_weight, mha.in_proj_bias
    if self_attn:
        qkv = ops.linear(x_q, w, b)                                              # [T*B, 3D], one GEMM
        q, k, v = qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:]
    else:
        wq = ops.derived_weight("mha_q", (w,), lambda: w[:D].contiguous())
        wkv = ops.derived_weight("mha_kv", (w,), lambda: w[D:].contiguous())
        bq = ops.derived_weight("mha_bq", (b,), lambda: b[:D].contiguous())
        bkv = ops.derived_weight("mha_bkv", (b,), lambda: b[D:].contiguous())
        q = ops.linear(x_q, wq, bq)
        kv = ops.linear(x_kv, wkv, bkv)                                          # [S*B, 2D]
        k, v = kv[:, :D], kv[:, D:]
    Tq, Tk, H = q.size(0) // B, k.size(0) // B, mha.num_heads
    if ops.mha_rows_supported(Tq, Tk, H, D // H) and ops.reads_planes32(q.size(0), mha.out_proj.weight.size(0), D):
        att = ops.mha_small(q, k, v, B, H, key_bias, planes_out=True)            # out_proj's operand leaves the kernel as planes32
    else:
        att = ops.mha_small(q, k, v, B, H, key_bias, want_rowmax=True)           # + max |att| per (row, head)
    return ops.linear(att, mha.out_proj.weight, mha.out_proj.bias)


def _ln(norm: torch.nn.LayerNorm, x: Tensor, residual: Tensor = None) -> Tensor:
    """LayerNorm(x + residual) as one launch; the result carries its row maxima, so none of the Linears that read it
    (in_proj, the cross-attention projections, linear1) makes a pass of its own for the fp16 planes' row scales."""
    return ops.add_layernorm(x, residual, norm)


def _ffn(layer, x: Tensor) -> Tensor:
    # ReLU is the layers' default activation; linear1's epilogue leaves one maximum per 32 columns for linear2's K-chunks
    w1, w2 = layer.linear1.weight, layer.linear2.weight
    if ops.H3P_CHAIN and ops.reads_planes32(x.size(0), *w1.shape) and ops.reads_planes32(x.size(0), *w2.shape) and w1.size(0) % 32 == 0:
        # the 2048-wide intermediate never exists as fp32 rows: linear1's epilogue writes it as the planes linear2 reads
        h = ops.linear_h3p(x, w1, layer.linear1.bias, relu=True, planes_out=True)
        return ops.linear_h3p(h, w2, layer.linear2.bias)
    h = ops.linear(x, w1, layer.linear1.bias, relu=True, want_rowmax=True)
    return ops.linear(h, w2, layer.linear2.bias)


# ---- training walk ---------------------------------------------------------------------------------------------------------
def _base_seed(seed) -> int:
    if seed is not None:
        return int(seed)
    return int(torch.randint(0, 2 ** 62, (1,)).item())           # torch's CPU generator: no device sync


def _train_fits(t_q: int, t_kv: int, d_model: int, heads: int) -> bool:
    from .. import autograd
    return (d_model % heads == 0 and ops.mha_small_train_supported(t_q, t_kv, d_model // heads)
            and autograd.add_layernorm_supported(d_model))


def _p(module: torch.nn.Module, p: float) -> float:
    return float(p) if module.training else 0.0


def _train_attention(mha: torch.nn.MultiheadAttention, x_q: Tensor, x_kv: Tensor, B: int, key_bias, self_attn: bool, p: float,
                     seed: int) -> Tensor:
    """_attention under autograd: the fused in_proj's gradient arrives as ONE [T*B, 3D] tensor from isg_mha_small_bwd; the
    cross-attention's projections read plain views of in_proj_weight, which autograd differentiates."""
    from .. import autograd
    D = x_q.size(1)
    w, b = mha.in_proj_weight, mha.in_proj_bias
    if self_attn:
        qkv = autograd.linear(x_q, w, b, False)
        q, k, v = qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:]
    else:
        q = autograd.linear(x_q, w[:D], None if b is None else b[:D], False)
        kv = autograd.linear(x_kv, w[D:], None if b is None else b[D:], False)
        k, v = kv[:, :D], kv[:, D:]
    att = autograd.mha_small(q, k, v, B, mha.num_heads, key_bias, p, seed)
    return autograd.linear(att, mha.out_proj.weight, mha.out_proj.bias, False)


def _train_ffn(layer, x: Tensor, p: float, seed: int) -> Tensor:
    from .. import autograd
    h = autograd.linear(x, layer.linear1.weight, layer.linear1.bias, False, relu=True)
    return autograd.linear(autograd.dropout(h, p, seed), layer.linear2.weight, layer.linear2.bias, False)


def _relu_ffn(layers) -> bool:
    return all(getattr(l, "activation", None) is torch.nn.functional.relu or getattr(l, "activation_relu_or_gelu", 0) == 1
               for l in layers)


class CLIPTextEmbeddings(torch.nn.Module):
    def __init__(self, vocab_size: int = 49408, hidden_size: int = 512, max_position_embeddings: int = 77):
        super().__init__()
        self.token_embedding = torch.nn.Embedding(vocab_size, hidden_size)
        self.position_embedding = torch.nn.Embedding(max_position_embeddings, hidden_size)
        self.register_buffer("position_ids", torch.arange(max_position_embeddings).unsqueeze(0), persistent=False)

    def forward(self, input_ids: Tensor) -> Tensor:
        T = input_ids.shape[-1]
        return self.token_embedding(input_ids) + self.position_embedding(self.position_ids[:, :T])


class PositionalEncoding(torch.nn.Module):
    """Sinusoidal table (ISubGVQA/models/positional_encoding.py); only its buffer key matters here."""

    def __init__(self, d_model, dropout=0.1, max_len=5000):
        super().__init__()
        self.dropout = torch.nn.Dropout(p=dropout)
        pos = torch.arange(max_len, dtype=torch.float).unsqueeze(1)
        freq = torch.exp(torch.arange(0, d_model, 2).float() * (-math.log(10000.0) / d_model))
        pe = torch.zeros(max_len, d_model)
        pe[:, 0::2] = torch.sin(pos * freq)
        pe[:, 1::2] = torch.cos(pos * freq)
        self.register_buffer("pe", pe.unsqueeze(1))

    def forward(self, x):
        return self.dropout(x + self.pe[: x.size(0), :])


class QuestionEncoder(torch.nn.Module):
    def __init__(self, text_vocab_embedding, text_emb_dim, ninp, nhead, nhid, nlayers, dropout=0.5):
        super().__init__()
        self.text_vocab_embedding = text_vocab_embedding
        self.model_type = "Transformer"
        self.emb_proj = torch.nn.Linear(text_emb_dim, ninp)
        self.pos_encoder = PositionalEncoding(ninp, dropout)
        layer = torch.nn.TransformerEncoderLayer(ninp, nhead, nhid, dropout)
        self.transformer_encoder = torch.nn.TransformerEncoder(layer, nlayers, norm=torch.nn.LayerNorm(ninp),
                                                               enable_nested_tensor=False)
        self.ninp = ninp

    def _forward_train(self, src: Tensor, mask: Tensor, seed) -> Tensor:
        from .. import autograd
        ops.COUNTERS["text_train_kernels"] += 1
        enc, base = self.transformer_encoder, _base_seed(seed)
        B, T, D = src.shape
        x = src.permute(1, 0, 2).reshape(T * B, D).contiguous()
        key_bias = mask.float().contiguous()
        for i, layer in enumerate(enc.layers):
            s0 = base + 4 * i
            att = _train_attention(layer.self_attn, x, x, B, key_bias, True, _p(self, layer.self_attn.dropout), s0)
            x = autograd.add_layernorm(att, x, layer.norm1, _p(self, layer.dropout1.p), s0 + 1)
            x = autograd.add_layernorm(_train_ffn(layer, x, _p(self, layer.dropout.p), s0 + 2), x, layer.norm2,
                                       _p(self, layer.dropout2.p), s0 + 3)
        return autograd.add_layernorm(x, None, enc.norm).view(T, B, D)

    def forward(self, src: Tensor, mask: Tensor, seed=None) -> Tensor:
        src = self.text_vocab_embedding(src)                                             # :32
        enc = self.transformer_encoder
        if (FUSED_TEXT_TRAIN and src.is_cuda and src.dtype == torch.float32 and _recording(self, src) and _relu_ffn(enc.layers)
                and _train_fits(src.size(1), src.size(1), src.size(2), enc.layers[0].self_attn.num_heads)):
            return self._forward_train(src, mask, seed)
        if (not FUSED_TEXT or not src.is_cuda or _recording(self, src)
                or not _kernels_fit(src.size(1), src.size(2) // enc.layers[0].self_attn.num_heads)):
            if src.is_cuda and not torch.is_grad_enabled():
                ops.COUNTERS["torch_attention"] += 1
            return enc(src.permute(1, 0, 2), src_key_padding_mask=mask.float())          # :35-37
        B, T, D = src.shape
        x = src.permute(1, 0, 2).reshape(T * B, D).contiguous()                          # torch's [T, B, D] row order
        key_bias = mask.float().contiguous()                                             # :36: ADDED to the scores (Q5)
        for layer in enc.layers:                                                         # post-norm encoder layers
            x = _ln(layer.norm1, x, _attention(layer.self_attn, x, x, B, key_bias))
            x = _ln(layer.norm2, x, _ffn(layer, x))
        out = _ln(enc.norm, x)
        return ops.carry_row_maxima(out.view(T, B, D), out)      # the decoder's cross-attention reads these rows


class QuestionDecoder(torch.nn.Module):
    def __init__(self, n_instructions, ninp, nhead, nhid, nlayers, dropout=0.1):
        super().__init__()
        self.model_type = "Transformer"
        self.num_queries = n_instructions
        self.query_embed = torch.nn.Embedding(self.num_queries, ninp)
        layer = torch.nn.TransformerDecoderLayer(ninp, nhead, nhid, dropout)
        self.coarse_decoder = torch.nn.TransformerDecoder(layer, nlayers, norm=torch.nn.LayerNorm(ninp))

    def _forward_train(self, queries: Tensor, memory: Tensor, seed) -> Tensor:
        from .. import autograd
        ops.COUNTERS["text_train_kernels"] += 1
        dec, base = self.coarse_decoder, _base_seed(seed)
        (S, B, D), n = memory.shape, queries.size(0)
        x = queries.reshape(n * B, D).contiguous()
        mem = memory.reshape(S * B, D).contiguous()
        for i, layer in enumerate(dec.layers):
            s0 = base + 6 * i
            att = _train_attention(layer.self_attn, x, x, B, None, True, _p(self, layer.self_attn.dropout), s0)
            x = autograd.add_layernorm(att, x, layer.norm1, _p(self, layer.dropout1.p), s0 + 1)
            att = _train_attention(layer.multihead_attn, x, mem, B, None, False, _p(self, layer.multihead_attn.dropout), s0 + 2)
            x = autograd.add_layernorm(att, x, layer.norm2, _p(self, layer.dropout2.p), s0 + 3)
            x = autograd.add_layernorm(_train_ffn(layer, x, _p(self, layer.dropout.p), s0 + 4), x, layer.norm3,
                                       _p(self, layer.dropout3.p), s0 + 5)
        return autograd.add_layernorm(x, None, dec.norm).view(n, B, D)

    def forward(self, memory: Tensor, seed=None) -> Tensor:
        B = memory.size(1)
        queries = self.query_embed.weight.unsqueeze(1).repeat(1, B, 1)                   # :61-63
        dec = self.coarse_decoder
        if (FUSED_TEXT_TRAIN and memory.is_cuda and memory.dtype == torch.float32 and _recording(self, memory)
                and _relu_ffn(dec.layers) and
                _train_fits(max(memory.size(0), queries.size(0)), max(memory.size(0), queries.size(0)), memory.size(2),
                            dec.layers[0].self_attn.num_heads)):
            return self._forward_train(queries, memory, seed)
        if (not FUSED_TEXT or not memory.is_cuda or _recording(self, memory)
                or not _kernels_fit(max(memory.size(0), queries.size(0)), memory.size(2) // dec.layers[0].self_attn.num_heads)):
            if memory.is_cuda and not torch.is_grad_enabled():
                ops.COUNTERS["torch_attention"] += 1
            return dec(tgt=queries, memory=memory, tgt_mask=None)                        # :64-66
        S, _, D = memory.shape
        n = queries.size(0)
        x = queries.reshape(n * B, D).contiguous()
        mem = memory.reshape(S * B, D).contiguous()
        if mem.data_ptr() == memory.data_ptr():
            ops.carry_row_maxima(mem, memory)                                            # same rows, same order
        for layer in dec.layers:                                                         # post-norm decoder layers, no masks
            x = _ln(layer.norm1, x, _attention(layer.self_attn, x, x, B))
            x = _ln(layer.norm2, x, _attention(layer.multihead_attn, x, mem, B, self_attn=False))
            x = _ln(layer.norm3, x, _ffn(layer, x))
        return _ln(dec.norm, x).view(n, B, D)
