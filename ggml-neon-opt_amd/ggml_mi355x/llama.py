"""llm_build_llama (non-flash attention) as ggml-mirror nodes on the MI355X backend
(SURVEY.md §8f rank 4), for one token, a prompt and a batch of several sequences.

The reference builds this graph in llama.cpp (llama_model::build_graph ->
llm_build_llama, artifacts/perf/out.folded:249-251) and ggml-cpu computes it node by
node (ggml_graph_compute_thread -> ggml_compute_forward, out.folded:91-234). Here the
same nodes go to mi355x_backend_graph_compute, which fuses RMS_NORM -> MUL -> MUL_MAT,
SWIGLU -> MUL_MAT and MUL_MAT -> ADD into the GEMV launches, and replays a graph's
launches from a hipGraph (a node list is identical for every step; the token ids,
positions and the rest of ggml's inp_* tensors are device inputs written before each
step).

Per layer:
  rms_norm(x)*attn_norm -> q, k, v (MUL_MAT) -> attention (rope, f16 KV cache, KQ,
  soft_max, KQV) -> attn_output (MUL_MAT) -> +x -> rms_norm*ffn_norm ->
  gate, up (MUL_MAT) -> swiglu -> down (MUL_MAT) -> +ffn_inp
  (a MoE model, hp["n_expert"] > 0: after ffn_norm, MOE_ROUTE -> up, gate (MUL_MAT_ID) -> swiglu ->
  down (MUL_MAT_ID) -> MOE_COMBINE -> +ffn_inp: build_moe_ffn, the experts chosen on the device)
then rms_norm*output_norm -> output (MUL_MAT) -> logits.

LlamaDecoder's entry points and the graph each runs; all of them are emitted by the one
layer body and the one head below (LlamaDecoder._layers, ._head) over a _Graph:
  step            the token graph, built with the decoder: one row, ATTN_DECODE; under a
                  row split with the ALL_GATHER / ALL_REDUCE nodes of its mode
  prompt          _prompt_graph(n_tok): n_tok rows, ATTN_DECODE over the batch, the last
                  layer's inp_out_ids selection, logits of the last token
  step_batch      _batch_graph(n_tok, n_kv): n_tok rows of any sequences, ATTN_BATCH with
                  cells and mask from the inputs, logits of every row
  generate,       the token graph / the batch graph plus one ARGMAX / ARGMAX_BATCH node
  generate_batch  that stages the next step's inputs on the device; with a Sampler that last
                  node is a SAMPLE / SAMPLE_BATCH, which reads its draws from a device table; with
                  a Sampler that edits the logits (penalties, logit bias) a PENALIZE node stands
                  between the logits and that node and reads the history the steps write
  shift           one KV_SHIFT node a layer (DISCARD form) over the caches: llama.cpp's context
                  shift, which generate(keep=) runs whenever the cache is full
  logprobs,       _prompt_graph(n_tok, all_rows=True): the prompt's layers with no row selection,
  perplexity      the head over all n_tok rows and one LOGPROB_BATCH node on the logits and the
                  targets: 24 bytes a token come back, not a row of the vocabulary
"""
from __future__ import annotations

import ctypes

from . import (ARGMAX_STEP_INPUTS, BLOCK_BYTES, FLAG_OUTPUT, LOGIT_BIAS_MAX, LOGPROB_MAX_N, OP_ADD, OP_ALL_GATHER,
               OP_ALL_REDUCE, OP_ARGMAX, OP_ARGMAX_BATCH, OP_ATTN_BATCH, OP_ATTN_DECODE, OP_GET_ROWS, OP_KV_SHIFT,
               OP_LOGPROB_BATCH, OP_MOE_COMBINE, OP_MOE_ROUTE, OP_MUL, OP_MUL_MAT, OP_MUL_MAT_ID, OP_PENALIZE,
               OP_RMS_NORM, OP_SAMPLE, OP_SAMPLE_BATCH, OP_SWIGLU, PENALTY_MAX_LAST_N, QK_K, SAMPLE_MAX_K,
               SAMPLE_STEP_INPUTS, TYPE_F16, TYPE_F32, TYPE_I32, Backend, Mi355xError, bias_pairs, f32_bits, kv_shift_params, logprob_dtype, logprob_value, make_tensor,
               penalize_params, rope_table, sampler_params)


def torch_tensor(values):
    import torch
    return torch.tensor(list(values), dtype=torch.int32)


LAYER_MATS = ("attn_q", "attn_k", "attn_v", "attn_output", "ffn_gate", "ffn_up", "ffn_down")
# a MoE layer (hp["n_expert"] > 0): the attention's matrices, then the router (f32) and the expert tensors
MOE_LAYER_MATS = LAYER_MATS[:4] + ("ffn_gate_exps", "ffn_up_exps", "ffn_down_exps")
MOE_ROUTER = "ffn_gate_inp"


def hparams(n_embd, n_layer, n_head, n_head_kv, n_ff, n_vocab, eps=1e-5, freq_base=10000.0, n_expert=0,
            n_expert_used=0):
    """n_expert > 0: every layer's FFN is the MoE arm (llama.expert_count / llama.expert_used_count; n_ff is one
    expert's width). A dense model's dict has no MoE keys: it is the dict of before."""
    hp = dict(n_embd=n_embd, n_layer=n_layer, n_head=n_head, n_head_kv=n_head_kv, head_dim=n_embd // n_head,
              n_ff=n_ff, n_vocab=n_vocab, eps=eps, freq_base=freq_base)
    if n_expert:
        if not 1 <= n_expert_used <= n_expert:
            raise Mi355xError(f"hparams: n_expert_used {n_expert_used} must lie in [1, n_expert {n_expert}]")
        hp.update(n_expert=int(n_expert), n_expert_used=int(n_expert_used))
    return hp


def layer_mats(hp):
    """The names of a layer's K-quant tensors: LAYER_MATS, or for a MoE model MOE_LAYER_MATS."""
    return MOE_LAYER_MATS if hp.get("n_expert", 0) else LAYER_MATS


def gguf_hparams(f):
    """hparams of an open llama-architecture GGUFFile, the MoE keys included; None if it is not one."""
    arch = f.kv.get("general.architecture", "llama")
    kv = lambda k, d=None: f.kv.get(f"{arch}.{k}", d)  # noqa: E731
    E, L, nh = kv("embedding_length"), kv("block_count"), kv("attention.head_count")
    if arch != "llama" or None in (E, L, nh) or "token_embd.weight" not in f.tensors:
        return None
    return hparams(E, L, nh, kv("attention.head_count_kv", nh), kv("feed_forward_length"),
                   f.tensors["token_embd.weight"]["ne"][1], eps=kv("attention.layer_norm_rms_epsilon", 1e-5),
                   freq_base=kv("rope.freq_base", 10000.0), n_expert=kv("expert_count", 0),
                   n_expert_used=kv("expert_used_count", 0))


TINYLLAMA = hparams(2048, 22, 32, 4, 5632, 32000)
LLAMA3_8B = hparams(4096, 32, 32, 8, 14336, 128256, eps=1e-5, freq_base=500000.0)


def _check(rc, what):
    if rc:
        raise Mi355xError(f"{what} failed ({rc})")


def ppl_of(nll, count):
    """exp(nll / count), the perplexity of `count` scored tokens (inf where the double overflows)."""
    import math
    try:
        return math.exp(nll / count)
    except OverflowError:
        return math.inf


def _as_f32(v):
    """v rounded to float32, as a Python float (inf where it overflows)."""
    import struct
    try:
        return struct.unpack("<f", struct.pack("<f", float(v)))[0]
    except OverflowError:
        return float("inf") if v > 0 else float("-inf")


def _node_array(nodes):
    return (ctypes.POINTER(type(nodes[0])) * len(nodes))(*[ctypes.pointer(n) for n in nodes])


class Sampler:
    """llama.cpp's default sampler chain, top-k -> top-p -> min-p -> temperature -> one draw, with
    its defaults [U] (the exact rule: include/ggml_mi355x.h, mi355x_sample). seed: the draws of
    generate / generate_batch are numpy's PCG64(seed) float32 stream (sequence i of a batch:
    PCG64([seed, i])), entry p the draw of the token that will stand at position p, so the same
    seed and context give the same tokens whatever chunk, n or use_graph is. A generate(keep=)
    call that shifts the context refills the table after its e-th shift (e >= 1) with the draws of
    epoch e, PCG64([seed, 0, e]), so the positions that repeat after a shift get fresh draws;
    epoch 0 is PCG64(seed).
    Before the chain the logits can be edited on the device (mi355x_penalize_rows' rule; llama.cpp's
    logit-bias and penalties samplers [U], in its order: the bias, then the penalties, then top-k):
    repeat_penalty, freq_penalty and presence_penalty over the last repeat_last_n tokens (defaults:
    off, as llama.cpp's [U]) and logit_bias, a dict {token: bias} or a list of (token, bias) pairs
    of at most 256 entries, added in list order; float("-inf") bans a token. Greedy decoding with
    penalties is temp=0."""

    def __init__(self, top_k=40, top_p=0.95, min_p=0.05, temp=0.8, seed=0, repeat_last_n=64, repeat_penalty=1.0,
                 freq_penalty=0.0, presence_penalty=0.0, logit_bias=None):
        import math
        self.top_k, self.top_p, self.min_p, self.temp, self.seed = int(top_k), float(top_p), float(min_p), float(temp), seed
        if not (1 <= self.top_k <= SAMPLE_MAX_K and math.isfinite(self.temp) and self.temp >= 0 and
                0 < self.top_p <= 1 and 0 <= self.min_p <= 1):
            raise Mi355xError(f"Sampler: top_k {top_k} in [1, {SAMPLE_MAX_K}], temp {temp} finite and >= 0, top_p {top_p} "
                              f"in (0, 1] and min_p {min_p} in [0, 1] are required")
        self.repeat_last_n = int(repeat_last_n)
        # the values the device takes: float32
        self.repeat_penalty, self.freq_penalty, self.presence_penalty = (_as_f32(v) for v in (repeat_penalty, freq_penalty,
                                                                                            presence_penalty))
        if not (0 <= self.repeat_last_n <= PENALTY_MAX_LAST_N and self.repeat_last_n == repeat_last_n and
                math.isfinite(self.repeat_penalty) and self.repeat_penalty > 0 and math.isfinite(self.freq_penalty) and
                math.isfinite(self.presence_penalty)):
            raise Mi355xError(f"Sampler: repeat_last_n {repeat_last_n} an integer in [0, {PENALTY_MAX_LAST_N}], repeat_penalty "
                              f"{repeat_penalty} finite and > 0 (as float32), freq_penalty {freq_penalty} and "
                              f"presence_penalty {presence_penalty} finite are required")
        try:
            self.logit_bias = [(t, _as_f32(v)) for t, v in bias_pairs(logit_bias)]
        except (TypeError, ValueError) as e:
            raise Mi355xError(f"Sampler: logit_bias must be a dict {{token: bias}} or a list of (token, bias) pairs ({e})")
        if any(math.isnan(v) for _, v in self.logit_bias):
            raise Mi355xError("Sampler: a logit bias is NaN")

    def penalizes(self):
        """True when the window penalty is not the identity."""
        return self.repeat_last_n > 0 and (self.repeat_penalty != 1.0 or self.freq_penalty != 0.0 or
                                           self.presence_penalty != 0.0)

    def edits(self):
        """True when the sampler edits the logits before the chain: a window penalty that is not the
        identity or a bias list that is not empty (a PENALIZE node then precedes the SAMPLE node)."""
        return self.penalizes() or bool(self.logit_bias)

    def penalize_params(self):
        """The PENALIZE node's op_params (the graphs are cached by them too): last_n is 0 where the
        window penalty is the identity, so that node reads no window."""
        return penalize_params(self.repeat_last_n if self.penalizes() else 0, self.repeat_penalty, self.freq_penalty,
                               self.presence_penalty, len(self.logit_bias))

    def params(self, form=SAMPLE_STEP_INPUTS):
        """The SAMPLE nodes' leading op_params (the graphs are cached by them: the seed is not part)."""
        return sampler_params(form, self.top_k, self.temp, self.top_p, self.min_p)

    def draws(self, n, row=None, epoch=0):
        import numpy as np
        seed = self.seed if row is None else [self.seed, row]
        if epoch:  # after the epoch-th context shift of a generate call
            seed = [self.seed, 0 if row is None else row, epoch]
        return np.random.Generator(np.random.PCG64(seed)).random(n, dtype=np.float32)


class _Graph:
    """One graph under construction: its node list, every node's zeroed f32 output buffer and
    every Tensor descriptor (kept alive here; the nodes point at them)."""

    def __init__(self, hp, weights):
        self.hp, self.w, self.dev = hp, weights, weights["output_norm"].device
        self.tensors, self.bufs, self.nodes = [], [], []

    def leaf(self, t, type_, ne0, ne1=1, row_stride=None):
        x = make_tensor(type_, ne0, ne1, t.data_ptr(), row_stride=row_stride)
        self.tensors.append(x)
        return x

    def node(self, op, n, srcs, params=None, flags=0, ne1=1):
        """A node of ne1 rows of n floats: (its descriptor, its output buffer)."""
        import torch
        b = torch.zeros(n * ne1, dtype=torch.float32, device=self.dev)
        self.bufs.append(b)
        x = make_tensor(TYPE_F32, n, ne1, b.data_ptr(), op=op, srcs=srcs, op_params=params, flags=flags)
        self.tensors.append(x)
        self.nodes.append(x)
        return x, b

    def mat(self, name):
        """The leaf of a K-quant matrix (type, uint8 [rows, rowbytes])."""
        t, w = self.w[name]
        return self.leaf(w, t, w.shape[1] // BLOCK_BYTES[t] * QK_K, w.shape[0], row_stride=w.stride(0))

    def experts(self, name):
        """The leaf of an expert tensor (type, uint8 [n_expert, rows, rowbytes]): ne = [K, rows, n_expert]."""
        t, w = self.w[name]
        x = self.leaf(w, t, w.shape[2] // BLOCK_BYTES[t] * QK_K, w.shape[1], row_stride=w.stride(1))
        x.ne[2], x.nb[2], x.nb[3] = w.shape[0], w.stride(0), w.stride(0) * w.shape[0]
        return x

    def rows3(self, x, ne1, ne2):
        """x's descriptor reshaped in place to [ne0, ne1, ne2] packed (ne1 * ne2 its rows); returns x."""
        assert x.ne[1] == ne1 * ne2 and x.ne[2] == 1
        x.ne[1], x.ne[2], x.nb[2], x.nb[3] = ne1, ne2, x.nb[1] * ne1, x.nb[1] * ne1 * ne2
        return x

    def moe_ffn(self, p, cur):
        """build_moe_ffn over cur's T rows in upstream's order [U]: route, up, gate, swiglu, down, combine.
        Returns the combined output's node (f32 [n_embd, T])."""
        import torch
        hp = self.hp
        E, ne, nu, T = hp["n_embd"], hp["n_expert"], hp["n_expert_used"], cur.ne[1]
        gi = self.leaf(self.w[p + MOE_ROUTER], TYPE_F32, E, ne)
        rec = torch.zeros(2 * nu * T, dtype=torch.int32, device=self.dev)  # per row: ids, then the weights' bits
        self.bufs.append(rec)
        route = make_tensor(TYPE_I32, 2 * nu, T, rec.data_ptr(), op=OP_MOE_ROUTE, srcs=[gi, cur], op_params=[nu])
        self.tensors.append(route)
        self.nodes.append(route)
        cur3 = self.rows3(make_tensor(TYPE_F32, E, T, cur.data), 1, T)  # one row a token, for every slot
        self.tensors.append(cur3)

        def mm_id(name, x):
            wt = self.experts(p + name)
            return self.rows3(self.node(OP_MUL_MAT_ID, wt.ne[1], [wt, x, route], ne1=nu * T)[0], nu, T)

        up, gate = mm_id("ffn_up_exps", cur3), mm_id("ffn_gate_exps", cur3)
        par = self.rows3(self.node(OP_SWIGLU, up.ne[0], [gate, up], ne1=nu * T)[0], nu, T)
        ex = mm_id("ffn_down_exps", par)
        return self.node(OP_MOE_COMBINE, E, [ex, route], ne1=T)[0]

    def mm(self, name, x, flags=0):
        wt = self.mat(name)
        return self.node(OP_MUL_MAT, wt.ne[1], [wt, x], flags=flags, ne1=x.ne[1])

    def embed(self, tok):
        et, ew = self.w["token_embd"]
        emb_t = self.leaf(ew, et, self.hp["n_embd"], ew.shape[0], row_stride=ew.stride(0) * ew.element_size())
        return self.node(OP_GET_ROWS, self.hp["n_embd"], [emb_t, tok], ne1=tok.ne[0])

    def norm(self, x, name):
        """rms_norm(x) * the norm weight `name`, over x's rows."""
        n, _ = self.node(OP_RMS_NORM, x.ne[0], [x], [f32_bits(self.hp["eps"])], ne1=x.ne[1])
        return self.node(OP_MUL, x.ne[0], [n, self.leaf(self.w[name], TYPE_F32, x.ne[0])], ne1=x.ne[1])[0]

    def arr(self):
        return _node_array(self.nodes)


class LlamaDecoder:
    """Device state (weights, KV caches, rope table) of one llama model and the graphs that run
    on it: the token graph built here (step, generate) and, built at first use and kept, one
    prompt graph per length (prompt) and one batch graph per (tokens, cells) pair (step_batch,
    generate_batch). Every graph reads the same weights, caches and table.

    weights: dict with "token_embd", "output", "output_norm" and per layer i
    "blk.{i}.<name>" for name in LAYER_MATS + ("attn_norm", "ffn_norm"); a K-quant
    matrix is (type, uint8 cuda tensor [rows, rowbytes]), a norm is an f32 cuda tensor.
    A MoE model (hp["n_expert"] > 0, Mixtral) has per layer, in place of ffn_gate / ffn_up / ffn_down,
    "blk.{i}.ffn_gate_inp", an f32 cuda tensor [n_expert, n_embd], and "blk.{i}.ffn_gate_exps" /
    "ffn_up_exps" / "ffn_down_exps", (type, uint8 cuda tensor [n_expert, rows, rowbytes]); its FFN is
    the MOE_ROUTE / MUL_MAT_ID / MOE_COMBINE nodes, in every graph (they all come from the one layer
    body). A MoE model takes no row split.

    split: a rowsplit.TokenSplit — this process is one rank of a row split; the
    matrices in `weights` are then the rank's row slices (TokenSplit.slice_weights),
    the KV caches hold the rank's KV heads, and every stage's slice is ALL_GATHERed
    (RCCL, the backend's communicator) before the next stage reads it. The logits
    (and every gathered vector) are bit-identical to the single-GPU token. Only the
    token graph is split: prompt, step_batch and the generate calls refuse.
    """

    HOST_SLOTS = 1024
    BATCH_SLOTS = 64  # pinned staging rows of a step_batch graph (tokens | pos | cells | mask)

    def __init__(self, backend: Backend, hp: dict, weights: dict, n_ctx: int, fuse: bool = True, split=None,
                 rope_src: str = "row"):
        """backend None: describe only (host tensors, no device work) — the node list
        the ggml lowering must reproduce (tests/test_lower.py). rope_src "row": the
        attention reads the position's rope row staged with the inputs (the default);
        "table": the whole table (what mi355x_lower_ggml_graph passes)."""
        import torch
        self.b, self.hp, self.w, self.n_ctx, self.split = backend, hp, weights, n_ctx, split
        if split is not None and hp.get("n_expert", 0):
            raise Mi355xError("a MoE model runs on one GPU (no row split)")
        dev = weights["output_norm"].device
        hd = hp["head_dim"]
        kvw = (split.n_head_kv if split is not None else hp["n_head_kv"]) * hd  # this rank's KV heads
        self.gathers = []  # (node output buffer) of every ALL_GATHER, in graph order
        self.reduces = []  # (input partial, output) buffers of every ALL_REDUCE (split mode "reduce")
        self._prompts, self._batches, self._gen_batches, self._batch_hists, self._gen = {}, {}, {}, {}, None
        self._gen_sampled, self._draws, self._batch_draws, self.history, self._bias = {}, None, {}, None, None
        self._shifts = {}  # (n_past, keep, discard) -> the KV_SHIFT node list of shift()
        # inp_tokens, inp_pos and the rope row of that position side by side: one
        # set_tensor of 8 + 4*head_dim bytes per token. The attention reads its cos/sin
        # with q/k/v instead of after the position (one dependent round trip less);
        # the row is the table's row, so the values are those of the device table.
        self.inp = torch.zeros(2 + hd, dtype=torch.int32, device=dev)
        self.token, self.pos = self.inp[0:1], self.inp[1:2]
        if backend is not None:
            self.table = rope_table(n_ctx, hd, hp["freq_base"], 1.0, device=dev, stream=backend.stream)
            self._table_host = self.table.cpu().reshape(n_ctx, hd).view(torch.int32)
        else:
            self.table = torch.zeros(n_ctx * hd, dtype=torch.float32, device=dev)
        self.k_cache = [torch.zeros((n_ctx, kvw), dtype=torch.int16, device=dev) for _ in range(hp["n_layer"])]
        self.v_cache = [torch.zeros((kvw, n_ctx), dtype=torch.int16, device=dev) for _ in range(hp["n_layer"])]

        g = self._graph = _Graph(hp, weights)
        tok = g.leaf(self.token, TYPE_I32, 1)
        pos = g.leaf(self.pos, TYPE_I32, 1)
        if rope_src == "row":
            tab = g.leaf(self.inp[2:], TYPE_F32, hd, 1)  # the position's rope row (ne1 = 1)
        else:
            tab = g.leaf(self.table, TYPE_F32, hd, n_ctx)
        x, self.last_hidden = self._layers(g, tok, pos, tab, split=split)
        self.logits = self._head(g, x, split=split)
        self.nodes, self._arr = g.nodes, g.arr()
        if backend is None:
            return
        # pinned staging slots for (token, pos): a slot is reused only after the stream
        # has been synchronized (the H2D copies are asynchronous)
        self._host = torch.zeros((self.HOST_SLOTS, 2 + hd), dtype=torch.int32).pin_memory()
        self._slot = 0
        backend.set_fusion(fuse)
        torch.cuda.synchronize()  # weights / zeroed caches (torch's stream) before the backend stream runs

    def reset(self):
        for c in self.k_cache + self.v_cache:
            c.zero_()

    def _run(self, L, g, use_graph, times=1):
        """Enqueue the graph g (its "arr" and "nodes") `times` times back to back."""
        for _ in range(times):
            _check(L.mi355x_backend_graph_compute(self.b.h, g["arr"], len(g["nodes"]), 1 if use_graph else 0),
                   "graph_compute")

    # ------------------------------------------------------------ the one layer body and head
    def _gather(self, g, split, part, part_buf, n_local, flags=0):
        """ALL_GATHER of a row-split stage's slice (emitted for every split, a
        world-1 split included: one RCCL copy; none without a split)."""
        if split is None:
            return part, part_buf
        full, b = g.node(OP_ALL_GATHER, n_local * split.world, [part], flags=flags)
        self.gathers.append(b)
        return full, b

    def _layers(self, g, tok, pos, tab, batch=None, out_ids=None, split=None):
        """Embedding and every layer over tok's rows; returns the last residual and its buffer.
        batch (cells, mask, n_kv): the attention is an ATTN_BATCH node that takes every row's
        cache cell and mask row from these; without it ATTN_DECODE (cell == position, causal).
        out_ids: llm_build_llama's inp_out_ids, applied in the last layer of more than one row.
        split: the rank's TokenSplit; the gather and reduce arms below are its exchange nodes."""
        import torch
        hp = self.hp
        E, F, hd, n_ctx = hp["n_embd"], hp["n_ff"], hp["head_dim"], self.n_ctx
        nh, nkv = (split.n_head, split.n_head_kv) if split is not None else (hp["n_head"], hp["n_head_kv"])
        kvw = nkv * hd
        world = split.world if split is not None else 1
        reduce_mode = split is not None and split.mode == "reduce"
        El = E // world
        r_e0 = split.rows["attn_output"][0] if split is not None else 0
        scale = f32_bits(float(torch.tensor(1.0) / torch.sqrt(torch.tensor(float(hd)))))

        def project(name, inp, n_local, res, res_buf, select=None):
            """MUL_MAT `name` of inp (a slice of n_local under a split) plus the residual res."""
            if reduce_mode:
                # K-split over the rank's heads / ffn rows; the residual rides on rank 0's
                # partial, so the ALL_REDUCE(sum) delivers mul_mat + res
                o, ob = g.mm(name, inp)
                if split.rank == 0:
                    o, ob = g.node(OP_ADD, E, [o, res])
                full, b = g.node(OP_ALL_REDUCE, o.ne[0], [o])
                self.reduces.append((ob, b))
                return full, b
            inp, _ = self._gather(g, split, inp, None, n_local)
            o, _ = g.mm(name, inp)
            if select is not None:
                # llm_build_llama's inp_out_ids: after the last attention only the rows whose
                # logits are wanted (the last token's) go on: GET_ROWS of attn_out and inpSA
                o, _ = g.node(OP_GET_ROWS, E, [o, select])
                res, _ = g.node(OP_GET_ROWS, E, [res, select])
            if split is not None:  # the rows [r_e0, r_e0 + El) of the full residual
                res = g.leaf(res_buf[r_e0:r_e0 + El], TYPE_F32, El)
            y, yb = g.node(OP_ADD, El, [o, res], ne1=o.ne[1])
            return self._gather(g, split, y, yb, El)

        x, xb = g.embed(tok)
        for i in range(hp["n_layer"]):
            p = f"blk.{i}."
            m1 = g.norm(x, p + "attn_norm")
            q, k, v = g.mm(p + "attn_q", m1)[0], g.mm(p + "attn_k", m1)[0], g.mm(p + "attn_v", m1)[0]
            kc = g.leaf(self.k_cache[i], TYPE_F16, kvw, n_ctx)
            vc = g.leaf(self.v_cache[i], TYPE_F16, n_ctx, kvw)
            if batch is None:
                att, _ = g.node(OP_ATTN_DECODE, nh * hd, [q, k, v, pos, kc, vc, tab], [nh, nkv, hd, scale],
                                ne1=q.ne[1])
            else:
                cells, mask, n_kv = batch
                att, _ = g.node(OP_ATTN_BATCH, nh * hd, [q, k, v, pos, kc, vc, tab, cells, mask],
                                [nh, nkv, hd, scale, n_kv], ne1=q.ne[1])
            last_rows = out_ids if i == hp["n_layer"] - 1 and x.ne[1] > 1 else None
            ffn_inp, fb = project(p + "attn_output", att, nh * hd, x, xb, select=last_rows)
            m2 = g.norm(ffn_inp, p + "ffn_norm")
            if hp.get("n_expert", 0):  # llm_build_llama's MoE arm: build_moe_ffn, then + ffn_inp
                x, xb = g.node(OP_ADD, E, [g.moe_ffn(p, m2), ffn_inp], ne1=m2.ne[1])
                continue
            gt, up = g.mm(p + "ffn_gate", m2)[0], g.mm(p + "ffn_up", m2)[0]
            glu, _ = g.node(OP_SWIGLU, gt.ne[0], [gt, up], ne1=gt.ne[1])
            x, xb = project(p + "ffn_down", glu, F // world, ffn_inp, fb)
        return x, xb

    def _head(self, g, x, split=None):
        """output_norm -> output over x's rows; returns the logits' buffer."""
        m3 = g.norm(x, "output_norm")
        if split is None:
            return g.mm("output", m3, flags=FLAG_OUTPUT)[1]
        lg, lb = g.mm("output", m3)
        return self._gather(g, split, lg, lb, self.hp["n_vocab"] // split.world, flags=FLAG_OUTPUT)[1]

    # ------------------------------------------------------------ prompt processing
    def _prompt_graph(self, n_tok: int, all_rows: bool = False):
        """Node list of a prompt batch of n_tok tokens (llm_build_llama over a ubatch,
        ggml's batched non-flash attention; llama-bench pp): the same weights, caches and
        rope table as the decode token. MUL_MATs take ne11 = n_tok columns (the int8-MFMA
        GEMMs), RMS_NORM/MUL/ADD/SWIGLU run on [n, n_tok], the attention node writes the
        batch's cells then runs every query causally, and only the last token's row goes
        through the output norm and head (llama.cpp computes the logits of the last token
        of a prompt).
        all_rows: the graph of logprobs, a cache entry of its own: the same layers with no row
        selection, the head over all n_tok rows and a LOGPROB_BATCH node (flagged output) on the
        logits and one more input section, the rows' targets: token ids | positions | targets."""
        import torch
        cached = self._prompts.get(("all_rows", n_tok) if all_rows else n_tok)
        if cached is not None:
            return cached
        if self.split is not None:
            raise Mi355xError("prompt processing runs on one GPU (no row split)")
        g = _Graph(self.hp, self.w)
        if all_rows:
            inp = torch.zeros(3 * n_tok, dtype=torch.int32, device=g.dev)
            tok = g.leaf(inp[:n_tok], TYPE_I32, n_tok)
            pos = g.leaf(inp[n_tok:2 * n_tok], TYPE_I32, n_tok)
            targets = g.leaf(inp[2 * n_tok:], TYPE_I32, n_tok)
            tab = g.leaf(self.table, TYPE_F32, self.hp["head_dim"], self.n_ctx)
            x, hidden = self._layers(g, tok, pos, tab)
            logits = self._head(g, x)
            rec = torch.zeros(6 * n_tok, dtype=torch.int32, device=g.dev)  # [n_tok] struct mi355x_logprob
            lp = make_tensor(TYPE_I32, 6, n_tok, rec.data_ptr(), op=OP_LOGPROB_BATCH, srcs=[g.nodes[-1], targets],
                             flags=FLAG_OUTPUT)
            g.tensors.append(lp)
            g.nodes.append(lp)
            on_dev = self.b is not None
            pg = dict(graph=g, inp=inp, nodes=g.nodes, logits=logits.view(n_tok, self.hp["n_vocab"]), hidden=hidden,
                      rec=rec, arr=g.arr(), host=torch.zeros(3 * n_tok, dtype=torch.int32).pin_memory() if on_dev else None,
                      rec_host=torch.zeros(6 * n_tok, dtype=torch.int32).pin_memory() if on_dev else None)
            self._prompts[("all_rows", n_tok)] = pg
            if on_dev:
                torch.cuda.synchronize()  # zeroed buffers (torch's stream) before the backend stream runs
            return pg
        inp = torch.zeros(2 * n_tok + 1, dtype=torch.int32, device=g.dev)  # token ids | positions | out id
        tok = g.leaf(inp[:n_tok], TYPE_I32, n_tok)
        pos = g.leaf(inp[n_tok:2 * n_tok], TYPE_I32, n_tok)
        out_ids = g.leaf(inp[2 * n_tok:], TYPE_I32, 1)  # inp_out_ids: the last token's row
        tab = g.leaf(self.table, TYPE_F32, self.hp["head_dim"], self.n_ctx)
        x, hidden = self._layers(g, tok, pos, tab, out_ids=out_ids)
        logits = self._head(g, x)
        pg = dict(graph=g, inp=inp, nodes=g.nodes, logits=logits, hidden=hidden, arr=g.arr(),
                  host=torch.zeros(2 * n_tok + 1, dtype=torch.int32).pin_memory() if self.b is not None else None)
        self._prompts[n_tok] = pg
        if self.b is not None:
            torch.cuda.synchronize()  # zeroed buffers (torch's stream) before the backend stream runs
        return pg

    def prompt(self, tokens, start_pos: int = 0, use_graph: bool = True):
        """Enqueue a prompt batch (positions start_pos ..): writes its KV cells and returns
        the device logits of its last token (no synchronization). The logits and the cache
        equal those of decoding the tokens one by one with step(), bit for bit."""
        n_tok = len(tokens)
        if n_tok < 1 or start_pos < 0 or start_pos + n_tok > self.n_ctx:
            raise Mi355xError(f"prompt of {n_tok} tokens at {start_pos} outside the KV cache (n_ctx {self.n_ctx})")
        if any(not 0 <= t < self.hp["n_vocab"] for t in tokens):
            raise Mi355xError("prompt token outside the vocabulary")
        from . import lib
        g = self._prompt_graph(n_tok)
        self.b.synchronize()  # the pinned staging row is reused: the previous prompt's copy is done
        host = g["host"]
        host[:n_tok] = torch_tensor(tokens)
        host[n_tok:2 * n_tok] = torch_tensor(range(start_pos, start_pos + n_tok))
        host[2 * n_tok] = n_tok - 1
        L = lib()
        _check(L.mi355x_backend_set_tensor(self.b.h, g["inp"].data_ptr(), host.data_ptr(), 4 * host.numel()),
               "set_tensor")
        self._run(L, g, use_graph)
        self.prompt_hidden = g["hidden"]
        return g["logits"]

    # ------------------------------------------------------------ log-probabilities and perplexity
    def _check_logprobs(self, who: str, tokens):
        """What logprobs and perplexity refuse whatever the positions are, in the name of `who`."""
        V = self.hp["n_vocab"]
        if self.split is not None:
            raise Mi355xError(f"{who} runs on one GPU (no row split)")
        if V % 4 or V > LOGPROB_MAX_N:
            raise Mi355xError(f"{who}: the vocabulary must be a multiple of 4 entries up to {LOGPROB_MAX_N} "
                              "(LOGPROB_BATCH's rows)")
        if any(not 0 <= t < V for t in tokens):
            raise Mi355xError(f"{who}: token outside the vocabulary")

    def logprobs(self, tokens, start_pos: int = 0, targets=None, use_graph: bool = True, records: bool = False):
        """The log-probabilities of given tokens under the model: runs the tokens as one prompt batch
        at positions start_pos .. (writing their KV cells as prompt does), the head over every row
        and mi355x_logprob_rows on the logits, synchronizes and copies back 24 bytes a token.
        targets None: row i is scored on tokens[i + 1]; returns len(tokens) - 1 float64 values,
        log softmax(logits of row i)[tokens[i + 1]]. targets: one index per row (an index outside
        the vocabulary scores NaN); returns len(tokens) values. records: the rows' records
        themselves (ggml_mi355x.logprob_dtype(): max, x_target, argmax, pad, sum) instead of
        logprob_value of them. The rule is exact (include/ggml_mi355x.h): the records equal
        tests/logprob_ref.py's on the logits step() produces token by token, bit for bit."""
        n_tok = len(tokens)
        self._check_logprobs("logprobs", tokens)
        if n_tok < 1 or start_pos < 0 or start_pos + n_tok > self.n_ctx:
            raise Mi355xError(f"logprobs: {n_tok} tokens at {start_pos} outside the KV cache (n_ctx {self.n_ctx})")
        tg = list(tokens[1:]) + [-1] if targets is None else [int(t) for t in targets]  # (-1: no target, NaN)
        if len(tg) != n_tok or any(not -2 ** 31 <= t < 2 ** 31 for t in tg):
            raise Mi355xError("logprobs: targets need one int32 per token")
        from . import lib
        g = self._prompt_graph(n_tok, all_rows=True)
        self.b.synchronize()  # the pinned staging rows are reused: the previous call's copies are done
        host = g["host"]
        host[:n_tok] = torch_tensor(tokens)
        host[n_tok:2 * n_tok] = torch_tensor(range(start_pos, start_pos + n_tok))
        host[2 * n_tok:] = torch_tensor(tg)
        L = lib()
        _check(L.mi355x_backend_set_tensor(self.b.h, g["inp"].data_ptr(), host.data_ptr(), 4 * host.numel()),
               "set_tensor")
        self._run(L, g, use_graph)
        _check(L.mi355x_backend_get_tensor(self.b.h, g["rec_host"].data_ptr(), g["rec"].data_ptr(), 24 * n_tok),
               "get_tensor")
        self.b.synchronize()
        rec = g["rec_host"].numpy().view(logprob_dtype()).copy()
        if targets is None:
            rec = rec[:-1]
        return rec if records else logprob_value(rec)

    def perplexity(self, tokens, n_ctx=None, n_batch: int = 512, bos=None, progress=None):
        """llama-perplexity's procedure [U] over a text of token ids: len(tokens) // n_ctx chunks of
        n_ctx tokens (n_ctx None: the decoder's), each run from position 0 in batches of n_batch
        (a batch continues its chunk at start_pos; the cells a previous chunk left above the
        position are never read by the causal attention); bos: that id replaces each chunk's first
        token. Scored are the rows n_ctx // 2 .. n_ctx - 2 of each chunk, row i on the chunk's
        token i + 1; the negative log-likelihood is summed in float64 in that order. Returns
        dict(ppl=exp(nll / count), nll, count, top1): top1 the share of scored rows whose argmax is
        their target. progress(chunks done, chunks, nll, count) is called after each chunk."""
        n_ctx = self.n_ctx if n_ctx is None else int(n_ctx)
        if not 3 <= n_ctx <= self.n_ctx or n_batch < 1:
            raise Mi355xError(f"perplexity: n_ctx {n_ctx} must lie in [3, {self.n_ctx}] and n_batch {n_batch} be >= 1")
        n_chunk = len(tokens) // n_ctx
        if n_chunk < 1:
            raise Mi355xError(f"perplexity: {len(tokens)} tokens are less than one chunk of {n_ctx}")
        if bos is not None and not 0 <= bos < self.hp["n_vocab"]:
            raise Mi355xError("perplexity: bos outside the vocabulary")
        self._check_logprobs("perplexity", tokens[:n_chunk * n_ctx])
        first, nll, count, hits = n_ctx // 2, 0.0, 0, 0
        for c in range(n_chunk):
            chunk = [int(t) for t in tokens[c * n_ctx:(c + 1) * n_ctx]]
            tg = chunk[1:] + [-1]
            if bos is not None:
                chunk[0] = bos
            for j in range(0, n_ctx, n_batch):
                rec = self.logprobs(chunk[j:j + n_batch], start_pos=j, targets=tg[j:j + n_batch], records=True)
                lo, hi = max(first, j), min(n_ctx - 1, j + len(rec))  # the scored rows of this batch
                if lo >= hi:
                    continue
                lp = logprob_value(rec[lo - j:hi - j])
                for v in lp.tolist():
                    nll += -v
                count += hi - lo
                hits += int((rec["argmax"][lo - j:hi - j] == tg[lo:hi]).sum())
            if progress is not None:
                progress(c + 1, n_chunk, nll, count)
        return dict(ppl=ppl_of(nll, count), nll=nll, count=count, top1=hits / count)

    # ------------------------------------------------------------ several sequences per step
    def _batch_graph(self, n_tok: int, n_kv: int):
        """Node list of one batch of n_tok tokens that may belong to different sequences
        (llm_build_llama over a ubatch with a unified KV cache): like _prompt_graph, but each
        attention block is an ATTN_BATCH node that takes every token's cache cell and mask row
        from the inputs, and the output norm and head run over all n_tok rows (every sequence
        needs its logits). Inputs, one device buffer: token ids | positions | cells (int32
        [n_tok] each) | the mask, f32 [n_tok, n_kv]."""
        import torch
        key = (n_tok, n_kv)
        cached = self._batches.get(key)
        if cached is not None:
            return cached
        if self.split is not None:
            raise Mi355xError("batched decoding runs on one GPU (no row split)")
        g = _Graph(self.hp, self.w)
        inp = torch.zeros(3 * n_tok + n_tok * n_kv, dtype=torch.int32, device=g.dev)
        tok = g.leaf(inp[:n_tok], TYPE_I32, n_tok)
        pos = g.leaf(inp[n_tok:2 * n_tok], TYPE_I32, n_tok)
        cells = g.leaf(inp[2 * n_tok:3 * n_tok], TYPE_I32, n_tok)
        mask = g.leaf(inp[3 * n_tok:], TYPE_F32, n_kv, n_tok)
        tab = g.leaf(self.table, TYPE_F32, self.hp["head_dim"], self.n_ctx)
        x, _ = self._layers(g, tok, pos, tab, batch=(cells, mask, n_kv))
        logits = self._head(g, x)
        bg = dict(graph=g, inp=inp, nodes=g.nodes, logits=logits.view(n_tok, self.hp["n_vocab"]), arr=g.arr(),
                  host=torch.zeros((self.BATCH_SLOTS, inp.numel()), dtype=torch.int32).pin_memory()
                  if self.b is not None else None, slot=0)
        self._batches[key] = bg
        if self.b is not None:
            torch.cuda.synchronize()  # zeroed buffers (torch's stream) before the backend stream runs
        return bg

    def step_batch(self, tokens, pos, cells, mask, n_kv: int, use_graph: bool = True):
        """Enqueue one batch of T tokens of any sequences (no synchronization): token i has
        position pos[i] (its rope row), is stored at cache cell cells[i] and attends over cells
        [0, n_kv) under mask[i] (additive: 0 visible, -inf hidden; [T, >= n_kv] floats, numpy or
        torch on the host). Returns the device logits [T, n_vocab]. The graph of a (T, n_kv)
        pair is built once and replayed with new input contents."""
        m = self._check_batch("step_batch", tokens, pos, cells, mask, n_kv)
        g = self._batch_graph(len(tokens), n_kv)
        L = self._stage_batch(g, tokens, pos, cells, m)
        self._run(L, g, use_graph)
        return g["logits"]

    def _check_batch(self, who: str, tokens, pos, cells, mask, n_kv: int):
        """The argument checks of a batch step, raised in the name of the caller `who` (nothing is
        enqueued); returns the mask as a float32 tensor."""
        import numpy as np
        import torch
        n_tok = len(tokens)
        if n_tok < 1 or len(pos) != n_tok or len(cells) != n_tok:
            raise Mi355xError(f"{who}: tokens, pos and cells need one entry per token")
        if n_kv < 32 or n_kv % 32 or n_kv > self.n_ctx:
            raise Mi355xError(f"{who}: n_kv {n_kv} must be a multiple of 32 in [32, n_ctx {self.n_ctx}]")
        if any(not 0 <= t < self.hp["n_vocab"] for t in tokens):
            raise Mi355xError(f"{who}: token outside the vocabulary")
        if any(not 0 <= c < self.n_ctx for c in cells) or any(not 0 <= p < self.n_ctx for p in pos):
            raise Mi355xError(f"{who}: cell or position outside the KV cache (n_ctx {self.n_ctx})")
        m = torch.as_tensor(np.asarray(mask, dtype=np.float32) if not torch.is_tensor(mask) else mask).to(torch.float32)
        if m.dim() != 2 or m.shape[0] != n_tok or m.shape[1] < n_kv:
            raise Mi355xError(f"{who}: mask must be [{n_tok}, >= {n_kv}]")
        return m

    def _stage_batch(self, g, tokens, pos, cells, m):
        """(tokens | pos | cells | mask) from a pinned row into the batch graph's input block."""
        import torch
        from . import lib
        n_tok = len(tokens)
        n_kv = (g["inp"].numel() - 3 * n_tok) // n_tok
        if g["slot"] == self.BATCH_SLOTS:  # a pinned staging row is reused only after its copy is done
            self.b.synchronize()
            g["slot"] = 0
        host = g["host"][g["slot"]]
        g["slot"] += 1
        host[:n_tok] = torch_tensor(tokens)
        host[n_tok:2 * n_tok] = torch_tensor(pos)
        host[2 * n_tok:3 * n_tok] = torch_tensor(cells)
        host[3 * n_tok:].view(torch.float32).view(n_tok, n_kv).copy_(m[:, :n_kv])
        L = lib()
        _check(L.mi355x_backend_set_tensor(self.b.h, g["inp"].data_ptr(), host.data_ptr(), 4 * host.numel()),
               "set_tensor")
        return L

    # ------------------------------------------------------------ the samplers' draws
    def _draws_table(self, rows=None):
        """The device table the SAMPLE node (rows None) or the SAMPLE_BATCH node of `rows` sequences
        reads its draws from: f32 [n_ctx + 1] a sequence, entry p the draw of the token that
        will stand at position p. Allocated once (the graphs hold its address), filled by _seed."""
        import torch
        if rows is None:
            if self._draws is None:
                self._draws = dict(dev=torch.zeros(self.n_ctx + 1, dtype=torch.float32, device=self.inp.device), seed=None)
            return self._draws
        if rows not in self._batch_draws:
            self._batch_draws[rows] = dict(dev=torch.zeros((rows, self.n_ctx + 1), dtype=torch.float32,
                                                           device=self.inp.device), seed=None)
        return self._batch_draws[rows]

    def _seed(self, sampler, rows=None, epoch=0):
        """Fills the draws table for sampler.seed unless it holds that seed's draws already: the
        backend is synchronized first (a run may still read the table), torch's stream after.
        epoch >= 1 (the token graph's table): the draws after that many context shifts."""
        import numpy as np
        import torch
        d = self._draws_table(rows)
        held = (sampler.seed,) if epoch == 0 else (sampler.seed, epoch)
        if d["seed"] is not None and d["seed"] == held:
            return
        n = self.n_ctx + 1
        host = sampler.draws(n, epoch=epoch) if rows is None else np.stack([sampler.draws(n, i) for i in range(rows)])
        self.b.synchronize()
        d["dev"].copy_(torch.from_numpy(host))
        torch.cuda.synchronize()
        d["seed"] = held

    # ------------------------------------------------------------ the samplers' edits of the logits
    def _bias_lists(self):
        """The device lists every PENALIZE node reads the logit bias from: LOGIT_BIAS_MAX (token, bias)
        entries a decoder, shared by all rows and graphs. Allocated once (the graphs hold its
        address), filled by _set_bias."""
        import torch
        if self._bias is None:
            dev = self.inp.device
            self._bias = dict(tok=torch.full((LOGIT_BIAS_MAX,), -1, dtype=torch.int32, device=dev),
                              val=torch.zeros(LOGIT_BIAS_MAX, dtype=torch.float32, device=dev), held=[])
        return self._bias

    def _set_bias(self, sampler):
        """Fills the bias lists with sampler.logit_bias unless they hold it already, as _seed fills the
        draws: the backend is synchronized first (a run may still read them), torch's stream after."""
        import torch
        d = self._bias_lists()
        if d["held"] == sampler.logit_bias:
            return
        self.b.synchronize()
        n = len(sampler.logit_bias)
        if n:
            d["tok"][:n].copy_(torch.tensor([t for t, _ in sampler.logit_bias], dtype=torch.int32))
            d["val"][:n].copy_(torch.tensor([v for _, v in sampler.logit_bias], dtype=torch.float32))
        torch.cuda.synchronize()
        d["held"] = list(sampler.logit_bias)

    def _penalize_node(self, sampler, logits, end, hist):
        """sampler's PENALIZE node in place on the node `logits`, with the positions `end` and the
        history `hist` (both left out where the node reads no window): (the node, the descriptors it
        keeps alive). The SAMPLE node that follows takes it as its src0."""
        pp = sampler.penalize_params()
        d, n_bias, win = self._bias_lists(), pp[4], pp[0] > 0
        srcs = [logits, end if win else None, hist if win else None,
                make_tensor(TYPE_I32, n_bias, 1, d["tok"].data_ptr()) if n_bias else None,
                make_tensor(TYPE_F32, n_bias, 1, d["val"].data_ptr()) if n_bias else None]
        pen = make_tensor(TYPE_F32, logits.ne[0], logits.ne[1], logits.data, op=OP_PENALIZE, srcs=srcs, op_params=pp,
                          flags=FLAG_OUTPUT)
        return pen, [s for s in srcs[1:] if s is not None]

    def _check_context(self, who: str, context, pos: int):
        """The sampler's memory of the tokens before `pos` as a list of ints (None: empty)."""
        ctx = [] if context is None else [int(t) for t in context]
        if len(ctx) > pos or any(not -2 ** 31 <= t < 2 ** 31 for t in ctx):
            raise Mi355xError(f"{who}: the context holds at most pos ({pos}) int32 tokens, the last at pos - 1")
        return ctx

    def _stage_history(self, L, host, dev, token: int, pos: int, ctx, last_n: int):
        """What an editing sampler's first window reads, from the pinned row `host` into the history
        row `dev` with one copy: entries [max(0, pos - last_n + 1), pos] = the context's tail, -1
        where the context does not reach, and the start token at pos."""
        import torch
        if last_n < 1:
            return
        lo = max(0, pos - last_n + 1)
        k = min(len(ctx), pos - lo)
        host[lo:pos - k] = -1
        if k:
            host[pos - k:pos] = torch_tensor(ctx[len(ctx) - k:])
        host[pos] = token
        _check(L.mi355x_backend_set_tensor(self.b.h, dev[lo:].data_ptr(), host[lo:].data_ptr(), 4 * (pos - lo + 1)),
               "set_tensor")

    # ------------------------------------------------------------ greedy generation of several sequences
    def _generate_batch_graph(self, n_tok: int, n_kv: int, cell_stride: int, sampler=None):
        """_batch_graph(n_tok, n_kv)'s nodes plus one step-inputs ARGMAX_BATCH on the logits: it ends
        the step by writing every sequence's next token, position and cell into that graph's own
        input block, showing the new cell in the sequence's mask row and filing the token in
        self.batch_history[i][pos + 1], so the one captured graph is replayed with no host copy."""
        import torch
        edits = sampler is not None and sampler.edits()
        key = (n_tok, n_kv, cell_stride) + (() if sampler is None else tuple(sampler.params())) + \
            (tuple(sampler.penalize_params()) if edits else ())
        cached = self._gen_batches.get(key)
        if cached is not None:
            return cached
        g = self._batch_graph(n_tok, n_kv)
        hists = self._batch_hists
        if n_tok not in hists:  # one per T: every step, the last cell's included, has an entry
            hists[n_tok] = dict(dev=torch.zeros((n_tok, self.n_ctx + 1), dtype=torch.int32, device=g["inp"].device),
                                host=torch.zeros((n_tok, self.n_ctx + 1), dtype=torch.int32).pin_memory())
        hist, inp, T = hists[n_tok]["dev"], g["inp"], n_tok
        srcs = [g["nodes"][-1],
                make_tensor(TYPE_I32, T, 1, inp[T:2 * T].data_ptr()),
                make_tensor(TYPE_I32, T, 1, inp[2 * T:3 * T].data_ptr()),
                make_tensor(TYPE_F32, n_kv, T, inp[3 * T:].data_ptr()),
                make_tensor(TYPE_I32, self.n_ctx + 1, T, hist.data_ptr())]
        if sampler is None:
            am = make_tensor(TYPE_I32, T, 1, inp.data_ptr(), op=OP_ARGMAX_BATCH, srcs=srcs,
                             op_params=[ARGMAX_STEP_INPUTS, cell_stride, n_kv], flags=FLAG_OUTPUT)
        else:  # the same writes with sampled tokens: one more source, the sequences' draws
            srcs.append(make_tensor(TYPE_F32, self.n_ctx + 1, T, self._draws_table(T)["dev"].data_ptr()))
            keep = []
            if edits:  # ... logits, PENALIZE, SAMPLE_BATCH(src0 = PENALIZE): the edit in place, before the top-k
                pen, keep = self._penalize_node(sampler, srcs[0], srcs[1], srcs[4])
                srcs[0] = pen
            am = make_tensor(TYPE_I32, T, 1, inp.data_ptr(), op=OP_SAMPLE_BATCH, srcs=srcs,
                             op_params=sampler.params() + [cell_stride, n_kv], flags=FLAG_OUTPUT)
            srcs = srcs + keep
        nodes = g["nodes"] + ([srcs[0]] if edits else []) + [am]
        gg = dict(batch=g, nodes=nodes, keep=srcs + [am], hist=hists[n_tok], arr=_node_array(nodes))
        self._gen_batches[key] = gg
        torch.cuda.synchronize()  # the zeroed history (torch's stream) before the backend stream runs
        return gg

    def generate_batch(self, tokens, pos, cells, mask, n: int, n_kv: int, cell_stride: int = 1, eos=None,
                       chunk: int = 32, use_graph: bool = True, sampler=None, contexts=None):
        """Greedy decoding of n steps of T sequences together: sequence i starts from tokens[i] at
        position pos[i] in cache cell cells[i] under mask[i] (step_batch's inputs), and its step k
        runs at position pos[i] + k in cell cells[i] + k * cell_stride. Returns a list of T lists of
        ints: sequence i's tokens, each the argmax of its row of that step's logits
        (mi355x_argmax's rule). The inputs are staged from the host once; then the graph runs
        `chunk` times back to back, each step's ARGMAX_BATCH node staging the next (tokens,
        positions, cells, and the new cell made visible in its own sequence's mask row), and only
        after a chunk the host synchronizes and reads the chunk's tokens from the history
        (self.batch_history, int32 [T, n_ctx + 1]: row i holds the token picked at position p in
        entry p + 1). No mask is rebuilt or copied per step, so the cells the steps after the
        first will write must be hidden (-inf) in every row of `mask`: the device shows each to
        its own sequence when its turn comes, and to no other sequence ever.
        eos: a sequence's list ends with its first such token; the call returns when every
        sequence has ended or after n steps. A finished sequence keeps running on the device to
        the end of the call's steps (the last chunk's included): its later cells and history
        entries are written too. A following step_batch or generate_batch works as ever: it
        restages the whole input block.
        sampler: a Sampler: every token is sampled on the device instead (a SAMPLE_BATCH node ends
        the step), sequence i's token for position p with entry p of its own row of draws.
        contexts: with a sampler that edits the logits (Sampler.edits()), sequence i's tokens before
        pos[i] as generate's `context` (None, or one list or None per sequence); every row's window
        is its own. Ignored otherwise. The logits buffer then holds the edited logits after a step."""
        import numpy as np
        if self.split is not None:
            raise Mi355xError("generate_batch runs on one GPU (no row split)")
        m = self._check_batch("generate_batch", tokens, pos, cells, mask, n_kv)
        T = len(tokens)
        if n < 0 or chunk < 1 or cell_stride < 1:
            raise Mi355xError(f"generate_batch: n {n}, chunk {chunk} and cell_stride {cell_stride} must be >= 0, >= 1 "
                              "and >= 1")
        if self.hp["n_vocab"] % 4:
            raise Mi355xError("generate_batch: the vocabulary must be a multiple of 4 entries (ARGMAX_BATCH's rows)")
        if n == 0:
            return [[] for _ in range(T)]
        if any(c + (n - 1) * cell_stride >= n_kv for c in cells) or any(p + n - 1 >= self.n_ctx for p in pos):
            raise Mi355xError(f"generate_batch: {n} steps leave the cells [0, n_kv {n_kv}) or the positions "
                              f"[0, n_ctx {self.n_ctx})")
        written = np.asarray(cells, dtype=np.int64)[:, None] + cell_stride * np.arange(n, dtype=np.int64)[None, :]
        if np.unique(written).size != written.size:
            raise Mi355xError("generate_batch: two steps would write the same cache cell")
        if not np.isneginf(m[:, :n_kv].numpy()[:, written[:, 1:].ravel()]).all():
            raise Mi355xError("generate_batch: a cell that a later step writes is visible in the mask (every such cell "
                              "must be -inf in every row; the device shows it to its own sequence)")
        edits = sampler is not None and sampler.edits()
        if edits:
            if contexts is not None and len(contexts) != T:
                raise Mi355xError("generate_batch: contexts needs one entry per sequence")
            ctxs = [self._check_context("generate_batch", None if contexts is None else contexts[i], pos[i])
                    for i in range(T)]
        g = self._generate_batch_graph(T, n_kv, cell_stride, sampler)
        if sampler is not None:
            self._seed(sampler, T)
        if edits:
            self._set_bias(sampler)
        self.batch_history = g["hist"]["dev"]
        L = self._stage_batch(g["batch"], tokens, pos, cells, m)
        dev, host = g["hist"]["dev"], g["hist"]["host"]
        if edits:
            for i in range(T):
                self._stage_history(L, host[i], dev[i], tokens[i], pos[i], ctxs[i], sampler.repeat_last_n)
        out, live, done = [[] for _ in range(T)], [True] * T, 0
        while done < n and any(live):
            c = min(chunk, n - done)
            self._run(L, g, use_graph, times=c)
            # the chunk's tokens of sequence i: history[i][p + 1] for its steps at p
            for i in range(T):
                lo = pos[i] + done + 1
                _check(L.mi355x_backend_get_tensor(self.b.h, host[i, lo:].data_ptr(), dev[i, lo:].data_ptr(), 4 * c),
                       "get_tensor")
            self.b.synchronize()
            for i in range(T):
                if not live[i]:
                    continue
                lo = pos[i] + done + 1
                for t in host[i, lo:lo + c].tolist():
                    out[i].append(t)
                    if eos is not None and t == eos:
                        live[i] = False
                        break
            done += c
        return out

    def _stage_inputs(self, token: int, pos: int):
        """(token, pos, the position's rope row) from a pinned slot into the input block."""
        if not 0 <= pos < self.n_ctx:
            raise Mi355xError(f"position {pos} outside the KV cache (n_ctx {self.n_ctx})")
        if not 0 <= token < self.hp["n_vocab"]:
            raise Mi355xError(f"token {token} outside the vocabulary (n_vocab {self.hp['n_vocab']})")
        from . import lib
        if self._slot == self.HOST_SLOTS:
            self.b.synchronize()
            self._slot = 0
        row = self._host[self._slot]
        row[0] = token
        row[1] = pos
        row[2:] = self._table_host[pos]
        L = lib()
        self._slot += 1
        _check(L.mi355x_backend_set_tensor(self.b.h, self.inp.data_ptr(), row.data_ptr(), 4 * row.numel()),
               "set_tensor")
        return L

    def step(self, token: int, pos: int, use_graph: bool = True):
        """Enqueue one token (no synchronization); returns the device logits tensor."""
        L = self._stage_inputs(token, pos)
        _check(L.mi355x_backend_graph_compute(self.b.h, self._arr, len(self.nodes), 1 if use_graph else 0),
               "graph_compute")
        return self.logits

    # ------------------------------------------------------------ greedy generation on the device
    def _generate_graph(self, sampler=None):
        """The decode token's nodes plus one step-inputs ARGMAX on the logits: it ends the token
        by writing the next one's (token, pos, rope row) into the input block and the token into
        self.history[pos + 1], so the one captured graph is replayed with no host copy. With a
        sampler the last node is a step-inputs SAMPLE instead: the same writes with the sampled
        token, one more source (the draws); one graph per sampler parameters."""
        import torch
        edits = sampler is not None and sampler.edits()
        key = None if sampler is None else tuple(sampler.params()) + (tuple(sampler.penalize_params()) if edits else ())
        cached = self._gen if sampler is None else self._gen_sampled.get(key)
        if cached is not None:
            return cached
        hd = self.hp["head_dim"]
        if self.history is None:
            self.history = torch.zeros(self.n_ctx, dtype=torch.int32, device=self.inp.device)
        srcs = [self.nodes[-1],
                make_tensor(TYPE_I32, 1, 1, self.pos.data_ptr()),
                make_tensor(TYPE_F32, hd, self.n_ctx, self.table.data_ptr()),
                make_tensor(TYPE_I32, self.n_ctx, 1, self.history.data_ptr())]
        if sampler is None:
            am = make_tensor(TYPE_I32, 2 + hd, 1, self.inp.data_ptr(), op=OP_ARGMAX, srcs=srcs,
                             op_params=[ARGMAX_STEP_INPUTS], flags=FLAG_OUTPUT)
        else:
            srcs.append(make_tensor(TYPE_F32, self.n_ctx + 1, 1, self._draws_table()["dev"].data_ptr()))
            keep = []
            if edits:  # ... logits, PENALIZE, SAMPLE(src0 = PENALIZE): the edit in place, before the top-k
                pen, keep = self._penalize_node(sampler, srcs[0], srcs[1], srcs[3])
                srcs[0] = pen
            am = make_tensor(TYPE_I32, 2 + hd, 1, self.inp.data_ptr(), op=OP_SAMPLE, srcs=srcs,
                             op_params=sampler.params(), flags=FLAG_OUTPUT)
            srcs = srcs + keep
        nodes = self.nodes + ([srcs[0]] if edits else []) + [am]
        g = dict(nodes=nodes, keep=srcs + [am], arr=_node_array(nodes))
        if sampler is None:
            self._gen = g
        else:
            self._gen_sampled[key] = g
        if self.b is not None:  # (describe only: no device work)
            g["host"] = torch.zeros(self.n_ctx + 1, dtype=torch.int32).pin_memory()
            torch.cuda.synchronize()  # the zeroed history (torch's stream) before the backend stream runs
        return g

    def generate(self, token: int, pos: int, n: int, eos=None, chunk: int = 32, use_graph: bool = True, sampler=None,
                 context=None, keep=None, discard=None):
        """Greedy decoding of n tokens at positions pos .. pos + n - 1, starting from `token` at
        `pos`: returns the generated tokens as a list of ints (the token picked after position p
        is the argmax of that step's logits, mi355x_argmax's rule). The inputs are staged from the
        host once; then the graph runs `chunk` times back to back, each step's ARGMAX node staging
        the next, and only after a chunk the host synchronizes and reads its tokens with one copy.
        eos: stop at the first such token, which is returned as the last one (the device may have
        run on to the end of that chunk: its later cells and history entries are then written
        too). A following step() works as ever: it restages the whole input block.
        sampler: a Sampler: every token is sampled on the device instead (mi355x_sample's rule; a
        SAMPLE node ends the token), the token for position p with entry p of the seed's draws.
        A sampler that edits the logits (Sampler.edits(): penalties, logit bias) puts a PENALIZE node
        between the logits and the SAMPLE node: mi355x_penalize_rows' rule on the window
        history[pos - repeat_last_n + 1 .. pos] of every step, which the steps themselves extend.
        context: the sampler's memory of the tokens before `pos` (llama.cpp's accepted tokens): at
        most pos tokens, the last standing at pos - 1; it is not checked against the cache. Before
        the first step the host writes the history entries [max(0, pos - repeat_last_n + 1), pos]
        with one copy: the context's tail, -1 where the context does not reach, `token` at pos.
        Without such a sampler context is ignored and the history below pos + 1 is not written.
        Under an editing sampler the logits buffer holds the edited logits after a step (llama.cpp
        edits a copy; here a copy would cost another pass over the row).
        keep: None: n tokens must fit the cache from pos. An integer in [0, n_ctx - 1): generation
        goes on past the end of the cache by llama.cpp's context shift [U]: the chunks are cut so
        that one ends with the step on cell n_ctx - 1; then, the host being synchronized for that
        chunk, shift(n_ctx, keep, d) drops the cells [keep, keep + d), d = discard or
        (n_ctx - keep) // 2 (llama.cpp main's n_left / 2), the history moves with the cells, the
        inputs are restaged with the last token at position n_ctx - d, and the steps go on. Under a
        sampler the draws after the e-th shift of the call are those of epoch e (Sampler).
        discard: an integer in [1, n_ctx - keep]; it needs keep."""
        if self.split is not None:
            raise Mi355xError("generate runs on one GPU (no row split)")
        if n < 0 or chunk < 1:
            raise Mi355xError(f"generate: n {n} and chunk {chunk} must be >= 0 and >= 1")
        n_ctx = self.n_ctx
        if keep is None:
            if discard is not None:
                raise Mi355xError("generate: discard needs keep")
            if not 0 <= pos < n_ctx or n > n_ctx - pos:
                raise Mi355xError(f"generate: {n} tokens from position {pos} outside the KV cache (n_ctx {n_ctx})")
        else:
            if not 0 <= pos < n_ctx:
                raise Mi355xError(f"generate: position {pos} outside the KV cache (n_ctx {n_ctx})")
            if not 0 <= keep < n_ctx - 1 or keep != int(keep):
                raise Mi355xError(f"generate: keep {keep} must be an integer in [0, n_ctx - 1 = {n_ctx - 1})")
            if discard is not None and (not 1 <= discard <= n_ctx - keep or discard != int(discard)):
                raise Mi355xError(f"generate: discard {discard} must be an integer in [1, n_ctx - keep = {n_ctx - keep}]")
        if n == 0:
            return []
        edits = sampler is not None and sampler.edits()
        if edits:
            ctx = self._check_context("generate", context, pos)
        g = self._generate_graph(sampler)
        if sampler is not None:
            self._seed(sampler)
        if edits:
            self._set_bias(sampler)
        L = self._stage_inputs(token, pos)
        host, out, done, epoch = g["host"], [], 0, 0
        if edits:
            self._stage_history(L, host, self.history, token, pos, ctx, sampler.repeat_last_n)
        while done < n:
            c = min(chunk, n - done, n_ctx - pos)  # (a chunk ends with the step on the last cell)
            self._run(L, g, use_graph, times=c)
            # the chunk's tokens: history[p + 1] for the step at p; the step on the last cell has
            # no history entry, its token is the input block's
            lo, hi = pos + 1, pos + c + 1
            in_hist = min(hi, n_ctx) - lo
            if in_hist > 0:
                _check(L.mi355x_backend_get_tensor(self.b.h, host[lo:].data_ptr(), self.history[lo:].data_ptr(),
                                                   4 * in_hist), "get_tensor")
            if hi > n_ctx:
                _check(L.mi355x_backend_get_tensor(self.b.h, host[n_ctx:].data_ptr(), self.inp.data_ptr(), 4),
                       "get_tensor")
            self.b.synchronize()
            for t in host[lo:hi].tolist():
                out.append(t)
                if eos is not None and t == eos:
                    return out
            done += c
            pos += c
            if done < n and pos == n_ctx:  # the cache is full (keep is set: n fits it otherwise)
                epoch += 1
                pos = self._shift_context(L, g, out[-1], keep, discard or (n_ctx - keep) // 2, use_graph)
                if sampler is not None:
                    self._seed(sampler, epoch=epoch)
                L = self._stage_inputs(out[-1], pos)
        return out

    # ------------------------------------------------------------ context shift
    def shift(self, n_past: int, keep: int, discard: int, use_graph: bool = True):
        """llama.cpp's context shift on every layer's caches (mi355x_kv_shift's DISCARD form): the
        cells [keep, keep + discard) are dropped, the cells up to n_past slide down over them and
        their K rows are re-roped by -discard, so the sequence goes on at position
        n_past - discard. One KV_SHIFT node a layer over the decoder's own caches and table,
        enqueued without synchronization; the node list is built once per (n_past, keep, discard).
        self.history, the draws and the input block are not touched."""
        if self.split is not None:
            raise Mi355xError("shift runs on one GPU (no row split)")
        if not (0 <= keep and 1 <= discard and keep + discard <= n_past <= self.n_ctx):
            raise Mi355xError(f"shift: keep {keep} >= 0, discard {discard} >= 1 and keep + discard <= n_past {n_past} <= "
                              f"n_ctx {self.n_ctx} are required")
        if keep + discard == n_past:
            return  # no cell moves
        key = (n_past, keep, discard)
        g = self._shifts.get(key)
        if g is None:
            hd, n_ctx = self.hp["head_dim"], self.n_ctx
            kvw = self.k_cache[0].shape[1]
            tab = make_tensor(TYPE_F32, hd, n_ctx, self.table.data_ptr())
            keep_alive, nodes = [tab], []
            for k, v in zip(self.k_cache, self.v_cache):
                kt = make_tensor(TYPE_F16, kvw, n_ctx, k.data_ptr())
                vt = make_tensor(TYPE_F16, n_ctx, kvw, v.data_ptr())
                nodes.append(make_tensor(TYPE_F16, kvw, n_ctx, k.data_ptr(), op=OP_KV_SHIFT, srcs=[kt, vt, tab],
                                         op_params=kv_shift_params(kvw // hd, hd, keep=keep, discard=discard,
                                                                   n_past=n_past)))
                keep_alive += [kt, vt]
            g = self._shifts[key] = dict(nodes=nodes, keep=keep_alive, arr=_node_array(nodes))
        if self.b is None:  # (describe only: no device work)
            return
        from . import lib
        self._run(lib(), g, use_graph)

    def _shift_context(self, L, g, last: int, keep: int, d: int, use_graph: bool) -> int:
        """generate's step at a full cache (the host is synchronized): shift(n_ctx, keep, d), and the
        history follows the cells: the tokens of positions [keep + d, n_ctx) move down by d and
        `last`, the token picked on the last cell, stands at the new position n_ctx - d, which is
        returned. So the penalty window goes on reading the tokens that stand before the position."""
        n_ctx = self.n_ctx
        self.shift(n_ctx, keep, d, use_graph)
        host, new = g["host"], n_ctx - d
        if new > keep:
            _check(L.mi355x_backend_get_tensor(self.b.h, host[keep:].data_ptr(), self.history[keep + d:].data_ptr(),
                                               4 * (new - keep)), "get_tensor")
            self.b.synchronize()
        host[new] = last
        _check(L.mi355x_backend_set_tensor(self.b.h, self.history[keep:].data_ptr(), host[keep:].data_ptr(),
                                           4 * (new - keep + 1)), "set_tensor")
        return new
