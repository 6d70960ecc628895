"""Generation on the HIP kernels with a resident KV cache: generate(), the greedy surface the reference's inference scripts use,
sample(), its seeded temperature / top-k / top-p twin (transformers' do_sample=True) with several draws per prompt, and beam_search()
(transformers' num_beams > 1), whose step and cache reorder run on the device inside the same captured step:
`model.text_model.generate(inputs_embeds=, attention_mask=, max_new_tokens=, do_sample=False, num_beams=1,
repetition_penalty=, no_repeat_ngram_size=, eos_token_id=, pad_token_id=)` (src/inference/qa_inference.py:207-216,
arkit_inference.py:274-284) plus the vision-token INSERTION splice those scripts perform before calling it
(qa_inference.py:119-145) - different from training's overwrite splice.

Design (MI355X): prompts are prefilled without their padding (left-padded rows are compacted, so no pad token is ever
computed and positions are 0..n-1 exactly as transformers derives them from the mask); K/V live in one
[layers, B, Hkv, Lmax, 128] bf16 buffer per operand; a decode step streams every weight once through the skinny
GEMM (up to 8 rows, FMA) or the decode GEMM (9 to 64 rows with max_rows=, MFMA: csrc/decode_gemm.hip); all step state is in device memory, so the whole step is captured once in a HIP graph and replayed per token -
the host only checks the `finished` flags every few steps. One row at Qwen3-4B's shape (the reference's case): the 36
layers of a step are ONE persistent launch (csrc/decode_layers.hip) + lm_head + pick; otherwise ~220 launches.

Sessions (transformers' `past_key_values`): a KVCache keeps K/V between calls; extend() runs only the positions it does not hold yet
against it (csrc/qwen_append.hip: a chunk of new positions over the resident cache) and generate(kv_cache=) / sample(kv_cache=)
decode on its buffers - multi-turn sessions, chunked prefill, KVCache.truncate to roll a turn back.
"""
from __future__ import annotations

import os
from typing import List, Optional, Sequence, Tuple, Union

import torch

from . import ops
from .ops import BF16, F32, round_up


def insert_vision_tokens(input_ids: torch.Tensor, attention_mask: torch.Tensor, inputs_embeds: torch.Tensor,
                         vis_tokens: torch.Tensor, image_token_id: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """qa_inference.py:119-145 / arkit_inference.py:182-214: the FIRST <image> position found (row-major) is replaced,
    in every row, by the visual span; the sequence grows by vis_len - 1 and the span is attended. No <image> -> inputs
    returned unchanged."""
    positions = (input_ids == image_token_id).nonzero(as_tuple=False)
    if positions.numel() == 0:
        return inputs_embeds, attention_mask
    pos = int(positions[0, 1])
    vis_len = vis_tokens.shape[1]
    new_inputs = torch.cat([inputs_embeds[:, :pos, :], vis_tokens.to(inputs_embeds.dtype), inputs_embeds[:, pos + 1:, :]], dim=1)
    vis_attn = torch.ones((attention_mask.size(0), vis_len), device=attention_mask.device, dtype=attention_mask.dtype)
    new_mask = torch.cat([attention_mask[:, :pos], vis_attn, attention_mask[:, pos + 1:]], dim=1)
    return new_inputs, new_mask


def _row_spans(attention_mask: torch.Tensor) -> List[Tuple[int, int]]:
    """(first attended column, count) per row; the attended columns must be one contiguous run (left and/or right
    padding) - the only masks generate() produces or the reference feeds."""
    m = (attention_mask != 0).cpu()
    spans = []
    for r in m:
        nz = r.nonzero().flatten()
        if nz.numel() == 0:
            raise ValueError("generate: a row of attention_mask attends to nothing")
        lo, hi = int(nz[0]), int(nz[-1]) + 1
        if hi - lo != nz.numel():
            raise ValueError("generate: attention_mask rows must be contiguous runs of ones (padding on the sides only)")
        spans.append((lo, hi - lo))
    return spans


KV_MAX_CAPACITY = 12288     # rows per cache row: the decode attention's limit (csrc/decode.hip)


class KVCache:
    """A session's K/V - transformers' `past_key_values`: K, V bf16 [layers, batch, Hkv, capacity, 128], zero-initialised and laid out
    as DecodeState's, so generate(kv_cache=) decodes on them in place. `capacity` is rounded up to 64. Row b holds the K/V of the first
    lengths[b] positions of its sequence; `lens` is the same count as i32 on the device. What lies behind lengths[b] (pad steps decoded
    after the row's eos, a turn rolled back) is never read and is overwritten by the next extend()."""

    def __init__(self, tm, batch: int, capacity: int):
        if batch < 1 or capacity < 1:
            raise ValueError(f"KVCache: batch and capacity must be >= 1, got {batch}, {capacity}")
        self.capacity = round_up(int(capacity), 64)
        if self.capacity > KV_MAX_CAPACITY:
            raise ValueError(f"KVCache: capacity {self.capacity} exceeds the decode attention's {KV_MAX_CAPACITY} rows")
        c, dev = tm.config, tm.flat_w.device
        self.batch = int(batch)
        self.K = torch.zeros((c.num_hidden_layers, batch, tm.Hkv, self.capacity, tm.D), device=dev, dtype=BF16)
        self.V = torch.zeros_like(self.K)
        self.lens = torch.zeros(batch, device=dev, dtype=torch.int32)
        self.lengths: List[int] = [0] * batch

    def _set_lengths(self, lengths: Sequence[int]) -> None:
        self.lengths = [int(n) for n in lengths]
        self.lens.copy_(torch.tensor(self.lengths, dtype=torch.int32))

    def truncate(self, lengths: Union[int, Sequence[int]]) -> None:
        """Roll rows back to their first lengths[b] positions (an int applies to every row). Only shrinks: host arithmetic and one
        small copy - the rows behind the new lengths stay in memory and are never read."""
        want = [int(lengths)] * self.batch if isinstance(lengths, int) else [int(n) for n in lengths]
        if len(want) != self.batch:
            raise ValueError(f"KVCache.truncate: {len(want)} lengths for {self.batch} rows")
        for b, (n, have) in enumerate(zip(want, self.lengths)):
            if n < 0 or n > have:
                raise ValueError(f"KVCache.truncate: row {b} holds {have} positions, cannot be set to {n} (truncate only shrinks)")
        self._set_lengths(want)

    def clone(self) -> "KVCache":
        other = object.__new__(KVCache)
        other.capacity, other.batch = self.capacity, self.batch
        other.K, other.V, other.lens = self.K.clone(), self.V.clone(), self.lens.clone()
        other.lengths = list(self.lengths)
        return other


def _plan_extend(spans: Sequence[Tuple[int, int]], cached: Sequence[int], capacity: int, max_new: int = 0) -> List[Tuple[int, int]]:
    """Which columns of each row extend() computes: (first new column, count) per row, for attended runs `spans` (_row_spans) whose
    first cached[b] positions are in the cache already. Host arithmetic only; raises before anything is launched: the cache's batch
    is not the number of rows, a row has nothing new, or a row (+ max_new tokens to decode after it) would pass the capacity."""
    if len(cached) != len(spans):
        raise ValueError(f"kv_cache: the cache holds {len(cached)} rows, the call has {len(spans)}")
    plan = []
    for b, ((lo, n), have) in enumerate(zip(spans, cached)):
        if n <= have:
            raise ValueError(f"kv_cache: row {b} has {n} attended positions and {have} of them cached: nothing new to compute "
                             "(pass each row's whole sequence so far; KVCache.truncate rolls a row back)")
        if n + max_new > capacity:
            raise ValueError(f"kv_cache: row {b} needs {n} + {max_new} positions, the cache's capacity is {capacity}")
        plan.append((lo + have, n - have))
    return plan


def _extend_planned(tm, cache: KVCache, embeds: torch.Tensor, plan: Sequence[Tuple[int, int]]) -> torch.Tensor:
    """Compute the planned columns of every row against the cache, append their K/V and advance the lengths. -> last hidden [B, H]."""
    B, _, H = embeds.shape
    counts = [n for _, n in plan]
    chunk = torch.zeros((B, max(counts), H), device=embeds.device, dtype=BF16)
    for b, (lo, n) in enumerate(plan):
        chunk[b, :n] = embeds[b, lo:lo + n]
    new_lens = torch.tensor(counts, dtype=torch.int32).to(embeds.device)
    h_last = tm.forward_append(chunk, cache.K, cache.V, cache.lens, new_lens, counts)
    cache.lens.add_(new_lens)
    cache.lengths = [have + n for have, n in zip(cache.lengths, counts)]
    return h_last


@torch.no_grad()
def extend(tm, cache: KVCache, inputs_embeds: Optional[torch.Tensor] = None, input_ids: Optional[torch.Tensor] = None,
           attention_mask: Optional[torch.Tensor] = None) -> torch.Tensor:
    """transformers' forward with `past_key_values`: the caller passes each row's WHOLE sequence so far (left or right padded, the
    attended run found as generate() finds it); its first cache.lengths[b] positions are taken as cached and not looked at, the rest
    is run through the model against the cache (tm.forward_append) and appended. Rows may differ in cached and new lengths; a row with
    nothing new or one that would pass the capacity raises ValueError before any launch. Returns the last hidden state, bf16 [B, H]
    (pre-final-norm: tm.logits_all turns it into logits). A prompt can go through in pieces: extend() the first part, then the whole."""
    if (inputs_embeds is None) == (input_ids is None):
        raise ValueError("pass exactly one of inputs_embeds / input_ids")
    dev = tm.flat_w.device
    shape_src = inputs_embeds if inputs_embeds is not None else input_ids
    if attention_mask is None:
        attention_mask = torch.ones(tuple(shape_src.shape[:2]), dtype=torch.int64)
    plan = _plan_extend(_row_spans(attention_mask), cache.lengths, cache.capacity)
    embeds = tm.get_input_embeddings()(input_ids.to(dev)) if input_ids is not None else inputs_embeds.to(dev, BF16)
    return _extend_planned(tm, cache, embeds, plan)


def _eos_list(eos_token_id) -> List[int]:
    return [] if eos_token_id is None else ([int(eos_token_id)] if isinstance(eos_token_id, int) else [int(e) for e in eos_token_id])


def _id_list(who: str, name: str, ids, vocab: int) -> List[int]:
    out = []
    for t in ([] if ids is None else ids):
        if isinstance(t, bool) or int(t) != t or not (0 <= int(t) < vocab):
            raise ValueError(f"{who}: {name} holds {t!r}, not an id in [0, {vocab})")
        out.append(int(t))
    return out


def _plan_constraints(who: str, vocab: int, max_new_tokens: int, eos_token_id=None, suppress_tokens=None, begin_suppress_tokens=None,
                      min_new_tokens: int = 0, allowed_token_ids=None, bad_words_ids=None) -> Optional[dict]:
    """The decoding constraints of a call as the three id sets of ops.mask_planes, host arithmetic only; raises before the GPU is
    touched. None when no keyword constrains anything (the call then runs the unmasked entries, launch for launch as without them).
      always    suppress_tokens, one-token bad_words_ids and, with allowed_token_ids, every id outside that set;
      until_min the eos ids while fewer than min_new_tokens ids are out (nothing without eos_token_id);
      at_begin  begin_suppress_tokens."""
    sup = _id_list(who, "suppress_tokens", suppress_tokens, vocab)
    for entry in ([] if bad_words_ids is None else bad_words_ids):
        entry = list(entry)
        if len(entry) != 1:
            raise NotImplementedError(f"{who}: bad_words_ids entry {entry} has {len(entry)} ids; only one-token entries are supported "
                                      "(they mean suppress_tokens)")
        sup += _id_list(who, "bad_words_ids", entry, vocab)
    begin = _id_list(who, "begin_suppress_tokens", begin_suppress_tokens, vocab)
    if min_new_tokens is None:
        min_new_tokens = 0
    if isinstance(min_new_tokens, bool) or int(min_new_tokens) != min_new_tokens or not (0 <= min_new_tokens <= max_new_tokens):
        raise ValueError(f"{who}: min_new_tokens must be an integer in 0..max_new_tokens ({max_new_tokens}), got {min_new_tokens}")
    eos = _id_list(who, "eos_token_id", _eos_list(eos_token_id), vocab) if int(min_new_tokens) > 0 else []
    always = set(sup)
    if allowed_token_ids is not None:
        allowed = set(_id_list(who, "allowed_token_ids", allowed_token_ids, vocab))
        if not (allowed - always):
            raise ValueError(f"{who}: allowed_token_ids is empty once the suppressed ids are removed: no id could ever be emitted")
        always |= set(range(vocab)) - allowed
    if not always and not begin and not eos:
        return None
    return dict(always=sorted(always), until_min=sorted(set(eos)), at_begin=sorted(set(begin)), min_new=int(min_new_tokens) if eos else 0)


class DecodeState:
    """Device-resident state of one generate() call."""

    def __init__(self, tm, B: int, Lmax: int, gen_cols: int, logprob_cols: int = 0, prompt_cols: int = 0, sampling: bool = False,
                 kv: Optional[KVCache] = None, constraints: Optional[dict] = None):
        c, dev = tm.config, tm.flat_w.device
        # decoding constraints (_plan_constraints): three bit planes over the vocabulary, built once, read by the masked picks
        self.mask = None
        if constraints is not None:
            self.mask = ops.PickMask(ops.mask_planes(tm.vocab, constraints["always"], constraints["until_min"], constraints["at_begin"]),
                                     constraints["min_new"], prompt_cols, dev)
        self.B, self.Lmax = B, Lmax
        nl = c.num_hidden_layers
        if kv is not None:      # a session's cache: decode on its own K / V and lengths (Lmax is its capacity)
            assert kv.batch == B and kv.capacity == Lmax
            self.K, self.V, self.lens = kv.K, kv.V, kv.lens
        else:
            self.K = torch.zeros((nl, B, tm.Hkv, Lmax, tm.D), device=dev, dtype=BF16)
            self.V = torch.zeros((nl, B, tm.Hkv, Lmax, tm.D), device=dev, dtype=BF16)
            self.lens = torch.zeros(B, device=dev, dtype=torch.int32)
        self.step = torch.zeros(1, device=dev, dtype=torch.int32)
        self.finished = torch.zeros(B, device=dev, dtype=torch.int32)
        self.next_ids = torch.zeros(B, device=dev, dtype=torch.int32)
        self.generated = torch.zeros((B, gen_cols), device=dev, dtype=torch.int64)
        self.work = torch.zeros(B * 128 + 8, device=dev, dtype=F32)     # pick partials + overflow flag
        # sample(): the histogram workspace of vq3_sample_pick (zero now; every pick leaves it zero again)
        self.sample_work = ops.sample_workspace(B, dev) if sampling else None
        # output_logprobs: one f32 per new token, the kernel's own record of the finished flags before each pick, its partials
        self.logprobs = None
        if logprob_cols > 0:
            self.logprobs = torch.zeros((B, logprob_cols), device=dev, dtype=F32)
            self.prompt_cols = prompt_cols
            self.lp_done = torch.zeros(B, device=dev, dtype=torch.int32)
            self.lp_work = torch.zeros(B * ops.LOGPROB_WORK_PER_ROW, device=dev, dtype=F32)
        # B = 1 at Qwen3-4B's shape: all decoder layers of a step in ONE persistent launch (csrc/decode_layers.hip) instead of six
        # launches per layer; every other case decodes with one launch per projection
        self.persistent = None
        if (B == 1 and getattr(tm, "_fp8", None) is None and not tm.lora_frozen and os.environ.get("VQ3_DECODE_PERSISTENT", "1") != "0"
                and ops.decode_layers_supported(c.hidden_size, c.intermediate_size, tm.Hq, tm.Hkv, tm.D, Lmax)):
            names = ("qkv", "o", "gu", "down", "ln1", "ln2", "qn", "kn")
            assert all(tm._w[f"l{i}.{n}"].is_contiguous() for i in range(nl) for n in names)
            self.persistent = dict(
                wtab=torch.tensor([[tm._w[f"l{i}.{n}"].data_ptr() for n in names] for i in range(nl)], dtype=torch.int64, device=dev),
                h=torch.empty((1, c.hidden_size), device=dev, dtype=BF16), workspace=ops.decode_layers_workspace(dev),
                barrier=torch.zeros(1024, device=dev, dtype=torch.int32),
                status=torch.zeros(1, device=dev, dtype=torch.int32))


def _prefill(tm, st: DecodeState, embeds: torch.Tensor, spans: Sequence[Tuple[int, int]], n_draws: int = 1) -> torch.Tensor:
    """Run the prompt through the training-path forward (batched MFMA GEMMs) and keep K/V. Rows of equal length go in
    one pass; otherwise row by row, each without its padding. Prompt row b fills the n_draws cache rows b * n_draws ..: its K/V rows
    and last hidden state are copied, the prompt is computed once. Returns the last prompt position's hidden state [B * n_draws, H]."""
    B, H = embeds.shape[0], embeds.shape[2]
    groups = {}
    for b, (lo, n) in enumerate(spans):
        groups.setdefault(n, []).append(b)
    h_last = torch.empty((B * n_draws, H), device=embeds.device, dtype=BF16)
    rep = (lambda t: t) if n_draws == 1 else (lambda t: t.repeat_interleave(n_draws, dim=0))
    for n, rows in groups.items():
        x = torch.stack([embeds[b, spans[b][0]:spans[b][0] + n] for b in rows], dim=0).contiguous()
        mask = torch.ones((len(rows), n), device=embeds.device, dtype=torch.int64)
        h, saved = tm.forward_hidden(x, mask, save=True)
        Lp = saved["L"]
        idx = torch.tensor([b * n_draws + j for b in rows for j in range(n_draws)], device=embeds.device)
        for i, ctx in enumerate(saved["layers"]):
            st.K[i, idx, :, :n] = rep(ctx["K"][:, :, :n])
            st.V[i, idx, :, :n] = rep(ctx["V"][:, :, :n])
        h_last[idx] = rep(h.view(len(rows), Lp, H)[:, n - 1])
        del saved
    st.lens.copy_(torch.tensor([n for _, n in spans for _ in range(n_draws)], dtype=torch.int32))
    return h_last


def _logits_and_pick(tm, st: DecodeState, h: torch.Tensor, opts) -> None:
    c = tm.config
    logits = ops.decode_linear(h, tm._w["embed"], n=tm.vocab, ln_w=tm._w["norm"], eps=c.rms_norm_eps)
    sm, bm = opts.get("sample"), opts.get("beam")
    if bm is not None:              # beam search: the beam step in the pick's place, then the cache rows follow the surviving beams
        bs = bm["state"]
        ops.beam_step(logits, tm.vocab, bs, st.step, st.next_ids, opts["penalty"], opts["ngram"], bm["eos"], bm["length_penalty"],
                      bm["early_stopping"])
        ops.beam_reorder(st.K, st.V, bs.src_row, st.lens, bs.n_prompts, bs.num_beams, bs.all_done)
        return
    if sm is None and st.mask is None:
        ops.greedy_pick(logits, st.work, st.generated, st.step, st.finished, opts["penalty"], opts["ngram"], opts["eos"],
                        opts["pad"], st.next_ids, tm.vocab)
    elif sm is None:
        ops.greedy_pick_masked(logits, st.work, st.generated, st.step, st.finished, opts["penalty"], opts["ngram"], opts["eos"],
                               opts["pad"], st.next_ids, tm.vocab, st.mask)
    else:
        ops.sample_pick(logits, st.work, st.generated, st.step, st.finished, opts["penalty"], opts["ngram"], opts["eos"],
                        opts["pad"], st.next_ids, tm.vocab, sm["temperature"], sm["top_k"], sm["top_p"], sm["seed"], st.sample_work,
                        mask=st.mask)
    if st.logprobs is not None:     # the raw logits' log-probability of the id just picked, into column step - prompt_cols
        ops.token_logprob_step(logits, tm.vocab, st.next_ids, st.step, st.prompt_cols, st.finished, st.lp_done, st.logprobs, st.lp_work)


def _decode_step(tm, st: DecodeState, cos, sin, opts) -> None:
    """One token for every row. Fixed launch sequence, every varying quantity read from device memory."""
    c = tm.config
    B, Hq, Hkv, D = st.B, tm.Hq, tm.Hkv, tm.D
    ps = st.persistent
    if ps is not None:
        h = ops.gather_rows(tm._w["embed"], st.next_ids, B, B, out=ps["h"])
        ops.decode_layers(ps["wtab"], h, ps["workspace"], cos, sin, st.lens, st.K, st.V, ps["barrier"], ps["status"], c.hidden_size,
                          c.intermediate_size, tm.Hq, tm.Hkv, c.rms_norm_eps, D ** -0.5)
        _logits_and_pick(tm, st, h, opts)
        ops.decode_advance(st.lens, B, st.step)
        return
    h = ops.gather_rows(tm._w["embed"], st.next_ids, B, B)
    f8 = tm._fp8 if (tm._fp8 is not None and B <= 2) else None     # e4m3 weight stream (config C5): half the bytes per token

    def proj(x, name, **kw):
        if f8 is not None:
            wq, ws = f8[name]
            return ops.skinny_linear_fp8(x, wq, ws, **kw)
        return ops.decode_linear(x, tm._w[name], **kw)       # <= 8 rows: the FMA skinny GEMM; 9..64: the MFMA decode GEMM

    lo = tm.lora if tm.lora_frozen else None                        # unmerged LoRA adapters: their terms after q|k|v and o
    for i in range(c.num_hidden_layers):
        qkv = proj(h, f"l{i}.qkv", ln_w=tm._w[f"l{i}.ln1"], eps=c.rms_norm_eps)
        if lo is not None and lo.attn:
            lo.fwd_qkv(i, ops.rmsnorm_fwd(h, tm._w[f"l{i}.ln1"], c.rms_norm_eps), qkv, training=False)
        Q = ops.qwen_decode_qkprep(qkv, tm._w[f"l{i}.qn"], tm._w[f"l{i}.kn"], cos, sin, st.lens, st.K[i], st.V[i], B, Hq, Hkv,
                                   D, st.Lmax, c.rms_norm_eps)
        ao = ops.qwen_decode_attn(Q, st.K[i], st.V[i], st.lens, B, Hq, Hkv, D, st.Lmax, D ** -0.5)
        h_mid = proj(ao, f"l{i}.o", residual=h)
        if lo is not None:
            lo.fwd_o(i, ao, h_mid, training=False)
        gu = proj(h_mid, f"l{i}.gu", ln_w=tm._w[f"l{i}.ln2"], eps=c.rms_norm_eps)
        h = proj(gu, f"l{i}.down", residual=h_mid, swiglu=True)
    _logits_and_pick(tm, st, h, opts)
    ops.decode_advance(st.lens, B, st.step)         # the processed token is now cached; one more id has been picked


@torch.no_grad()
def generate(tm, inputs_embeds: Optional[torch.Tensor] = None, attention_mask: Optional[torch.Tensor] = None,
             input_ids: Optional[torch.Tensor] = None, max_new_tokens: int = 20, do_sample: bool = False,
             num_beams: int = 1, repetition_penalty: float = 1.0, no_repeat_ngram_size: int = 0,
             eos_token_id: Union[int, Sequence[int], None] = None, pad_token_id: Optional[int] = None,
             use_graph: Optional[bool] = None, check_every: int = 8, return_stats: bool = False,
             output_logprobs: bool = False, kv_cache: Optional[KVCache] = None, max_rows: int = 8,
             suppress_tokens: Optional[Sequence[int]] = None, begin_suppress_tokens: Optional[Sequence[int]] = None,
             min_new_tokens: int = 0, allowed_token_ids: Optional[Sequence[int]] = None,
             bad_words_ids: Optional[Sequence[Sequence[int]]] = None, **unused):
    """transformers `generate` for the greedy case. With `inputs_embeds` only the NEW tokens are returned (as
    transformers does); with `input_ids` the prompt is prepended and, like transformers, takes part in the repetition
    penalty and n-gram ban. Finished rows emit pad_token_id; generation stops when every row has produced eos or after
    max_new_tokens.
    output_logprobs=True returns (ids, logprobs[, stats]): logprobs f32 [B, n_new], one entry per NEW token (no entry for prompt
    columns), trimmed at the same stop column as the ids. An entry is the log-probability of the emitted id under the model's own
    distribution - log_softmax of the RAW logits, before the repetition penalty and the n-gram ban (transformers'
    compute_transition_scores on `output_logits`) - so with either processor on, an emitted id need not be the raw argmax. The step
    that emits a row's eos carries that token's log-probability; every later (pad) step of the row is exactly 0.0.
    kv_cache=KVCache (transformers' `past_key_values`): pass each row's whole sequence so far; only what the cache does not hold yet is
    computed (extend()), decoding runs on the cache's own K/V (Lmax = its capacity) and on return cache.lengths[b] counts the leading
    positions of "attended prompt + emitted ids up to and including the first eos" whose K/V are cached: prompt_b + min(steps_run - 1,
    index of the row's first eos + 1). The id picked last has no K/V yet - the next turn's extend() computes it with the new tokens.
    A row longer than capacity - max_new_tokens raises ValueError before anything is launched.
    max_rows: the caller's cap on the rows decoded per call, 1..64 (ops.DECODE_MAX_ROWS); more rows than that raise ValueError before
    the GPU is touched. Up to 8 rows a step runs the FMA skinny GEMMs whatever max_rows says; 9..64 rows (bf16 weights, frozen LoRA
    adapters included) run one MFMA weight-streaming GEMM per projection, so a step still streams every weight once. With kv_cache
    the cache's batch is the row count.
    Decoding constraints, applied on the device inside the captured step (the masked picks of csrc; a masked id scores -inf exactly as
    an n-gram-banned one - never picked, and id 0 if a whole row is -inf); they combine with each other and with every keyword above:
      suppress_tokens        ids that are never emitted (SuppressTokensLogitsProcessor);
      begin_suppress_tokens  ids that are not emitted as the first new token (SuppressTokensAtBeginLogitsProcessor);
      min_new_tokens         no eos id before that many new tokens (MinNewTokensLengthLogitsProcessor); nothing without eos_token_id;
      allowed_token_ids      only these ids are emitted - transformers' prefix_allowed_tokens_fn=lambda b, ids: allowed; put the eos ids
                             in if rows are to stop; a finished row still emits pad_token_id (pad does not go through the logits);
      bad_words_ids          one-token entries only, meaning suppress_tokens; a longer entry raises NotImplementedError.
    An id outside [0, vocab), min_new_tokens outside 0..max_new_tokens or an allowed set that the suppressed ids empty raise ValueError
    before the GPU is touched. output_logprobs stays the log-probability under the RAW logits. Without any of these keywords the call
    allocates and launches exactly what it did before they existed."""
    shape_src = inputs_embeds if inputs_embeds is not None else input_ids
    _check_rows("generate", max_rows, 0 if shape_src is None else int(shape_src.shape[0]))
    constraints = dict(suppress_tokens=suppress_tokens, begin_suppress_tokens=begin_suppress_tokens, min_new_tokens=min_new_tokens,
                       allowed_token_ids=allowed_token_ids, bad_words_ids=bad_words_ids)
    if do_sample or num_beams != 1:
        raise NotImplementedError("generate() is greedy decoding (do_sample=False, num_beams=1) - what the reference's callers use; "
                                  "sample() draws with temperature / top-k / top-p; beam_search() searches with num_beams beams")
    return _run(tm, inputs_embeds, attention_mask, input_ids, max_new_tokens, repetition_penalty, no_repeat_ngram_size, eos_token_id,
                pad_token_id, use_graph, check_every, return_stats, output_logprobs, None, 1, kv_cache, constraints)


def _check_rows(who: str, max_rows, n_prompts: int, n_draws: int = 1) -> None:
    """max_rows itself, then the output rows (prompts x draws) against it; host arithmetic only."""
    if isinstance(max_rows, bool) or int(max_rows) != max_rows or not (1 <= max_rows <= ops.DECODE_MAX_ROWS):
        raise ValueError(f"{who}: max_rows must be an integer in 1..{ops.DECODE_MAX_ROWS}, got {max_rows}")
    if n_prompts * n_draws > max_rows:
        raise ValueError(f"{who}: at most {max_rows} rows per call (max_rows=, up to {ops.DECODE_MAX_ROWS}), got {n_prompts} prompts x "
                         f"{n_draws} draws")


def _check_sample_args(temperature, top_k, top_p, num_return_sequences, n_prompts, max_rows=8) -> None:
    """sample()'s own arguments; host arithmetic only."""
    if not (temperature > 0 and temperature < float("inf")):
        raise ValueError(f"sample: temperature must be > 0 and finite, got {temperature}")
    if int(top_k) != top_k or top_k < 0:
        raise ValueError(f"sample: top_k must be an integer >= 0 (0 turns it off), got {top_k}")
    if not (0 < top_p <= 1):
        raise ValueError(f"sample: top_p must be in (0, 1], got {top_p}")
    if int(num_return_sequences) != num_return_sequences or num_return_sequences < 1:
        raise ValueError(f"sample: num_return_sequences must be an integer >= 1, got {num_return_sequences}")
    _check_rows("sample", max_rows, n_prompts, int(num_return_sequences))


@torch.no_grad()
def sample(tm, inputs_embeds: Optional[torch.Tensor] = None, attention_mask: Optional[torch.Tensor] = None,
           input_ids: Optional[torch.Tensor] = None, max_new_tokens: int = 20, repetition_penalty: float = 1.0,
           no_repeat_ngram_size: int = 0, eos_token_id: Union[int, Sequence[int], None] = None, pad_token_id: Optional[int] = None,
           use_graph: Optional[bool] = None, check_every: int = 8, return_stats: bool = False, output_logprobs: bool = False,
           temperature: float = 1.0, top_k: int = 50, top_p: float = 1.0, num_return_sequences: int = 1, seed: Optional[int] = None,
           kv_cache: Optional[KVCache] = None, max_rows: int = 8, suppress_tokens: Optional[Sequence[int]] = None,
           begin_suppress_tokens: Optional[Sequence[int]] = None, min_new_tokens: int = 0,
           allowed_token_ids: Optional[Sequence[int]] = None, bad_words_ids: Optional[Sequence[Sequence[int]]] = None, **unused):
    """transformers `generate(do_sample=True)`: every keyword of generate() above with the same meaning (same processors, same
    eos / pad handling, same return values, output_logprobs included), the pick drawn instead of maximised (vq3_sample_pick, inside
    the captured step like the greedy pick). After the repetition penalty and the n-gram ban, with s = logit / temperature:
      top_k   keeps an id iff fewer than top_k ids score higher (ties at the k-th score all stay; 0 = off; 50 is transformers' default);
      top_p   then keeps an id iff the softmax mass, over the top-k set, of the ids that score higher is < top_p (ids of equal score
              stand or fall together, the best id always stays; without ties this is TopPLogitsWarper);
      draw    Gumbel-max over what is left, noise from Philox4x32-10 keyed by `seed`, counted by (id, step, output row).
    The noise has 24 bits: g = -log(-log(u)) lies in about [-2.9, 17.3], so an id more than ~e^-20 below the best score is never drawn.
    A draw depends on (logits, ids so far, seed, step, row) only: the same seed gives the same ids on every run, with or without the
    HIP graph, on either step route. seed=None takes a 64-bit seed from torch's default CPU generator (torch.manual_seed governs it);
    return_stats reports the seed used.
    num_return_sequences = n draws n continuations of every prompt row: output row b * n + j is draw j of prompt b (transformers'
    order), B * n <= max_rows (8 unless the caller raises it, up to 64: see generate()). Each prompt is prefilled once; its K/V rows and
    last hidden state are copied to its n cache rows.
    output_logprobs=True: an entry is log_softmax of the RAW logits at the sampled id (compute_transition_scores on `output_logits`),
    not the probability the id was drawn with after the warpers.
    kv_cache: as in generate(); with a cache num_return_sequences must be 1 (the cache rows would have to be fanned out).
    suppress_tokens / begin_suppress_tokens / min_new_tokens / allowed_token_ids / bad_words_ids: as in generate(); here a masked id is
    never kept and never drawn, and carries no mass in the top-k / top-p cuts."""
    shape_src = inputs_embeds if inputs_embeds is not None else input_ids
    _check_sample_args(temperature, top_k, top_p, num_return_sequences, 0 if shape_src is None else int(shape_src.shape[0]), max_rows)
    constraints = dict(suppress_tokens=suppress_tokens, begin_suppress_tokens=begin_suppress_tokens, min_new_tokens=min_new_tokens,
                       allowed_token_ids=allowed_token_ids, bad_words_ids=bad_words_ids)
    if seed is None:
        seed = int(torch.randint(-(1 << 63), (1 << 63) - 1, (1,), dtype=torch.int64).item())
    sampling = dict(temperature=float(temperature), top_k=int(top_k), top_p=float(top_p), seed=int(seed) & 0xFFFFFFFFFFFFFFFF)
    return _run(tm, inputs_embeds, attention_mask, input_ids, max_new_tokens, repetition_penalty, no_repeat_ngram_size, eos_token_id,
                pad_token_id, use_graph, check_every, return_stats, output_logprobs, sampling, int(num_return_sequences), kv_cache,
                constraints)


def _run(tm, inputs_embeds, attention_mask, input_ids, max_new_tokens, repetition_penalty, no_repeat_ngram_size, eos_token_id,
         pad_token_id, use_graph, check_every, return_stats, output_logprobs, sampling, n_draws, kv_cache=None, constraints=None):
    """The body of generate() (sampling None, n_draws 1) and sample(): prefill, one eager pick, then the decode steps. constraints:
    the five constraint keywords as given (planned here, on the host, before anything touches the GPU)."""
    if kv_cache is not None and n_draws != 1:
        raise ValueError("kv_cache: num_return_sequences must be 1 (fanning a cache row out to several draws is not implemented)")
    if (inputs_embeds is None) == (input_ids is None):
        raise ValueError("pass exactly one of inputs_embeds / input_ids")
    if max_new_tokens < 1:
        raise ValueError("max_new_tokens must be >= 1")
    if constraints is not None:
        constraints = _plan_constraints("sample" if sampling is not None else "generate", tm.vocab, max_new_tokens, eos_token_id,
                                        **constraints)
    dev = tm.flat_w.device
    if input_ids is not None:
        input_ids = input_ids.to(dev)
        embeds = tm.get_input_embeddings()(input_ids)
    else:
        embeds = inputs_embeds.to(dev, BF16)
    B, L0, H = embeds.shape                     # (generate() / sample() have checked the rows against max_rows)
    if attention_mask is None:
        attention_mask = torch.ones((B, L0), device=dev, dtype=torch.int64)
    spans = _row_spans(attention_mask)
    plan = None if kv_cache is None else _plan_extend(spans, kv_cache.lengths, kv_cache.capacity, max_new_tokens)
    B *= n_draws                                # output rows: n_draws per prompt row, prompt-major
    eos = None
    if eos_token_id is not None:
        eos_list = [eos_token_id] if isinstance(eos_token_id, int) else list(eos_token_id)
        eos = torch.tensor(eos_list, device=dev, dtype=torch.int64)
        if pad_token_id is None:
            pad_token_id = eos_list[0]          # transformers' fallback (with a warning)
    opts = dict(penalty=float(repetition_penalty), ngram=int(no_repeat_ngram_size), eos=eos,
                pad=0 if pad_token_id is None else int(pad_token_id), sample=sampling)
    n_prompt = L0 if input_ids is not None else 0
    Lmax = round_up(max(n for _, n in spans) + max_new_tokens, 64) if kv_cache is None else kv_cache.capacity
    st = DecodeState(tm, B, Lmax, n_prompt + max_new_tokens, logprob_cols=max_new_tokens if output_logprobs else 0, prompt_cols=n_prompt,
                     sampling=sampling is not None, kv=kv_cache, constraints=constraints)
    if input_ids is not None:
        st.generated[:, :L0] = input_ids.repeat_interleave(n_draws, dim=0)
        st.step.fill_(L0)
    cos, sin = tm.rope(Lmax)
    if kv_cache is None:
        h_last = _prefill(tm, st, embeds, spans, n_draws)
    else:                                       # only what the cache does not hold; st.K / st.V / st.lens are the cache's own
        h_last = _extend_planned(tm, kv_cache, embeds, plan)
    _logits_and_pick(tm, st, h_last, opts)
    ops.decode_advance(None, B, st.step)
    if use_graph is None:
        use_graph = os.environ.get("VQ3_DECODE_GRAPH", "1") != "0"
    graph = None
    done_steps = 1
    if max_new_tokens > 1 and use_graph:
        # warm the allocator, then capture one step; replay mutates the same state tensors
        side = torch.cuda.Stream(device=dev)
        mutated = snap = None
        if st.persistent is not None:            # what the step mutates, should it have to be redone on the other route (see below)
            mutated = [st.lens, st.step, st.finished, st.next_ids, st.generated] + ([st.lp_done] if st.logprobs is not None else [])
            snap = [t.clone() for t in mutated]
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            _decode_step(tm, st, cos, sin, opts)
        torch.cuda.current_stream().wait_stream(side)
        done_steps += 1
        if st.persistent is not None and int(st.persistent["status"].item()) & 1:
            # The persistent kernel needs its 256 workgroups co-resident; a bounded barrier wait ran out (other tenants / streams hold CUs,
            # a CU mask): its step's hidden row and the cache rows it appended are garbage. Nothing is lost: the state is put back, the
            # K / V rows at position lens (the only ones the step wrote) are rewritten by the redo, and this call decodes with one launch
            # per projection from here on.
            import warnings
            warnings.warn("vq3: the persistent decode kernel's workgroups were not co-resident (a grid-barrier wait ran out); this "
                          "generate() call continues with one launch per projection (VQ3_DECODE_PERSISTENT=0 selects that route up front)")
            st.persistent = None
            for dst, src in zip(mutated, snap):
                dst.copy_(src)
            _decode_step(tm, st, cos, sin, opts)
        elif st.persistent is not None:
            ops.decode_layers_status(st.persistent["status"])   # (cache full)
        if max_new_tokens > 2:
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                _decode_step(tm, st, cos, sin, opts)
    while done_steps < max_new_tokens:
        if eos is not None and (done_steps % check_every == 0 or graph is None) and bool(st.finished.all()):
            break
        if graph is not None:
            graph.replay()
            if st.persistent is not None and done_steps % check_every == 0:
                ops.decode_layers_status(st.persistent["status"])       # a failure mid-way surfaces within check_every tokens, not after all of them
        else:
            _decode_step(tm, st, cos, sin, opts)
            if st.persistent is not None and done_steps % check_every == 0:
                ops.decode_layers_status(st.persistent["status"])
        done_steps += 1
    if st.persistent is not None:
        ops.decode_layers_status(st.persistent["status"])
    gen = st.generated[:, : n_prompt + done_steps].cpu()
    # transformers stops right after the step in which the last row finished: trim what ran past it
    stop = done_steps
    if eos is not None:
        new = gen[:, n_prompt:]
        hit = torch.zeros_like(new, dtype=torch.bool)
        for e in eos.tolist():
            hit |= new == e
        first = torch.where(hit.any(1), hit.float().argmax(1), torch.full((B,), 1 << 30))
        if int(first.max()) < (1 << 30):
            stop = min(done_steps, int(first.max()) + 1)
    if kv_cache is not None:
        # every decode step cached the id picked before it: done_steps - 1 of them, valid up to and including the row's first eos
        # (the pad steps of a finished row lie behind that and are overwritten by the next extend)
        new = gen[:, n_prompt:]
        kept = [done_steps - 1] * B
        if eos is not None:
            hit = torch.zeros_like(new, dtype=torch.bool)
            for e in eos.tolist():
                hit |= new == e
            kept = [min(done_steps - 1, int(hit[b].float().argmax()) + 1) if bool(hit[b].any()) else done_steps - 1 for b in range(B)]
        kv_cache._set_lengths([n + k for (_, n), k in zip(spans, kept)])
    out = gen[:, : n_prompt + stop].to(dev)
    ret = (out,) if st.logprobs is None else (out, st.logprobs[:, :stop].clone())
    if return_stats:
        stats = {"steps_run": done_steps, "graph": graph is not None, "Lmax": Lmax, "persistent": st.persistent is not None,
                 "prefilled": [n for _, n in (spans if plan is None else plan)]}
        if sampling is not None:
            stats["seed"] = sampling["seed"]
        ret += (stats,)
    return ret[0] if len(ret) == 1 else ret


def _check_beam_args(num_beams, num_return_sequences, length_penalty, early_stopping, eos_token_id, n_prompts) -> List[int]:
    """beam_search()'s own arguments; host arithmetic only. Returns the eos ids as a list."""
    if isinstance(num_beams, bool) or int(num_beams) != num_beams or not (2 <= num_beams <= ops.BEAM_MAX_ROWS):
        raise ValueError(f"beam_search: num_beams must be an integer in 2..{ops.BEAM_MAX_ROWS}, got {num_beams}")
    if n_prompts * num_beams > ops.BEAM_MAX_ROWS:
        raise ValueError(f"beam_search: at most {ops.BEAM_MAX_ROWS} rows per call (skinny GEMM width), got {n_prompts} prompts x {num_beams} beams")
    if int(num_return_sequences) != num_return_sequences or not (1 <= num_return_sequences <= num_beams):
        raise ValueError(f"beam_search: num_return_sequences must be an integer in 1..num_beams, got {num_return_sequences}")
    eos = [] if eos_token_id is None else ([int(eos_token_id)] if isinstance(eos_token_id, int) else [int(e) for e in eos_token_id])
    if len(eos) > ops.BEAM_MAX_EOS:
        raise ValueError(f"beam_search: at most {ops.BEAM_MAX_EOS} eos ids (32 candidates per prompt), got {len(eos)}")
    if not any(early_stopping is v for v in (False, True)) and early_stopping != "never":
        raise ValueError(f"beam_search: early_stopping must be False, True or 'never', got {early_stopping!r}")
    if not (float("-inf") < length_penalty < float("inf")):
        raise ValueError(f"beam_search: length_penalty must be finite, got {length_penalty}")
    return eos


@torch.no_grad()
def beam_search(tm, inputs_embeds: Optional[torch.Tensor] = None, attention_mask: Optional[torch.Tensor] = None,
                input_ids: Optional[torch.Tensor] = None, max_new_tokens: int = 20, num_beams: int = 4, num_return_sequences: int = 1,
                length_penalty: float = 1.0, early_stopping: Union[bool, str] = False, repetition_penalty: float = 1.0,
                no_repeat_ngram_size: int = 0, eos_token_id: Union[int, Sequence[int], None] = None, pad_token_id: Optional[int] = None,
                use_graph: Optional[bool] = None, check_every: int = 8, return_scores: bool = False, return_stats: bool = False):
    """transformers `generate(num_beams=n, do_sample=False)` - GenerationMixin._beam_search of transformers 5.15, step for step: per
    prompt n running beams, n finished slots and K = max(2, 1 + number of eos ids) * n candidates per step; the processors act on the
    LOG-PROBABILITIES (log_softmax first, then repetition penalty and n-gram ban - unlike generate() / sample(), which apply them to the
    raw logits); a hypothesis' score is its summed log-probability / length ** length_penalty; early_stopping False / True / "never"
    as there. The beam step (vq3_beam_step) and the move of the K/V cache rows to the surviving beams (vq3_beam_reorder) run inside the
    captured decode step; the host reads one `all_done` word every check_every steps. Each prompt is prefilled once and fanned out to
    its n cache rows; B * n <= 8. Exact ties are ordered by the device's rule (higher score, then smaller beam * V + id, then smaller
    candidate rank) where torch.topk's order is unspecified.
    Returns `sequences` i64 [B * num_return_sequences, n_prompt + longest]: prompt-major, best first, cropped to the longest returned
    hypothesis, pad_token_id (else the first eos id) past a shorter one's end; with inputs_embeds the new ids only. return_scores adds
    `sequences_scores` f32; return_stats adds a dict with steps_run, graph, Lmax and the search trace the device recorded: parents /
    tokens i32 and running_scores f32 [steps_run, B * n] - the parent row, last id and score of every running beam after each step -
    and `finished`, the n finished slots of every prompt as the device holds them (sequences i32 [B * n, n_prompt + max_new_tokens],
    lengths, scores, flags).
    The decoding constraints of generate() / sample() (suppress_tokens, ...) are not offered here: passing one is a TypeError."""
    shape_src = inputs_embeds if inputs_embeds is not None else input_ids
    eos_list = _check_beam_args(num_beams, num_return_sequences, length_penalty, early_stopping, eos_token_id,
                                0 if shape_src is None else int(shape_src.shape[0]))
    if (inputs_embeds is None) == (input_ids is None):
        raise ValueError("beam_search: pass exactly one of inputs_embeds / input_ids")
    if max_new_tokens < 1:
        raise ValueError("beam_search: max_new_tokens must be >= 1")
    nb, nret = int(num_beams), int(num_return_sequences)
    dev = tm.flat_w.device
    if input_ids is not None:
        input_ids = input_ids.to(dev)
        embeds = tm.get_input_embeddings()(input_ids)
    else:
        embeds = inputs_embeds.to(dev, BF16)
    Bp, L0, _ = embeds.shape
    if attention_mask is None:
        attention_mask = torch.ones((Bp, L0), device=dev, dtype=torch.int64)
    spans = _row_spans(attention_mask)
    R = Bp * nb
    if pad_token_id is None:
        pad_token_id = eos_list[0] if eos_list else 0       # without an eos every hypothesis has full length: nothing is filled
    n_prompt = L0 if input_ids is not None else 0
    max_len = n_prompt + max_new_tokens
    Lmax = round_up(max(n for _, n in spans) + max_new_tokens, 64)
    st = DecodeState(tm, R, Lmax, 1)
    bs = ops.BeamState(Bp, nb, max_len, n_prompt, max_new_tokens, dev)
    opts = dict(penalty=float(repetition_penalty), ngram=int(no_repeat_ngram_size), sample=None,
                beam=dict(state=bs, eos=eos_list, length_penalty=float(length_penalty), early_stopping=early_stopping))
    if input_ids is not None:
        bs.run_seq[:, :L0] = input_ids.repeat_interleave(nb, dim=0).to(torch.int32)
        st.step.fill_(L0)
    cos, sin = tm.rope(Lmax)
    h_last = _prefill(tm, st, embeds, spans, nb)
    _logits_and_pick(tm, st, h_last, opts)
    ops.decode_advance(None, R, st.step)
    if use_graph is None:
        use_graph = os.environ.get("VQ3_DECODE_GRAPH", "1") != "0"
    graph = None
    done_steps = 1
    if max_new_tokens > 1 and use_graph:
        side = torch.cuda.Stream(device=dev)                # warm the allocator, then capture one step; replay mutates the same state
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            _decode_step(tm, st, cos, sin, opts)
        torch.cuda.current_stream().wait_stream(side)
        done_steps += 1
        if max_new_tokens > 2:
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                _decode_step(tm, st, cos, sin, opts)
    while done_steps < max_new_tokens:
        # a search ends before max_new_tokens only through finished hypotheses, and those need an eos
        if eos_list and (done_steps % check_every == 0 or graph is None) and bool(bs.all_done.item()):
            break
        if graph is not None:
            graph.replay()
        else:
            _decode_step(tm, st, cos, sin, opts)
        done_steps += 1
    # the finished slots are kept best first: the first num_return_sequences of every prompt, cropped to the longest of them
    steps_run = int((bs.trace_parent[:, 0] >= 0).sum())     # steps launched after all_done wrote nothing
    fin_len = bs.fin_len.view(Bp, nb)[:, :nret].reshape(-1)
    longest = int(fin_len.max())
    out = bs.fin_seq.view(Bp, nb, max_len)[:, :nret].reshape(Bp * nret, max_len)[:, :longest].to(torch.int64)
    out = torch.where(torch.arange(longest, device=dev)[None, :] < fin_len[:, None], out, torch.full_like(out, int(pad_token_id)))
    ret = (out[:, n_prompt:] if input_ids is None else out,)
    if return_scores:
        ret += (bs.fin_score.view(Bp, nb)[:, :nret].reshape(-1).clone(),)
    if return_stats:
        ret += ({"steps_run": steps_run, "graph": graph is not None, "Lmax": Lmax, "parents": bs.trace_parent[:steps_run].clone(),
                 "tokens": bs.trace_token[:steps_run].clone(), "running_scores": bs.trace_score[:steps_run].clone(),
                 "finished": {"sequences": bs.fin_seq.clone(), "lengths": bs.fin_len.clone(), "scores": bs.fin_score.clone(),
                              "flags": bs.fin_flag.clone()}},)
    return ret[0] if len(ret) == 1 else ret
