"""Writes tests/golden/constrain_tiny.npz: transformers' own generate() under suppress_tokens, begin_suppress_tokens, min_new_tokens,
prefix_allowed_tokens_fn (a fixed allowed set) and one-token bad_words_ids on the tiny Qwen3 of qwen3_tiny.npz (same weights), greedy
and beam search, with the raw logits (output_logits) and the processed scores (output_scores) of every step. tests/test_constrain_host.py
replays tests/constrain_ref.py on the raw logits and must reproduce the -inf pattern of the processed scores and the sequences;
tests/test_constrain_gpu.py compares generate() / beam_search() with the sequences. Run in the build container only (CPU).

For every keyword one greedy case is "strong": at every step of every row the two best processed scores are at least 4 x TIE_TOL apart
(TIE_TOL of tests/test_generate_gpu.py), so bf16 noise cannot flip a pick and the GPU test demands the case in full. The prompts are
searched for by seed until that holds; the assertion below fails the recording otherwise."""
import json
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from tests.golden_io import load, weights  # noqa: E402
from tools.make_golden import bf16_bits, tiny_qwen_cfg  # noqa: E402

TIE_TOL = 0.08                     # tests/test_generate_gpu.py
STRONG = 4 * TIE_TOL
V = 320
NGRAM = 2                          # the model repeats its last token: a small n-gram ban keeps the cases from being one id ten times


def main():
    import transformers
    from transformers import Qwen3ForCausalLM
    z = load("qwen3_tiny.npz")
    cfg = tiny_qwen_cfg(V)
    model = Qwen3ForCausalLM(cfg).to(torch.bfloat16).eval()
    sd = weights(z)
    sd["lm_head.weight"] = sd["model.embed_tokens.weight"]
    model.load_state_dict(sd)
    model.generation_config.pad_token_id = None
    H = cfg.hidden_size
    arrays, cases = {}, []

    def gen(src, **kw):
        kw = dict(kw)
        allowed = kw.pop("allowed_token_ids", None)
        if allowed is not None:
            kw["prefix_allowed_tokens_fn"] = lambda b, ids: allowed
        with torch.no_grad():
            return model.generate(**src, do_sample=False, return_dict_in_generate=True, output_scores=True, output_logits=True, **kw)

    def margin(out, src, kw):
        """The smallest top-2 gap of the processed scores over all steps and rows; a greedy row counts up to the step that emits its eos
        (after it the row emits pad whatever the scores say)."""
        n_prompt = src["input_ids"].shape[1] if "input_ids" in src else 0
        new = out.sequences[:, n_prompt:]
        eos = kw.get("eos_token_id")
        eos = [] if eos is None else ([eos] if isinstance(eos, int) else list(eos))
        m = float("inf")
        for t, s in enumerate(out.scores):
            top = torch.topk(s.float(), 2, dim=-1).values
            gap = top[:, 0] - top[:, 1]
            for b in range(gap.shape[0]):
                live = "num_beams" in kw or not any(int(x) in eos for x in new[b, :t])
                if live:
                    m = min(m, float(gap[b]))
        return m

    def record(name, src, out, kw, strong):
        for k, v in src.items():
            arrays[f"{name}:{k}"] = bf16_bits(v) if v.dtype == torch.bfloat16 else v.numpy()
        arrays[f"{name}:logits"] = torch.stack(out.logits, 0).float().numpy()
        arrays[f"{name}:scores"] = torch.stack(out.scores, 0).float().numpy()
        arrays[f"{name}:out"] = out.sequences.numpy()
        if "num_beams" in kw:
            arrays[f"{name}:sequences_scores"] = out.sequences_scores.numpy()
        cases.append({"name": name, "input": "input_ids" if "input_ids" in src else "inputs_embeds", "kw": kw, "strong": bool(strong),
                      "margin": margin(out, src, kw)})
        print(name, "strong" if strong else "", f"margin {margin(out, src, kw):.3f}", out.sequences.tolist())

    def embeds_src(seed, rows=2):
        g = torch.Generator().manual_seed(seed)
        emb = (torch.randn(rows, 11, H, generator=g) * 0.5).to(torch.bfloat16)
        mask = torch.ones(rows, 11, dtype=torch.long)
        if rows > 1:
            mask[1, :4] = 0
        return dict(inputs_embeds=emb, attention_mask=mask)

    def keywords_for(which, free, base):
        """The keyword arguments of one greedy case, built from the ids the run without the keyword emits, so that the constraint bites."""
        f = free.tolist()
        if len(f) == 1:                  # the strong cases: one row, six new ids
            return dict(base, **{"suppress": dict(suppress_tokens=sorted({f[0][0], f[0][3]})),
                                 "begin": dict(begin_suppress_tokens=[f[0][0]]),
                                 "min_new": dict(eos_token_id=[f[0][1]], min_new_tokens=4),
                                 "bad_words": dict(bad_words_ids=[[f[0][0]], [f[0][2]]])}[which])
        if which == "suppress":
            return dict(base, suppress_tokens=sorted({f[0][0], f[0][3], f[-1][1], f[-1][5]}))
        if which == "begin":
            return dict(base, begin_suppress_tokens=sorted({f[0][0], f[-1][0], f[0][4]}))
        if which == "min_new":
            return dict(base, eos_token_id=[f[0][1], f[-1][2]], min_new_tokens=5)       # eos ids that run emits at steps 1 / 2
        if which == "bad_words":
            return dict(base, bad_words_ids=[[f[0][0]], [f[0][2]], [f[-1][4]]])
        raise KeyError(which)

    def allowed_set(seed, n, eos=True):
        g = torch.Generator().manual_seed(seed)
        return sorted(set(torch.randperm(V - 2, generator=g)[:n].tolist()) | ({319} if eos else set()))

    base = dict(max_new_tokens=8, no_repeat_ngram_size=NGRAM, eos_token_id=319, pad_token_id=318)
    # every keyword on its own, 2 left-padded prompts: whatever margins the model gives (the GPU test follows these up to a near-tie)
    src = embeds_src(200)
    free = gen(src, **base).sequences
    for which in ("suppress", "begin", "min_new", "bad_words"):
        kw = keywords_for(which, free, base)
        out = gen(src, **kw)
        assert out.sequences.shape != free.shape or not torch.equal(out.sequences, free), which
        record(which, src, out, kw, False)
    kw = dict(base, allowed_token_ids=allowed_set(5, 24))
    out = gen(src, **kw)
    assert not torch.equal(out.sequences, free)
    record("allowed", src, out, kw, False)
    # one strong case per keyword. The tiny model's own top-2 gaps are a few hundredths at most steps (no prompt in 40 holds 0.16 over six
    # steps), so the strong cases decode inside a small allowed set, where the competitors are few and the gaps wide; the keyword under
    # test acts on ids of that set. Prompts and sets are searched by seed until the margin holds at every step.
    for which in ("allowed", "suppress", "begin", "min_new", "bad_words"):
        found = False
        for seed in range(300, 1300):
            src = embeds_src(seed, rows=1)
            abase = dict(base, max_new_tokens=6, allowed_token_ids=allowed_set(seed, 6, eos=False))
            free = gen(src, **abase).sequences
            assert free.shape[1] == 6              # (eos 319 is outside the set: the row cannot stop)
            if which == "allowed":
                kw, out = abase, gen(src, **abase)
                changed = not torch.equal(out.sequences, gen(src, **dict(base, max_new_tokens=6)).sequences)
            else:
                kw = keywords_for(which, free, abase)
                out = gen(src, **kw)
                changed = out.sequences.shape != free.shape or not torch.equal(out.sequences, free)
            if changed and margin(out, src, kw) >= STRONG:
                record(which + "_strong", src, out, kw, True)
                found = True
                break
        assert found, f"no prompt gives keyword {which} a margin of {STRONG} at every step: widen the search, do not lower the floor"
    # the keywords combined with the penalty and the ban, on an input_ids prompt
    g = torch.Generator().manual_seed(93)
    ids = torch.randint(0, 300, (2, 9), generator=g)
    src = dict(input_ids=ids, attention_mask=torch.ones_like(ids))
    free = gen(src, max_new_tokens=10, repetition_penalty=1.1, no_repeat_ngram_size=2, eos_token_id=319, pad_token_id=318).sequences[:, 9:]
    f = free.tolist()
    kw = dict(max_new_tokens=10, repetition_penalty=1.1, no_repeat_ngram_size=2, eos_token_id=[f[0][2], 319], pad_token_id=318,
              min_new_tokens=6, suppress_tokens=[f[0][0], f[1][3]], begin_suppress_tokens=[f[1][0], int(ids[0, 0])],
              bad_words_ids=[[f[0][4]]],
              allowed_token_ids=sorted(set(range(0, V, 2)) | set(f[0]) | set(f[1]) | {319}))
    out = gen(src, **kw)
    assert not torch.equal(out.sequences[:, 9:], free)
    record("combined_ids", src, out, kw, False)
    # beam search, 2 left-padded prompts x 3 beams, suppress + min_new_tokens + begin_suppress_tokens
    src = embeds_src(91)
    free = gen(src, num_beams=3, max_new_tokens=8, eos_token_id=319, pad_token_id=318).sequences
    f = free.tolist()
    for name, extra in (("beam_a", dict(num_return_sequences=1)), ("beam_b", dict(num_return_sequences=2, no_repeat_ngram_size=2,
                                                                                     length_penalty=0.5))):
        kw = dict(num_beams=3, max_new_tokens=8, eos_token_id=[f[0][2], f[1][3]], pad_token_id=317, min_new_tokens=4,
                  suppress_tokens=[f[0][1], f[1][5]], begin_suppress_tokens=[f[0][0], f[1][0]], **extra)
        out = gen(src, **kw)
        plain = gen(src, **{k: v for k, v in kw.items() if k not in ("min_new_tokens", "suppress_tokens", "begin_suppress_tokens")})
        assert out.sequences.shape != plain.sequences.shape or not torch.equal(out.sequences, plain.sequences), name
        record(name, src, out, kw, False)
    for which in ("suppress", "begin", "min_new", "allowed", "bad_words"):
        assert any(c["name"] == which + "_strong" and c["strong"] and c["margin"] >= STRONG for c in cases), which
    arrays["meta"] = np.frombuffer(json.dumps({"cases": cases, "transformers": transformers.__version__, "tie_tol": TIE_TOL}).encode(),
                                   np.uint8)
    np.savez_compressed(ROOT / "tests" / "golden" / "constrain_tiny.npz", **arrays)


if __name__ == "__main__":
    main()
