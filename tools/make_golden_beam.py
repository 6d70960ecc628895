"""Writes tests/golden/beam_tiny.npz: transformers' own beam search (generate(num_beams=..., do_sample=False)) on the tiny Qwen3 of
qwen3_tiny.npz (same weights), with the per-step processed scores it searched on. tests/test_beam_host.py replays tests/beam_ref.py on
those scores and must reproduce the sequences, beam indices and scores recorded here. Run in the build container only (CPU)."""
import json
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from tests.golden_io import load, weights  # noqa: E402
from tools.make_golden import bf16_bits, tiny_qwen_cfg  # noqa: E402


def main():
    import transformers
    from transformers import Qwen3ForCausalLM
    z = load("qwen3_tiny.npz")
    cfg = tiny_qwen_cfg(320)
    model = Qwen3ForCausalLM(cfg).to(torch.bfloat16).eval()
    sd = weights(z)
    sd["lm_head.weight"] = sd["model.embed_tokens.weight"]
    model.load_state_dict(sd)
    model.generation_config.pad_token_id = None
    H = cfg.hidden_size
    arrays, cases = {}, []
    g = torch.Generator().manual_seed(91)
    emb = (torch.randn(2, 14, H, generator=g) * 0.5).to(torch.bfloat16)
    mask = torch.ones(2, 14, dtype=torch.long)
    mask[1, :5] = 0
    ids = torch.randint(0, 300, (1, 9), generator=g)
    arrays["embeds"] = bf16_bits(emb)
    arrays["mask"] = mask.numpy()
    arrays["input_ids"] = ids.numpy()

    def run(name, use_ids, **kw):
        src = dict(input_ids=ids, attention_mask=torch.ones_like(ids)) if use_ids else dict(inputs_embeds=emb, attention_mask=mask)
        with torch.no_grad():
            out = model.generate(**src, do_sample=False, return_dict_in_generate=True, output_scores=True, **kw)
        scores = torch.stack(out.scores, 0)
        assert scores.dtype == torch.float32 and scores.shape[1:] == (src["attention_mask"].shape[0] * kw["num_beams"], 320)
        arrays[f"{name}:scores"] = scores.numpy()
        arrays[f"{name}:sequences"] = out.sequences.numpy()
        arrays[f"{name}:sequences_scores"] = out.sequences_scores.numpy()
        arrays[f"{name}:beam_indices"] = out.beam_indices.numpy()
        cases.append({"name": name, "input": "input_ids" if use_ids else "inputs_embeds", "kw": kw})
        print(name, out.sequences.tolist(), out.sequences_scores.tolist())
        return out.sequences

    # inputs_embeds, 2 left-padded prompts x 3 beams; no eos is hit: every hypothesis runs to max_length
    free = run("emb_free", False, num_beams=3, max_new_tokens=10, eos_token_id=319, pad_token_id=318)
    # eos ids taken from that run, so that some beams finish early
    e1, e2 = int(free[0, 3]), int(free[1, 5])
    run("emb_eos2", False, num_beams=3, num_return_sequences=2, max_new_tokens=10, eos_token_id=[e1, e2], pad_token_id=317)
    # one case per early_stopping value, length_penalty 0 / 1 / 2
    run("es_false_lp1", False, num_beams=3, num_return_sequences=3, max_new_tokens=8, eos_token_id=e1, pad_token_id=317,
        early_stopping=False, length_penalty=1.0)
    run("es_true_lp0", False, num_beams=3, num_return_sequences=3, max_new_tokens=8, eos_token_id=[e1, e2], pad_token_id=317,
        early_stopping=True, length_penalty=0.0)
    run("es_never_lp2", False, num_beams=3, num_return_sequences=3, max_new_tokens=8, eos_token_id=e1, pad_token_id=317,
        early_stopping="never", length_penalty=2.0)
    run("es_never_lp0", False, num_beams=3, num_return_sequences=1, max_new_tokens=8, eos_token_id=[e1, e2], early_stopping="never",
        length_penalty=0.0)
    # input_ids, 1 prompt x 4 beams: the prompt takes part in the penalty and the ban and is returned in front
    run("ids", True, num_beams=4, num_return_sequences=4, max_new_tokens=12, repetition_penalty=1.1, no_repeat_ngram_size=2,
        eos_token_id=319, pad_token_id=318)
    arrays["meta"] = np.frombuffer(json.dumps({"cases": cases, "transformers": transformers.__version__}).encode(), np.uint8)
    np.savez_compressed(ROOT / "tests" / "golden" / "beam_tiny.npz", **arrays)


if __name__ == "__main__":
    main()
