"""The sampling pick (vq3_sample_pick) against the greedy pick (vq3_greedy_pick) at Qwen3-4B's vocabulary, and sample() against
generate() end to end.
  1. Pick time in isolation: each pick alone at V = 151936 for B = 1 and B = 8, top-k / top-p on (50, 0.9) and off (0, 1.0), with the
     processors as the reference's callers set them (penalty 1.1, 4-gram ban) over a 64-id history. Timed as decode runs them: back to
     back inside a captured graph, buffers allocated once, so the host's cost per call is not in the figure (tools/bench_logprob.py).
  2. End-to-end B = 1 decode rate at Qwen3-4B's shape (random weights): tokens/s of sample() and of generate() in the same process,
     alternating runs; the run-to-run spread of the greedy step is reported beside the difference.
Writes one JSON document (DESIGN.md quotes it).
Usage: python tools/bench_sample.py [--out profiles/sample_bench.json] [--layers 36] [--prompt 200] [--new 64] [--rounds 5] [--skip-e2e]"""
import argparse
import json
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

import torch

from tools.bench_logprob import time_us
from vggt_qwen3_amd import ops

V = 151936
HISTORY = 64


def pick_table():
    g = torch.Generator(device="cuda").manual_seed(0)
    table = []
    for B in (1, 8):
        logits = (torch.randn(B, V, generator=g, device="cuda") * 3).to(torch.bfloat16)
        gen = torch.randint(0, V, (B, 512), generator=g, device="cuda")
        gen[:, 40:44] = gen[:, 60:64]                           # a repeated 4-gram: the ban has something to do
        step = torch.full((1,), HISTORY, device="cuda", dtype=torch.int32)
        fin = torch.zeros(B, device="cuda", dtype=torch.int32)
        nxt = torch.zeros(B, device="cuda", dtype=torch.int32)
        work = torch.zeros(B * 128 + 8, device="cuda")
        sw = ops.sample_workspace(B, "cuda")
        row = {"B": B}
        med, lo, hi, calls = time_us(lambda: ops.greedy_pick(logits, work, gen, step, fin, 1.1, 4, None, 0, nxt, V))
        row["greedy"] = {"us": round(med, 2), "us_min": round(lo, 2), "us_max": round(hi, 2), "calls_per_window": calls}
        for name, (k, p) in (("sample_k50_p0.9", (50, 0.9)), ("sample_k0_p1", (0, 1.0))):
            med, lo, hi, calls = time_us(lambda k=k, p=p: ops.sample_pick(logits, work, gen, step, fin, 1.1, 4, None, 0, nxt, V, 0.7, k, p, 1234, sw))
            row[name] = {"us": round(med, 2), "us_min": round(lo, 2), "us_max": round(hi, 2), "calls_per_window": calls}
        table.append(row)
        print(json.dumps(row), flush=True)
    return table


def decode_rates(layers, prompt, new, rounds):
    from vggt_qwen3_amd.qwen3 import Qwen3Config, Qwen3ForCausalLM
    cfg = Qwen3Config.qwen3_4b()
    cfg.num_hidden_layers = layers
    tm = Qwen3ForCausalLM(cfg, device="cuda", seed=0)
    emb = (torch.randn(1, prompt, cfg.hidden_size, device="cuda") * 0.02).to(torch.bfloat16)
    mask = torch.ones(1, prompt, dtype=torch.long, device="cuda")
    kw = dict(inputs_embeds=emb, attention_mask=mask, repetition_penalty=1.1, no_repeat_ngram_size=4, use_graph=True)
    runs = {"generate": lambda n: tm.generate(max_new_tokens=n, return_stats=True, **kw),
            "sample": lambda n: tm.sample(max_new_tokens=n, return_stats=True, temperature=0.7, top_k=50, top_p=0.9, seed=1234, **kw)}

    def timed(fn, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = fn(n)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, res[-1]

    for fn in runs.values():                                    # warm-up: library load, allocator, both graphs' shapes
        fn(4)
    per_tok = {k: [] for k in runs}
    persistent = {}
    for _ in range(rounds):
        for name, fn in runs.items():                           # alternating: both see the same machine
            t_short, _ = timed(fn, 2)
            t_long, stats = timed(fn, new)
            per_tok[name].append((t_long - t_short) / (new - 2) * 1e3)
            persistent[name] = stats["persistent"]
    out = {"layers": layers, "prompt": prompt, "new_tokens": new, "rounds": rounds, "persistent_layers_kernel": persistent}
    for name, ms in per_tok.items():
        s = sorted(ms)
        out[name] = {"ms_per_token_median": round(s[len(s) // 2], 4), "ms_per_token_min": round(s[0], 4), "ms_per_token_max": round(s[-1], 4),
                     "tokens_per_s": round(1e3 / s[len(s) // 2], 1), "ms_per_token_runs": [round(x, 4) for x in ms]}
    out["sample_minus_generate_us_per_token"] = round((out["sample"]["ms_per_token_median"] - out["generate"]["ms_per_token_median"]) * 1e3, 1)
    out["generate_spread_us_per_token"] = round((out["generate"]["ms_per_token_max"] - out["generate"]["ms_per_token_min"]) * 1e3, 1)
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--layers", type=int, default=36)
    ap.add_argument("--prompt", type=int, default=200)
    ap.add_argument("--new", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--skip-e2e", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_sample.py measures on the GPU"
    doc = {"kernel": "vq3_sample_pick", "V": V, "dtype": "bf16", "history_ids": HISTORY,
           "note": "pick: us = device time per call, 100 calls chained in a captured graph, median / min / max of 5 windows of about "
                   "100 ms; processors: penalty 1.1, 4-gram ban; temperature 0.7. decode: (time of a run of `new` tokens - time of a run "
                   "of 2) / (new - 2), host clock around a synchronise, graph replay, sample() and generate() alternating",
           "pick": pick_table()}
    if not a.skip_e2e:
        doc["decode_b1"] = decode_rates(a.layers, a.prompt, a.new, a.rounds)
    if a.out:
        Path(a.out).write_text(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
