"""Beam search (csrc/beam.hip) at Qwen3-4B's shape: the two kernels alone, and beam_search() against generate() at the same width.
  1. vq3_beam_step alone: V = 151936, 1 prompt x 2 / 4 / 8 beams, penalty 1.1 and a 4-gram ban over a 64-id history, no eos (the state
     never finishes, so every chained call does the full work). Timed as decode runs it: 100 calls chained in a captured graph.
  2. vq3_beam_reorder alone: 36 layers x 8 KV heads, 1 x 2 / 4 / 8 beams, 200 and 2000 cached positions; a full permutation cycle (every
     row moves) and the identity (nothing moves). GB/s counts the bytes actually moved: each moved row read once and written once.
  3. End to end, random weights: per-token time of beam_search(num_beams=n) and of generate() with n rows, alternating in one process.
Writes one JSON document (DESIGN.md quotes it).
Usage: python tools/bench_beam.py [--out profiles/beam_bench.json] [--layers 36] [--prompt 200] [--new 64] [--rounds 5] [--skip-e2e]"""
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
HBM_GBS = 6300.0        # the achievable rate this project measures against


def _stat(med, lo, hi, calls):
    return {"us": round(med, 2), "us_min": round(lo, 2), "us_max": round(hi, 2), "calls_per_window": calls}


def step_table():
    g = torch.Generator(device="cuda").manual_seed(0)
    table = []
    for nb in (2, 4, 8):
        logits = (torch.randn(nb, V, generator=g, device="cuda") * 3).to(torch.bfloat16)
        bs = ops.BeamState(1, nb, 512, 0, 0, "cuda")
        bs.run_seq.copy_(torch.randint(0, V, (nb, 512), generator=g, device="cuda").to(torch.int32))
        bs.run_seq[:, 40:44] = bs.run_seq[:, 60:64]             # a repeated 4-gram: the ban has something to do
        bs.run_score.copy_(-torch.arange(nb, device="cuda", dtype=torch.float32))
        step = torch.full((1,), HISTORY, device="cuda", dtype=torch.int32)
        nxt = torch.zeros(nb, device="cuda", dtype=torch.int32)
        row = {"num_beams": nb, "K": 2 * nb}
        row.update(_stat(*time_us(lambda: ops.beam_step(logits, V, bs, step, nxt, 1.1, 4, None, 1.0, False))))
        assert int(bs.all_done.item()) == 0
        table.append(row)
        print(json.dumps(row), flush=True)
    return table


def reorder_table(layers, Hkv=8):
    table = []
    for positions in (200, 2000):
        Lmax = ops.round_up(positions + 64, 64)
        for nb in (2, 4, 8):
            K = torch.randn((layers, nb, Hkv, Lmax, 128), device="cuda", dtype=torch.bfloat16)
            Vc = torch.randn_like(K)
            lens = torch.full((nb,), positions - 1, device="cuda", dtype=torch.int32)
            moved = 2 * 2 * layers * nb * Hkv * positions * 256    # both operands, read + written
            row = {"num_beams": nb, "positions": positions, "bytes_moved": moved}
            for name, src in (("cycle", [(r + 1) % nb for r in range(nb)]), ("identity", list(range(nb)))):
                src_t = torch.tensor(src, device="cuda", dtype=torch.int32)
                st = _stat(*time_us(lambda: ops.beam_reorder(K, Vc, src_t, lens, 1, nb)))
                if name == "cycle":
                    st["GBps"] = round(moved / st["us"] * 1e-3, 1)
                    st["fraction_of_6300"] = round(st["GBps"] / HBM_GBS, 3)
                row[name] = st
            table.append(row)
            print(json.dumps(row), flush=True)
            del K, Vc
    return table


def decode_rates(layers, prompt, new, rounds):
    from vggt_qwen3_amd.qwen3 import Qwen3Config, Qwen3ForCausalLM
    cfg = Qwen3Config.qwen3_4b()
    cfg.num_hidden_layers = layers
    tm = Qwen3ForCausalLM(cfg, device="cuda", seed=0)
    out = {"layers": layers, "prompt": prompt, "new_tokens": new, "rounds": rounds, "widths": []}

    def timed(fn, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(n)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    for nb in (2, 4, 8):
        e1 = (torch.randn(1, prompt, cfg.hidden_size, device="cuda") * 0.02).to(torch.bfloat16)
        en = e1.expand(nb, -1, -1).contiguous()
        m1 = torch.ones(1, prompt, dtype=torch.long, device="cuda")
        runs = {"generate": lambda n: tm.generate(inputs_embeds=en, attention_mask=m1.expand(nb, -1), max_new_tokens=n, use_graph=True),
                "beam_search": lambda n: tm.beam_search(inputs_embeds=e1, attention_mask=m1, max_new_tokens=n, num_beams=nb, use_graph=True)}
        for fn in runs.values():
            fn(4)
        per_tok = {k: [] for k in runs}
        for _ in range(rounds):
            for name, fn in runs.items():                       # alternating: both see the same machine
                t_short = timed(fn, 2)
                t_long = timed(fn, new)
                per_tok[name].append((t_long - t_short) / (new - 2) * 1e3)
        row = {"rows": nb}
        for name, ms in per_tok.items():
            s = sorted(ms)
            row[name] = {"ms_per_step_median": round(s[len(s) // 2], 4), "ms_per_step_min": round(s[0], 4), "ms_per_step_max": round(s[-1], 4),
                         "ms_per_step_runs": [round(x, 4) for x in ms]}
        row["beam_minus_generate_us_per_step"] = round((row["beam_search"]["ms_per_step_median"] - row["generate"]["ms_per_step_median"]) * 1e3, 1)
        row["generate_spread_us_per_step"] = round((row["generate"]["ms_per_step_max"] - row["generate"]["ms_per_step_min"]) * 1e3, 1)
        out["widths"].append(row)
        print(json.dumps(row), flush=True)
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
    assert torch.cuda.is_available(), "bench_beam.py measures on the GPU"
    doc = {"kernels": ["vq3_beam_step", "vq3_beam_reorder"], "V": V, "dtype": "bf16", "history_ids": HISTORY,
           "note": "kernels: us = device time per call, 100 calls chained in a captured graph, median / min / max of 5 windows of about "
                   "100 ms. beam_step: penalty 1.1, 4-gram ban, no eos. reorder: GBps = bytes moved (read + written) / time. decode: (time "
                   "of a run of `new` tokens - time of a run of 2) / (new - 2), host clock around a synchronise, graph replay, "
                   "beam_search(num_beams=n) and generate() with n rows alternating",
           "beam_step": step_table(), "beam_reorder": reorder_table(a.layers)}
    if not a.skip_e2e:
        doc["decode"] = decode_rates(a.layers, a.prompt, a.new, a.rounds)
    if a.out:
        Path(a.out).write_text(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
