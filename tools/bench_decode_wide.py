"""Decode throughput of Qwen3-4B (random weights) at 8 to 64 rows per call, and the decode GEMM (csrc/decode_gemm.hip) alone on the
five projection shapes of a step. Settings of tools/bench_decode.py: prompt 200, 64 new tokens, graph on, repetition_penalty 1.1,
no_repeat_ngram_size 4. Usage: python tools/bench_decode_wide.py [--rows 8 16 32 64] [--kernel-rows 16 64] [--out FILE]

End to end: ms per step = (time of generate(64 new) - time of generate(2 new)) / 62, each the minimum of three calls on one session
cache (kv_cache=) so that both make the same allocations; tokens/s = rows / that, and the weight stream's share of the 8 TB/s HBM
peak (every weight once per step; the K/V cache read and the activations are not counted).
Kernel alone: one HIP graph of `iters` calls per shape, the weight rotating over copies that together exceed the 256 MB infinity cache,
timed by device events over 3 replays after one warm-up replay; us per call and the weight bytes per second."""
import argparse
import json
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

import torch

from vggt_qwen3_amd import ops
from vggt_qwen3_amd.qwen3 import Qwen3Config, Qwen3ForCausalLM

BF16 = torch.bfloat16


def end_to_end(tm, cfg, rows, prompt, new):
    emb = (torch.randn(rows, prompt, cfg.hidden_size, device="cuda") * 0.02).to(BF16)
    mask = torch.ones(rows, prompt, dtype=torch.long, device="cuda")
    kw = dict(inputs_embeds=emb, attention_mask=mask, repetition_penalty=1.1, no_repeat_ngram_size=4, use_graph=True, max_rows=max(8, rows))
    # Both timed calls decode on ONE session cache of the long call's capacity: a call that allocates its own K/V (1.2 GB per operand at
    # 64 rows, another size for 2 new tokens than for 64) pays the allocator more than 62 decode steps take, and not the same in both.
    cache = tm.kv_cache(rows, ops.round_up(prompt + new, 64))

    def timed(n):
        cache.truncate(0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = tm.generate(max_new_tokens=n, return_stats=True, kv_cache=cache, **kw)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, res

    for n in (2, new):                                        # warm-up of both timed calls (allocator, code objects, the prefill GEMMs' tuner)
        timed(n)
    t_short = t_long = float("inf")
    for _ in range(3):                                        # the minimum of three
        t_short = min(t_short, timed(2)[0])
        t, (out, stats) = timed(new)
        t_long = min(t_long, t)
    per_step = (t_long - t_short) / (new - 2)
    wbytes = 2 * sum(p.numel() for n, p in tm.named_parameters() if n != "lm_head.weight")   # every weight once (embedding = lm_head)
    kv_bytes = 2 * 2 * cfg.num_hidden_layers * rows * cfg.num_key_value_heads * cfg.head_dim * (prompt + new // 2)   # K and V, mid-run length
    return {"rows": rows, "prompt": prompt, "new_tokens": int(out.shape[1]), "graph": stats["graph"], "ms_per_step": per_step * 1e3,
            "tokens_per_s": rows / per_step, "weight_GB_per_step": wbytes / 1e9, "kv_read_GB_per_step": kv_bytes / 1e9,
            "weight_stream_GBps": wbytes / per_step / 1e9, "weight_stream_frac_of_8TBps": wbytes / per_step / 8e12}


def kernel_alone(M, iters=40):
    c = Qwen3Config.qwen3_4b()
    H, I, D = c.hidden_size, c.intermediate_size, c.head_dim
    qkv_n, o_k = (c.num_attention_heads + 2 * c.num_key_value_heads) * D, c.num_attention_heads * D
    shapes = [("qkv", qkv_n, H, "ln"), ("o", H, o_k, "res"), ("gu", 2 * I, H, "ln"), ("down", H, I, "swiglu+res"), ("lm_head", c.vocab_size, H, "ln")]
    out = []
    for name, N, K, mode in shapes:
        copies = max(2, -(-(768 << 20) // (2 * N * K)))
        ws = [(torch.randn(N, K, device="cuda") * 0.02).to(BF16) for _ in range(copies)]
        x = torch.randn(M, 2 * K if "swiglu" in mode else K, device="cuda").to(BF16)
        kw = {}
        if "ln" in mode:
            kw.update(ln_w=torch.ones(K, device="cuda", dtype=BF16), eps=1e-6)
        if "swiglu" in mode:
            kw.update(swiglu=True)
        if "res" in mode:
            kw.update(residual=torch.randn(M, N, device="cuda").to(BF16))
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for w in ws:
                ops.decode_linear(x, w, **kw)
        torch.cuda.current_stream().wait_stream(side)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for i in range(iters):
                ops.decode_linear(x, ws[i % copies], **kw)
        g.replay()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(3):
            g.replay()
        e1.record()
        torch.cuda.synchronize()
        us = e0.elapsed_time(e1) * 1e3 / (3 * iters)
        out.append({"shape": name, "M": M, "N": N, "K": K, "x": mode, "us_per_call": us, "weight_GBps": 2 * N * K / us / 1e3,
                    "weight_frac_of_8TBps": 2 * N * K / us / 1e3 / 8000})
        del ws, g
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="*", default=[8, 16, 32, 64])
    ap.add_argument("--kernel-rows", type=int, nargs="*", default=[16, 64])
    ap.add_argument("--prompt", type=int, default=200)
    ap.add_argument("--new", type=int, default=64)
    ap.add_argument("--layers", type=int, default=36)
    ap.add_argument("--out", type=str, default=None, help="also write the JSON document to this file")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_decode_wide.py needs a GPU"
    res = {"end_to_end": [], "kernel_alone": []}
    for M in a.kernel_rows:
        res["kernel_alone"] += kernel_alone(M)
    if a.rows:
        cfg = Qwen3Config.qwen3_4b()
        cfg.num_hidden_layers = a.layers
        tm = Qwen3ForCausalLM(cfg, device="cuda", seed=0)
        for rows in a.rows:
            res["end_to_end"].append(end_to_end(tm, cfg, rows, a.prompt, a.new))
            print(json.dumps(res["end_to_end"][-1]), flush=True)
    doc = json.dumps(res, indent=1)
    print(doc)
    if a.out:
        Path(a.out).write_text(doc + "\n")


if __name__ == "__main__":
    main()
