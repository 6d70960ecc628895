"""What a KV-cache session saves at Qwen3-4B's shape (36 layers, random weights, B = 1), timed as tools/bench_decode.py times: a host
clock around work that ends in a device synchronise. Every cell alternates its two sides in one process for --rounds rounds and reports
each side's median and max - min.
  (a) extend() of a 32-position chunk behind a cached prefix of 200 / 1000 / 2000 positions, against forward_hidden over the whole
      232 / 1032 / 2032 - without a cache the only way to the same state;
  (b) extend() of 200 positions on an empty cache against generate()'s _prefill of the same 200;
  and the device time of one vq3_qwen_append_attn launch at (prefix 2000, chunk 32): Hkv workgroups of one query block each.
Usage: python tools/bench_kvcache.py [--out profiles/kvcache_bench.json] [--layers 36] [--rounds 5]"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

import torch

from vggt_qwen3_amd import generate as G
from vggt_qwen3_amd import ops
from vggt_qwen3_amd.qwen3 import Qwen3Config, Qwen3ForCausalLM

BF16 = torch.bfloat16


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def alternate(side_a, side_b, rounds, before_a=None):
    """ms of both sides, alternating; before_a (untimed) puts side a's state back."""
    a, b = [], []
    for r in range(rounds + 1):                 # round 0 warms both sides up and is dropped
        if before_a is not None:
            before_a()
        ta = timed(side_a)
        tb = timed(side_b)
        if r:
            a.append(ta)
            b.append(tb)
    stat = lambda v: {"median_ms": statistics.median(v), "spread_ms": max(v) - min(v), "runs_ms": v}
    return stat(a), stat(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(Path(__file__).resolve().parents[1] / "profiles" / "kvcache_bench.json"))
    ap.add_argument("--layers", type=int, default=36)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--chunk", type=int, default=32)
    ap.add_argument("--prefixes", type=int, nargs="+", default=[200, 1000, 2000])
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_kvcache needs a GPU"
    cfg = Qwen3Config.qwen3_4b()
    cfg.num_hidden_layers = a.layers
    tm = Qwen3ForCausalLM(cfg, device="cuda", seed=0)
    H = cfg.hidden_size
    torch.manual_seed(0)
    res = {"model": "Qwen3-4B shape, random weights", "layers": a.layers, "batch": 1, "rounds": a.rounds, "chunk": a.chunk,
           "device": torch.cuda.get_device_name(0), "extend_vs_whole_forward": [], "timing": "host clock around a device synchronise"}
    for P in a.prefixes:
        L = P + a.chunk
        emb = (torch.randn(1, L, H, device="cuda") * 0.02).to(BF16)
        mask = torch.ones(1, L, dtype=torch.long, device="cuda")
        cache = tm.kv_cache(1, L)
        tm.extend(cache, inputs_embeds=emb[:, :P])
        ext, whole = alternate(lambda: tm.extend(cache, inputs_embeds=emb), lambda: tm.forward_hidden(emb, mask, save=False), a.rounds,
                               before_a=lambda: cache.truncate(P))
        gain = whole["median_ms"] - ext["median_ms"]
        res["extend_vs_whole_forward"].append({"prefix": P, "chunk": a.chunk, "extend": ext, "forward_hidden_whole": whole,
                                               "gain_ms": gain, "gain_exceeds_spreads": gain > ext["spread_ms"] + whole["spread_ms"]})
        if P == max(a.prefixes):
            # one layer's append_attn alone, device events around 50 launches
            Q =(torch.randn(1, tm.Hq, a.chunk, tm.D, device="cuda")).to(BF16)
            lens = torch.tensor([P], dtype=torch.int32, device="cuda")
            new = torch.tensor([a.chunk], dtype=torch.int32, device="cuda")
            run = lambda: ops.qwen_append_attn(Q, cache.K[0], cache.V[0], lens, new, 1, a.chunk, tm.Hq, tm.Hkv, tm.D, cache.capacity, tm.D ** -0.5)
            for _ in range(5):
                run()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(50):
                run()
            e1.record()
            torch.cuda.synchronize()
            per = e0.elapsed_time(e1) / 50
            res["append_attn_one_layer"] = {"prefix": P, "chunk": a.chunk, "workgroups": tm.Hkv, "ms_per_launch": per,
                                            "ms_all_layers": per * a.layers, "share_of_extend": per * a.layers / ext["median_ms"]}
        del cache
    # (b) an empty cache: extend() against generate()'s _prefill
    n = 200
    emb = (torch.randn(1, n, H, device="cuda") * 0.02).to(BF16)
    cache = tm.kv_cache(1, 256)
    st = G.DecodeState(tm, 1, 256, 1)
    ext, pre = alternate(lambda: tm.extend(cache, inputs_embeds=emb), lambda: G._prefill(tm, st, emb, [(0, n)]), a.rounds,
                         before_a=lambda: cache.truncate(0))
    res["empty_cache_extend_vs_prefill"] = {"positions": n, "extend": ext, "prefill": pre, "extend_minus_prefill_ms": ext["median_ms"] - pre["median_ms"],
                                            "extend_slower_beyond_spreads": ext["median_ms"] - pre["median_ms"] > ext["spread_ms"] + pre["spread_ms"]}
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
