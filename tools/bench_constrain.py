"""What the decoding constraints cost per pick at Qwen3-4B's vocabulary: vq3_greedy_pick and vq3_sample_pick (top-k 50 / top-p 0.9)
unmasked - today's entries - against their masked twins under a 16-id suppress set and under a 1000-id allowed set, at 1 and 8 rows,
V = 151936, processors as the reference's callers set them (penalty 1.1,
4-gram ban over a 64-id history). Timed as decode runs them, with the method of tools/bench_sample.py: 100 calls chained
in one captured graph, median / min / max of 5 windows (tools/bench_logprob.py: time_us). The planes add V / 8 bytes to the 2 V bytes
of a row; `expected_us` is the unmasked time of the same run plus 6 % plus that time's own max - min spread.
Writes one JSON document (DESIGN.md quotes it).
Usage: python tools/bench_constrain.py [--out profiles/constrain_bench.json]"""
import argparse
import json
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

import numpy as np
import torch

from tools.bench_logprob import time_us
from vggt_qwen3_amd import ops

V = 151936
HISTORY = 64


def _stat(med, lo, hi, calls):
    return {"us": round(med, 2), "us_min": round(lo, 2), "us_max": round(hi, 2), "calls_per_window": calls}


def _masks(prompt_cols):
    rng = np.random.default_rng(0)
    sup = rng.choice(V, 16, replace=False)
    allowed = np.sort(rng.choice(V, 1000, replace=False))
    return {"suppress_16": ops.PickMask(ops.mask_planes(V, always=sup), 0, prompt_cols, "cuda"),
            "allowed_1000": ops.PickMask(ops.mask_planes(V, always=np.setdiff1d(np.arange(V), allowed)), 0, prompt_cols, "cuda")}


def _with_expectation(row):
    base = row["unmasked"]
    row["expected_us"] = round(base["us"] * 1.06 + (base["us_max"] - base["us_min"]), 2)
    for k in ("suppress_16", "allowed_1000"):
        row[k]["over_unmasked_us"] = round(row[k]["us"] - base["us"], 2)
        row[k]["within_expectation"] = bool(row[k]["us"] <= row["expected_us"])
    return row


def pick_table():
    g = torch.Generator(device="cuda").manual_seed(0)
    masks = _masks(0)
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
        row = {"case": "greedy", "rows": B,
               "unmasked": _stat(*time_us(lambda: ops.greedy_pick(logits, work, gen, step, fin, 1.1, 4, None, 0, nxt, V)))}
        for name, m in masks.items():
            row[name] = _stat(*time_us(lambda m=m: ops.greedy_pick_masked(logits, work, gen, step, fin, 1.1, 4, None, 0, nxt, V, m)))
        table.append(_with_expectation(row))
        print(json.dumps(row), flush=True)
        row = {"case": "sample_k50_p0.9", "rows": B}
        for name, m in [("unmasked", None)] + list(masks.items()):
            row[name] = _stat(*time_us(lambda m=m: ops.sample_pick(logits, work, gen, step, fin, 1.1, 4, None, 0, nxt, V, 0.7, 50, 0.9, 1234, sw,
                                                                  mask=m)))
        table.append(_with_expectation(row))
        print(json.dumps(row), flush=True)
    return table


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_constrain.py measures on the GPU"
    doc = {"kernels": ["vq3_greedy_pick[_masked]", "vq3_sample_pick[_masked]"], "V": V, "dtype": "bf16",
           "history_ids": HISTORY,
           "note": "us = device time per call, 100 calls chained in a captured graph, median / min / max of 5 windows of about 100 ms; "
                   "processors: penalty 1.1, 4-gram ban; sample: temperature 0.7, top-k 50, top-p 0.9. "
                   "expected_us = unmasked us * 1.06 + (unmasked us_max - us_min)",
           "picks": pick_table()}
    if a.out:
        Path(a.out).write_text(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
