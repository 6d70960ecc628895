"""vq3_token_logprob at Qwen3-4B's vocabulary: kernel time and algorithmic GB/s (the bytes of the logits rows, read once) of both
launch shapes per row count, against the 6300 GB/s DESIGN.md uses as the achievable HBM rate. The launches are timed as decode runs
them: back to back inside a captured graph, outputs and scratch allocated once, so the host's cost per call is not in the figure (the
split shape's figure is its two kernels). Writes one JSON document (the table of DESIGN.md's per-token log-probability subsection;
the row-count switch of csrc/logprob.hip is read off it).
Usage: python tools/bench_logprob.py [--out profiles/logprob_bench.json] [--rows 1 8 32 64 128 256 2048]"""
import argparse
import json
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

import torch

from vggt_qwen3_amd import _lib, ops

V = 151936
HBM_GBPS = 6300


WINDOW_MS = 100     # device time per timed window
CHAIN = 100         # launches per graph replay


def time_us(launch):
    """Median / min / max over 5 windows of about WINDOW_MS each of one call's device time: CHAIN calls captured into a graph, the
    graph replayed back to back between two events."""
    launch(); torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(CHAIN):
            launch()

    def window(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            graph.replay()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / reps                # ms per replay

    window(3)
    reps = max(3, int(WINDOW_MS / window(3)))
    res = sorted(window(reps) * 1e3 / CHAIN for _ in range(5))
    return res[2], res[0], res[4], reps * CHAIN


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rows", type=int, nargs="+", default=[1, 8, 32, 64, 128, 256, 2048])
    a = ap.parse_args()
    g = torch.Generator(device="cuda").manual_seed(0)
    lib = _lib.load()
    table = []
    # 512 MB of other data between batches would be the cold-cache figure; rows of 2048 x 300 KB = 622 MB exceed the 256 MB last-level
    # cache on their own, the small row counts are measured as decode meets them: the logits were just written (cache-warm)
    for n in a.rows:
        logits = (torch.randn(n, V, generator=g, device="cuda") * 3).to(torch.bfloat16)
        tgt = torch.randint(0, V, (n,), generator=g, device="cuda").to(torch.int32)
        work = torch.empty(n * ops.LOGPROB_WORK_PER_ROW, device="cuda")
        lp, lse, rank = torch.empty(n, device="cuda"), torch.empty(n, device="cuda"), torch.empty(n, device="cuda", dtype=torch.int32)
        gb = n * V * 2 / 1e9
        row = {"n": n, "MB": round(gb * 1e3, 3)}
        for name, sl in (("rows", 1), ("split", 64)):
            def launch(sl=sl):
                _lib.check(lib.vq3_token_logprob(logits.data_ptr(), logits.stride(0), n, V, tgt.data_ptr(), lp.data_ptr(), lse.data_ptr(),
                                                rank.data_ptr(), work.data_ptr(), sl, torch.cuda.current_stream().cuda_stream),
                          "vq3_token_logprob")
            med, lo, hi, calls = time_us(launch)
            row[name] = {"us": round(med, 2), "us_min": round(lo, 2), "us_max": round(hi, 2), "calls_per_window": calls,
                         "GBps": round(gb / (med * 1e-6), 1),
                         "frac_of_6300": round(gb / (med * 1e-6) / HBM_GBPS, 3)}
        row["faster"] = "rows" if row["rows"]["us"] <= row["split"]["us"] else "split"
        table.append(row)
        print(json.dumps(row), flush=True)
    doc = {"kernel": "vq3_token_logprob", "V": V, "dtype": "bf16", "hbm_GBps_reference": HBM_GBPS,
           "note": "us = device time per call, calls chained in a captured graph (outputs preallocated); split = 64 vocabulary slices "
                   "+ combine launch; 5 windows of about %d ms each" % WINDOW_MS,
           "table": table}
    if a.out:
        Path(a.out).write_text(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
