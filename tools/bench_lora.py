"""LoRA kernels at the production shapes (algorithmic GB/s) and Stage-1 samples/s with stage-1 LoRA (r 16, q/k/v/o) against full
fine-tuning at config C2, in one process. Prints one JSON line.

    python tools/bench_lora.py [--layers 36] [--accum 20] [--no-stage1]
"""
from __future__ import annotations

import argparse
import gc
import json
import sys
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

BF16, F32 = torch.bfloat16, torch.float32


def timed(fn, reps=20):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e-3


def kernels(M=12000, r=16):
    from vggt_qwen3_amd import ops
    dev = "cuda"
    H, Ho, nq, nkv = 2560, 4096, 4096, 1024
    g = torch.Generator(device=dev).manual_seed(0)
    rnd = lambda *s: (torch.randn(*s, device=dev, generator=g) * 0.05).to(BF16)
    xn1, ao = rnd(M, H), rnd(M, Ho)
    A3, Ao = rnd(3 * r, H), rnd(r, Ho)
    Bs = [rnd(nq, r), rnd(nkv, r), rnd(nkv, r)]
    Bo = rnd(H, r)
    qkv, hmid = rnd(M, nq + 2 * nkv), rnd(M, H)
    cols = [(0, nq), (nq, nkv), (nq + nkv, nkv)]
    out = {}

    def rec(name, sec, nbytes):
        out[name] = {"us": round(sec * 1e6, 1), "GB_s": round(nbytes / sec / 1e9, 1)}

    for p in (0.0, 0.05):
        down = [dict(w=A3[k * r:(k + 1) * r], k=H, u_col0=k * r, mask=p > 0, mask_offset=k * M * H) for k in range(3)]
        U = ops.lora_down(xn1, down, r, p=p, seed=1)
        rec(f"down_xn1_R48_p{p}", timed(lambda: ops.lora_down(xn1, down, r, U=U, p=p, seed=1)), M * H * 2 + M * 3 * r * 2)
        Uo = ops.lora_down(ao, [dict(w=Ao, k=Ho, mask=p > 0)], r, p=p, seed=1)
        rec(f"down_ao_R16_p{p}", timed(lambda: ops.lora_down(ao, [dict(w=Ao, k=Ho, mask=p > 0)], r, U=Uo, p=p, seed=1)), M * Ho * 2 + M * r * 2)
    up = [dict(w=Bs[k], y_col0=c0, n=n, u_col0=k * r) for k, (c0, n) in enumerate(cols)]
    rec("up_add_N6144", timed(lambda: ops.lora_up_add(qkv, U, up, r, 2.0)), M * (nq + 2 * nkv) * 4 + M * 3 * r * 2)
    rec("up_add_N2560", timed(lambda: ops.lora_up_add(hmid, Uo, [dict(w=Bo, n=H)], r, 2.0)), M * H * 4 + M * r * 2)
    dX = rnd(M, H)
    dxt = [dict(w=A3[k * r:(k + 1) * r], kmajor=1, ldw=H, n=H, u_col0=k * r, mask=1, mask_offset=k * M * H) for k in range(3)]
    rec("up_add_dX_N2560_masked", timed(lambda: ops.lora_up_add(dX, U, dxt, r, 2.0, p=0.05, seed=1, mask_ld=H)), M * H * 4 + M * 3 * r * 2)
    gB = torch.zeros((nq + 2 * nkv) * r, device=dev, dtype=F32)
    bt = [dict(y_col0=c0, n=n, x_col0=k * r, k=r, u_col0=c0 * r) for k, (c0, n) in enumerate(cols)]
    rec("wgrad_dB_qkv", timed(lambda: ops.lora_wgrad(qkv, U, bt, gB, alpha=2.0)), M * (nq + 2 * nkv) * 2 + M * 3 * r * 2)
    gA = torch.zeros(3 * r * H, device=dev, dtype=F32)
    at = [dict(y_col0=k * r, n=r, k=H, u_col0=k * r * H, mask=1, mask_offset=k * M * H) for k in range(3)]
    rec("wgrad_dA_qkv_masked", timed(lambda: ops.lora_wgrad(U, xn1, at, gA, alpha=2.0, p=0.05, seed=1)), M * H * 2 + M * 3 * r * 2)
    return out


def stage1(lora: bool, layers: int, accum: int, windows: int = 2):
    import yaml
    from bench import BatchStream, synthetic_batch
    from vggt_qwen3_amd.perceiver import PerceiverConfig
    from vggt_qwen3_amd.qwen3 import Qwen3Config
    from vggt_qwen3_amd.trainer import Stage1Trainer
    from vggt_qwen3_amd.vlm import VGGTQwen3VLM, VisionLanguageConfig
    dev = torch.device("cuda", 0)
    qcfg = Qwen3Config.qwen3_4b()
    qcfg.num_hidden_layers = layers
    pcfg = PerceiverConfig(**yaml.safe_load((ROOT / "configs" / "perceiver_small.yaml").read_text()))
    vcfg = VisionLanguageConfig(text_model_name="synthetic", vision_ckpt_dir="none", num_vis_tokens=128, geom_tokens=0,
                                projector_cfg=pcfg, text_config=qcfg, device=str(dev), seed=0, init_on_device=True)
    model = VGGTQwen3VLM(vcfg).train()
    if lora:
        model.enable_lora(r=16, alpha=32, dropout=0.05, target_modules=["q_proj", "k_proj", "v_proj", "o_proj"])
    tr = Stage1Trainer(model, grad_accum=accum, max_steps=30000)
    tr.overlap_optimizer = True
    B, V, L = 6, 1, 200
    stream = BatchStream(2 * tr.text_group, lambda i: synthetic_batch(B, V, L, 448, 151936, model.image_id, 151643, 198, 1234 + i, dev, False))

    def window():
        batches = [stream._draw() for _ in range(accum)]
        for i, b in enumerate(batches):
            tr.micro_step(b, upcoming=batches[i + 1:])

    window()                                   # warm-up (one-time costs)
    tr.sync_optimizer()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(windows):
        window()
    tr.sync_optimizer()
    torch.cuda.synchronize()
    sec = time.perf_counter() - t0
    res = round(windows * accum * B / sec, 2)
    del tr, model, stream
    gc.collect()
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=36)
    ap.add_argument("--accum", type=int, default=20)
    ap.add_argument("--no-stage1", action="store_true")
    a = ap.parse_args()
    from vggt_qwen3_amd import _lib
    _lib.load()
    res = {"metric": "LoRA kernels (M = 12000, r = 16) and Stage-1 C2 samples/s, LoRA vs full fine-tuning", "kernels": kernels(),
           "hbm_peak_GB_s": 6300}
    if not a.no_stage1:
        full = stage1(False, a.layers, a.accum)
        lo = stage1(True, a.layers, a.accum)
        res["stage1"] = {"full_samples_s": full, "lora_samples_s": lo, "ratio": round(lo / full, 3), "layers": a.layers,
                         "grad_accum": a.accum}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
