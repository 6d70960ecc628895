"""bench.py's plain run (the headline only) and its --dump-outputs, and the device-side random initialisation it builds its model with."""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]


def test_plain_bench_run_times_its_steps_and_dumps_outputs(tmp_path):
    """A plain run prints one line with the headline fields and --steps timed steps, runs none of what --full adds, and writes the last
    step's outputs as float32 .npy files within 64 MB. 2 Qwen3 layers: plumbing, the line says valid: false."""
    out = tmp_path / "dump"
    cmd = [sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--layers", "2",
           "--dump-outputs", str(out)]
    pr = subprocess.run(cmd, cwd=str(ROOT), capture_output=True, text=True, timeout=900)
    assert pr.returncode == 0, pr.stderr[-3000:]
    lines = [l for l in pr.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["config"]["grad_accum"] == 3 and d["full"] is False and d["config"]["valid"] is False
    assert d["value"] > 0 and d["ms_per_step"] > 0 and d["unit"] == "samples/s" and d["higher_is_better"] is True and d["dtype"] == "bf16"
    assert abs(d["ms_per_step"] - 6e3 / d["value"]) < 0.02 * d["ms_per_step"] + 0.01       # 6 samples per step, one GPU
    assert d["roofline"] is None and d["forward_only"] is None and d["trimmed_padding_variant"] is None
    assert not [k for k in d if k.endswith("_variant") and d[k] is not None] and "cpu_baseline" not in d
    files = {p.stem: np.load(p) for p in out.glob("*.npy")}
    assert {"loss", "grad_norm", "text_weights_sample", "text_master_sample", "text_adam_m_sample", "geom_master_sample"} <= set(files)
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in files.values())
    assert sum(a.nbytes for a in files.values()) <= 64 << 20
    assert abs(float(files["loss"][0]) - d["loss"]) < 1e-3 and float(files["grad_norm"][0]) > 0
    assert np.abs(files["text_adam_m_sample"]).max() > 0                   # the timed window's optimiser step ran


def test_init_on_device_is_seeded_and_keeps_the_distributions():
    """VisionLanguageConfig(init_on_device=True): the same seed gives the same weights twice, a different one different weights, and the
    draws keep the host-side initialisation's rules (normal std 0.02 matrices, unit norm weights, zero biases, xavier-bounded Perceiver)."""
    from vggt_qwen3_amd.perceiver import PerceiverConfig
    from vggt_qwen3_amd.qwen3 import Qwen3Config
    from vggt_qwen3_amd.vlm import VGGTQwen3VLM, VisionLanguageConfig

    def build(seed):
        qcfg = Qwen3Config(hidden_size=256, num_hidden_layers=2, num_attention_heads=2, num_key_value_heads=1, head_dim=128,
                           intermediate_size=256, vocab_size=300)
        pcfg = PerceiverConfig(latent_dim=128, num_latents=16, num_heads=2, num_layers=1, ffn_dim=256, dropout=0.0)
        cfg = VisionLanguageConfig(text_model_name="synthetic", vision_ckpt_dir="none", num_vis_tokens=16, geom_tokens=4,
                                   projector_cfg=pcfg, text_config=qcfg, seed=seed, device="cuda:0", init_on_device=True,
                                   vision_config=dict(img_size=70, embed_dim=128, depth=1, dino_depth=1))
        return VGGTQwen3VLM(cfg)

    a, b, c = build(0), build(0), build(5)
    ta = a.text_model
    assert torch.equal(ta.flat_w, b.text_model.flat_w) and not torch.equal(ta.flat_w, c.text_model.flat_w)
    w = ta._w["l0.gu"].float()
    assert abs(float(w.std()) - 0.02) < 2e-3 and abs(float(w.mean())) < 1e-3
    assert (ta._w["l0.ln1"] == 1).all() and (ta._w["norm"] == 1).all()
    va, vb = a.vision_model.aggregator.named_tensors(), b.vision_model.aggregator.named_tensors()
    assert all(torch.equal(va[n], vb[n]) for n in va)
    qkv = va["frame_blocks.0.attn.qkv.weight"].float()
    assert qkv.is_cuda and abs(float(qkv.std()) - 0.02) < 2e-3 and (va["frame_blocks.0.attn.qkv.bias"] == 0).all()
    pa, pb = dict(a.projector.named_parameters()), dict(b.projector.named_parameters())
    assert all(p.is_cuda and torch.equal(p, pb[n]) for n, p in pa.items())
    W = pa["layers.0.mlp.0.weight"].detach()
    assert float(W.abs().max()) <= (6.0 / sum(W.shape)) ** 0.5 and (pa["layers.0.mlp.0.bias"] == 0).all()
