"""LoRA host logic without a GPU: the reference's `lora:` stage-config blocks, what is rejected, peft's names and adapter config, and
the adapters' initialisation (vggt_qwen3_amd/lora.py)."""
import math

import pytest
import torch

from vggt_qwen3_amd import lora

# configs/stage1_3d.yaml and configs/stage2_arkit.yaml of the reference, restated (the reference tree is not shipped with the tests)
STAGE1 = {"lora": {"enable": True, "rank": 16, "alpha": 32, "dropout": 0.05, "target_modules": ["q_proj", "k_proj", "v_proj", "o_proj"]}}
STAGE2 = {"lora": {"enable": True, "rank": 32, "alpha": 64, "dropout": 0.05, "target_modules": ["q_proj", "v_proj", "o_proj"]}}


def test_stage_config_blocks():
    s1 = lora.lora_settings_from_stage_config(STAGE1)
    assert s1 == dict(r=16, alpha=32.0, dropout=0.05, target_modules=["q_proj", "k_proj", "v_proj", "o_proj"])
    s2 = lora.lora_settings_from_stage_config(STAGE2)
    assert s2 == dict(r=32, alpha=64.0, dropout=0.05, target_modules=["q_proj", "v_proj", "o_proj"])
    assert lora.lora_settings_from_stage_config({"lora": {"enable": False, "rank": 16}}) is None
    assert lora.lora_settings_from_stage_config({}) is None
    assert lora.validate(16, 32, 0.0, ["o_proj", "q_proj"]).target_modules == ["q_proj", "o_proj"]


def test_vlm_reexports_the_parser():
    from vggt_qwen3_amd.vlm import lora_settings_from_stage_config
    assert lora_settings_from_stage_config(STAGE2)["r"] == 32


@pytest.mark.parametrize("t", ["gate_proj", "up_proj", "down_proj"])
def test_mlp_targets_not_implemented(t):
    with pytest.raises(NotImplementedError):
        lora.validate(16, 32, 0.0, ["q_proj", t])


@pytest.mark.parametrize("r", [0, 4, 12, 72, 128, 15.5])
def test_bad_ranks(r):
    with pytest.raises(ValueError):
        lora.validate(r, 32, 0.0, ["q_proj"])


def test_other_rejections():
    for bad in (["embed_tokens"], [], ["q_proj", "q_proj"]):
        with pytest.raises(ValueError):
            lora.validate(16, 32, 0.0, bad)
    with pytest.raises(ValueError):
        lora.validate(16, 32, 1.0, ["q_proj"])
    for r in (8, 16, 24, 32, 40, 48, 56, 64):
        assert lora.validate(r, 2 * r, 0.0, ["v_proj"]).scaling == 2.0


def test_peft_names_and_adapter_config():
    assert lora.peft_key(3, "q_proj", "A") == "base_model.model.model.layers.3.self_attn.q_proj.lora_A.weight"
    assert lora.runtime_name(0, "o_proj", "B") == "model.layers.0.self_attn.o_proj.lora_B.default.weight"
    cfg = lora.adapter_config(lora.validate(16, 32, 0.05, ["q_proj", "v_proj"]))
    want = {"peft_type": "LORA", "r": 16, "lora_alpha": 32.0, "lora_dropout": 0.05, "target_modules": ["q_proj", "v_proj"],
            "bias": "none", "task_type": "CAUSAL_LM", "use_rslora": False, "use_dora": False}
    assert {k: cfg[k] for k in want} == want


def _cpu_model(layers=2):
    from vggt_qwen3_amd.qwen3 import Qwen3Config, Qwen3ForCausalLM
    cfg = Qwen3Config(hidden_size=256, num_hidden_layers=layers, num_attention_heads=4, num_key_value_heads=2, head_dim=128,
                      intermediate_size=256, vocab_size=128)
    return Qwen3ForCausalLM(cfg, device="cpu", seed=0)


def test_init_bounds_names_and_freezing():
    m = _cpu_model()
    assert lora.init_bounds(2560) == pytest.approx(1 / math.sqrt(2560))
    lo = m.enable_lora(r=16, alpha=32, dropout=0.05, target_modules=["q_proj", "k_proj", "v_proj", "o_proj"], seed=1)
    named = dict(m.named_parameters())
    for i, t, w in lo.named():
        p = named[lora.runtime_name(i, t, w)]
        assert p.requires_grad
        a = lo.tensor(lo.master, i, t, w)
        if w == "A":
            b = lora.init_bounds(a.shape[1])
            assert a.shape[0] == 16 and a.abs().max() <= b and a.abs().max() > 0.9 * b
        else:
            assert a.shape[1] == 16 and not a.any()
    assert named["model.layers.0.self_attn.q_proj.lora_A.default.weight"].shape == (16, 256)
    assert named["model.layers.1.self_attn.k_proj.lora_B.default.weight"].shape == (2 * 128, 16)
    assert named["model.layers.1.self_attn.o_proj.lora_A.default.weight"].shape == (16, 4 * 128)
    frozen = [n for n, p in named.items() if ".lora_" not in n]
    assert frozen and not any(named[n].requires_grad for n in frozen)
    # the compute copy is the masters rounded to bf16
    assert torch.equal(lo.w, lo.master.to(torch.bfloat16))


def test_enable_twice_and_merge_without_adapters():
    m = _cpu_model(1)
    with pytest.raises(RuntimeError):
        m.merge_lora()
    m.enable_lora(r=8, target_modules=["q_proj"])
    with pytest.raises(RuntimeError):
        m.enable_lora(r=8, target_modules=["v_proj"])
