"""LoRA adapters on the Qwen3 attention projections, as peft.get_peft_model(text_model, LoraConfig(r, lora_alpha, lora_dropout,
target_modules)) gives them to the reference (its stage configs' `lora:` block, configs/stage1_3d.yaml / stage2_arkit.yaml):

    y = base(x) + lora_B(lora_A(dropout(x))) * (alpha / r)       (peft tuners/lora/layer.py, lora.Linear.forward)

lora_A [r, in] ~ U(-1/sqrt(in), 1/sqrt(in)) (kaiming_uniform_(a=sqrt(5))), lora_B [out, r] = 0; no bias, rsLoRA or DoRA; one dropout
mask per target, in training mode only. Every base parameter of the text model is frozen.

Storage: one flat buffer per kind - `master` f32 (peft keeps fp32 adapters next to a bf16 base; the adapter parameters ARE views of
it, so any optimiser updates the fp32 values), `w` bf16 (the compute copy the kernels read, re-derived from `master` before a forward
whenever the masters were written through torch), `g` f32 (the gradient; the parameters' .grad are views of it).
Per layer: [A_attn | B_q | B_k | B_v | A_o | B_o] for the targets present, A_attn being the row-concatenation of the q/k/v targets' lora_A: q, k and v are one fused weight (l{i}.qkv), so one
down-projection launch reads the normalised input once for all three (csrc/lora.hip).
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

import torch

from . import ops
from .ops import BF16, F32, round_up

ATTN_TARGETS = ("q_proj", "k_proj", "v_proj", "o_proj")
MLP_TARGETS = ("gate_proj", "up_proj", "down_proj")
MAX_RANK = 64


@dataclass
class LoraSettings:
    r: int = 16
    alpha: float = 32.0
    dropout: float = 0.05
    target_modules: List[str] = field(default_factory=lambda: list(ATTN_TARGETS))

    @property
    def scaling(self) -> float:
        return self.alpha / self.r


def validate(r, alpha, dropout, target_modules) -> LoraSettings:
    """The supported subset of peft's LoraConfig; anything else is rejected rather than silently trained differently."""
    tm = list(target_modules)
    if not tm:
        raise ValueError("LoRA: target_modules is empty")
    for t in tm:
        if t in MLP_TARGETS:
            raise NotImplementedError(f"LoRA on the MLP projection {t!r} is not implemented (supported: {', '.join(ATTN_TARGETS)})")
        if t not in ATTN_TARGETS:
            raise ValueError(f"LoRA: unknown target module {t!r} (supported: {', '.join(ATTN_TARGETS)})")
    if len(set(tm)) != len(tm):
        raise ValueError(f"LoRA: repeated target modules in {tm}")
    if int(r) != r or r < 8 or r > MAX_RANK or int(r) % 8:
        raise ValueError(f"LoRA: rank r must be a multiple of 8 in [8, {MAX_RANK}], got {r}")
    if not 0.0 <= float(dropout) < 1.0:
        raise ValueError(f"LoRA: dropout must be in [0, 1), got {dropout}")
    ordered = [t for t in ATTN_TARGETS if t in tm]
    return LoraSettings(r=int(r), alpha=float(alpha), dropout=float(dropout), target_modules=ordered)


def lora_settings_from_stage_config(cfg) -> Optional[dict]:
    """The reference's stage-config `lora:` block ({enable, rank, alpha, dropout, target_modules}) -> keyword arguments of
    enable_lora(), or None when the block is absent or `enable` is false. `cfg`: the loaded YAML mapping."""
    block = (cfg or {}).get("lora")
    if not block or not block.get("enable", False):
        return None
    s = validate(block.get("rank", block.get("r", 8)), block.get("alpha", block.get("lora_alpha", 8)),
                 block.get("dropout", block.get("lora_dropout", 0.0)), block.get("target_modules", ["q_proj", "v_proj"]))
    return dict(r=s.r, alpha=s.alpha, dropout=s.dropout, target_modules=list(s.target_modules))


def peft_key(layer: int, target: str, which: str) -> str:
    """Key of an adapter tensor in peft's adapter_model.safetensors for a Qwen3ForCausalLM base."""
    return f"base_model.model.model.layers.{layer}.self_attn.{target}.lora_{which}.weight"


def runtime_name(layer: int, target: str, which: str) -> str:
    """peft's parameter name at run time (the adapter named "default"), relative to the text model."""
    return f"model.layers.{layer}.self_attn.{target}.lora_{which}.default.weight"


def adapter_config(s: LoraSettings) -> dict:
    return {"peft_type": "LORA", "task_type": "CAUSAL_LM", "r": s.r, "lora_alpha": s.alpha, "lora_dropout": s.dropout,
            "target_modules": list(s.target_modules), "bias": "none", "use_rslora": False, "use_dora": False,
            "fan_in_fan_out": False, "modules_to_save": None, "inference_mode": False}


def init_bounds(in_features: int) -> float:
    """kaiming_uniform_(a=sqrt(5)) on [r, in]: gain sqrt(2 / (1 + 5)), bound gain * sqrt(3 / in) = 1 / sqrt(in)."""
    return 1.0 / math.sqrt(in_features)


class LoraAdapters:
    """The adapter state of one Qwen3ForCausalLM (built by Qwen3ForCausalLM.enable_lora)."""

    def __init__(self, tm, settings: LoraSettings, seed: int = 0):
        c = tm.config
        self.s = settings
        self.r = settings.r
        self.scale = settings.scaling
        self.p = settings.dropout
        H, D = c.hidden_size, tm.D
        self.H, self.Ho = H, tm.Hq * D
        # q | k | v row blocks of the fused weight
        blocks = {"q_proj": (0, tm.Hq * D), "k_proj": (tm.Hq * D, tm.Hkv * D), "v_proj": ((tm.Hq + tm.Hkv) * D, tm.Hkv * D)}
        self.attn = [(t, blocks[t][0], blocks[t][1]) for t in settings.target_modules if t in blocks]     # (name, row0, rows)
        self.has_o = "o_proj" in settings.target_modules
        self.layers = c.num_hidden_layers
        r = self.r
        ent: List[Tuple[str, Tuple[int, int]]] = []
        for i in range(self.layers):
            if self.attn:
                ent.append((f"l{i}.A_attn", (len(self.attn) * r, H)))
                for t, _, n in self.attn:
                    ent.append((f"l{i}.B_{t}", (n, r)))
            if self.has_o:
                ent += [(f"l{i}.A_o", (r, self.Ho)), (f"l{i}.B_o", (H, r))]
        self.table: Dict[str, Tuple[int, Tuple[int, int]]] = {}
        off = 0
        for name, shape in ent:
            self.table[name] = (off, shape)
            off += round_up(math.prod(shape), 64)
        self.numel = off
        dev = tm.device_
        self.master = torch.zeros(off, device=dev, dtype=F32)
        self.w = torch.zeros(off, device=dev, dtype=BF16)
        self.g = torch.zeros(off, device=dev, dtype=F32)
        g = torch.Generator().manual_seed(seed)
        for name, (o, shape) in self.table.items():
            if ".A_" in name:          # every lora_A: U(-1/sqrt(in), 1/sqrt(in)); lora_B stays zero (peft's init_lora_weights=True)
                bound = init_bounds(shape[1])
                self.master[o:o + math.prod(shape)].copy_((torch.rand(shape, generator=g, dtype=torch.float64) * 2 - 1).mul_(bound)
                                                          .to(F32).reshape(-1))
        self.sync_compute_copy()
        self.active = True
        self.drop_seed = (seed * 0x9E3779B1 + 0x5EED) & (2 ** 63 - 1)
        self.drop_offset = 0

    # -------------------------------------------------------------- views
    def _view(self, buf: torch.Tensor, name: str) -> torch.Tensor:
        o, shape = self.table[name]
        return buf[o:o + math.prod(shape)].view(shape)

    def wv(self, name):
        return self._view(self.w, name)

    def gv(self, name):
        return self._view(self.g, name)

    def mv(self, name):
        return self._view(self.master, name)

    def tensors(self, layer: int) -> Dict[Tuple[str, str], str]:
        """(target, "A" | "B") -> table name and row range: lora_A of an attention target is a row block of A_attn."""
        out = {}
        for t_idx, (t, _, _) in enumerate(self.attn):
            out[(t, "A")] = (f"l{layer}.A_attn", t_idx * self.r, (t_idx + 1) * self.r)
            out[(t, "B")] = (f"l{layer}.B_{t}", None, None)
        if self.has_o:
            out[("o_proj", "A")] = (f"l{layer}.A_o", None, None)
            out[("o_proj", "B")] = (f"l{layer}.B_o", None, None)
        return out

    def tensor(self, buf: torch.Tensor, layer: int, target: str, which: str) -> torch.Tensor:
        name, lo, hi = self.tensors(layer)[(target, which)]
        v = self._view(buf, name)
        return v if lo is None else v[lo:hi]

    def named(self):
        """(layer, target, "A" | "B") for every adapter tensor, in a fixed order."""
        for i in range(self.layers):
            for t in self.s.target_modules:
                for which in ("A", "B"):
                    yield i, t, which

    def sync_compute_copy(self) -> None:
        self.w.copy_(self.master.to(BF16))
        self._synced = self.master._version

    def refresh_compute_copy(self) -> None:
        """Before a forward: the bf16 compute copy follows masters that were written through torch (an optimiser over the adapter
        parameters, a copy_) - the tensor version counter tells. Stage1Trainer's fused AdamW writes both itself."""
        if self.master._version != getattr(self, "_synced", None):
            self.sync_compute_copy()

    def zero_grad(self) -> None:
        self.g.zero_()

    # -------------------------------------------------------------- dropout streams
    def dropout_on(self, training: bool) -> bool:
        return training and self.p > 0.0

    def take_offsets(self, n_targets: int, elems: int) -> List[int]:
        """Disjoint element ranges of the counter-based hash for n masks of `elems` elements (one per target)."""
        offs = [self.drop_offset + k * elems for k in range(n_targets)]
        self.drop_offset += n_targets * elems
        return offs

    # -------------------------------------------------------------- forward
    def fwd_qkv(self, i: int, xn1: torch.Tensor, qkv: torch.Tensor, training: bool):
        """qkv += s * B_t . A_t . dropout_t(xn1) on each target's row block of the fused projection. Returns the saved state."""
        if not self.attn:
            return None
        r, H = self.r, xn1.shape[1]
        drop = self.dropout_on(training)
        offs = self.take_offsets(len(self.attn), xn1.shape[0] * H) if drop else [0] * len(self.attn)
        A = self.wv(f"l{i}.A_attn")
        down = [dict(w=A[k * r:(k + 1) * r], k=H, u_col0=k * r, mask=drop, mask_offset=offs[k]) for k in range(len(self.attn))]
        U = ops.lora_down(xn1, down, r, p=self.p if drop else 0.0, seed=self.drop_seed, mask_ld=H)
        up = [dict(w=self.wv(f"l{i}.B_{t}"), y_col0=c0, n=n, u_col0=k * r) for k, (t, c0, n) in enumerate(self.attn)]
        ops.lora_up_add(qkv, U, up, r, self.scale)
        return dict(U=U, offs=offs, drop=drop)

    def fwd_o(self, i: int, ao: torch.Tensor, h_mid: torch.Tensor, training: bool):
        """h_mid += s * B_o . A_o . dropout(ao)."""
        if not self.has_o:
            return None
        r, K = self.r, ao.shape[1]
        drop = self.dropout_on(training)
        offs = self.take_offsets(1, ao.shape[0] * K) if drop else [0]
        U = ops.lora_down(ao, [dict(w=self.wv(f"l{i}.A_o"), k=K, mask=drop, mask_offset=offs[0])], r, p=self.p if drop else 0.0,
                          seed=self.drop_seed, mask_ld=K)
        ops.lora_up_add(h_mid, U, [dict(w=self.wv(f"l{i}.B_o"), n=h_mid.shape[1])], r, self.scale)
        return dict(U=U, offs=offs, drop=drop)

    # -------------------------------------------------------------- backward
    def bwd_qkv(self, i: int, st, dqkv: torch.Tensor, xn1: torch.Tensor, d_xn1: torch.Tensor, accumulate: bool) -> None:
        """d_xn1 += sum_t mask_t o (s dV_t . A_t) with dV_t = dqkv_t . B_t; dB_t (+)= s dqkv_t^T . U_t; dA_t (+)= s dV_t^T . mask_t(xn1)."""
        if st is None:
            return
        r, H = self.r, xn1.shape[1]
        p = self.p if st["drop"] else 0.0
        n_t = len(self.attn)
        dV = ops.lora_down(dqkv, [dict(w=self.wv(f"l{i}.B_{t}"), kmajor=1, ldw=r, x_col0=c0, k=n, u_col0=k * r)
                                  for k, (t, c0, n) in enumerate(self.attn)], r, mask_ld=dqkv.shape[1])
        A = self.wv(f"l{i}.A_attn")
        ops.lora_up_add(d_xn1, dV, [dict(w=A[k * r:(k + 1) * r], kmajor=1, ldw=H, n=H, u_col0=k * r, mask=st["drop"],
                                         mask_offset=st["offs"][k]) for k in range(n_t)], r, self.scale, p=p, seed=self.drop_seed, mask_ld=H)
        # dB of every attention target in one launch: their blocks follow A_attn back to back in the gradient buffer
        b0 = self.table[f"l{i}.B_{self.attn[0][0]}"][0]
        bl = self.table[f"l{i}.B_{self.attn[-1][0]}"]
        gB = self.g[b0:bl[0] + math.prod(bl[1])]
        ops.lora_wgrad(dqkv, st["U"], [dict(y_col0=c0, n=n, x_col0=k * r, k=r, u_col0=self.table[f"l{i}.B_{t}"][0] - b0)
                                       for k, (t, c0, n) in enumerate(self.attn)], gB, alpha=self.scale, accumulate=accumulate)
        ops.lora_wgrad(dV, xn1, [dict(y_col0=k * r, n=r, k=H, u_col0=k * r * H, mask=st["drop"], mask_offset=st["offs"][k])
                                 for k in range(n_t)], self.gv(f"l{i}.A_attn").view(-1), alpha=self.scale, accumulate=accumulate,
                       p=p, seed=self.drop_seed, mask_ld=H)

    def bwd_o(self, i: int, st, dh_mid: torch.Tensor, ao: torch.Tensor, d_ao: torch.Tensor, accumulate: bool) -> None:
        if st is None:
            return
        r, K, H = self.r, ao.shape[1], dh_mid.shape[1]
        p = self.p if st["drop"] else 0.0
        dV = ops.lora_down(dh_mid, [dict(w=self.wv(f"l{i}.B_o"), kmajor=1, ldw=r, k=H)], r, mask_ld=H)
        ops.lora_up_add(d_ao, dV, [dict(w=self.wv(f"l{i}.A_o"), kmajor=1, ldw=K, n=K, mask=st["drop"], mask_offset=st["offs"][0])],
                        r, self.scale, p=p, seed=self.drop_seed, mask_ld=K)
        ops.lora_wgrad(dh_mid, st["U"], [dict(n=H, k=r)], self.gv(f"l{i}.B_o").view(-1), alpha=self.scale, accumulate=accumulate)
        ops.lora_wgrad(dV, ao, [dict(n=r, k=K, mask=st["drop"], mask_offset=st["offs"][0])], self.gv(f"l{i}.A_o").view(-1),
                       alpha=self.scale, accumulate=accumulate, p=p, seed=self.drop_seed, mask_ld=K)

    # -------------------------------------------------------------- merge
    def merge_into(self, tm) -> None:
        """W += s * B . A for every target (bf16 compute copies, f32 accumulation, one rounding per weight)."""
        r = self.r
        self.refresh_compute_copy()
        for i in range(self.layers):
            W = tm._w[f"l{i}.qkv"]
            A = self.wv(f"l{i}.A_attn") if self.attn else None
            for k, (t, c0, n) in enumerate(self.attn):
                ops.lora_up_add(W[c0:c0 + n], self.wv(f"l{i}.B_{t}"),
                                [dict(w=A[k * r:(k + 1) * r], kmajor=1, ldw=W.shape[1], n=W.shape[1])], r, self.scale)
            if self.has_o:
                Wo = tm._w[f"l{i}.o"]
                ops.lora_up_add(Wo, self.wv(f"l{i}.B_o"), [dict(w=self.wv(f"l{i}.A_o"), kmajor=1, ldw=Wo.shape[1], n=Wo.shape[1])],
                                r, self.scale)
