"""LoRA adapters on the Qwen3 attention projections (vggt_qwen3_amd/lora.py, csrc/lora.hip) on the GPU: the kernels against fp32 torch,
their dropout masks against vq3_dropout, bit-reproducibility, and the model with adapters against the CPU oracle on W + s B A."""
import pytest
import torch

from tests.golden_io import bf16, load, meta, weights

pytestmark = pytest.mark.gpu
BF16, F32 = torch.bfloat16, torch.float32


@pytest.fixture(scope="module")
def ops():
    from vggt_qwen3_amd import _lib
    from vggt_qwen3_amd import ops as _ops
    _lib.load()
    return _ops


def relerr(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


def _rnd(*shape, scale=1.0, g=None):
    return (torch.randn(*shape, generator=g) * scale).to(BF16).cuda()


@pytest.mark.parametrize("M", [1, 3, 8, 37, 200])
@pytest.mark.parametrize("r", [8, 16, 24, 64])
def test_down_up_wgrad_vs_fp32(ops, M, r):
    """q | k | v row blocks of a fused projection (the k block without an adapter, as stage 2's q, v, o): down, block up-add, the
    backward's dV, masked-free dX and dA / dB against fp32 torch on the same bf16 operands."""
    g = torch.Generator().manual_seed(M * 100 + r)
    K, nq, nk, nv = 256, 128, 64, 64
    X = _rnd(M, K, g=g)
    A = _rnd(2 * r, K, scale=0.1, g=g)                       # q and v targets
    Bq, Bv = _rnd(nq, r, scale=0.1, g=g), _rnd(nv, r, scale=0.1, g=g)
    s = 2.0
    U = ops.lora_down(X, [dict(w=A[:r], k=K, u_col0=0), dict(w=A[r:], k=K, u_col0=r)], r)
    Uref = X.float() @ A.float().t()
    assert relerr(U, Uref) < 1e-2
    Y0 = _rnd(M, nq + nk + nv, g=g)
    Y = Y0.clone()
    ops.lora_up_add(Y, U, [dict(w=Bq, y_col0=0, n=nq, u_col0=0), dict(w=Bv, y_col0=nq + nk, n=nv, u_col0=r)], r, s)
    ref = Y0.float().clone()
    ref[:, :nq] += s * U[:, :r].float() @ Bq.float().t()
    ref[:, nq + nk:] += s * U[:, r:].float() @ Bv.float().t()
    assert relerr(Y, ref) < 1e-2
    assert torch.equal(Y[:, nq:nq + nk], Y0[:, nq:nq + nk])              # the k block is untouched
    # backward: dV = dY_t . B_t (B k-major), dX += s dV . A, dB = s dY^T U, dA = s dV^T X
    dY = _rnd(M, nq + nk + nv, g=g)
    dV = ops.lora_down(dY, [dict(w=Bq, kmajor=1, ldw=r, x_col0=0, k=nq, u_col0=0),
                            dict(w=Bv, kmajor=1, ldw=r, x_col0=nq + nk, k=nv, u_col0=r)], r)
    dVref = torch.cat([dY[:, :nq].float() @ Bq.float(), dY[:, nq + nk:].float() @ Bv.float()], 1)
    assert relerr(dV, dVref) < 1e-2
    dX0 = _rnd(M, K, g=g)
    dX = dX0.clone()
    ops.lora_up_add(dX, dV, [dict(w=A[:r], kmajor=1, ldw=K, n=K, u_col0=0), dict(w=A[r:], kmajor=1, ldw=K, n=K, u_col0=r)], r, s)
    assert relerr(dX, dX0.float() + s * dV.float() @ A.float()) < 1e-2
    gB = torch.zeros((nq + nv) * r, device="cuda", dtype=F32)
    ops.lora_wgrad(dY, U, [dict(y_col0=0, n=nq, x_col0=0, k=r, u_col0=0), dict(y_col0=nq + nk, n=nv, x_col0=r, k=r, u_col0=nq * r)],
                   gB, alpha=s)
    gBref = torch.cat([(s * dY[:, :nq].float().t() @ U[:, :r].float()).reshape(-1),
                       (s * dY[:, nq + nk:].float().t() @ U[:, r:].float()).reshape(-1)])
    assert relerr(gB, gBref) < 1e-3
    gA = torch.zeros(2 * r * K, device="cuda", dtype=BF16)
    ops.lora_wgrad(dV, X, [dict(y_col0=0, n=r, k=K, u_col0=0), dict(y_col0=r, n=r, k=K, u_col0=r * K)], gA, alpha=s)
    assert relerr(gA, (s * dV.float().t() @ X.float()).reshape(-1)) < 1e-2


def test_merge_shape_and_kmajor_down(ops):
    """The merge form of up-add (M = out_features, W += s B . A) and a down-projection whose narrow operand is k-major."""
    g = torch.Generator().manual_seed(3)
    out_f, in_f, r, s = 192, 320, 16, 0.5
    W0 = _rnd(out_f, in_f, g=g)
    A, B = _rnd(r, in_f, scale=0.1, g=g), _rnd(out_f, r, scale=0.1, g=g)
    W = W0.clone()
    ops.lora_up_add(W, B, [dict(w=A, kmajor=1, ldw=in_f, n=in_f)], r, s)
    assert relerr(W, W0.float() + s * B.float() @ A.float()) < 1e-2
    X = _rnd(50, in_f, g=g)
    At = A.t().contiguous()                                 # [in, r]: k-major
    U1 = ops.lora_down(X, [dict(w=A, k=in_f)], r)
    U2 = ops.lora_down(X, [dict(w=At, kmajor=1, ldw=r, k=in_f)], r)
    assert torch.equal(U1, U2)


def test_masks_equal_dropout_and_are_independent(ops):
    """With A = identity the down-projection returns the masked operand itself: bit-equal to ops.dropout_ at the target's offset,
    and two targets at different offsets draw different masks. The masked dX and dA use the same decisions."""
    M, K, r, p, seed = 40, 8, 8, 0.3, 1234
    X = _rnd(M, K, g=torch.Generator().manual_seed(0))
    eye = torch.eye(r, K).to(BF16).cuda()
    offs = [17, 17 + M * K]
    U = ops.lora_down(X, [dict(w=eye, k=K, u_col0=0, mask=1, mask_offset=offs[0]),
                          dict(w=eye, k=K, u_col0=r, mask=1, mask_offset=offs[1])], r, p=p, seed=seed)
    for t in range(2):
        ref = ops.dropout_(X.clone(), p, seed, offs[t])
        assert torch.equal(U[:, t * r:(t + 1) * r], ref), t
    assert not torch.equal(U[:, :r] == 0, U[:, r:] == 0)
    # dX += mask o (s dV . A): with A = I, s = 1 and dX = 0 it is the mask applied to dV (scaled by 1 / (1 - p))
    dV = _rnd(M, r, g=torch.Generator().manual_seed(1))
    dX = torch.zeros(M, K, device="cuda", dtype=BF16)
    ops.lora_up_add(dX, dV, [dict(w=eye, kmajor=1, ldw=K, n=K, mask=1, mask_offset=offs[0])], r, 1.0, p=p, seed=seed, mask_ld=K)
    assert torch.equal(dX, ops.dropout_(dV.clone(), p, seed, offs[0]))
    # dA = dV^T . mask(X)
    gA = torch.zeros(r * K, device="cuda", dtype=F32)
    ops.lora_wgrad(dV, X, [dict(n=r, k=K, mask=1, mask_offset=offs[1])], gA, p=p, seed=seed)
    ref = dV.float().t() @ ops.dropout_(X.clone(), p, seed, offs[1]).float()
    assert relerr(gA, ref.reshape(-1)) < 1e-5


def test_three_launches_same_bits(ops):
    g = torch.Generator().manual_seed(9)
    M, K, r = 6000, 2560, 16
    X, dY = _rnd(M, K, g=g), _rnd(M, 1024, g=g)
    A, B = _rnd(3 * r, K, scale=0.05, g=g), _rnd(1024, r, scale=0.05, g=g)
    outs = []
    for _ in range(3):
        U = ops.lora_down(X, [dict(w=A[k * r:(k + 1) * r], k=K, u_col0=k * r, mask=1, mask_offset=k * M * K) for k in range(3)], r,
                          p=0.05, seed=5)
        gB = torch.zeros(1024 * r, device="cuda", dtype=F32)
        ops.lora_wgrad(dY, U, [dict(n=1024, k=r)], gB, alpha=2.0)
        gA = torch.zeros(3 * r * K, device="cuda", dtype=F32)
        ops.lora_wgrad(U, X, [dict(y_col0=k * r, n=r, k=K, u_col0=k * r * K, mask=1, mask_offset=k * M * K) for k in range(3)], gA,
                       p=0.05, seed=5)
        outs.append((U, gB, gA))
    for o in outs[1:]:
        for a, b in zip(o, outs[0]):
            assert torch.equal(a, b)


def _tiny():
    from tests.test_parity_gpu import _tiny_qcfg
    from vggt_qwen3_amd.qwen3 import Qwen3ForCausalLM
    z = load("qwen3_tiny.npz")
    m = Qwen3ForCausalLM(_tiny_qcfg(meta(z, "config")), device="cuda", seed=None)
    m.load_hf_state_dict(weights(z))
    return m, z


def test_zero_B_forward_is_bit_identical():
    base, z = _tiny()
    lm, _ = _tiny()
    lm.enable_lora(r=16, alpha=32, dropout=0.0, target_modules=["q_proj", "k_proj", "v_proj", "o_proj"])
    emb = bf16(z["inputs_embeds"]).cuda()
    mask = torch.from_numpy(z["attention_mask"]).cuda()
    h0, _ = base.forward_hidden(emb, mask, save=False)
    h1, _ = lm.forward_hidden(emb, mask, save=False)
    assert torch.equal(h0, h1)


def _set_random_B(lm, seed=0, scale=0.05):
    lo = lm.lora
    g = torch.Generator().manual_seed(seed)
    for i, t, w in lo.named():
        if w == "B":
            dst = lo.tensor(lo.master, i, t, w)
            dst.copy_((torch.randn(dst.shape, generator=g) * scale).cuda())
    lo.sync_compute_copy()


@pytest.mark.parametrize("targets", [["q_proj", "k_proj", "v_proj", "o_proj"], ["q_proj", "v_proj", "o_proj"]])
def test_tiny_golden_loss_and_adapter_grads_vs_oracle(targets):
    """Without dropout LoRA is the base model with W_eff = W + s B A: the CPU oracle on that state dict (A, B fp32 leaves) gives the
    loss and, through autograd, every dA / dB."""
    from oracle import qwen3 as oq
    from vggt_qwen3_amd.lora import runtime_name
    lm, z = _tiny()
    c = meta(z, "config")
    r, alpha = 8, 16.0
    lo = lm.enable_lora(r=r, alpha=alpha, dropout=0.0, target_modules=targets, seed=3)
    _set_random_B(lm)
    emb = bf16(z["inputs_embeds"]).cuda()
    mask = torch.from_numpy(z["attention_mask"]).cuda()
    labels = torch.from_numpy(z["labels"]).cuda()
    B, L, H = emb.shape
    h_last, saved = lm.forward_hidden(emb, mask, save=True)
    loss, head = lm.loss_head(h_last, labels, save=True, L=saved["L"])
    dh = lm.backward_loss_head(head, B * saved["L"], 1.0, accumulate=False)
    lm.backward_hidden(saved, dh, accumulate=False)
    # oracle
    sd = {n: p.detach().float().cpu() for n, p in lm.named_parameters() if ".lora_" not in n}
    leaves = {}
    s = alpha / r
    for i, t, w in lo.named():
        leaves[(i, t, w)] = lo.tensor(lo.w, i, t, w).detach().float().cpu().requires_grad_(True)
    for i in range(c["num_hidden_layers"]):
        for t in targets:
            k = f"model.layers.{i}.self_attn.{t}.weight"
            sd[k] = sd[k] + s * leaves[(i, t, "B")] @ leaves[(i, t, "A")]
    ocfg = oq.Qwen3Cfg(hidden_size=c["hidden_size"], num_hidden_layers=c["num_hidden_layers"], num_attention_heads=c["num_attention_heads"],
                       num_key_value_heads=c["num_key_value_heads"], head_dim=c["head_dim"], intermediate_size=c["intermediate_size"],
                       vocab_size=lm.vocab, rms_norm_eps=c["rms_norm_eps"], rope_theta=c["rope_theta"])
    loss_ref, _ = oq.causal_lm(emb.float().cpu(), mask.cpu(), labels.cpu(), sd, ocfg)
    loss_ref.backward()
    assert abs(loss.item() - loss_ref.item()) < 1e-2 * abs(loss_ref.item()), (loss.item(), loss_ref.item())
    views = lm.lora_grad_views()
    bad = {}
    for (i, t, w), leaf in leaves.items():
        e = relerr(views[runtime_name(i, t, w)], leaf.grad)
        if e > 4e-2:
            bad[(i, t, w)] = e
    assert not bad, bad


def _small_vlm():
    from vggt_qwen3_amd.perceiver import PerceiverConfig
    from vggt_qwen3_amd.qwen3 import Qwen3Config
    from vggt_qwen3_amd.vlm import VGGTQwen3VLM, VisionLanguageConfig
    qcfg = Qwen3Config(hidden_size=256, num_hidden_layers=2, num_attention_heads=2, num_key_value_heads=1, head_dim=128,
                       intermediate_size=256, vocab_size=300)
    pcfg = PerceiverConfig(latent_dim=128, num_latents=16, num_heads=2, num_layers=2, ffn_dim=256, dropout=0.0)
    cfg = VisionLanguageConfig(text_model_name="synthetic", vision_ckpt_dir="none", num_vis_tokens=16, geom_tokens=4,
                               projector_cfg=pcfg, text_config=qcfg,
                               vision_config=dict(img_size=70, embed_dim=128, depth=2, dino_depth=2), device="cuda:0")
    model = VGGTQwen3VLM(cfg).train()
    B, V, L = 2, 2, 40
    g = torch.Generator().manual_seed(1)
    images = torch.rand(B, V, 3, 56, 56, generator=g)
    ids = torch.randint(1, 300, (B, L), generator=g)
    ids[:, 30:] = 0
    ids[0, 6] = model.image_id; ids[1, 9] = model.image_id
    labels = torch.full((B, L), -100); labels[0, 27:30] = ids[0, 27:30]; labels[1, 28:30] = ids[1, 28:30]
    mask = (ids != 0).long()
    geom = {"R": torch.randn(B, V, 9, generator=g), "t": torch.randn(B, V, 3, generator=g),
            "K": torch.randn(B, V, 9, generator=g), "depth_hist": torch.rand(B, V, 16, generator=g)}
    batch = (images.cuda(), {k: v.cuda() for k, v in geom.items()}, ids.cuda(), mask.cuda(), labels.cuda())
    return model, batch


def test_autograd_route_fills_adapter_grads_only():
    from vggt_qwen3_amd.lora import lora_settings_from_stage_config
    model, batch = _small_vlm()
    kw = lora_settings_from_stage_config({"lora": {"enable": True, "rank": 16, "alpha": 32, "dropout": 0.05,
                                                   "target_modules": ["q_proj", "k_proj", "v_proj", "o_proj"]}})
    model.enable_lora(**kw)
    names = [n for n, p in model.named_parameters() if p.requires_grad and n.startswith("text_model.")]
    assert names and all(".lora_" in n for n in names)
    assert "text_model.model.layers.1.self_attn.o_proj.lora_B.default.weight" in names
    tm = model.text_model
    base_before = tm.flat_w.clone()
    loss = model(*batch)
    loss.backward()
    for n, p in model.text_model.named_parameters():
        if ".lora_" in n:
            assert p.grad is not None and p.grad.data_ptr() in {v.data_ptr() for v in tm.lora_grad_views().values()}
        else:
            assert p.grad is None and not p.requires_grad, n
    # lora_B = 0 at init: dB carries the signal, dA is exactly zero (dV = dY . B = 0)
    gB = [p.grad for n, p in tm.named_parameters() if ".lora_B" in n]
    gA = [p.grad for n, p in tm.named_parameters() if ".lora_A" in n]
    assert all(torch.isfinite(g.float()).all() for g in gB) and any(g.float().abs().sum() > 0 for g in gB)
    assert all(g.float().abs().sum() == 0 for g in gA)
    # a second backward accumulates into the live views
    g1 = tm.lora.g.clone()
    loss2 = model(*batch)
    loss2.backward()
    assert not torch.equal(tm.lora.g, g1)
    assert torch.equal(tm.flat_w, base_before)


def test_save_load_adapter_round_trip(tmp_path):
    import json
    from safetensors.torch import load_file
    from vggt_qwen3_amd.checkpoint import load_lora_adapter, save_lora_adapter
    lm, _ = _tiny()
    lo = lm.enable_lora(r=16, alpha=32, dropout=0.05, target_modules=["q_proj", "v_proj", "o_proj"], seed=4)
    _set_random_B(lm, seed=2)
    save_lora_adapter(lm, tmp_path)
    cfg = json.loads((tmp_path / "adapter_config.json").read_text())
    assert cfg["peft_type"] == "LORA" and cfg["r"] == 16 and cfg["lora_alpha"] == 32
    sd = load_file(str(tmp_path / "adapter_model.safetensors"))
    assert all(v.dtype == F32 for v in sd.values())
    assert "base_model.model.model.layers.0.self_attn.v_proj.lora_B.weight" in sd
    lm2, _ = _tiny()
    load_lora_adapter(lm2, tmp_path)
    assert torch.equal(lm2.lora.master, lo.master) and torch.equal(lm2.lora.w, lo.w)


def test_merge_matches_unmerged_logits():
    lm, z = _tiny()
    lm.enable_lora(r=16, alpha=32, dropout=0.0, target_modules=["q_proj", "k_proj", "v_proj", "o_proj"])
    _set_random_B(lm, seed=5, scale=0.1)
    emb = bf16(z["inputs_embeds"]).cuda()
    mask = torch.from_numpy(z["attention_mask"]).cuda()
    h0, _ = lm.forward_hidden(emb, mask, save=False)
    l0 = lm.logits_all(h0)
    base, _ = _tiny()
    hb, _ = base.forward_hidden(emb, mask, save=False)
    lm.merge_lora()
    assert not lm.lora_frozen
    h1, _ = lm.forward_hidden(emb, mask, save=False)
    l1 = lm.logits_all(h1)
    valid = mask.reshape(-1).bool()
    assert relerr(l1[valid], l0[valid]) < 1e-2
    assert relerr(base.logits_all(hb)[valid], l0[valid]) > 3e-2       # the adapters did change the model


def test_generate_unmerged_and_merged_persistent():
    """Unmerged adapters decode on the per-projection route, merged ones on the persistent kernel (B = 1, Qwen3-4B width, 2 layers):
    each pick is the argmax of a cache-free forward of the same model over prompt + generated tokens, up to the bf16 near-tie rule."""
    from tests.test_generate_gpu import TIE_TOL, _qwen4b_dims
    from vggt_qwen3_amd import ops
    tm, cfg = _qwen4b_dims(2)
    tm.eval()
    tm.enable_lora(r=16, alpha=32, dropout=0.05, target_modules=["q_proj", "k_proj", "v_proj", "o_proj"])
    _set_random_B(tm, seed=8, scale=0.05)
    torch.manual_seed(7)
    L = 40
    emb = (torch.randn(1, L, cfg.hidden_size) * 0.5).to(BF16).cuda()
    mask = torch.ones(1, L, dtype=torch.long).cuda()

    def check(out):
        full = torch.cat([emb, tm.get_input_embeddings()(out[:, :-1])], dim=1)
        h, _ = tm.forward_hidden(full, torch.ones(1, full.shape[1], dtype=torch.long).cuda(), save=False)
        logits = tm.logits_all(h).view(1, h.shape[0], -1).float()
        for t in range(out.shape[1]):
            row = logits[:, L - 1 + t]
            assert ((row.max(-1).values - row.gather(1, out[:, t][:, None]).squeeze(1)) < TIE_TOL).all(), t

    out, stats = tm.generate(inputs_embeds=emb, attention_mask=mask, max_new_tokens=6, return_stats=True)
    assert not stats["persistent"]
    check(out)
    tm.merge_lora()
    out2, stats2 = tm.generate(inputs_embeds=emb, attention_mask=mask, max_new_tokens=6, return_stats=True)
    if ops.decode_layers_supported(2560, 9728, 32, 8, 128, 128):
        assert stats2["persistent"]
    check(out2)


def test_rejections_on_the_gpu_model():
    lm, _ = _tiny()
    with pytest.raises(NotImplementedError):
        lm.enable_lora(r=8, target_modules=["gate_proj"])
    with pytest.raises(ValueError):
        lm.enable_lora(r=12, target_modules=["q_proj"])
    lm.enable_lora(r=8, target_modules=["q_proj"])
    with pytest.raises(NotImplementedError):
        lm.enable_fp8_forward(True)
    model, _ = _small_vlm()
    model.enable_lora(r=8, target_modules=["q_proj"])
    from vggt_qwen3_amd.trainer import Stage1Trainer
    with pytest.raises(NotImplementedError):
        Stage1Trainer(model, grad_accum=1, dp_mode="sharded")


def test_down_k_tail_and_unaligned_rows(ops):
    """K not a multiple of the 32-wide chunk and an X that starts 3 elements into its rows (the scalar load path), with dropout."""
    g = torch.Generator().manual_seed(11)
    M, K, r = 45, 100, 16
    big = _rnd(M, K + 7, g=g)
    X = big[:, 3:3 + K]
    A = _rnd(2 * r, K, scale=0.1, g=g)
    U = ops.lora_down(X, [dict(w=A[:r], k=K, u_col0=0, mask=1, mask_offset=5), dict(w=A[r:], k=K, u_col0=r, mask=1, mask_offset=5 + M * K)],
                      r, p=0.1, seed=77, mask_ld=K)
    ref = torch.cat([ops.dropout_(X.contiguous(), 0.1, 77, 5).float() @ A[:r].float().t(),
                     ops.dropout_(X.contiguous(), 0.1, 77, 5 + M * K).float() @ A[r:].float().t()], 1)
    assert relerr(U, ref) < 1e-2


def test_dropout_offsets_advance_and_backward_uses_the_saved_masks():
    """With dropout two training forwards draw different masks; the backward of the first uses the first forward's masks even after a
    second forward ran (same adapter gradients as a model that ran only the first forward); eval mode applies no dropout."""
    def make():
        lm, z = _tiny()
        lm.enable_lora(r=8, alpha=16, dropout=0.3, target_modules=["q_proj", "v_proj", "o_proj"], seed=1)
        _set_random_B(lm, seed=3, scale=0.1)
        return lm, z
    lm, z = make()
    emb = bf16(z["inputs_embeds"]).cuda()
    mask = torch.from_numpy(z["attention_mask"]).cuda()
    labels = torch.from_numpy(z["labels"]).cuda()
    B = emb.shape[0]
    h1, s1 = lm.forward_hidden(emb, mask, save=True)
    h2, s2 = lm.forward_hidden(emb, mask, save=True)
    assert not torch.equal(h1, h2)
    assert s1["layers"][0]["lora_qkv"]["offs"] != s2["layers"][0]["lora_qkv"]["offs"]
    loss, head = lm.loss_head(h1, labels, save=True, L=s1["L"])
    lm.backward_hidden(s1, lm.backward_loss_head(head, B * s1["L"], 1.0, accumulate=False), accumulate=False)
    ref, _ = make()
    hr, sr = ref.forward_hidden(emb, mask, save=True)
    assert torch.equal(hr, h1)
    lr_, headr = ref.loss_head(hr, labels, save=True, L=sr["L"])
    ref.backward_hidden(sr, ref.backward_loss_head(headr, B * sr["L"], 1.0, accumulate=False), accumulate=False)
    assert torch.equal(lm.lora.g, ref.lora.g) and lm.lora.g.abs().sum() > 0
    lm.eval()
    he1, _ = lm.forward_hidden(emb, mask, save=False)
    he2, _ = lm.forward_hidden(emb, mask, save=False)
    assert torch.equal(he1, he2)


def test_torch_optimizer_trains_the_fp32_masters_and_save_load_keeps_them(tmp_path):
    """The adapter parameters are the fp32 masters: an optimiser over lora_parameters() updates them, the next forward follows, and
    save / load round-trips the trained values bit-exactly."""
    from vggt_qwen3_amd.checkpoint import load_lora_adapter, save_lora_adapter
    lm, z = _tiny()
    lm.enable_lora(r=8, alpha=16, dropout=0.0, target_modules=["q_proj", "k_proj", "v_proj", "o_proj"], seed=2)
    params = lm.lora_parameters()
    assert all(p.dtype == F32 for p in params)
    opt = torch.optim.SGD(params, lr=1.0)
    emb = bf16(z["inputs_embeds"]).cuda()
    mask = torch.from_numpy(z["attention_mask"]).cuda()
    labels = torch.from_numpy(z["labels"]).cuda()
    B = emb.shape[0]
    h0, _ = lm.forward_hidden(emb, mask, save=False)
    for _ in range(2):
        h, s = lm.forward_hidden(emb, mask, save=True)
        loss, head = lm.loss_head(h, labels, save=True, L=s["L"])
        lm.backward_hidden(s, lm.backward_loss_head(head, B * s["L"], 1.0, accumulate=False), accumulate=False)
        lm.publish_grads()
        assert all(p.grad is not None and p.grad.dtype == F32 for p in params)
        opt.step()
    assert lm.lora.master.abs().sum() > 0
    h1, _ = lm.forward_hidden(emb, mask, save=False)
    assert not torch.equal(h0, h1)                                 # the forward follows the trained masters
    assert torch.equal(lm.lora.w, lm.lora.master.to(BF16))
    save_lora_adapter(lm, tmp_path)
    lm2, _ = _tiny()
    load_lora_adapter(lm2, tmp_path)
    assert torch.equal(lm2.lora.master, lm.lora.master)
    h2, _ = lm2.forward_hidden(emb, mask, save=False)
    assert torch.equal(h2, h1)


def test_merge_unloads_the_adapters(tmp_path):
    """After merge_lora() the adapter modules are gone (plain HF keys in state_dict and in save_model's files) and the base trains."""
    from vggt_qwen3_amd.checkpoint import checkpoint_items
    model, _ = _small_vlm()
    model.enable_lora(r=8, alpha=16, target_modules=["q_proj", "o_proj"])
    assert any(".lora_" in k for k in model.state_dict())
    model.merge_lora()
    assert not any(".lora_" in k for k in model.state_dict())
    assert not any(".lora_" in k for k, _ in checkpoint_items(model))
    assert all(p.requires_grad for p in model.text_model.parameters())


def _trainer(dropout=0.05, seed=0):
    from tests.test_trainer_gpu import _vlm
    from vggt_qwen3_amd.trainer import Stage1Trainer
    z, m, build, batch = _vlm()
    model = build()
    model.enable_lora(r=16, alpha=32, dropout=dropout, target_modules=["q_proj", "k_proj", "v_proj", "o_proj"], seed=seed)
    tr = Stage1Trainer(model, lr=1e-3, proj_lr=1e-3, weight_decay=0.1, warmup_ratio=0.0, max_steps=100, grad_accum=2,
                       max_grad_norm=None)
    return model, tr, batch


def test_stage1_trainer_with_lora():
    """Stage1Trainer with adapters: the base (flat_w) is bit-identical after the steps and has no fp32 master; the adapters and
    geom_head moved; the adapter AdamW equals torch.optim.AdamW fed the same gradients; two identical runs leave identical bits."""
    model, tr, batch = _trainer()
    tm = model.text_model
    w0 = tm.flat_w.clone()
    geom0 = [p.detach().clone() for p in model.geom_head.parameters()]
    assert tr.master.data_ptr() == tm.lora.master.data_ptr() and tr.m.numel() == tm.lora.numel < tm.flat_w.numel()
    for _ in range(4):
        tr.micro_step(batch)
    tr.sync_optimizer()
    assert torch.equal(tm.flat_w, w0)
    assert not torch.equal(tm.lora.master[tm.lora.table["l0.B_q_proj"][0]:][:100], torch.zeros(100, device="cuda"))
    assert any(not torch.equal(p, q) for p, q in zip(model.geom_head.parameters(), geom0))
    # one more window against torch.optim.AdamW on a copy of the state, fed this window's gradient
    master0, m0, v0 = tr.master.clone(), tr.m.clone(), tr.v.clone()
    tr.micro_step(batch)
    tr.micro_step(batch)
    tr.sync_optimizer()
    g = tm.lora.g.to(BF16).float()
    ref = torch.nn.Parameter(master0.clone())
    opt = torch.optim.AdamW([ref], lr=tr.lr * tr.lr_mult(tr.opt_step), betas=tr.betas, eps=tr.eps, weight_decay=tr.wd)
    opt.state[ref] = {"step": torch.tensor(float(tr.opt_step - 1)), "exp_avg": m0.clone(), "exp_avg_sq": v0.clone()}
    ref.grad = g
    opt.step()
    assert relerr(tr.master, ref.detach()) < 1e-5
    assert torch.equal(tm.lora.w, tm.lora.master.to(BF16))
    # two identical runs (dropout on) leave identical bits
    runs = []
    for _ in range(2):
        model2, tr2, batch2 = _trainer()
        for _ in range(4):
            tr2.micro_step(batch2)
        tr2.sync_optimizer()
        runs.append(model2.text_model.lora.master.clone())
    assert torch.equal(runs[0], runs[1])


def test_stage1_trainer_lora_state_round_trip(tmp_path):
    from vggt_qwen3_amd.checkpoint import load_trainer_state, save_trainer_state
    model, tr, batch = _trainer(dropout=0.0)
    for _ in range(2):
        tr.micro_step(batch)
    tr.sync_optimizer()
    save_trainer_state(tr, tmp_path)
    model2, tr2, _ = _trainer(dropout=0.0)
    load_trainer_state(tr2, tmp_path)
    assert torch.equal(tr2.master, tr.master) and torch.equal(tr2.m, tr.m) and torch.equal(tr2.v, tr.v)
    assert torch.equal(model2.text_model.lora.w, model.text_model.lora.w)
