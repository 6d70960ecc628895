"""KV-cache sessions on the GPU: the two kernels of csrc/qwen_append.hip (a chunk of new positions against the resident cache), the
model's forward_append through extend(), and generate() / sample() with kv_cache=.
  append_qkprep  bit-equal to the prefill kernel (ops.qwen_qkprep_fwd) on the same rows, nothing written outside the chunk's rows;
  append_attn    against the fp64 reference and the per-32-row-block bound tests/test_qwen_attention_long_gpu.py holds the fused
                 forward to, NaN behind every row's last valid cache row, spiked keys on and one past the diagonal;
  extend         two chunks against the one-shot forward, both measured against the fp32 CPU oracle;
  generate       every pick of two turns under the tie rule of tests/test_generate_gpu.py against a cache-free forward."""
import pytest
import torch

from tests.test_generate_gpu import TIE_TOL, _full_forward_logits, _qwen4b_dims, _tiny_model
from tests.test_qwen_attention_long_gpu import O_TOL, _assert_blocks, attn_ref64

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
D = 128
SCALE = D ** -0.5
LMAX = 192


@pytest.fixture(scope="module")
def ops():
    from vggt_qwen3_amd import _lib
    from vggt_qwen3_amd import ops as _ops
    _lib.load()
    return _ops


def _i32(xs):
    return torch.tensor(xs, dtype=torch.int32, device="cuda")


# ------------------------------------------------------------------------------------------------ append_qkprep
@pytest.mark.parametrize("Hq,Hkv", [(8, 2), (2, 2)])
def test_append_qkprep_is_bit_equal_to_the_prefill_kernel(ops, Hq, Hkv):
    """Rows (P, n) = (0, 40), (3, 5), (37, 40), (152, 40 - ends exactly at Lmax): a whole sequence of Lmax positions goes through
    ops.qwen_qkprep_fwd; its rows P .. P+n-1 then go through the new kernel with lens = P, behind them (t >= n) junk that must be
    ignored. Q and the written cache rows equal the prefill kernel's bits, every other cache row keeps its sentinel, Q rows t >= n are 0."""
    rows = [(0, 40), (3, 5), (37, 40), (152, 40)]
    B, Ln, HT = len(rows), 40, Hq + 2 * Hkv
    g = torch.Generator().manual_seed(Hq)
    qkv_full = torch.randn(B, LMAX, HT * D, generator=g).to(BF16).cuda()
    qw = (1 + 0.2 * torch.randn(D, generator=g)).to(BF16).cuda()
    kw = (1 + 0.2 * torch.randn(D, generator=g)).to(BF16).cuda()
    ang = torch.rand(LMAX, D // 2, generator=g) * 6.28
    emb = torch.cat([ang, ang], -1)
    cos, sin = emb.cos().to(BF16).cuda().contiguous(), emb.sin().to(BF16).cuda().contiguous()
    Qr, Kr, Vr = ops.qwen_qkprep_fwd(qkv_full.view(B * LMAX, HT * D), qw, kw, cos, sin, B, LMAX, Hq, Hkv, D, 1e-6, want_rstd=False)[:3]
    chunk = torch.randn(B, Ln, HT * D, generator=g).to(BF16).cuda()              # junk wherever t >= n
    for b, (P, n) in enumerate(rows):
        chunk[b, :n] = qkv_full[b, P:P + n]
    SENT = -768.0                                                                # exact in bf16
    Kc = torch.full((B, Hkv, LMAX, D), SENT, device="cuda", dtype=BF16)
    Vc = torch.full_like(Kc, SENT)
    Q = ops.qwen_append_qkprep(chunk.view(B * Ln, HT * D), qw, kw, cos, sin, _i32([P for P, _ in rows]), _i32([n for _, n in rows]),
                               Kc, Vc, B, Ln, Hq, Hkv, D, LMAX, 1e-6)
    assert Q.shape == (B, Hq, Ln, D)
    for b, (P, n) in enumerate(rows):
        assert torch.equal(Q[b, :, :n], Qr[b, :, P:P + n]), b
        assert (Q[b, :, n:] == 0).all(), b
        assert torch.equal(Kc[b, :, P:P + n], Kr[b, :, P:P + n]) and torch.equal(Vc[b, :, P:P + n], Vr[b, :, P:P + n]), b
        keep = torch.ones(LMAX, dtype=torch.bool, device="cuda")
        keep[P:P + n] = False
        assert (Kc[b][:, keep] == SENT).all() and (Vc[b][:, keep] == SENT).all(), b


# ------------------------------------------------------------------------------------------------ append_attn
def _attn_operands(Hq, Hkv, Ln, rows, seed):
    """Random Q [B, Hq, Ln, D] (rows t >= new too: they must come out 0 all the same) and caches [B, Hkv, LMAX, D] whose rows at and
    past lens + new are NaN."""
    B = len(rows)
    g = torch.Generator().manual_seed(seed)
    Q = torch.randn(B, Hq, Ln, D, generator=g)
    Kc = torch.randn(B, Hkv, LMAX, D, generator=g)
    Vc = torch.randn(B, Hkv, LMAX, D, generator=g)
    return Q, Kc, Vc


def _poison(Kc, Vc, rows):
    for b, (n0, n) in enumerate(rows):
        Kc[b, :, n0 + n:] = float("nan")
        Vc[b, :, n0 + n:] = float("nan")


def _ref_chunk(Q, Kc, Vc, rows):
    """fp64 causal reference of the chunk: per row, the whole sequence of lens + new positions through attn_ref64 with the chunk's
    queries at its last `new` positions; [B, Hq, Ln, D], zero where t >= new."""
    B, Hq, Ln, _ = Q.shape
    ref = torch.zeros(B, Hq, Ln, D, device=Q.device, dtype=torch.float64)
    for b, (n0, n) in enumerate(rows):
        T = n0 + n
        Qf = torch.zeros(1, Hq, T, D, device=Q.device, dtype=Q.dtype)
        Qf[0, :, n0:] = Q[b, :, :n]
        mask = torch.ones(1, T, dtype=torch.uint8, device=Q.device)
        O = attn_ref64(Qf, Kc[b:b + 1, :, :T], Vc[b:b + 1, :, :T], None, mask, bwd=False)[0]
        ref[b, :, :n] = O[0, :, n0:]
    return ref


ATTN_CASES = {64: ([(0, 40), (31, 33), (32, 1), (97, 64)], (3, 1, 40), (1, 0, 10)),
              8: ([(0, 1), (63, 8), (64, 5), (184, 8)], (1, 1, 5), (3, 0, 3))}


@pytest.mark.parametrize("Hq,Hkv", [(8, 2), (2, 2)])
@pytest.mark.parametrize("Ln", [64, 8])
def test_append_attn_vs_fp64(ops, Hq, Hkv, Ln):
    """Rows (lens, new) on both sides of the 32-query block and 32-key tile edges, the last one ending at Lmax - 8 / Lmax. Cache rows
    at and past lens + new are NaN: the output is finite, rows t >= new exactly 0, live rows within the fused forward's per-block
    bound of the fp64 reference. A key of 8.5 x a query on its diagonal row saturates that query (O = that row of V within 2e-2); a
    key of 8.5 x another query one PAST its diagonal - inside the chunk - must not move it from the causal reference. Two runs agree
    bit for bit."""
    rows, diag, past = ATTN_CASES[Ln]
    B, G = len(rows), Hq // Hkv
    Q, Kc, Vc = _attn_operands(Hq, Hkv, Ln, rows, seed=Ln + Hq)
    Q = Q.to(BF16)
    b, h, t = diag
    Kc[b, h // G, rows[b][0] + t] = 8.5 * Q[b, h, t].float()
    b2, h2, t2 = past
    assert t2 + 1 < rows[b2][1]
    Kc[b2, h2 // G, rows[b2][0] + t2 + 1] = 8.5 * Q[b2, h2, t2].float()
    _poison(Kc, Vc, rows)
    Q, Kc, Vc = Q.cuda(), Kc.to(BF16).cuda(), Vc.to(BF16).cuda()
    lens, new = _i32([r[0] for r in rows]), _i32([r[1] for r in rows])
    O = ops.qwen_append_attn(Q, Kc, Vc, lens, new, B, Ln, Hq, Hkv, D, LMAX, SCALE)
    assert O.shape == (B * Ln, Hq * D)
    Oh = O.view(B, Ln, Hq, D).permute(0, 2, 1, 3)
    assert torch.isfinite(Oh.float()).all(), "O not finite: something behind a row's last valid cache row was read"
    for i, (n0, n) in enumerate(rows):
        assert (Oh[i, :, n:] == 0).all(), f"row {i}: O of a padded query must be exactly 0"
    ref = _ref_chunk(Q, Kc, Vc, rows)
    _assert_blocks("O", Oh, ref, O_TOL)
    assert (Oh[b, h, t].float() - Vc[b, h // G, rows[b][0] + t].float()).abs().max().item() < 2e-2
    O2 = ops.qwen_append_attn(Q, Kc, Vc, lens, new, B, Ln, Hq, Hkv, D, LMAX, SCALE)
    assert torch.equal(O, O2)


@pytest.mark.parametrize("Hq,Hkv", [(8, 2), (2, 2)])
def test_append_attn_on_an_empty_cache_matches_the_fused_forward(ops, Hq, Hkv):
    """lens = 0, new = Ln = 64: the same operation as vq3_qwen_flash_fwd on the same operands, held to the same per-block bound."""
    B, Ln = 2, 64
    rows = [(0, Ln)] * B
    Q, Kc, Vc = _attn_operands(Hq, Hkv, Ln, rows, seed=7 + Hq)
    _poison(Kc, Vc, rows)
    Q, Kc, Vc = Q.to(BF16).cuda(), Kc.to(BF16).cuda(), Vc.to(BF16).cuda()
    O = ops.qwen_append_attn(Q, Kc, Vc, _i32([0] * B), _i32([Ln] * B), B, Ln, Hq, Hkv, D, LMAX, SCALE)
    mask = torch.ones(B, Ln, dtype=torch.uint8, device="cuda")
    Of, _ = ops.qwen_flash_fwd(Q, Kc[:, :, :Ln].contiguous(), Vc[:, :, :Ln].contiguous(), mask, B, Ln, Hq, Hkv, D, SCALE)
    to_heads = lambda x: x.view(B, Ln, Hq, D).permute(0, 2, 1, 3)
    assert torch.isfinite(O.float()).all()
    _assert_blocks("O vs qwen_flash_fwd", to_heads(O), to_heads(Of), O_TOL)
    _assert_blocks("O vs fp64", to_heads(O), _ref_chunk(Q, Kc, Vc, rows), O_TOL)


@pytest.mark.parametrize("bad", ["Lmax=63", "Lmax=12352", "Ln=0", "G=8"])
def test_append_kernels_reject_out_of_range(ops, bad):
    from vggt_qwen3_amd._lib import Vq3Error
    B, Hq, Hkv, Ln, Lmax = 1, 4, 1, 8, 64
    if bad.startswith("Lmax"):
        Lmax = int(bad.split("=")[1])
    if bad == "Ln=0":
        Ln = 0
    if bad == "G=8":
        Hq = 8
    z = lambda *shape: torch.zeros(shape, device="cuda", dtype=BF16)
    Kc = z(B, Hkv, Lmax, D)
    lens, new = _i32([0]), _i32([max(Ln, 1)])
    with pytest.raises(Vq3Error):
        ops.qwen_append_attn(z(B, Hq, Ln, D), Kc, Kc.clone(), lens, new, B, Ln, Hq, Hkv, D, Lmax, SCALE)
    with pytest.raises(Vq3Error):
        ops.qwen_append_qkprep(z(B * Ln, (Hq + 2 * Hkv) * D), z(D), z(D), z(max(Lmax, 1), D), z(max(Lmax, 1), D), lens, new, Kc, Kc.clone(),
                               B, Ln, Hq, Hkv, D, Lmax, 1e-6)


# ------------------------------------------------------------------------------------------------ extend
def test_extend_in_two_chunks_vs_one_shot_forward():
    """B = 2, prompts of 29 and 19 positions (the second left-padded), split at 11 and 7: extend() on an empty cache, then extend()
    with the full sequence. The logits (final norm + tied lm_head) at each row's last position are compared with the fp32 CPU oracle
    (oracle.qwen3.model_forward on the row without its padding), as are those of the existing one-shot forward_hidden on the same
    row: the chunked path makes the same bf16 roundings in another order, so its max abs error may be at most 1.5 x the one-shot's.
    Measured on an MI355X: 4.8675e-03 for both; the assertion message carries both numbers."""
    from oracle import qwen3 as oq
    tm, sd, cfg = _tiny_model()
    ocfg = oq.Qwen3Cfg(**cfg)
    sd32 = {k: v.float() for k, v in sd.items()}
    H = cfg["hidden_size"]
    torch.manual_seed(21)
    n, cut, L0 = [29, 19], [11, 7], 29
    emb = (torch.randn(2, L0, H) * 0.5).to(BF16)
    mask = torch.zeros(2, L0, dtype=torch.long)
    first = torch.zeros(2, L0, dtype=torch.long)
    for b in range(2):
        mask[b, L0 - n[b]:] = 1
        first[b, L0 - n[b]:L0 - n[b] + cut[b]] = 1
    cache = tm.kv_cache(2, 40)
    assert cache.capacity == 64 and cache.lengths == [0, 0]
    tm.extend(cache, inputs_embeds=emb.cuda(), attention_mask=first.cuda())
    assert cache.lengths == cut and cache.lens.tolist() == cut
    h2 = tm.extend(cache, inputs_embeds=emb.cuda(), attention_mask=mask.cuda())
    assert cache.lengths == n and cache.lens.tolist() == n
    assert h2.shape == (2, H)
    chunked = tm.logits_all(h2).float().cpu()
    err_one = err_two = 0.0
    for b in range(2):
        row = emb[b:b + 1, L0 - n[b]:]
        ones = torch.ones(1, n[b], dtype=torch.long)
        ref = torch.nn.functional.linear(oq.model_forward(row.float(), ones, sd32, ocfg)[0, -1], sd32["model.embed_tokens.weight"])
        h1, _ = tm.forward_hidden(row.cuda(), ones.cuda(), save=False)
        one = tm.logits_all(h1[n[b] - 1:n[b]]).float().cpu()[0]
        err_one = max(err_one, (one - ref).abs().max().item())
        err_two = max(err_two, (chunked[b] - ref).abs().max().item())
    assert err_two <= 1.5 * err_one, f"two-chunk extend: max abs logit error {err_two:.4e} vs one-shot forward {err_one:.4e} (bound 1.5 x)"
    print(f"extend in two chunks: max abs logit error {err_two:.4e}; one-shot forward_hidden {err_one:.4e}")


# ------------------------------------------------------------------------------------------------ generate / sample with a cache
def _assert_picks(tm, emb_row, ids, what):
    """Tie rule of tests/test_generate_gpu.py: every id is within TIE_TOL of the maximum of a cache-free forward over emb_row + ids."""
    if ids.numel() > 1:
        logits = _full_forward_logits(tm, emb_row, ids)
    else:                                                   # a row that stopped at its first pick: the prompt alone
        h, _ = tm.forward_hidden(emb_row[None], torch.ones(1, emb_row.shape[0], dtype=torch.long).cuda(), save=False)
        logits = tm.logits_all(h).float()
    n = emb_row.shape[0]
    for t in range(ids.numel()):
        row = logits[n - 1 + t]
        assert row.max() - row[ids[t]] < TIE_TOL, (what, t, float(row.max() - row[ids[t]]))


def _left_pad(rows, H):
    """Rows of embeddings [n_b, H] -> ([B, L, H], mask [B, L]) left-padded to the longest."""
    L = max(r.shape[0] for r in rows)
    emb = torch.zeros(len(rows), L, H, device="cuda", dtype=BF16)
    mask = torch.zeros(len(rows), L, dtype=torch.long, device="cuda")
    for b, r in enumerate(rows):
        emb[b, L - r.shape[0]:] = r
        mask[b, L - r.shape[0]:] = 1
    return emb, mask


def _first_eos(ids_row, eos):
    hit = (ids_row == eos).nonzero().flatten()
    return int(hit[0]) if hit.numel() else None


def _two_turns(tm, H, prompt_lens, use_graph, seed, new1=9, new2=5, want_early_stop=True):
    """Turn 1 on a fresh cache (eos chosen so that row 0 stops early), turn 2 = prompt + emitted ids up to eos + 6 new positions.
    Checks every pick of both turns, the cache lengths after turn 1 and the `prefilled` counts of turn 2. Returns what later checks
    need."""
    B = len(prompt_lens)
    torch.manual_seed(seed)
    prompts = [(torch.randn(n, H) * 0.5).to(BF16).cuda() for n in prompt_lens]
    emb1, mask1 = _left_pad(prompts, H)
    eos = None
    if want_early_stop:
        # a probing run without eos: row 0's id at some step 0..5 that row 0 has not emitted before and row 1 never emits
        probe = tm.generate(inputs_embeds=emb1, attention_mask=mask1, max_new_tokens=new1, use_graph=False, kv_cache=tm.kv_cache(B, 64)).cpu()
        for k in range(6):
            cand = int(probe[0, k])
            if cand not in probe[0, :k].tolist() and all(cand not in probe[b].tolist() for b in range(1, B)):
                eos = cand
                break
        assert eos is not None, probe.tolist()
    cache = tm.kv_cache(B, 64)
    kw1 = dict(inputs_embeds=emb1, attention_mask=mask1, max_new_tokens=new1, eos_token_id=eos, pad_token_id=0, use_graph=use_graph,
               return_stats=True)
    out1, st1 = tm.generate(kv_cache=cache, **kw1)
    assert st1["prefilled"] == list(prompt_lens) and st1["Lmax"] == 64 and st1["graph"] == use_graph
    steps = st1["steps_run"]
    emitted, want_lengths = [], []
    for b in range(B):
        k = _first_eos(out1[b], eos) if eos is not None else None
        emitted.append(out1[b, : (k + 1) if k is not None else out1.shape[1]])
        want_lengths.append(prompt_lens[b] + min(steps - 1, (k + 1) if k is not None else steps - 1))
        _assert_picks(tm, prompts[b], emitted[b], ("turn 1", b))
    if want_early_stop:
        assert _first_eos(out1[0], eos) is not None and _first_eos(out1[0], eos) + 1 < steps - 1, out1.tolist()   # row 0 stopped early
        assert all(_first_eos(out1[b], eos) is None for b in range(1, B)), out1.tolist()
    assert cache.lengths == want_lengths and cache.lens.tolist() == want_lengths
    after1 = cache.clone()
    # turn 2: the whole sequence so far + 6 new positions
    seqs = [torch.cat([prompts[b], tm.get_input_embeddings()(emitted[b]), (torch.randn(6, H) * 0.5).to(BF16).cuda()]) for b in range(B)]
    emb2, mask2 = _left_pad(seqs, H)
    out2, st2 = tm.generate(inputs_embeds=emb2, attention_mask=mask2, max_new_tokens=new2, use_graph=use_graph, return_stats=True,
                            kv_cache=cache)
    # the uncached suffix: the 6 new positions, + 1 where only the id emitted last was missing (a row that did not stop early)
    assert st2["prefilled"] == [seqs[b].shape[0] - want_lengths[b] for b in range(B)]
    assert st2["prefilled"] == [6 if (want_early_stop and b == 0) else 7 for b in range(B)], st2["prefilled"]
    for b in range(B):
        _assert_picks(tm, seqs[b], out2[b], ("turn 2", b))
    assert cache.lengths == [seqs[b].shape[0] + st2["steps_run"] - 1 for b in range(B)]
    return dict(cache=cache, after1=after1, kw1=kw1, out1=out1, emb2=emb2, mask2=mask2, prompt_lens=list(prompt_lens))


@pytest.mark.parametrize("use_graph", [True, False])
def test_generate_two_turns_with_a_cache(use_graph):
    """B = 2, ragged left-padded prompts, row 0 stops early at an eos: picks, lengths and `prefilled` as described in _two_turns; then
    the cache is rolled back to the turn-1 prompt and turn 1 repeated - the same ids."""
    tm, _, cfg = _tiny_model()
    s = _two_turns(tm, cfg["hidden_size"], (21, 13), use_graph, seed=31)
    cache, n = s["cache"], s["prompt_lens"]
    cache.truncate(n)
    assert cache.lengths == n and cache.lens.tolist() == n
    with pytest.raises(ValueError, match="nothing new"):          # the whole prompt is cached: there is no position to take a pick from
        tm.generate(kv_cache=cache, **s["kw1"])
    assert cache.lengths == n                                     # raised before anything ran
    cache.truncate([m - 1 for m in n])                            # so the repeat recomputes each row's last prompt position
    again, st = tm.generate(kv_cache=cache, **s["kw1"])
    assert st["prefilled"] == [1, 1]
    assert torch.equal(again, s["out1"])
    with pytest.raises(ValueError):
        cache.truncate([m + 50 for m in n])


def test_sample_with_a_cache_is_repeatable_and_checks_its_arguments():
    tm, _, cfg = _tiny_model()
    s = _two_turns(tm, cfg["hidden_size"], (17, 22), True, seed=32, want_early_stop=False)
    kw = dict(inputs_embeds=s["emb2"], attention_mask=s["mask2"], max_new_tokens=6, seed=31, temperature=0.9, top_k=20)
    a = tm.sample(kv_cache=s["after1"].clone(), **kw)
    b = tm.sample(kv_cache=s["after1"].clone(), **kw)
    assert a.shape == (2, 6) and torch.equal(a, b)
    fresh = s["after1"].clone()
    with pytest.raises(ValueError, match="num_return_sequences"):
        tm.sample(kv_cache=fresh, num_return_sequences=2, **kw)
    with pytest.raises(ValueError, match="capacity"):             # 64 rows of cache: the rows are 31 / 36 long already
        tm.generate(inputs_embeds=s["emb2"], attention_mask=s["mask2"], max_new_tokens=40, kv_cache=fresh)
    with pytest.raises(ValueError, match="rows"):
        tm.generate(inputs_embeds=s["emb2"][:1], attention_mask=s["mask2"][:1], max_new_tokens=2, kv_cache=fresh)
    assert fresh.lengths == s["after1"].lengths and torch.equal(fresh.lens, s["after1"].lens)


def test_generate_with_a_cache_on_the_persistent_route():
    """B = 1 at Qwen3-4B's widths, 2 layers, a cache of capacity 256: decoding takes the persistent kernel on the cache's own K/V; two
    turns under the tie rule."""
    from vggt_qwen3_amd import ops
    if not ops.decode_layers_supported(2560, 9728, 32, 8, 128, 256):
        pytest.skip("needs an MI355X (256 CUs)")
    tm, cfg = _qwen4b_dims(2)
    H = cfg.hidden_size
    torch.manual_seed(33)
    prompt = (torch.randn(37, H) * 0.5).to(BF16).cuda()
    cache = tm.kv_cache(1, 256)
    out1, st1 = tm.generate(inputs_embeds=prompt[None], max_new_tokens=6, return_stats=True, kv_cache=cache)
    assert st1["persistent"] is True and st1["graph"] and st1["Lmax"] == 256 and st1["prefilled"] == [37]
    _assert_picks(tm, prompt, out1[0], "turn 1")
    assert cache.lengths == [37 + 5]
    seq = torch.cat([prompt, tm.get_input_embeddings()(out1[0]), (torch.randn(6, H) * 0.5).to(BF16).cuda()])
    out2, st2 = tm.generate(inputs_embeds=seq[None], max_new_tokens=6, return_stats=True, kv_cache=cache)
    assert st2["persistent"] is True and st2["prefilled"] == [7]
    _assert_picks(tm, seq, out2[0], "turn 2")
    assert cache.lengths == [seq.shape[0] + 5]


def test_generate_with_a_cache_and_frozen_lora():
    """Unmerged LoRA adapters (tests/test_lora_gpu.py's set-up on the tiny model): the chunk forward applies lora.fwd_qkv / fwd_o, so
    both turns pass the tie rule against the model's own cache-free forward."""
    from tests.test_lora_gpu import _set_random_B, _tiny
    tm, z = _tiny()
    tm.eval()
    tm.enable_lora(r=16, alpha=32, dropout=0.05, target_modules=["q_proj", "k_proj", "v_proj", "o_proj"])
    _set_random_B(tm, seed=8, scale=0.05)
    assert tm.lora_frozen
    _two_turns(tm, tm.config.hidden_size, (18, 12), True, seed=34, want_early_stop=False)
