"""generate() / sample() / KV-cache sessions with 9 to 64 rows per call (max_rows=): every decode step runs the MFMA decode GEMM
(csrc/decode_gemm.hip) once per projection instead of the FMA skinny GEMM. Tiny model of tests/golden/qwen3_tiny.npz; the criterion is
the one of tests/test_generate_gpu.py::test_decode_logits_match_full_forward - the logits of a cache-free forward over prompt +
emitted ids have their maximum within TIE_TOL of the emitted id's logit at every step - applied to the processed scores where the
repetition penalty and the n-gram ban are on (they act on the scores the pick maximises)."""
import pytest
import torch

from tests.test_generate_gpu import _full_forward_logits, _tiny_model

pytestmark = pytest.mark.gpu
BF16, F32 = torch.bfloat16, torch.float32
TIE_TOL = 0.08      # as in tests/test_generate_gpu.py: logits are bf16 of magnitude ~4-8, one ulp is 0.03


@pytest.fixture(scope="module")
def tiny():
    tm, _, cfg = _tiny_model()
    return tm, cfg["hidden_size"]


def _left_pad(rows, H):
    """Rows of embeddings [n_b, H] -> ([B, L, H], mask [B, L]) left-padded to the longest."""
    L = max(r.shape[0] for r in rows)
    emb = torch.zeros(len(rows), L, H, device="cuda", dtype=BF16)
    mask = torch.zeros(len(rows), L, dtype=torch.long, device="cuda")
    for b, r in enumerate(rows):
        emb[b, L - r.shape[0]:] = r
        mask[b, L - r.shape[0]:] = 1
    return emb, mask


def _assert_row(tm, emb_row, ids, what, penalty=1.0, ngram=0):
    """Every id of `ids` is within TIE_TOL of the maximum of the (processed) scores of a cache-free forward over emb_row + ids."""
    from oracle import generate as og
    n = emb_row.shape[0]
    if ids.numel() > 1:
        logits = _full_forward_logits(tm, emb_row, ids).cpu()
    else:                                                   # a row that stopped at its first pick: the prompt alone
        h, _ = tm.forward_hidden(emb_row[None], torch.ones(1, n, dtype=torch.long).cuda(), save=False)
        logits = tm.logits_all(h).float().cpu()
    for t in range(ids.numel()):
        sc = logits[n - 1 + t].clone()
        seen = ids[:t].tolist()
        og.repetition_penalty_(sc, seen, penalty)
        og.no_repeat_ngram_(sc, seen, ngram)
        assert sc.max() - sc[ids[t]] < TIE_TOL, (what, t, float(sc.max() - sc[ids[t]]))


@pytest.mark.parametrize("use_graph", [True, False])
def test_64_rows_of_equal_length(tiny, use_graph):
    tm, H = tiny
    torch.manual_seed(3)
    B, L = 64, 19
    emb = (torch.randn(B, L, H) * 0.5).to(BF16).cuda()
    out, stats = tm.generate(inputs_embeds=emb, attention_mask=torch.ones(B, L, dtype=torch.long).cuda(), max_new_tokens=9,
                             use_graph=use_graph, max_rows=64, return_stats=True)
    assert out.shape == (B, 9) and stats["graph"] == use_graph and not stats["persistent"]
    full = torch.cat([emb, tm.get_input_embeddings()(out[:, :-1])], dim=1)
    h, _ = tm.forward_hidden(full, torch.ones(B, full.shape[1], dtype=torch.long).cuda(), save=False)
    logits = tm.logits_all(h).view(B, h.shape[0] // B, -1).float()
    for t in range(9):
        row = logits[:, L - 1 + t]
        assert ((row.max(-1).values - row.gather(1, out[:, t:t + 1]).squeeze(1)) < TIE_TOL).all(), t


def test_11_ragged_rows_with_processors_and_eos(tiny):
    tm, H = tiny
    torch.manual_seed(5)
    lens = [19, 7, 13, 19, 13, 7, 19, 7, 13, 19, 7]
    prompts = [(torch.randn(n, H) * 0.5).to(BF16).cuda() for n in lens]
    emb, mask = _left_pad(prompts, H)
    kw = dict(inputs_embeds=emb, attention_mask=mask, max_new_tokens=9, repetition_penalty=1.1, no_repeat_ngram_size=2, max_rows=16,
              output_logprobs=True)
    probe, _ = tm.generate(use_graph=False, **kw)
    probe = probe.cpu()
    # an eos that some rows emit early and some never: the id of step 1..5 that the fewest (>= 1) rows contain
    cands = {int(v) for v in probe[:, 1:6].flatten()}
    eos = min(cands, key=lambda v: (sum(v in probe[b].tolist() for b in range(11)), v))
    assert 1 <= sum(eos in probe[b].tolist() for b in range(11)) < 11, probe.tolist()
    pad = 0 if eos != 0 else 1
    for use_graph in (True, False):
        out, lp = tm.generate(eos_token_id=eos, pad_token_id=pad, use_graph=use_graph, **kw)
        out, lp = out.cpu(), lp.cpu()
        assert out.shape == (11, 9) and lp.shape == (11, 9) and lp.dtype == F32
        stopped = 0
        for b in range(11):
            hit = (out[b] == eos).nonzero().flatten()
            k = int(hit[0]) + 1 if hit.numel() else 9
            assert torch.equal(out[b, :k], probe[b, :k]), (b, out[b].tolist(), probe[b].tolist())     # the eos changes nothing before it
            _assert_row(tm, prompts[b], out[b, :k].cuda(), ("ragged", use_graph, b), 1.1, 2)
            assert (lp[b, :k] < 0).all()
            if k < 9:
                stopped += 1
                assert (out[b, k:] == pad).all() and (lp[b, k:] == 0.0).all(), (b, out[b].tolist(), lp[b].tolist())
        assert 1 <= stopped < 11


def test_8_rows_take_the_same_route_whatever_max_rows_says(tiny):
    tm, H = tiny
    torch.manual_seed(7)
    emb = (torch.randn(8, 19, H) * 0.5).to(BF16).cuda()
    kw = dict(inputs_embeds=emb, attention_mask=torch.ones(8, 19, dtype=torch.long).cuda(), max_new_tokens=9, output_logprobs=True)
    out, lp = tm.generate(**kw)
    out64, lp64 = tm.generate(max_rows=64, **kw)
    assert torch.equal(out, out64) and torch.equal(lp, lp64)


def test_sample_12_draws_of_one_prompt(tiny):
    tm, H = tiny
    ones = torch.ones(1, 19, dtype=torch.long).cuda()
    # top_k = 1 keeps the maximum AND its exact ties, and the 12-row step rounds its sums in another order than generate()'s 1-row
    # step: "equals generate()'s row" is a statement about a prompt whose greedy path has no near-tie. The first of 16 seeded prompts
    # whose top-2 margin, in a cache-free forward, exceeds TIE_TOL at all 9 steps
    emb = greedy = None
    for seed in range(9, 25):
        torch.manual_seed(seed)
        e = (torch.randn(1, 19, H) * 0.5).to(BF16).cuda()
        g = tm.generate(inputs_embeds=e, attention_mask=ones, max_new_tokens=9)
        top2 = _full_forward_logits(tm, e[0], g[0])[18:27].topk(2, dim=-1)
        if torch.equal(top2.indices[:, 0], g[0]) and bool(((top2.values[:, 0] - top2.values[:, 1]) > TIE_TOL).all()):
            emb, greedy = e, g
            break
    assert emb is not None, "no prompt with a tie-free greedy path among 16"
    kw = dict(inputs_embeds=emb, attention_mask=ones, max_new_tokens=9, num_return_sequences=12, max_rows=16)
    a = tm.sample(seed=1234, temperature=1.3, top_k=0, use_graph=True, **kw)
    assert a.shape == (12, 9)
    assert torch.equal(a, tm.sample(seed=1234, temperature=1.3, top_k=0, use_graph=True, **kw))
    assert torch.equal(a, tm.sample(seed=1234, temperature=1.3, top_k=0, use_graph=False, **kw))
    assert len({tuple(r) for r in a.tolist()}) > 1                       # the draws differ from each other
    one = tm.sample(seed=99, top_k=1, **kw)
    assert torch.equal(one, greedy.expand(12, 9)), (one.tolist(), greedy.tolist())


def test_two_turns_on_a_12_row_cache(tiny):
    tm, H = tiny
    torch.manual_seed(11)
    lens = [21, 13, 9, 21, 13, 9, 17, 21, 13, 9, 17, 5]
    B, new1, new2 = len(lens), 6, 4
    prompts = [(torch.randn(n, H) * 0.5).to(BF16).cuda() for n in lens]
    emb1, mask1 = _left_pad(prompts, H)
    cache = tm.kv_cache(B, 64)
    out1, st1 = tm.generate(inputs_embeds=emb1, attention_mask=mask1, max_new_tokens=new1, kv_cache=cache, max_rows=16, return_stats=True)
    assert st1["prefilled"] == lens and st1["steps_run"] == new1
    for b in range(B):
        _assert_row(tm, prompts[b], out1[b], ("turn 1", b))
    # no eos: every decode step cached the id picked before it
    assert cache.lengths == [n + new1 - 1 for n in lens] and cache.lens.tolist() == cache.lengths
    seqs = [torch.cat([prompts[b], tm.get_input_embeddings()(out1[b]), (torch.randn(4, H) * 0.5).to(BF16).cuda()]) for b in range(B)]
    emb2, mask2 = _left_pad(seqs, H)
    out2, st2 = tm.generate(inputs_embeds=emb2, attention_mask=mask2, max_new_tokens=new2, kv_cache=cache, max_rows=16, return_stats=True)
    assert st2["prefilled"] == [5] * B                                   # the id emitted last + the 4 new positions
    for b in range(B):
        _assert_row(tm, seqs[b], out2[b], ("turn 2", b))
    assert cache.lengths == [seqs[b].shape[0] + new2 - 1 for b in range(B)]
    with pytest.raises(ValueError, match="max_rows"):                    # the cap is the caller's: 12 rows need it raised
        tm.generate(inputs_embeds=emb2, attention_mask=mask2, max_new_tokens=2, kv_cache=cache)


def test_20_rows_with_frozen_lora_adapters():
    """Unmerged LoRA adapters (tests/test_lora_gpu.py's set-up on the tiny model) on the wide route: their terms follow the decode
    GEMM's q|k|v and o, so every pick passes the tie rule against the model's own cache-free forward (which applies them too)."""
    from tests.test_lora_gpu import _set_random_B, _tiny
    tm, _ = _tiny()
    tm.eval()
    tm.enable_lora(r=16, alpha=32, dropout=0.05, target_modules=["q_proj", "k_proj", "v_proj", "o_proj"])
    _set_random_B(tm, seed=8, scale=0.05)
    assert tm.lora_frozen
    H = tm.config.hidden_size
    torch.manual_seed(13)
    lens = [15, 9] * 10
    prompts = [(torch.randn(n, H) * 0.5).to(BF16).cuda() for n in lens]
    emb, mask = _left_pad(prompts, H)
    out = tm.generate(inputs_embeds=emb, attention_mask=mask, max_new_tokens=6, max_rows=32)
    assert out.shape == (20, 6)
    for b in range(20):
        _assert_row(tm, prompts[b], out[b], ("lora", b))
