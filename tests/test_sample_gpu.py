"""Sampling (csrc/sample.hip, generate.py: sample): the kernel against the fp64 reference pick of tests/test_sample_host.py on
constructed bf16 logits - kept set exact, picked id exact, distribution, reproducibility - and sample() end to end on the tiny golden
model and at Qwen3-4B's layer shape.

Bounds. n_kept is an integer and must be equal. The inputs are seeded so that, in fp64, the softmax mass on either side of the top-p
boundary differs from top_p by more than 1e-4 (asserted here, on the CPU): the kernel's masses are f32 exponentials of f32 scores
summed in f64, relative error ~1e-5, far inside that. A pick is compared unless the reference's own two best perturbed scores are
closer than 1e-4 - a few f32 ulps at magnitude 64 (4e-6 each for the score, the noise and their sum) plus the error of two logs;
at most 1 % of picks may be skipped that way."""
import functools
import math

import numpy as np
import pytest
import torch

from tests.test_sample_host import noise, processed_logits, ref_cut, ref_prepare

pytestmark = pytest.mark.gpu
BF16, F32, I32 = torch.bfloat16, torch.float32, torch.int32
KP = [(0, 1.0), (1, 1.0), (50, 1.0), (0, 0.9), (50, 0.9), (0, 1e-6)]
TEMP, PENALTY, NGRAM = 0.7, 1.3, 2
H0, NT = 40, 32                      # ids of history at the first pick; values of the step counter tried: H0 .. H0 + NT - 1
PAD = 5
SEED = 0x9E3779B97F4A7C15            # both halves of the key are used
GAP = 1e-4


@pytest.fixture(scope="module")
def ops():
    from vggt_qwen3_amd import _lib
    from vggt_qwen3_amd import ops as _ops
    _lib.load()
    return _ops


# Which try of each row's generator is used, per (V, B, processors on): the first whose top-p boundaries, over all 32 steps and both
# top_p < 1 settings, stay more than 1.5e-4 clear of top_p in fp64 and whose two best perturbed scores are never closer than GAP
# (found once on the CPU with _row_ok below; the test asserts both conditions again, so a wrong entry fails, it cannot weaken a check)
ROW_TRY = {(1000, 1, True): [3], (1000, 1, False): [0], (1000, 8, True): [3, 7, 3, 2, 1, 4, 1, 2], (1000, 8, False): [0, 0, 0, 0, 0, 1, 0, 0],
           (4099, 1, True): [0], (4099, 1, False): [0], (4099, 8, True): [3, 5, 0, 2, 3, 2, 1, 2], (4099, 8, False): [0] * 8,
           (151936, 1, True): [0], (151936, 1, False): [0], (151936, 8, True): [0, 0, 1, 0, 0, 1, 1, 1],
           (151936, 8, False): [0, 0, 0, 0, 0, 0, 0, 1]}


def _row(V, B, on, b, attempt):
    """One row: bf16 logits ~ 4 N(0, 1) (ties are plentiful) and a history over a 12-id alphabet (the row's 8 best ids and 4 others):
    ids repeat, and positions 38-39 repeat the bigram at 10-11."""
    rng = np.random.default_rng([V, B, int(on), b, attempt])
    lg = torch.from_numpy((4 * rng.standard_normal(V)).astype(np.float32)).to(BF16)
    lf = lg.float().numpy()
    alphabet = np.concatenate([np.argsort(-lf, kind="stable")[:8], rng.integers(0, V, 4)])
    gen = rng.choice(alphabet, H0 + NT + 1)
    gen[38:40] = gen[10:12]
    return lg, lf, gen


def _row_reference(V, on, b, lf, gen):
    """Per (t, kp) of one row: n_kept, smallest kept s, top-p margin, the reference id, the gap between its two best perturbed scores;
    and the banned ids per t. Only ids within 20.25 of the best score are candidates for the pick: the noise spans [-2.88, 17.33]."""
    shape = (NT, len(KP))
    out = dict(n_kept=np.zeros(shape, np.int64), s_min=np.zeros(shape), margin=np.zeros(shape), pick=np.zeros(shape, np.int64),
               gap=np.zeros(shape), banned=[])
    prep = None
    for ti in range(NT):
        t = H0 + ti
        if on or prep is None:
            z = processed_logits(lf, gen[:t] if on else [], PENALTY if on else 1.0, NGRAM if on else 0)
            prep = ref_prepare(z, TEMP)
            cand = np.nonzero(prep["s"] >= prep["vals"][0] - 20.25)[0]
            banned = np.nonzero(np.isneginf(z))[0]
        out["banned"].append(banned)
        score = prep["s"][cand] + noise(cand, SEED, t, b)
        for ki, (k, p) in enumerate(KP):
            n_kept, s_min, margin = ref_cut(prep, k, p)
            sc = np.where(prep["s"][cand] >= s_min, score, -np.inf)
            first = int(sc.argmax())
            best = sc[first]
            sc[first] = -np.inf
            out["n_kept"][ti, ki], out["s_min"][ti, ki], out["margin"][ti, ki] = n_kept, s_min, margin
            out["pick"][ti, ki], out["gap"][ti, ki] = cand[first], best - sc.max()
    return out


def _row_ok(r):
    return min(r["margin"][:, ki].min() for ki, (k, p) in enumerate(KP) if p < 1.0) > 1.5e-4 and r["gap"].min() >= GAP


@functools.lru_cache(maxsize=None)
def _reference(V, B, on):
    """The case's inputs (rows padded to ld > V with columns that would win if they were read) and its per-row references stacked
    to [NT, len(KP), B]."""
    ld = (V + 15) // 8 * 8 + 3
    logits = torch.full((B, ld), 100.0).to(BF16)
    gen = np.zeros((B, H0 + NT + 1), np.int64)
    rows = []
    for b in range(B):
        lg, lf, gen[b] = _row(V, B, on, b, ROW_TRY[(V, B, on)][b])
        logits[b, :V] = lg
        rows.append(_row_reference(V, on, b, lf, gen[b]))
    out = {k: np.stack([r[k] for r in rows], axis=-1) for k in ("n_kept", "s_min", "margin", "pick", "gap")}
    out.update(banned=[[rows[b]["banned"][ti] for b in range(B)] for ti in range(NT)], logits=logits, gen=gen)
    return out


@pytest.mark.parametrize("on", [True, False], ids=["penalty-ngram", "plain"])
@pytest.mark.parametrize("B", [1, 8])
@pytest.mark.parametrize("V", [1000, 4099, 151936])
def test_kept_set_and_pick_are_exact(ops, V, B, on):
    """V = 1000 is smaller than 64 slices x 256 threads, 4099 has a ragged last slice, 151936 is Qwen3's vocabulary. For every
    (top_k, top_p) of KP and 32 values of the step counter: n_kept and the smallest kept score equal the fp64 reference's, the picked
    id is the reference's argmax of s + g, lies in the reference's kept set and is never a banned id; a finished row emits pad and stays
    finished; the workspace is left zero and only column `step` of `generated` is written."""
    ref = _reference(V, B, on)
    # conditions on the inputs, checked on the CPU: the top-p boundary is clear of top_p, and few picks are too close to call
    for ki, (k, p) in enumerate(KP):
        if p < 1.0:
            assert ref["margin"][:, ki].min() > 1e-4, (k, p, ref["margin"][:, ki].min())
    assert (ref["gap"] < GAP).mean() <= 0.01, (ref["gap"] < GAP).mean()

    dev = "cuda"
    logits, gen0 = ref["logits"].to(dev), torch.from_numpy(ref["gen"]).to(dev)
    gen = gen0.clone()
    fin0 = torch.zeros(B, dtype=I32, device=dev)
    if B > 2:
        fin0[2] = 1
    fin = fin0.clone()
    st = torch.zeros(1, dtype=I32, device=dev)
    nxt = torch.zeros(B, dtype=I32, device=dev)
    work = torch.zeros(B * 128 + 8, dtype=F32, device=dev)
    sw = ops.sample_workspace(B, dev)
    ids = torch.zeros((NT, len(KP), B), dtype=I32, device=dev)
    n_kept = torch.zeros((NT, len(KP), B), dtype=I32, device=dev)
    s_min = torch.zeros((NT, len(KP), B), dtype=F32, device=dev)
    written = torch.zeros((NT, len(KP), B), dtype=torch.int64, device=dev)
    fin_after = torch.zeros((NT, len(KP), B), dtype=I32, device=dev)
    for ti in range(NT):
        for ki, (k, p) in enumerate(KP):
            gen.copy_(gen0); fin.copy_(fin0); st.fill_(H0 + ti)
            ops.sample_pick(logits, work, gen, st, fin, PENALTY if on else 1.0, NGRAM if on else 0, None, PAD, nxt, V, TEMP, k, p, SEED, sw,
                            n_kept=n_kept[ti, ki], min_kept=s_min[ti, ki])
            ids[ti, ki] = nxt
            written[ti, ki] = gen[:, H0 + ti]
            fin_after[ti, ki] = fin
    keep = torch.ones(gen.shape[1], dtype=torch.bool, device=dev)
    keep[H0 + NT - 1] = False
    assert torch.equal(gen[:, keep], gen0[:, keep])
    assert int(sw.view(B, ops.SAMPLE_WORK_PER_ROW)[:, :65536].abs().sum()) == 0, "every pick leaves the histogram zero"
    ids, n_kept, s_min = ids.cpu().numpy(), n_kept.cpu().numpy(), s_min.cpu().numpy().astype(np.float64)
    assert np.array_equal(written.cpu().numpy(), ids) and np.array_equal(fin_after.cpu().numpy(), np.broadcast_to(fin0.cpu().numpy(), ids.shape))
    live = np.nonzero(fin0.cpu().numpy() == 0)[0]
    assert np.array_equal(n_kept, ref["n_kept"]), np.argwhere(n_kept != ref["n_kept"])[:8]
    assert np.all(np.abs(s_min - ref["s_min"]) <= 2e-7 * np.maximum(1.0, np.abs(ref["s_min"])))        # one f32 rounding of z / T
    if B > 2:
        assert (ids[:, :, 2] == PAD).all()
    skipped = 0
    for ti in range(NT):
        for b in live:
            assert not np.isin(ids[ti, :, b], ref["banned"][ti][b]).any()
    lf = ref["logits"][:, :V].float().numpy()
    for ti in range(NT):
        for ki in range(len(KP)):
            for b in live:
                got = int(ids[ti, ki, b])
                assert 0 <= got < V
                if ref["gap"][ti, ki, b] < GAP:
                    skipped += 1
                    continue
                assert got == ref["pick"][ti, ki, b], (ti, KP[ki], b, got, int(ref["pick"][ti, ki, b]), ref["gap"][ti, ki, b])
    assert skipped <= 0.01 * NT * len(KP) * len(live)
    # membership of the kept set for the skipped ones too: recompute the processed score of what was picked
    for ti in range(NT):
        for b in live:
            z = processed_logits(lf[b], ref["gen"][b, :H0 + ti] if on else [], PENALTY if on else 1.0, NGRAM if on else 0)
            s = z.astype(np.float64) / float(np.float32(TEMP))
            assert (s[ids[ti, :, b]] >= ref["s_min"][ti, :, b]).all(), (ti, b)


def _chi2_quantile(q_upper, dof):
    try:
        from scipy.stats import chi2
        return float(chi2.isf(q_upper, dof))
    except ImportError:                                      # Wilson-Hilferty
        from statistics import NormalDist
        zq = NormalDist().inv_cdf(1 - q_upper)
        return dof * (1 - 2 / (9 * dof) + zq * math.sqrt(2 / (9 * dof))) ** 3


def _draws(ops, logits, V, temperature, top_k, seed, steps=500):
    B = logits.shape[0]
    dev = logits.device
    gen = torch.zeros((B, 512), dtype=torch.int64, device=dev)
    fin = torch.zeros(B, dtype=I32, device=dev)
    st = torch.zeros(1, dtype=I32, device=dev)
    nxt = torch.zeros(B, dtype=I32, device=dev)
    work = torch.zeros(B * 128 + 8, dtype=F32, device=dev)
    sw = ops.sample_workspace(B, dev)
    nk = torch.zeros(B, dtype=I32, device=dev)
    out = torch.zeros((steps, B), dtype=I32, device=dev)
    for t in range(steps):
        st.fill_(t)
        ops.sample_pick(logits, work, gen, st, fin, 1.0, 0, None, 0, nxt, V, temperature, top_k, 1.0, seed, sw, n_kept=nk)
        out[t] = nxt
    return out.cpu().numpy(), nk.cpu().numpy()


def test_distribution_and_reproducibility(ops):
    """V = 1000, 8 identical rows, top_k = 12, temperature 0.7, step counter 0..499: 4000 draws from 4000 different Philox streams.
    Their counts pass a chi-square test against the fp64 probabilities of the kept set at the 1 - 1e-6 quantile (11 degrees of freedom);
    the draws at temperature 1.0 fail the same test against the 0.7 probabilities, so the test can see a wrong temperature. Same seed:
    the same bits; another seed: different draws."""
    V, B, K = 1000, 8, 12
    rng = np.random.default_rng(43)                          # (12 kept ids, two of them tied: a tie inside the set, none at its edge)
    row = torch.from_numpy((2 * rng.standard_normal(V)).astype(np.float32)).to(BF16)
    prep = ref_prepare(row.float().numpy(), 0.7)
    n_kept, s_min, _ = ref_cut(prep, K, 1.0)
    assert n_kept == K                                        # no tie at the 12th value: 11 degrees of freedom
    kept = np.nonzero(prep["s"] >= s_min)[0]
    prob = np.exp(prep["s"][kept] - prep["s"][kept].max())
    prob /= prob.sum()
    assert 4000 * prob.min() >= 5
    logits = row[None].repeat(B, 1).contiguous().cuda()
    bound = _chi2_quantile(1e-6, K - 1)

    def chi2_of(draws):
        assert np.isin(draws, kept).all()
        counts = np.array([(draws == i).sum() for i in kept])
        assert counts.sum() == draws.size == 4000
        return float(((counts - 4000 * prob) ** 2 / (4000 * prob)).sum())

    d07, nk = _draws(ops, logits, V, 0.7, K, SEED)
    assert (nk == K).all()
    x07 = chi2_of(d07)
    d10, _ = _draws(ops, logits, V, 1.0, K, SEED)
    x10 = chi2_of(d10)
    print(f"chi2 at T=0.7: {x07:.2f}, at T=1.0 against the 0.7 probabilities: {x10:.2f}, bound {bound:.2f}")
    assert x07 < bound
    assert x10 > bound
    again, _ = _draws(ops, logits, V, 0.7, K, SEED)
    assert np.array_equal(again, d07)
    other, _ = _draws(ops, logits, V, 0.7, K, SEED + 1)
    assert (other != d07).any()
    # rows hold the same logits and differ only in the row index of the counter: their streams differ
    assert (d07[:, 0] != d07[:, 1]).any()


# ================================================================================================ sample() end to end
from tests.test_generate_gpu import TIE_TOL, _qwen4b_dims          # noqa: E402
from tests.test_logprob_gpu import _full_logits, _tiny_model, bits   # noqa: E402


@pytest.fixture(scope="module")
def tiny():
    return _tiny_model()


def _prompts(cfg, B, L, seed):
    torch.manual_seed(seed)
    emb = (torch.randn(B, L, cfg["hidden_size"]) * 0.5).to(BF16).cuda()
    return emb, torch.ones(B, L, dtype=torch.long).cuda()


def test_seeded_runs_repeat(tiny):
    tm, cfg = tiny
    emb, mask = _prompts(cfg, 2, 19, 3)
    kw = dict(inputs_embeds=emb, attention_mask=mask, max_new_tokens=9, output_logprobs=True, return_stats=True, temperature=1.3, top_k=0)
    ids, lp, stats = tm.sample(seed=11, use_graph=True, **kw)
    assert ids.shape == (2, 9) and ids.dtype == torch.int64 and stats["graph"] and stats["seed"] == 11
    ids2, lp2, _ = tm.sample(seed=11, use_graph=True, **kw)
    assert torch.equal(ids, ids2) and torch.equal(bits(lp), bits(lp2))
    ids3, lp3, stats3 = tm.sample(seed=11, use_graph=False, **kw)
    assert not stats3["graph"] and torch.equal(ids, ids3) and torch.equal(bits(lp), bits(lp3))
    ids4, _, _ = tm.sample(seed=12, use_graph=True, **kw)
    assert not torch.equal(ids, ids4)
    torch.manual_seed(77)
    a, _, sa = tm.sample(**kw)
    torch.manual_seed(77)
    b, _, sb = tm.sample(**kw)
    c, _, sc = tm.sample(**kw)
    assert sa["seed"] == sb["seed"] != sc["seed"] and 0 <= sa["seed"] < 2 ** 64 and torch.equal(a, b)
    # generate() is untouched by all this: greedy, and it still refuses do_sample
    with pytest.raises(NotImplementedError, match="sample"):
        tm.generate(inputs_embeds=emb, attention_mask=mask, do_sample=True)


@pytest.mark.parametrize("use_graph", [True, False])
def test_top_k_1_is_greedy(tiny, use_graph):
    """top_k = 1 leaves the maximum (and its exact ties) only: every emitted id has the maximal processed logit of a cache-free forward
    within TIE_TOL - tests/test_generate_gpu.py's check of the greedy pick."""
    from oracle import generate as og
    tm, cfg = tiny
    emb, mask = _prompts(cfg, 2, 19, 3)
    NEW = 10
    out = tm.sample(inputs_embeds=emb, attention_mask=mask, max_new_tokens=NEW, top_k=1, repetition_penalty=1.1, no_repeat_ngram_size=4,
                    seed=5, use_graph=use_graph)
    assert out.shape == (2, NEW)
    for b in range(2):
        logits = _full_logits(tm, emb[b], out[b]).float().cpu()
        for t in range(NEW):
            sc = logits[19 - 1 + t].clone()
            seen = out[b, :t].tolist()
            og.repetition_penalty_(sc, seen, 1.1)
            og.no_repeat_ngram_(sc, seen, 4)
            assert sc[out[b, t]] >= sc.max() - TIE_TOL, (b, t)


def test_one_prefill_per_prompt(tiny):
    """num_return_sequences = 4 from one prompt equals the prompt repeated as 4 rows (same row indices, same streams): the K/V rows and
    the last hidden state reach every draw's cache row. Then 2 prompts of different lengths (left-padded) x 3 draws against the same
    6 rows spelled out; prompt-major order."""
    tm, cfg = tiny
    emb, mask = _prompts(cfg, 1, 19, 4)
    kw = dict(max_new_tokens=8, temperature=1.2, top_k=40, top_p=0.95, seed=21, output_logprobs=True)
    ids, lp = tm.sample(inputs_embeds=emb, attention_mask=mask, num_return_sequences=4, **kw)
    ids_r, lp_r = tm.sample(inputs_embeds=emb.repeat(4, 1, 1), attention_mask=mask.repeat(4, 1), **kw)
    assert ids.shape == (4, 8) and torch.equal(ids, ids_r) and torch.equal(bits(lp), bits(lp_r))
    assert len({tuple(r) for r in ids.tolist()}) > 1, "four draws of one prompt are four different streams"
    emb2, mask2 = _prompts(cfg, 2, 17, 6)
    mask2[1, :5] = 0
    ids, lp = tm.sample(inputs_embeds=emb2, attention_mask=mask2, num_return_sequences=3, **kw)
    ids_r, lp_r = tm.sample(inputs_embeds=emb2.repeat_interleave(3, 0), attention_mask=mask2.repeat_interleave(3, 0), **kw)
    assert ids.shape == (6, 8) and torch.equal(ids, ids_r) and torch.equal(bits(lp), bits(lp_r))
    # with input_ids the prompt comes back in front of each of its draws
    g = torch.Generator().manual_seed(7)
    ids0 = torch.randint(1, tm.vocab, (2, 12), generator=g).cuda()
    out = tm.sample(input_ids=ids0, max_new_tokens=5, num_return_sequences=2, seed=3, repetition_penalty=1.1)
    assert out.shape == (4, 17) and torch.equal(out[:, :12], ids0.repeat_interleave(2, 0))


@pytest.mark.parametrize("use_graph", [True, False])
def test_logprobs_are_the_raw_distribution_at_the_sampled_id(tiny, use_graph):
    """Every entry up to a row's eos is log_softmax of the cache-free forward's raw logits at the sampled id within TIE_TOL (the
    tolerance tests/test_logprob_gpu.py uses for generate()); entries after a row's eos are exactly 0.0 and the ids there are pad."""
    tm, cfg = tiny
    B, L, NEW = 2, 17, 10
    emb, mask = _prompts(cfg, B, L, 5)
    mask[1, :5] = 0
    rows = [emb[0], emb[1, 5:]]
    kw = dict(inputs_embeds=emb, attention_mask=mask, max_new_tokens=NEW, use_graph=use_graph, temperature=1.5, top_k=0, top_p=0.98,
              repetition_penalty=1.1, no_repeat_ngram_size=4, seed=9)
    free = tm.sample(**kw).cpu()
    pick = [(r, t) for r in (0, 1) for t in range(1, 6) if free[r, t] not in free[1 - r] and free[r, t] not in free[r, :t]]
    assert pick, free.tolist()
    r, t_eos = pick[0]
    kw.update(eos_token_id=int(free[r, t_eos]), pad_token_id=3)
    ids, lp = tm.sample(output_logprobs=True, **kw)
    assert torch.equal(ids[:, :t_eos + 1].cpu(), free[:, :t_eos + 1]) and int(ids[r, t_eos]) == kw["eos_token_id"]
    assert lp.dtype == F32 and lp.shape == ids.shape
    for b in range(B):
        ref = torch.log_softmax(_full_logits(tm, rows[b], ids[b]), -1)
        ended = False
        for t in range(ids.shape[1]):
            if ended:
                assert lp[b, t].item() == 0.0 and int(ids[b, t]) == 3, (b, t)
                continue
            want = ref[rows[b].shape[0] - 1 + t, ids[b, t]].item()
            assert abs(lp[b, t].item() - want) < TIE_TOL and lp[b, t].item() < 0.0, (b, t, lp[b, t].item(), want)
            ended = int(ids[b, t]) == kw["eos_token_id"]
    assert (lp[r, t_eos + 1:] == 0).all() and (lp[1 - r] < 0).all()


def test_sample_on_the_persistent_route(ops):
    """B = 1 at Qwen3-4B's layer shape, 2 layers, the full vocabulary: the persistent layers kernel + lm_head + vq3_sample_pick in the
    captured step."""
    if not ops.decode_layers_supported(2560, 9728, 32, 8, 128, 128):
        pytest.skip("needs an MI355X (256 CUs)")
    tm, cfg = _qwen4b_dims(2)
    torch.manual_seed(7)
    L = 21
    emb = (torch.randn(1, L, cfg.hidden_size) * 0.5).to(BF16).cuda()
    kw = dict(inputs_embeds=emb, attention_mask=torch.ones(1, L, dtype=torch.long).cuda(), max_new_tokens=9, output_logprobs=True,
              return_stats=True, temperature=0.9, top_k=50, top_p=0.95, repetition_penalty=1.1, seed=31)
    ids, lp, stats = tm.sample(use_graph=True, **kw)
    assert stats["persistent"] and stats["graph"] and ids.shape == (1, 9)
    ids2, lp2, _ = tm.sample(use_graph=True, **kw)
    ids3, lp3, stats3 = tm.sample(use_graph=False, **kw)
    assert stats3["persistent"] and not stats3["graph"]
    assert torch.equal(ids, ids2) and torch.equal(bits(lp), bits(lp2)) and torch.equal(ids, ids3) and torch.equal(bits(lp), bits(lp3))
    ids4, _, _ = tm.sample(use_graph=True, **dict(kw, seed=32))
    assert not torch.equal(ids, ids4)
    ref = torch.log_softmax(_full_logits(tm, emb[0], ids[0]), -1)
    for t in range(9):
        assert abs(lp[0, t].item() - ref[L - 1 + t, ids[0, t]].item()) < TIE_TOL, t
