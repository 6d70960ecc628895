"""Per-token log-probabilities: the kernels (csrc/logprob.hip) against fp64 on both launch shapes, the decode-step form after
greedy_pick, generate(output_logprobs=True) against a cache-free full forward, and score() against fp64 log_softmax of logits_all.

Tolerances are the ones the neighbouring tests apply to the same quantities: a row's logprob / lse is its cross entropy, so
tests/test_qwen_loss_head_gpu.py's `lse_err` (an f32 log-sum-exp against fp64 of the same bf16 logits); a decode step against a full
forward is tests/test_generate_gpu.py's TIE_TOL (the bf16 noise floor of the logits). Ranks are exact."""
import math

import pytest
import torch

from tests.golden_io import load, meta, weights
from tests.test_generate_gpu import TIE_TOL
from tests.test_qwen_loss_head_gpu import lse_err, report

pytestmark = pytest.mark.gpu
BF16, F32, F64, I32 = torch.bfloat16, torch.float32, torch.float64, torch.int32
NINF = float("-inf")


@pytest.fixture(scope="module")
def ops():
    from vggt_qwen3_amd import _lib
    from vggt_qwen3_amd import ops as _ops
    _lib.load()
    return _ops


def bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


# ================================================================================================ A. the kernel against fp64
SHAPES = [(151936, 151936), (151670, 151680), (1000, 1024), (9, 16), (8, 8)]      # (V, ld) of the loss-head tests
# (row kind, target kind): every kind of row and of target the kernel has a branch or an edge for
SPECS = [("std1", "col0"), ("std8", "last"), ("shift", "max"), ("const", "third"), ("ninf", "ninf"), ("tie", "second"),
         ("tie", "first"), ("std1", "ignore"), ("std8", "max"), ("ninf", "finite"), ("shift", "col0"), ("std1", "random")]


def make_rows(V, ld, n, seed, first=0):
    """n rows taken round-robin from SPECS (starting at `first`), the slack columns [V, ld) filled with NaN and +inf."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    lg = torch.randn(n, V, generator=g, device="cuda", dtype=F64)
    tgt = torch.randint(0, V, (n,), generator=g, device="cuda")
    kinds = [SPECS[(first + i) % len(SPECS)] for i in range(n)]
    ta, tb = 1, V - 2                                           # the two tied maxima
    for i, (row, _) in enumerate(kinds):
        if row == "std8":
            lg[i] *= 8
        elif row == "shift":
            lg[i] += 300
        elif row == "const":
            lg[i] = 1.75
        elif row == "ninf":
            lg[i, 2::5] = NINF                                   # a fifth of the columns
        elif row == "tie":
            lg[i, ta] = lg[i, tb] = 30.0
    lg = lg.to(BF16)
    for i, (row, t) in enumerate(kinds):
        tgt[i] = {"col0": 0, "last": V - 1, "max": int(lg[i].float().argmax()), "third": V // 3, "ninf": 2, "second": tb, "first": ta,
                  "ignore": -100, "finite": 0, "random": int(tgt[i])}[t]
    buf = torch.empty(n, ld, device="cuda", dtype=BF16)
    buf[:, :V] = lg
    if ld > V:
        buf[:, V:] = torch.tensor([float("nan"), float("inf")], device="cuda").repeat((ld - V + 1) // 2)[: ld - V].to(BF16)
    return buf, tgt.to(I32), kinds


def reference(buf, tgt, V):
    """fp64 from the same bf16 logits: lse, logprob (0 where ignored), rank (-1 where ignored), max finite |logit| per row."""
    lg = buf[:, :V].double()
    lse = torch.logsumexp(lg, 1)
    ok = (tgt >= 0) & (tgt < V)
    t = tgt.long().clamp(0, V - 1)
    tv = lg.gather(1, t[:, None])
    lp = torch.where(ok, tv.squeeze(1) - lse, torch.zeros_like(lse))
    col = torch.arange(V, device=buf.device)[None]
    rank = ((lg > tv) | ((lg == tv) & (col < t[:, None]))).sum(1)
    rank = torch.where(ok, rank, torch.full_like(rank, -1))
    lmax = torch.where(torch.isfinite(lg), lg.abs(), torch.zeros_like(lg)).amax(1)
    return lse, lp, rank, lmax


def check_against_fp64(name, got, buf, tgt, V):
    lp, lse, rank = got
    lse64, lp64, rank64, lmax = reference(buf, tgt, V)
    assert not torch.isnan(lp).any() and not torch.isnan(lse).any(), name
    bound = lse_err(lse64, lmax)
    report(name + " lse", (lse.double() - lse64).abs(), bound)
    fin = torch.isfinite(lp64)
    assert torch.equal(lp[~fin].double(), lp64[~fin]), f"{name}: a -inf target must give exactly -inf"
    report(name + " logprob", (lp.double() - lp64)[fin].abs(), bound[fin])
    assert torch.equal(rank.long(), rank64), (name, rank.tolist()[:12], rank64.tolist()[:12])
    assert (lp[tgt < 0] == 0).all() and (rank[tgt < 0] == -1).all()


@pytest.mark.parametrize("slices", [1, 64], ids=["rows", "split"])
@pytest.mark.parametrize("n", [1, 5, 67])
@pytest.mark.parametrize("V,ld", SHAPES)
def test_token_logprob_vs_fp64(ops, V, ld, n, slices):
    buf, tgt, kinds = make_rows(V, ld, n, seed=V + n, first=(V + n) % len(SPECS))
    before = buf.clone()
    got = ops.token_logprob(buf, tgt, V, slices=slices)
    again = ops.token_logprob(buf, tgt, V, slices=slices)
    torch.cuda.synchronize()
    assert torch.equal(bits(buf), bits(before)), "the logits must not be written"
    for a, b in zip(got, again):
        assert torch.equal(bits(a), bits(b)), "two runs must give the same bits"
    check_against_fp64(f"V={V} n={n} slices={slices}", got, buf, tgt, V)
    # lse / rank are optional outputs
    only = ops.token_logprob(buf, tgt, V, slices=slices, want_lse=False, want_rank=False)
    assert only[1] is None and only[2] is None and torch.equal(bits(only[0]), bits(got[0]))


@pytest.mark.parametrize("slices", [1, 64, 0, 7], ids=["rows", "split", "auto", "split7"])
@pytest.mark.parametrize("V,ld", [(151936, 151936), (1000, 1024), (9, 16), (8, 8)])
def test_token_logprob_every_kind_of_row_and_target(ops, V, ld, slices):
    """All twelve SPECS at once, with the statements the issue makes about them spelled out."""
    n = len(SPECS)
    buf, tgt, kinds = make_rows(V, ld, n, seed=3 * V + 1)
    lp, lse, rank = got = ops.token_logprob(buf, tgt, V, slices=slices)
    check_against_fp64(f"V={V} specs slices={slices}", got, buf, tgt, V)
    k = {s: i for i, s in enumerate(SPECS)}
    i = k[("const", "third")]
    assert abs(lp[i].item() + math.log(V)) <= lse_err(torch.tensor(1.75 + math.log(V)), torch.tensor(1.75)).item() and rank[i] == V // 3
    i = k[("ninf", "ninf")]
    assert lp[i].item() == NINF and math.isfinite(lse[i].item())
    assert rank[k[("tie", "second")]] == 1 and rank[k[("tie", "first")]] == 0
    assert rank[k[("shift", "max")]] == 0 and rank[k[("std8", "max")]] == 0
    i = k[("std1", "ignore")]
    assert lp[i] == 0 and rank[i] == -1 and math.isfinite(lse[i].item())
    assert torch.isfinite(lse).all(), "rows shifted by +300 or of std 8 must stay finite"


def test_token_logprob_unaligned_rows_and_automatic_switch(ops):
    """A row base that is not 16-byte aligned (a column slice, odd ld) takes the scalar loads; n on either side of the automatic
    switch between the two shapes gives what the forced shapes give."""
    V = 1000
    wide, tgt, _ = make_rows(V + 3, V + 3, 5, seed=9)
    view = wide[:, 3:]                                           # base 6 bytes off, ld = 1003
    tgt = tgt.clamp(-100, V - 1)
    got = ops.token_logprob(view, tgt, V, slices=64)
    check_against_fp64("unaligned split", got, view, tgt, V)
    check_against_fp64("unaligned rows", ops.token_logprob(view, tgt, V, slices=1), view, tgt, V)
    for n in (8, 127, 128, 200):
        buf, tgt, _ = make_rows(V, 1024, n, seed=n)
        check_against_fp64(f"auto n={n}", ops.token_logprob(buf, tgt, V), buf, tgt, V)


def test_token_logprob_row_of_minus_infinity_throughout(ops):
    """No column is finite: lse is -inf and every target's logprob is -inf (never NaN); rank counts the equal columns to the left."""
    V = 1000
    buf = torch.full((3, 1024), NINF, device="cuda", dtype=BF16)
    buf[:, V:] = float("nan")
    tgt = torch.tensor([0, 417, -100], device="cuda", dtype=I32)
    for slices in (1, 64):
        lp, lse, rank = ops.token_logprob(buf, tgt, V, slices=slices)
        assert lp.tolist() == [NINF, NINF, 0.0] and lse.tolist() == [NINF] * 3 and rank.tolist() == [0, 417, -1], slices


# ================================================================================================ B. the decode-step form
@pytest.mark.parametrize("off", [0, 7])
def test_token_logprob_step_after_greedy_pick(ops, off):
    """The layout of test_greedy_pick_matches_processors_exactly: B = 4, V = 1000, row 2 already finished, row 1 picks an eos, and
    pad == eos. Two consecutive steps: in the first the eos row holds its real value, in the second it is a finished row - which the
    emitted token (pad == eos both times) cannot tell."""
    import numpy as np
    rng = np.random.default_rng(11 + off)
    B, V, max_new, cols = 4, 1000, 40, 32
    step0 = int(rng.integers(off, off + 25))
    gen = torch.from_numpy(rng.integers(0, 12, (B, max_new))).to(torch.int64).cuda()
    logits = torch.from_numpy(rng.normal(0, 2, (B, V + 24)).astype(np.float32)).to(BF16).cuda()
    logits[1, 500] = logits[1, 700] = 30.0                                       # exact tie -> first index -> 500 = eos
    logits[:, V:] = float("nan")
    fin = torch.tensor([0, 0, 1, 0], dtype=I32).cuda()
    eos = torch.tensor([500, 3], dtype=torch.int64).cuda()
    pad = 500
    done = fin.clone()                                                            # the flags as they stand before the first pick
    nxt = torch.zeros(B, dtype=I32, device="cuda")
    st = torch.tensor([step0], dtype=I32, device="cuda")
    pick_work = torch.zeros(B * 128 + 8, device="cuda")
    work = torch.zeros(B * ops.LOGPROB_WORK_PER_ROW, device="cuda")
    lp = torch.full((B, cols), 7.5, device="cuda")
    rk = torch.full((B, cols), 99, dtype=I32, device="cuda")
    lse64, _, _, lmax = reference(logits, torch.zeros(B, dtype=I32, device="cuda"), V)
    before = logits.clone()
    for k, (was, fin_after) in enumerate([([0, 0, 1, 0], [0, 1, 1, 0]), ([0, 1, 1, 0], [0, 1, 1, 0])]):
        ops.greedy_pick(logits, pick_work, gen, st, fin, 1.0, 0, eos, pad, nxt, V)
        ops.token_logprob_step(logits, V, nxt, st, off, fin, done, lp, work, rank=rk)
        col = step0 + k - off
        assert fin.tolist() == fin_after and done.tolist() == fin_after
        assert int(nxt[1]) == 500 and int(nxt[2]) == pad
        for b in range(B):
            if was[b]:
                assert lp[b, col].item() == 0.0 and rk[b, col].item() == -1, (k, b)
            else:
                want = logits[b, int(nxt[b])].double() - lse64[b]
                assert abs(lp[b, col].item() - want.item()) <= lse_err(lse64[b], lmax[b]).item(), (k, b)
                assert rk[b, col].item() == 0, "no penalty, no ban: the pick is the raw argmax"
        if k == 0:
            assert lp[1, col].item() < -0.6, "the step that emits the eos carries its real log-probability (two tied maxima: < -log 2)"
        ops.decode_advance(None, B, st)
    written = torch.zeros(B, cols, dtype=torch.bool, device="cuda")
    written[:, step0 - off: step0 - off + 2] = True
    assert (lp[~written] == 7.5).all() and (rk[~written] == 99).all(), "only the step's column may be written"
    assert torch.equal(bits(logits), bits(before))
    # a column outside [0, cols) writes nothing (and still keeps the flags' record)
    st.fill_(off + cols)
    snap = lp.clone()
    ops.token_logprob_step(logits, V, nxt, st, off, fin, done, lp, work)
    assert torch.equal(lp, snap)


# ================================================================================================ C. generate(output_logprobs=True)
def _tiny_model():
    from tests.test_parity_gpu import _tiny_qcfg
    from vggt_qwen3_amd.qwen3 import Qwen3ForCausalLM
    z = load("qwen3_tiny.npz")
    c = meta(z, "config")
    model = Qwen3ForCausalLM(_tiny_qcfg(c), device="cuda", seed=0)
    model.load_hf_state_dict(weights(z))
    return model, c


@pytest.fixture(scope="module")
def tiny():
    return _tiny_model()


def _full_logits(tm, emb_row, new_ids):
    """fp64 logits of a cache-free forward over one row's prompt embeddings + its generated ids (all but the last)."""
    full = torch.cat([emb_row[None], tm.get_input_embeddings()(new_ids[None, :-1])], dim=1)
    h, _ = tm.forward_hidden(full, torch.ones(1, full.shape[1], dtype=torch.long).cuda(), save=False)
    return tm.logits_all(h).double()


def _check_generate(tm, kw, rows, n_prompt=0):
    """ids equal with and without the flag; log-probabilities agree with log_softmax of the full forward within TIE_TOL up to and
    including a row's eos, exactly 0.0 after it. rows: (prompt embeddings without padding) per row. Returns (ids, logprobs)."""
    want = tm.generate(**kw)
    ids, lp, stats = tm.generate(output_logprobs=True, return_stats=True, **kw)
    ids2, lp2 = tm.generate(output_logprobs=True, **kw)
    assert torch.equal(ids, want) and torch.equal(ids2, want), "output_logprobs must not change the ids"
    new = ids[:, n_prompt:]
    assert lp.dtype == F32 and tuple(lp.shape) == tuple(new.shape) and torch.equal(bits(lp), bits(lp2))
    eos = kw.get("eos_token_id")
    for b, emb_row in enumerate(rows):
        ref = torch.log_softmax(_full_logits(tm, emb_row, new[b]), -1)
        n0, ended = emb_row.shape[0], False
        for t in range(new.shape[1]):
            if ended:
                assert lp[b, t].item() == 0.0, (b, t, "columns after a row's eos are exactly 0.0")
                continue
            r = ref[n0 - 1 + t, new[b, t]].item()
            assert abs(lp[b, t].item() - r) < TIE_TOL, (b, t, lp[b, t].item(), r)
            assert lp[b, t].item() < 0.0
            ended = eos is not None and int(new[b, t]) == eos
    return ids, lp, stats


@pytest.mark.parametrize("use_graph", [True, False])
@pytest.mark.parametrize("procs", [{}, dict(repetition_penalty=1.1, no_repeat_ngram_size=4)], ids=["plain", "penalty-ngram"])
def test_generate_logprobs_match_full_forward(tiny, use_graph, procs):
    tm, cfg = tiny
    torch.manual_seed(3)
    B, L = 2, 19
    emb = (torch.randn(B, L, cfg["hidden_size"]) * 0.5).to(BF16).cuda()
    kw = dict(inputs_embeds=emb, attention_mask=torch.ones(B, L, dtype=torch.long).cuda(), max_new_tokens=9, use_graph=use_graph, **procs)
    ids, lp, stats = _check_generate(tm, kw, [emb[0], emb[1]])
    assert ids.shape == (B, 9) and stats["graph"] == use_graph


@pytest.mark.parametrize("use_graph", [True, False])
def test_generate_logprobs_unequal_prompts_and_an_early_eos(tiny, use_graph):
    """B = 2, row 1 left-padded; an eos that row 0 emits early and row 1 does not (found from a run without eos), pad_token_id left to
    its fallback (= eos): the eos step holds a real value, every later step of that row exactly 0.0, row 1 goes on."""
    tm, cfg = tiny
    torch.manual_seed(5)
    B, L, NEW = 2, 17, 10
    emb = (torch.randn(B, L, cfg["hidden_size"]) * 0.5).to(BF16).cuda()
    mask = torch.ones(B, L, dtype=torch.long).cuda()
    mask[1, :5] = 0
    kw = dict(inputs_embeds=emb, attention_mask=mask, max_new_tokens=NEW, use_graph=use_graph)
    free = tm.generate(**kw).cpu()
    pick = [(r, t) for r in (0, 1) for t in range(1, 6)
            if free[r, t] not in free[1 - r] and free[r, t] not in free[r, :t]]
    assert pick, free.tolist()
    r, t = pick[0]
    kw["eos_token_id"] = int(free[r, t])
    ids, lp, _ = _check_generate(tm, kw, [emb[0], emb[1, 5:]])
    assert ids.shape[1] == NEW and int(ids[r, t]) == kw["eos_token_id"]
    assert lp[r, t].item() < 0.0 and (lp[r, t + 1:] == 0).all() and (ids[r, t + 1:] == kw["eos_token_id"]).all()
    assert (lp[1 - r] < 0).all()


def test_generate_logprobs_with_input_ids(tiny):
    """With input_ids the prompt is returned in front of the new ids; the log-probabilities cover the new ids only."""
    tm, cfg = tiny
    g = torch.Generator().manual_seed(7)
    B, L0, NEW = 2, 12, 8
    ids0 = torch.randint(1, tm.vocab, (B, L0), generator=g).cuda()
    kw = dict(input_ids=ids0, attention_mask=torch.ones(B, L0, dtype=torch.long).cuda(), max_new_tokens=NEW,
              repetition_penalty=1.1, no_repeat_ngram_size=4)
    emb = tm.get_input_embeddings()(ids0)
    ids, lp, _ = _check_generate(tm, kw, [emb[0], emb[1]], n_prompt=L0)
    assert ids.shape == (B, L0 + NEW) and lp.shape == (B, NEW) and torch.equal(ids[:, :L0], ids0)


def test_generate_logprobs_on_the_persistent_route():
    """Qwen3-4B's width, 2 layers, the full vocabulary, B = 1: the persistent layers kernel + lm_head + pick + the split shape."""
    from vggt_qwen3_amd import ops
    from tests.test_generate_gpu import _qwen4b_dims
    if not ops.decode_layers_supported(2560, 9728, 32, 8, 128, 128):
        pytest.skip("needs an MI355X (256 CUs)")
    tm, cfg = _qwen4b_dims(2)
    torch.manual_seed(7)
    L = 21
    emb = (torch.randn(1, L, cfg.hidden_size) * 0.5).to(BF16).cuda()
    kw = dict(inputs_embeds=emb, attention_mask=torch.ones(1, L, dtype=torch.long).cuda(), max_new_tokens=9, use_graph=True)
    ids, lp, stats = _check_generate(tm, kw, [emb[0]])
    assert stats["persistent"] and stats["graph"] and ids.shape == (1, 9)


# ================================================================================================ D. score()
def _score_batch(tm, seed=13):
    """B = 3, L = 21: prompts of different lengths (labels -100), answers, right padding (mask 0, labels -100)."""
    g = torch.Generator().manual_seed(seed)
    B, L = 3, 21
    ids = torch.randint(1, tm.vocab, (B, L), generator=g)
    mask = torch.ones(B, L, dtype=torch.long)
    labels = ids.clone()
    for b, (prompt, total) in enumerate([(6, 21), (9, 15), (4, 18)]):
        labels[b, :prompt] = -100
        labels[b, total:] = -100
        mask[b, total:] = 0
    return ids.cuda(), mask.cuda(), labels.cuda()


def test_score_vs_fp64_log_softmax_and_loss_head(tiny):
    tm, cfg = tiny
    ids, mask, labels = _score_batch(tm)
    B, L = ids.shape
    out = tm.score(input_ids=ids, attention_mask=mask, labels=labels)
    h, saved = tm.forward_hidden(tm.get_input_embeddings()(ids), mask, save=False)
    Lp = saved["L"]
    lg = tm.logits_all(h).view(B, Lp, -1)[:, :L]
    V = lg.shape[-1]
    # position t - 1 predicts labels[:, t]
    tgt = torch.full((B, L), -100, dtype=I32, device="cuda")
    tgt[:, 1:] = labels[:, 1:].to(I32)
    rows = torch.cat([lg.new_zeros((B, 1, V)), lg[:, :-1]], 1).reshape(B * L, V).contiguous()
    lse64, lp64, rank64, lmax = reference(rows, tgt.view(-1), V)
    lab = (tgt.view(-1) >= 0)
    assert out["logprobs"].dtype == F32 and out["ranks"].dtype == I32 and out["n_tokens"].dtype == torch.int64
    assert out["logprobs"].shape == (B, L) and out["ranks"].shape == (B, L)
    report("score logprobs", (out["logprobs"].view(-1).double() - lp64)[lab].abs(), lse_err(lse64, lmax)[lab])
    assert torch.equal(out["ranks"].view(-1).long(), rank64)
    assert (out["logprobs"].view(-1)[~lab] == 0).all() and (out["logprobs"][:, 0] == 0).all() and (out["ranks"][:, 0] == -1).all()
    assert out["n_tokens"].tolist() == [15, 6, 14]
    assert torch.allclose(out["sum_logprob"], out["logprobs"].sum(1))
    # the mean negative log-probability is the loss of the same batch: n per-row bounds plus the f32 sum, as the loss-head test bounds it
    loss, _ = tm.loss_head(h, labels, save=False, L=Lp)
    n = int(out["n_tokens"].sum())
    mine = -out["sum_logprob"].double().sum() / n
    bound = (lse_err(lse64, lmax)[lab].sum() + 2.0 ** -23 * (-lp64[lab].sum()) * (n + 1)) / n
    report("score vs loss_head", (mine - loss.double()).abs().reshape(1), 2 * bound.reshape(1))   # (both sides carry the f32 error)
    # chunking: 8 labelled rows at a time and all at once are the same bits
    for cap in (8, 1 << 20, 5):
        o2 = tm.score(input_ids=ids, attention_mask=mask, labels=labels, chunk_rows=cap)
        assert torch.equal(bits(o2["logprobs"]), bits(out["logprobs"])) and torch.equal(o2["ranks"], out["ranks"]), cap
    # inputs_embeds is the same call
    o3 = tm.score(inputs_embeds=tm.get_input_embeddings()(ids), attention_mask=mask, labels=labels)
    assert torch.equal(bits(o3["logprobs"]), bits(out["logprobs"]))


def test_score_does_not_depend_on_the_chunking_across_the_kernel_shapes(tiny):
    """More labelled rows than the row count at which vq3_token_logprob's automatic choice changes shape (128), and chunk caps on
    both sides of it, some leaving a last chunk on the other side: the two shapes sum in different orders, so score() must name one."""
    tm, cfg = tiny
    g = torch.Generator().manual_seed(29)
    B, L = 3, 96
    ids = torch.randint(1, tm.vocab, (B, L), generator=g)
    mask = torch.ones(B, L, dtype=torch.long)
    labels = ids.clone()
    for b, (prompt, total) in enumerate([(5, 96), (11, 70), (3, 91)]):
        labels[b, :prompt] = -100
        labels[b, total:] = -100
        mask[b, total:] = 0
    ids, mask, labels = ids.cuda(), mask.cuda(), labels.cuda()
    out = tm.score(input_ids=ids, attention_mask=mask, labels=labels)
    n = int(out["n_tokens"].sum())
    assert out["n_tokens"].tolist() == [91, 59, 88] and n == 238
    for cap in (8, 100, 127, 128, 150, 1 << 20):          # 150: one chunk of 150 rows and one of 88
        o2 = tm.score(input_ids=ids, attention_mask=mask, labels=labels, chunk_rows=cap)
        assert torch.equal(bits(o2["logprobs"]), bits(out["logprobs"])) and torch.equal(o2["ranks"], out["ranks"]), cap
    # and they are the right numbers
    h, saved = tm.forward_hidden(tm.get_input_embeddings()(ids), mask, save=False)
    lg = tm.logits_all(h).view(B, saved["L"], -1)[:, :L]
    V = lg.shape[-1]
    tgt = torch.full((B, L), -100, dtype=I32, device="cuda")
    tgt[:, 1:] = labels[:, 1:].to(I32)
    rows = torch.cat([lg.new_zeros((B, 1, V)), lg[:, :-1]], 1).reshape(B * L, V).contiguous()
    lse64, lp64, rank64, lmax = reference(rows, tgt.view(-1), V)
    lab = tgt.view(-1) >= 0
    report("score logprobs, 238 rows", (out["logprobs"].view(-1).double() - lp64)[lab].abs(), lse_err(lse64, lmax)[lab])
    assert torch.equal(out["ranks"].view(-1).long(), rank64)


def test_score_all_ignored_batch_returns_zeros(tiny):
    tm, cfg = tiny
    ids, mask, labels = _score_batch(tm)
    out = tm.score(input_ids=ids, attention_mask=mask, labels=torch.full_like(labels, -100))
    assert (out["logprobs"] == 0).all() and (out["ranks"] == -1).all() and (out["sum_logprob"] == 0).all() and (out["n_tokens"] == 0).all()
    assert out["logprobs"].shape == ids.shape


def test_score_is_consistent_with_greedy_generation(tiny):
    """Scoring prompt + greedy continuation: every generated position whose top-2 gap in the full-forward logits exceeds the tie
    tolerance has rank 0, and its log-probability is the one generate() reported (within the decode-vs-full-forward tolerance)."""
    tm, cfg = tiny
    g = torch.Generator().manual_seed(17)
    B, L0, NEW = 2, 11, 9
    ids0 = torch.randint(1, tm.vocab, (B, L0), generator=g).cuda()
    ids, lp = tm.generate(input_ids=ids0, attention_mask=torch.ones(B, L0, dtype=torch.long).cuda(), max_new_tokens=NEW,
                          output_logprobs=True)
    labels = ids.clone()
    labels[:, :L0] = -100
    out = tm.score(input_ids=ids, labels=labels)
    h, saved = tm.forward_hidden(tm.get_input_embeddings()(ids), torch.ones_like(ids), save=False)
    lg = tm.logits_all(h).view(B, saved["L"], -1).float()
    top2 = lg[:, L0 - 1: L0 + NEW - 1].topk(2, -1).values
    clear = (top2[..., 0] - top2[..., 1]) > TIE_TOL
    assert clear.any()
    assert (out["ranks"][:, L0:][clear] == 0).all()
    assert ((out["logprobs"][:, L0:] - lp).abs() < TIE_TOL).all()
    assert out["n_tokens"].tolist() == [NEW, NEW]


def test_vlm_score_leaves_training_state_alone():
    """VGGTQwen3VLM.score on the small VLM of the parity tests, in train mode between a backward and the next forward: flat_g and the
    module modes are unchanged, the next forward gives the loss it gave before, and the scores add up to that loss."""
    import numpy as np
    from tests.test_parity_gpu import _build_vlm
    z = load("vlm_tiny.npz")
    m = meta(z)
    model = _build_vlm(z, m).train()
    geom = {k: torch.from_numpy(z["geom:" + k]).cuda() for k in ("R", "t", "K", "depth_hist")}
    geom["mask"] = torch.from_numpy(z["geom_mask"]).cuda()
    images = torch.from_numpy(z["pixel_values"].astype(np.float32)).cuda()
    ids, mask, labels = (torch.from_numpy(z[k]).cuda() for k in ("input_ids", "attention_mask", "labels"))
    args = dict(images=images, geom_token=geom, input_ids=ids, attention_mask=mask, labels=labels)
    loss0 = model(**args)
    loss0.backward()
    torch.cuda.synchronize()
    g0 = model.text_model.flat_g.clone()
    modes = [mod.training for mod in model.modules()]
    out = model.score(**args)
    torch.cuda.synchronize()
    assert torch.equal(bits(model.text_model.flat_g), bits(g0)), "score() must not touch the gradient buffer"
    assert [mod.training for mod in model.modules()] == modes and model.training
    assert out["logprobs"].shape == labels.shape and out["ranks"].shape == labels.shape
    want = labels.clone()
    want[:, 0] = -100
    assert torch.equal(out["ranks"] >= 0, want != -100)
    n = int(out["n_tokens"].sum())
    assert n == int((want != -100).sum()) and n > 0
    # (train-mode forward against eval-mode scoring: the loss tolerance the parity tests use between two implementations)
    assert abs(-out["sum_logprob"].sum().item() / n - loss0.item()) <= 5e-3 * abs(loss0.item())
    loss1 = model(**args)
    # the same kernels on the same inputs; the loss is an f32 atomic sum over n rows, whose order is free: n * 2^-24 relative
    assert abs(loss1.item() - loss0.item()) <= 1e-5 * abs(loss0.item()), (loss0.item(), loss1.item())
