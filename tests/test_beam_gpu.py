"""Beam search on the device (csrc/beam.hip, generate.beam_search).

A. vq3_beam_step against tests/beam_ref.py in fp64 (the restatement of transformers' _beam_search that tests/test_beam_host.py pins to
   transformers' own outputs): exact on every integer output, scores within 1e-5 * max(1, |score|) - the f32 rounding of a 1000-term
   logsumexp plus one add. Every case first asserts, on the reference alone, that neighbouring candidates are at least 1e-3 apart (100
   times the score tolerance) wherever an order is decided, so the kept sets cannot legitimately differ; the seeds are fixed so that
   this holds (checked on the CPU: _case() needs no GPU). The finished sequence of a slot whose flag is 0 is not compared: such slots
   tie at -1e9 and hold nothing a caller sees.
B. vq3_beam_reorder against torch's gather, exact, untouched past `lens` and in the guard bands.
C. beam_search() end to end on the tiny Qwen3."""
import numpy as np
import pytest
import torch

from tests import beam_ref
from tests.golden_io import load, meta, weights
from tests.test_generate_gpu import TIE_TOL

pytestmark = pytest.mark.gpu
BF16, F32, I32 = torch.bfloat16, torch.float32, torch.int32
GAP, SCORE_TOL = 1e-3, 1e-5
GUARD = 64
SENT_I, SENT_F = 0x5A5A5A5A, 12345.0


@pytest.fixture(scope="module")
def ops():
    from vggt_qwen3_amd import _lib
    from vggt_qwen3_amd import ops as _ops
    _lib.load()
    return _ops


# ================================================================================================ A. vq3_beam_step
def _distinct_bf16(n, g):
    """n distinct bf16 values of magnitude [0.5, 8): neighbours are at least 2^-8 apart."""
    bits = np.concatenate([np.arange(0x3F00, 0x4100), np.arange(0xBF00, 0xC100)]).astype(np.uint16)      # 4 binades x 128, both signs
    assert n <= bits.size
    pick = bits[torch.randperm(bits.size, generator=g).numpy()[:n]]
    return torch.from_numpy(pick.view(np.int16).copy()).view(BF16)


def _logits(R, V, ld, g):
    """Every row a shuffle of V distinct bf16 values; past 1024 ids (a bf16 has no more distinct values of one magnitude) the rest of
    the row lies in (-16, -8], far below anything a top K reaches. Columns [V, ld) hold +inf-like bait that must never be read."""
    out = torch.full((R, ld), 3.0e38, dtype=BF16)
    for r in range(R):
        if V <= 1024:
            row = _distinct_bf16(V, g)
        else:
            low = torch.from_numpy((0xC100 + torch.randint(0, 128, (V - 1024,), generator=g).numpy()).astype(np.uint16).view(np.int16)).view(BF16)
            row = torch.cat([_distinct_bf16(1024, g), low])
        out[r, :V] = row[torch.randperm(V, generator=g)]
    return out


CASES = [
    # name, (B, nb), V, ld, state, n_eos, length_penalty, early_stopping, penalty, ngram, prompt_len
    ("first_2x3", (2, 3), 1000, 1024, "first", 1, 1.0, False, 1.0, 0, 0),
    ("first_1x8_v40", (1, 8), 40, 40, "first", 0, 1.0, False, 1.0, 0, 0),
    ("first_4x2_ids", (4, 2), 1000, 1024, "first", 2, 1.0, False, 1.3, 2, 5),
    ("middle_2x3", (2, 3), 1000, 1024, "middle", 1, 1.0, False, 1.0, 0, 0),
    ("middle_2x3_proc", (2, 3), 1000, 1024, "middle", 1, 1.0, False, 1.3, 2, 0),
    ("middle_1x8_proc3", (1, 8), 1000, 1024, "middle", 2, 2.0, "never", 1.1, 3, 4),
    ("middle_4x2_noeos", (4, 2), 1000, 1024, "middle", 0, 0.0, False, 1.0, 0, 0),
    ("middle_2x4_eos2", (2, 4), 1000, 1001, "middle", 2, 1.0, True, 1.2, 0, 3),
    ("middle_2x4_eos3", (2, 4), 1000, 1024, "middle", 3, 0.0, True, 1.0, 2, 0),
    ("middle_1x8_v40", (1, 8), 40, 48, "middle", 1, 1.0, False, 1.0, 0, 0),
    ("last_2x3", (2, 3), 1000, 1024, "last", 1, 1.0, False, 1.0, 0, 0),
    ("last_2x4_lp2", (2, 4), 1000, 1024, "last", 2, 2.0, "never", 1.3, 2, 3),
    ("full_false", (2, 3), 1000, 1024, "full", 1, 1.0, False, 1.0, 0, 0),
    ("full_true", (2, 3), 1000, 1024, "full", 1, 1.0, True, 1.0, 0, 0),
    ("full_never", (2, 3), 1000, 1024, "full", 1, 1.0, "never", 1.0, 0, 0),
    ("full_never_lp0", (2, 4), 1000, 1024, "full", 2, 0.0, "never", 1.2, 2, 0),
    ("full_true_lp2", (4, 2), 1000, 1024, "full", 1, 2.0, True, 1.0, 0, 2),
    ("heur_false", (2, 3), 1000, 1024, "heur_false", 1, 1.0, False, 1.0, 0, 0),
    ("heur_false_one", (2, 4), 1000, 1024, "heur_one", 2, 1.0, False, 1.1, 2, 0),
    ("big_1x8", (1, 8), 151936, 151936, "middle", 2, 1.0, False, 1.3, 2, 0),
]
SEEDS = {"middle_1x8_v40": 100}          # name -> seed, where the default (the case's index) does not meet the precondition


def _case(idx):
    """Inputs, the initial state and the fp64 reference's next state of CASES[idx]; asserts the reference's own gaps. CPU only."""
    name, (B, nb), V, ld, state, n_eos, lpen, early, penalty, ngram, P = CASES[idx]
    g = torch.Generator().manual_seed(1000 + SEEDS.get(name, idx))
    R = B * nb
    new = {"first": 0, "last": 3}.get(state, 5)
    cur = P + new
    max_len = cur + 1 if state == "last" else P + 12
    logits = _logits(R, V, ld, g)
    alphabet = torch.randperm(min(V, 1000), generator=g)[:12]
    ref = beam_ref.BeamRef(alphabet[torch.randint(0, 12, (B, P), generator=g)], nb, max_len, [], lpen, early, fill=0)
    ref.cur_len = cur
    if state != "first":
        ref.running_sequences[:, :, P:cur] = alphabet[torch.randint(0, 12, (B, nb, new), generator=g)]
        ref.running_beam_indices[:, :, :new] = (torch.arange(B) * nb).to(I32)[:, None, None]      # (the reference counts lengths from these)
        ref.running_beam_scores = -(torch.rand((B, nb), generator=g, dtype=torch.float64) * 4 + 1).sort(dim=1, descending=True).values
        n_filled = {"middle": 1, "last": 1, "heur_one": nb}.get(state, nb)
        for b in range(B):
            k = n_filled if (state != "middle" or b == 0) else 0         # middle: prompt 0 has one finished hypothesis, the others none
            sc = -(torch.rand(k, generator=g, dtype=torch.float64) * 2 + 0.5)
            ref.beam_scores[b, :k] = sc.sort(descending=True).values
            for j in range(k):
                n = int(torch.randint(1, new + 1, (1,), generator=g))
                ref.sequences[b, j, P:P + n] = alphabet[torch.randint(0, 12, (n,), generator=g)]
                ref.beam_indices[b, j, :n] = b * nb
                ref.is_sent_finished[b, j] = True
        if state == "heur_false":
            ref.heuristic[:] = False
        if state == "heur_one":
            ref.heuristic[0] = False
    init = dict(run_seq=ref.running_sequences.clone(), run_score=ref.running_beam_scores.clone(), fin_seq=ref.sequences.clone(),
                fin_score=ref.beam_scores.clone(), fin_len=ref.finished_lengths() * ref.is_sent_finished, fin_flag=ref.is_sent_finished.clone(),
                heur=ref.heuristic.clone())
    lp = beam_ref.process(logits[:, :V], ref.rows(), penalty, ngram)
    # eos ids planted among the top candidates: the token of rank 1 of prompt 0, of rank nb of the last prompt, of rank 0 of prompt 0
    acc = (lp.reshape(B, nb, V) + ref.running_beam_scores[:, :, None]).reshape(B, nb * V)
    order = torch.topk(acc, 3 * nb)[1] % V
    eos = [int(order[0, 1]), int(order[B - 1, nb]), int(order[0, 0])][:n_eos]
    ref.eos, ref.K = eos, max(2, 1 + n_eos) * nb
    ref.step(lp)
    # the precondition, on the reference alone
    K, last = ref.K, ref.last
    top = torch.topk(last["acc"], K + 1)[0]
    assert (top[:, :-1] - top[:, 1:]).min() >= GAP, (name, "candidates")
    for b in range(B):
        real = last["merged_scores"][b][last["merged_scores"][b] > -1e8].sort(descending=True).values
        assert real.numel() < 2 or (real[:-1] - real[1:]).min() >= GAP, (name, "finished-slot merge")
        w = last["worst"][b][last["worst"][b] > -1e8]
        assert w.numel() == 0 or (last["best_running"][b] - w).abs().min() >= GAP, (name, "heuristic")
    return dict(name=name, B=B, nb=nb, V=V, ld=ld, P=P, cur=cur, max_len=max_len, logits=logits, eos=eos, lpen=lpen, early=early,
                penalty=penalty, ngram=ngram, init=init, ref=ref)


def _guarded(t, sent):
    """A copy of t on the device between two bands of sentinels -> (view, whole buffer)."""
    whole = torch.full((t.numel() + 2 * GUARD,), sent, dtype=t.dtype, device="cuda")
    view = whole[GUARD:GUARD + t.numel()].view(t.shape)
    view.copy_(t)
    return view, whole


def _device_state(ops, c):
    bs = ops.BeamState(c["B"], c["nb"], c["max_len"], c["P"], c["max_len"] - c["P"], "cuda")
    R, init, wholes = c["B"] * c["nb"], c["init"], {}
    src = dict(run_seq=init["run_seq"].reshape(R, -1).to(I32), fin_seq=init["fin_seq"].reshape(R, -1).to(I32),
               run_score=init["run_score"].reshape(R).to(F32), fin_score=init["fin_score"].reshape(R).to(F32),
               fin_len=init["fin_len"].reshape(R).to(I32), fin_flag=init["fin_flag"].reshape(R).to(I32), heur=init["heur"].reshape(-1).to(I32),
               all_done=bs.all_done.cpu(), src_row=torch.full((R,), -7, dtype=I32), trace_parent=bs.trace_parent.cpu(),
               trace_token=bs.trace_token.cpu(), trace_score=bs.trace_score.cpu(), work=bs.work.cpu())
    for k, t in src.items():
        view, wholes[k] = _guarded(t, SENT_F if t.dtype == F32 else SENT_I)
        setattr(bs, k, view)
    next_ids, wholes["next_ids"] = _guarded(torch.full((R,), -7, dtype=I32), SENT_I)
    return bs, next_ids, wholes


def _guards_intact(wholes):
    for k, w in wholes.items():
        sent = SENT_F if w.dtype == F32 else SENT_I
        assert bool((w[:GUARD] == sent).all()) and bool((w[-GUARD:] == sent).all()), f"{k}: guard band overwritten"


def _close(got, want, what):
    got, want = got.double().cpu().reshape(-1), want.double().reshape(-1)
    err = (got - want).abs()
    tol = SCORE_TOL * want.abs().clamp(min=1.0)
    print(f"{what}: max |err| / tol = {float((err / tol).max()):.3f}")
    assert bool((err <= tol).all()), (what, got.tolist(), want.tolist())


@pytest.mark.parametrize("idx", range(len(CASES)), ids=[c[0] for c in CASES])
def test_beam_step_matches_the_reference(ops, idx):
    c = _case(idx)
    ref, B, nb, cur, P = c["ref"], c["B"], c["nb"], c["cur"], c["P"]
    R = B * nb
    bs, next_ids, wholes = _device_state(ops, c)
    logits = c["logits"].cuda()
    step = torch.tensor([cur], dtype=I32, device="cuda")
    ops.beam_step(logits, c["V"], bs, step, next_ids, c["penalty"], c["ngram"], c["eos"], c["lpen"], c["early"])
    torch.cuda.synchronize()
    _guards_intact(wholes)
    parents, tokens = ref.last["parents"].to(I32), ref.last["tokens"].to(I32)
    assert torch.equal(bs.src_row.cpu(), parents) and torch.equal(next_ids.cpu(), tokens)
    assert torch.equal(bs.run_seq.cpu()[:, :cur + 1].long(), ref.running_sequences.reshape(R, -1)[:, :cur + 1])
    t = cur - P
    assert torch.equal(bs.trace_parent.cpu()[t], parents) and torch.equal(bs.trace_token.cpu()[t], tokens)
    assert bool((bs.trace_parent.cpu()[t + 1:] == -1).all()) and bool((bs.trace_parent.cpu()[:t] == -1).all())
    assert torch.equal(bs.trace_score.cpu()[t], bs.run_score.cpu())
    _close(bs.run_score, ref.running_beam_scores, "running scores")
    flags = ref.is_sent_finished.reshape(R)
    assert torch.equal(bs.fin_flag.cpu().bool(), flags)
    _close(bs.fin_score, ref.beam_scores, "finished scores")
    lens = ref.finished_lengths().reshape(R)
    fin_seq, fin_len = bs.fin_seq.cpu().long(), bs.fin_len.cpu().long()
    for r in range(R):
        if flags[r]:
            assert int(fin_len[r]) == int(lens[r]), (r, fin_len.tolist(), lens.tolist())
            assert torch.equal(fin_seq[r, :lens[r]], ref.sequences.reshape(R, -1)[r, :lens[r]]), r
    assert torch.equal(bs.heur.cpu().bool(), ref.heuristic.reshape(-1))
    assert int(bs.all_done.item()) == int(ref.done)
    if c["name"].startswith("last"):
        assert ref.done and bool(ref.last["hit"].all())
    if c["name"] == "first_1x8_v40":
        assert bool((parents == 0).all())                      # all 16 candidates came from beam 0
    # a call made after all_done leaves every buffer as it is, bit for bit (work included)
    bs.all_done.fill_(1)
    before = {k: w.clone() for k, w in wholes.items()}
    step += 1
    ops.beam_step(logits, c["V"], bs, step, next_ids, c["penalty"], c["ngram"], c["eos"], c["lpen"], c["early"])
    torch.cuda.synchronize()
    for k, w in wholes.items():
        assert torch.equal(w.view(I32), before[k].view(I32)), f"{k} changed after all_done"


def test_beam_step_repeats_its_bits(ops):
    c = _case(4)
    outs = []
    for _ in range(2):
        bs, next_ids, wholes = _device_state(ops, c)
        ops.beam_step(c["logits"].cuda(), c["V"], bs, torch.tensor([c["cur"]], dtype=I32, device="cuda"), next_ids, c["penalty"], c["ngram"],
                      c["eos"], c["lpen"], c["early"])
        torch.cuda.synchronize()
        outs.append({k: w.view(I32).clone() for k, w in wholes.items()})
    for k in outs[0]:
        assert torch.equal(outs[0][k], outs[1][k]), k


# ================================================================================================ B. vq3_beam_reorder
def _reorder_case(ops, R, nb, lens, src, Lmax=128, layers=2, Hkv=2):
    g = torch.Generator().manual_seed(5)
    shape = (layers, R, Hkv, Lmax, 128)
    K0 = torch.randn(shape, generator=g).to(BF16)
    V0 = torch.randn(shape, generator=g).to(BF16)
    Kd, Kw = _guarded(K0.view(torch.int16), 0x5A5A)
    Vd, Vw = _guarded(V0.view(torch.int16), 0x5A5A)
    lens_t = torch.tensor(lens, dtype=I32, device="cuda")
    ops.beam_reorder(Kd.view(BF16), Vd.view(BF16), torch.tensor(src, dtype=I32, device="cuda"), lens_t, R // nb, nb)
    torch.cuda.synchronize()
    for got, whole, old in ((Kd, Kw, K0), (Vd, Vw, V0)):
        assert bool((whole[:GUARD] == 0x5A5A).all()) and bool((whole[-GUARD:] == 0x5A5A).all()), "guard band overwritten"
        old = old.view(torch.int16)
        want = old.clone()
        for r in range(R):
            want[:, r, :, :lens[r] + 1] = old[:, src[r], :, :lens[r] + 1]           # positions past lens keep what they held
        assert torch.equal(got.cpu(), want)
    return Kd, K0


@pytest.mark.parametrize("lens", [(5, 5, 5, 126, 126, 126), (0, 0, 0, 77, 77, 77)])
def test_beam_reorder_gathers_rows_in_place(ops, lens):
    _reorder_case(ops, 6, 3, lens, [1, 1, 0, 5, 3, 3])          # duplicates, a swap-like pattern, a row that is someone else's source


def test_beam_reorder_identity_and_full_cycle(ops):
    Kd, K0 = _reorder_case(ops, 6, 3, (5, 5, 5, 126, 126, 126), [0, 1, 2, 3, 4, 5])
    assert torch.equal(Kd.cpu(), K0.view(torch.int16))
    _reorder_case(ops, 8, 8, (127,) * 8, [1, 2, 3, 4, 5, 6, 7, 0])
    _reorder_case(ops, 8, 8, (40,) * 8, [7, 0, 1, 2, 3, 4, 5, 6], Lmax=64)
    _reorder_case(ops, 8, 2, (3, 3, 9, 9, 0, 0, 63, 63), [1, 0, 2, 2, 4, 5, 7, 7], Lmax=64)


def test_beam_reorder_does_nothing_once_all_done(ops):
    g = torch.Generator().manual_seed(6)
    K0 = torch.randn((1, 4, 1, 64, 128), generator=g).to(BF16).cuda()
    V0 = K0 + 1
    Kd, Vd = K0.clone(), V0.clone()
    done = torch.ones(1, dtype=I32, device="cuda")
    ops.beam_reorder(Kd, Vd, torch.tensor([1, 0, 3, 2], dtype=I32, device="cuda"), torch.full((4,), 20, dtype=I32, device="cuda"), 2, 2, done)
    assert torch.equal(Kd, K0) and torch.equal(Vd, V0)


# ================================================================================================ C. beam_search() on the tiny model
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


@pytest.fixture(scope="module")
def search(tiny):
    """2 left-padded prompts x 3 beams, 10 steps, with an eos taken from a free run so that hypotheses finish on the way; run with the
    graph, without it, and once more with it. Shared by the tests below."""
    tm, cfg = tiny
    g = torch.Generator().manual_seed(91)
    emb = (torch.randn(2, 14, cfg["hidden_size"], generator=g) * 0.5).to(BF16).cuda()
    mask = torch.ones(2, 14, dtype=torch.long)
    mask[1, :5] = 0
    mask = mask.cuda()
    kw = dict(inputs_embeds=emb, attention_mask=mask, max_new_tokens=10, num_beams=3, num_return_sequences=2, return_scores=True,
              return_stats=True, check_every=4)
    _, _, free = tm.beam_search(**kw)
    toks = free["tokens"].cpu()
    early = set(toks[:3].reshape(-1).tolist())
    late = [int(t) for t in toks[3:8].reshape(-1).tolist() if int(t) not in early]
    eos = late[0] if late else int(toks[4, 0])             # an id some running beam emitted at steps 3..7 and none before
    kw.update(eos_token_id=eos, pad_token_id=317)
    runs = [tm.beam_search(use_graph=ug, **kw) for ug in (True, False, True)]
    return dict(tm=tm, emb=emb, mask=mask, eos=eos, kw=kw, runs=runs, free=free)


def test_search_graph_and_eager_give_the_same_bits(search):
    (s0, sc0, st0), (s1, sc1, st1), (s2, sc2, st2) = search["runs"]
    assert st0["graph"] and not st1["graph"] and st2["graph"]
    for s, sc, st in ((s1, sc1, st1), (s2, sc2, st2)):
        assert torch.equal(s, s0) and torch.equal(sc.view(I32), sc0.view(I32)) and st["steps_run"] == st0["steps_run"]
        for k in ("parents", "tokens"):
            assert torch.equal(st[k], st0[k]), k
        assert torch.equal(st["running_scores"].view(I32), st0["running_scores"].view(I32))
    assert st0["parents"].shape == (st0["steps_run"], 6) and 1 <= st0["steps_run"] <= 10


def _row_embeds(search, r, ids):
    """Prompt row r // 3 without its padding, then the embeddings of ids."""
    b = r // 3
    emb = search["emb"][b][search["mask"][b] != 0]
    if len(ids) == 0:
        return emb
    return torch.cat([emb, search["tm"].get_input_embeddings()(torch.tensor(ids, device="cuda")[None])[0]], dim=0)


def test_search_trace_agrees_with_the_cache_free_forward(search):
    """The cache rows follow the surviving beams: at every step, each candidate the device kept scores - under a forward WITHOUT a cache
    over the sequence the trace says its parent had - within TIE_TOL of the K-th best recomputed candidate. A cache row taken from the
    wrong beam misses by several units."""
    tm = search["tm"]
    _, _, st = search["runs"][0]
    nb, R, V, K = 3, 6, tm.vocab, 2 * 3
    seqs = [[] for _ in range(R)]
    scores = torch.tensor([0.0, -1e9, -1e9] * 2, dtype=torch.float64)
    assert st["steps_run"] >= 2
    for t in range(st["steps_run"]):
        acc = torch.empty((R, V), dtype=torch.float64)
        for b in range(2):                                  # the rows of a prompt have one length: one forward
            x = torch.stack([_row_embeds(search, r, seqs[r]) for r in range(b * nb, (b + 1) * nb)], dim=0)
            h, saved = tm.forward_hidden(x, torch.ones(x.shape[:2], dtype=torch.long, device="cuda"), save=False)
            lg = tm.logits_all(h).view(nb, saved["L"], -1)[:, x.shape[1] - 1, :V].double().cpu()
            acc[b * nb:(b + 1) * nb] = torch.log_softmax(lg, -1) + scores[b * nb:(b + 1) * nb, None]
        parents, tokens = st["parents"][t].cpu().tolist(), st["tokens"][t].cpu().tolist()
        for b in range(2):
            kth = torch.topk(acc[b * nb:(b + 1) * nb].reshape(-1), K)[0][-1]
            for r in range(b * nb, (b + 1) * nb):
                assert b * nb <= parents[r] < (b + 1) * nb
                assert acc[parents[r], tokens[r]] >= kth - TIE_TOL, (t, r, float(acc[parents[r], tokens[r]]), float(kth))
        seqs = [seqs[parents[r]] + [tokens[r]] for r in range(R)]
        scores = st["running_scores"][t].double().cpu()
    assert int(st["finished"]["lengths"].min()) < 10          # the eos let a hypothesis finish on the way


def test_search_scores_agree_with_score(search):
    """sequences_scores * n ** length_penalty is the summed raw log-probability of the hypothesis given its prompt (processors off)."""
    tm = search["tm"]
    seqs, sc, st = search["runs"][0]
    checked = 0
    for i in range(seqs.shape[0]):
        ids = seqs[i].tolist()
        n = int(st["finished"]["lengths"].view(2, 3)[i // 2, i % 2])
        assert all(t == 317 for t in ids[n:])
        x = _row_embeds(search, (i // 2) * 3, ids[:n])[None]
        P = x.shape[1] - n
        labels = torch.full((1, x.shape[1]), -100, dtype=torch.long, device="cuda")
        labels[0, P:] = torch.tensor(ids[:n], device="cuda")
        out = tm.score(inputs_embeds=x, attention_mask=torch.ones(x.shape[:2], dtype=torch.long, device="cuda"), labels=labels)
        assert int(out["n_tokens"][0]) == n
        assert abs(float(sc[i]) * n ** 1.0 - float(out["sum_logprob"][0])) < TIE_TOL * n, (i, float(sc[i]), float(out["sum_logprob"][0]), n)
        checked += 1
    assert checked == 4


def test_search_output_assembly(search):
    """Order, crop and fill of the returned rows: beam_ref's assembly fed the device's own finished slots."""
    for nret in (1, 2, 3):
        kw = dict(search["kw"], num_return_sequences=nret)
        seqs, sc, st = search["tm"].beam_search(**kw)
        fin = st["finished"]
        want = beam_ref.assemble(fin["sequences"].cpu().long().view(2, 3, -1), fin["lengths"].cpu().long().view(2, 3), nret, 317)
        assert seqs.dtype == torch.int64 and torch.equal(seqs.cpu(), want)
        assert torch.equal(sc.cpu(), fin["scores"].cpu().view(2, 3)[:, :nret].reshape(-1))
        assert bool((sc.view(2, nret)[:, :-1] >= sc.view(2, nret)[:, 1:]).all())           # best first
        assert seqs.shape[0] == 2 * nret and seqs.shape[1] == int(fin["lengths"].view(2, 3)[:, :nret].max())
        if nret == 3:
            assert bool((seqs == 317).any())              # a returned hypothesis is shorter than the longest: the fill is exercised


def test_search_with_input_ids_returns_the_prompt_in_front(tiny):
    tm, cfg = tiny
    z = load("beam_tiny.npz")
    ids = torch.from_numpy(z["input_ids"]).cuda()
    out, sc = tm.beam_search(input_ids=ids, num_beams=4, num_return_sequences=4, max_new_tokens=12, repetition_penalty=1.1,
                             no_repeat_ngram_size=2, eos_token_id=319, pad_token_id=318, return_scores=True)
    assert out.shape == (4, 9 + 12) and torch.equal(out[:, :9], ids.expand(4, -1))
    assert bool((sc[:-1] >= sc[1:]).all())
    new = out[:, 9:].tolist()
    for row in new:                                        # the 2-gram ban held along every returned hypothesis
        grams = list(zip(row[:-1], row[1:]))
        assert len(set(grams)) == len(grams)
    assert len({tuple(r) for r in new}) == 4


def test_generate_still_refuses_beams_and_names_beam_search(tiny):
    tm, cfg = tiny
    e = torch.zeros(1, 4, cfg["hidden_size"], device="cuda", dtype=BF16)
    with pytest.raises(NotImplementedError, match=r"beam_search\(\)"):
        tm.generate(inputs_embeds=e, num_beams=4)
