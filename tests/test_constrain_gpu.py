"""Decoding constraints on the device (the masked picks of csrc/decode.hip and sample.hip; generate.py's suppress_tokens,
begin_suppress_tokens, min_new_tokens, allowed_token_ids, bad_words_ids on generate() and sample()).

A. vq3_greedy_pick_masked / vq3_sample_pick_masked against tests/constrain_ref.py composed with the fp64 reference pick of
   tests/test_sample_host.py, on the same bf16 logits: the picked id, the kept-set size and the smallest kept score are equal (the
   score to the one f32 rounding of z / T, as in tests/test_sample_gpu.py). Every sample case first asserts, on the reference alone,
   that its two best perturbed scores are at least GAP apart and that the top-p boundary is clear of top_p - the preconditions of
   tests/test_sample_gpu.py, met by construction here, so no pick is skipped.
B. generate() / sample() end to end on the tiny golden model against tests/golden/constrain_tiny.npz."""
import functools

import numpy as np
import pytest
import torch

from tests.constrain_ref import constrain, masked_ids
from tests.golden_io import bf16, load, meta
from tests.test_sample_host import noise, processed_logits, ref_cut, ref_prepare

pytestmark = pytest.mark.gpu
BF16, F32, I32 = torch.bfloat16, torch.float32, torch.int32
GAP = 1e-4                            # tests/test_sample_gpu.py
SEED = 0x9E3779B97F4A7C15
TEMP = 0.7
PAD = 5
MAX_IDS = 64


@pytest.fixture(scope="module")
def ops():
    from vggt_qwen3_amd import _lib
    from vggt_qwen3_amd import ops as _ops
    _lib.load()
    return _ops


def _device_mask(ops, V, prompt_cols, garbage=True, **kw):
    """The product's own host path (plan -> planes -> PickMask); with `garbage` every bit at or past V is set, in the last word and in
    two words more than the vocabulary needs: the kernels must not look at them."""
    from vggt_qwen3_amd import generate as G
    plan = G._plan_constraints("test", V, MAX_IDS, **kw)
    assert plan is not None
    planes = ops.mask_planes(V, plan["always"], plan["until_min"], plan["at_begin"])
    if garbage:
        planes = np.concatenate([planes, np.full((3, 2), 0xFFFFFFFF, np.uint32)], axis=1)
        if V % 32:
            planes[:, V // 32] |= np.uint32((0xFFFFFFFF << (V % 32)) & 0xFFFFFFFF)
    return ops.PickMask(planes, plan["min_new"], prompt_cols, "cuda")


# ================================================================================================ A. the picks
def _special_ids(V):
    """Where a mask bit can go wrong: id 0, ids 31 / 32 (a word boundary), the first and last id of slices 1 and 17 and the last id of
    slice 0 (64 slices of ceil(V / 64) ids: at V = 2051, 33 ids - slices straddle the 32-bit words), V - 2 and V - 1."""
    per = (V + 63) // 64
    ids = list(dict.fromkeys([0, 31, 32, per - 1, per, 2 * per - 1, 17 * per, 18 * per - 1, V - 2, V - 1]))     # (at V = 2051, per - 1 is 32)
    assert len(ids) >= 9 and max(ids) < V
    return ids


@functools.lru_cache(maxsize=None)
def _rows(V, B=3):
    """B rows of bf16 logits ~ 4 N(0, 1) in which the special ids hold the row's best values, descending in the order of _special_ids
    rotated by the row index (distinct, 0.5 apart: masking the best moves the pick to the next special id), padded to ld > V with
    columns that would win if they were read; a history over a 12-id alphabet of special and ordinary ids whose last bigram repeats
    an earlier one."""
    rng = np.random.default_rng([V, B, 77])
    ld = (V + 15) // 8 * 8 + 3
    logits = torch.full((B, ld), 100.0).to(BF16)
    sp = _special_ids(V)
    gen = np.zeros((B, MAX_IDS), np.int64)
    for b in range(B):
        lf = np.clip(4 * rng.standard_normal(V), -30, 11.0).astype(np.float32)
        order = sp[b:] + sp[:b]
        lf[order] = 24.0 - 0.5 * np.arange(len(order))
        logits[b, :V] = torch.from_numpy(lf).to(BF16)
        alphabet = np.concatenate([order[:6], rng.integers(0, V, 6)])
        gen[b] = rng.choice(alphabet, MAX_IDS)
        gen[b, 18:20] = gen[b, 6:8]                                # at 20 ids the last bigram repeats the one at 6-7: id gen[b, 8] is banned
    return logits, gen


def _scenarios(V):
    """(name, keywords, n_new, prompt_cols, penalty, ngram); the step counter is prompt_cols + n_new: 20 ids of history everywhere but
    in the begin scenarios, prompt_cols 0 and 7."""
    logits, gen = _rows(V)
    lf = logits[:, :V].float().numpy()
    sp = _special_ids(V)
    top = [int(np.argmax(lf[b])) for b in range(lf.shape[0])]
    out = [("argmax", dict(suppress_tokens=top), 20, 0, 1.0, 0)]
    for k in (2, 4, 6, 8, len(sp)):
        out.append((f"special_{k}", dict(suppress_tokens=sp[:k]), 13, 7, 1.0, 0))
    out.append(("bad_words", dict(bad_words_ids=[[t] for t in sp[:3]]), 13, 7, 1.0, 0))
    out.append(("all_but_one", dict(allowed_token_ids=[sp[7]]), 20, 0, 1.0, 0))
    out.append(("all_but_last", dict(allowed_token_ids=[V - 1]), 20, 0, 1.3, 2))
    out.append(("all", dict(suppress_tokens=list(range(V))), 20, 0, 1.0, 0))
    out.append(("allowed_some", dict(allowed_token_ids=sp[3:] + [100, 101, 200], suppress_tokens=[sp[3]]), 13, 7, 1.0, 0))
    # a penalised id that is masked (the alphabet holds each row's six best ids, the penalty leaves them on top); an id that is
    # n-gram-banned and masked
    out.append(("penalised_masked", dict(suppress_tokens=sorted({int(gen[b, 0]) for b in range(3)} | set(top))), 20, 0, 1.3, 0))
    out.append(("banned_masked", dict(suppress_tokens=sorted({int(gen[b, 8]) for b in range(3)})), 20, 0, 1.3, 2))
    # gating: the eos ids are the rows' best ids
    for pc in (0, 7):
        out.append((f"min_new_before_p{pc}", dict(eos_token_id=top, min_new_tokens=20 - pc + 1), 20 - pc, pc, 1.0, 0))   # n_new = min_new - 1
        out.append((f"min_new_reached_p{pc}", dict(eos_token_id=top, min_new_tokens=20 - pc), 20 - pc, pc, 1.0, 0))       # n_new = min_new
    out.append(("begin_at_0_p0", dict(begin_suppress_tokens=top), 0, 0, 1.0, 0))
    out.append(("begin_at_1_p0", dict(begin_suppress_tokens=top), 1, 0, 1.0, 0))
    out.append(("begin_at_0_p7", dict(begin_suppress_tokens=top), 0, 7, 1.3, 2))
    out.append(("begin_at_1_p7", dict(begin_suppress_tokens=top), 1, 7, 1.3, 2))
    return out


def _reference_rows(V, kw, n_new, prompt_cols, penalty, ngram):
    logits, gen = _rows(V)
    step = prompt_cols + n_new
    zs = []
    for b in range(logits.shape[0]):
        z = processed_logits(logits[b, :V].float().numpy(), gen[b, :step], penalty, ngram)
        zs.append(constrain(z, gen[b, :step], n_new, **kw))
    return zs, step


def _pick_state(B, gen, step):
    dev = "cuda"
    return dict(gen=torch.from_numpy(gen).to(dev), fin=torch.zeros(B, dtype=I32, device=dev), st=torch.tensor([step], dtype=I32, device=dev),
                nxt=torch.full((B,), -7, dtype=I32, device=dev), work=torch.zeros(B * 128 + 8, dtype=F32, device=dev))


@pytest.mark.parametrize("V", [320, 2051])
def test_greedy_pick_masked_is_exact(ops, V):
    logits, gen = _rows(V)
    B = logits.shape[0]
    dl = logits.cuda()
    bit = 0
    for name, kw, n_new, pc, penalty, ngram in _scenarios(V):
        zs, step = _reference_rows(V, kw, n_new, pc, penalty, ngram)
        want = [int(np.argmax(z)) for z in zs]                      # first index of the maximum; 0 for a row that is -inf throughout
        eos = kw.get("eos_token_id")
        s = _pick_state(B, gen, step)
        mask = _device_mask(ops, V, pc, **kw)
        eos_t = None if eos is None else torch.tensor(eos, dtype=torch.int64, device="cuda")
        ops.greedy_pick_masked(dl, s["work"], s["gen"], s["st"], s["fin"], penalty, ngram, eos_t, PAD, s["nxt"], V, mask)
        got = s["nxt"].cpu().tolist()
        assert got == want, (name, got, want)
        assert s["gen"][:, step].cpu().tolist() == want
        assert s["fin"].cpu().tolist() == [int(eos is not None and w in eos) for w in want], name
        m = masked_ids(V, n_new, **kw)
        assert all(np.isneginf(zs[b]).all() or not m[want[b]] for b in range(B)), name
        # two calls are bit-equal, partials included
        again = _pick_state(B, gen, step)
        ops.greedy_pick_masked(dl, again["work"], again["gen"], again["st"], again["fin"], penalty, ngram, eos_t, PAD, again["nxt"], V, mask)
        assert torch.equal(again["nxt"], s["nxt"]) and torch.equal(again["work"].view(I32), s["work"].view(I32))
        plain = _pick_state(B, gen, step)
        ops.greedy_pick(dl, plain["work"], plain["gen"], plain["st"], plain["fin"], penalty, ngram, eos_t, PAD, plain["nxt"], V)
        bit += plain["nxt"].cpu().tolist() != want
    assert bit >= 12                                                # the scenarios are not vacuous: the unmasked pick differs
    assert float(s["work"][B * 128]) == 0.0                         # no overlay overflow


KP = [(0, 1.0), (50, 0.9)]


def _sample_reference(zs, step, k, p):
    """Per row: n_kept, smallest kept s, the reference id and the gap between its two best perturbed scores."""
    out = []
    for b, z in enumerate(zs):
        prep = ref_prepare(z, TEMP)
        n_kept, s_min, margin = ref_cut(prep, k, p)
        if n_kept == 0:
            out.append((0, np.inf, 0, np.inf, np.inf))
            continue
        ids = np.nonzero(prep["fin"] & (prep["s"] >= s_min))[0]
        sc = prep["s"][ids] + noise(ids, SEED, step, b)
        o = np.argsort(-sc, kind="stable")
        gap = sc[o[0]] - sc[o[1]] if ids.size > 1 else np.inf
        out.append((n_kept, s_min, int(ids[o[0]]), gap, margin))
    return out


@pytest.mark.parametrize("V", [320, 2051])
def test_sample_pick_masked_is_exact(ops, V):
    logits, gen = _rows(V)
    B = logits.shape[0]
    dl = logits.cuda()
    sw = ops.sample_workspace(B, "cuda")
    nk = torch.zeros(B, dtype=I32, device="cuda")
    mk = torch.zeros(B, dtype=F32, device="cuda")
    for name, kw, n_new, pc, penalty, ngram in _scenarios(V):
        zs, step = _reference_rows(V, kw, n_new, pc, penalty, ngram)
        mask = _device_mask(ops, V, pc, **kw)
        m = masked_ids(V, n_new, **kw)
        for k, p in KP:
            ref = _sample_reference(zs, step, k, p)
            assert min(r[3] for r in ref) >= GAP and min(r[4] for r in ref) > 1e-4, (name, k, p, "precondition on the inputs")
            s = _pick_state(B, gen, step)
            ops.sample_pick(dl, s["work"], s["gen"], s["st"], s["fin"], penalty, ngram, None, PAD, s["nxt"], V, TEMP, k, p, SEED, sw,
                            n_kept=nk, min_kept=mk, mask=mask)
            got, n_kept, s_min = s["nxt"].cpu().tolist(), nk.cpu().tolist(), mk.cpu().double().tolist()
            assert n_kept == [r[0] for r in ref], (name, k, p, n_kept)
            for b in range(B):
                if ref[b][0] == 0:
                    assert got[b] == 0 and s_min[b] == np.inf
                    continue
                assert abs(s_min[b] - ref[b][1]) <= 2e-7 * max(1.0, abs(ref[b][1])), (name, k, p, b)
                assert got[b] == ref[b][2] and not m[got[b]], (name, k, p, b, got[b], ref[b][2])
            again = _pick_state(B, gen, step)
            ops.sample_pick(dl, again["work"], again["gen"], again["st"], again["fin"], penalty, ngram, None, PAD, again["nxt"], V, TEMP, k, p,
                            SEED, sw, mask=mask)
            assert torch.equal(again["nxt"], s["nxt"]) and torch.equal(again["work"].view(I32), s["work"].view(I32))
    assert int(sw.view(B, ops.SAMPLE_WORK_PER_ROW)[:, :65536].abs().sum()) == 0, "every masked pick leaves the histogram zero"
    # an unmasked pick on the workspace the masked picks used gives what it gives on a fresh one
    outs = []
    for ws in (sw, ops.sample_workspace(B, "cuda")):
        s = _pick_state(B, gen, 20)
        ops.sample_pick(dl, s["work"], s["gen"], s["st"], s["fin"], 1.3, 2, None, PAD, s["nxt"], V, TEMP, 50, 0.9, SEED, ws, n_kept=nk, min_kept=mk)
        outs.append((s["nxt"].clone(), nk.clone(), mk.clone(), s["work"].clone()))
    assert all(torch.equal(a.view(I32) if a.dtype == F32 else a, b.view(I32) if b.dtype == F32 else b) for a, b in zip(*outs))


def test_picks_at_the_full_vocabulary(ops):
    """V = 151 936, B = 2: one greedy and one sample case (slices of 2374 ids, 75 words each, none aligned)."""
    V, B = 151936, 2
    rng = np.random.default_rng(9)
    lf = np.clip(4 * rng.standard_normal((B, V)), -30, 11.0).astype(np.float32)
    per = (V + 63) // 64
    sp = [0, 31, 32, per - 1, per, 40 * per + 5, 63 * per, V - 1]
    for b in range(B):
        lf[b, sp[b:] + sp[:b]] = 24.0 - 0.5 * np.arange(len(sp))
    logits = torch.from_numpy(lf).to(BF16)
    gen = rng.choice(np.array(sp + [7, 70000]), (B, MAX_IDS))
    gen[:, 18:20] = gen[:, 6:8]
    kw = dict(suppress_tokens=sp[:3] + [V - 1], begin_suppress_tokens=[sp[3]], eos_token_id=[sp[4]], min_new_tokens=14,
              allowed_token_ids=sorted(set(sp) | set(range(1000, 150000, 7))))
    n_new, pc, step = 13, 7, 20
    zs = [constrain(processed_logits(logits[b].float().numpy(), gen[b, :step], 1.3, 2), None, n_new, **kw) for b in range(B)]
    mask = _device_mask(ops, V, pc, **kw)
    dl = logits.cuda()
    s = _pick_state(B, gen, step)
    ops.greedy_pick_masked(dl, s["work"], s["gen"], s["st"], s["fin"], 1.3, 2, torch.tensor(kw["eos_token_id"], device="cuda"), PAD, s["nxt"], V,
                           mask)
    want = [int(np.argmax(z)) for z in zs]
    assert s["nxt"].cpu().tolist() == want, (s["nxt"].cpu().tolist(), want)
    plain = [int(np.argmax(processed_logits(logits[b].float().numpy(), gen[b, :step], 1.3, 2))) for b in range(B)]
    assert all(w != p and not masked_ids(V, n_new, **kw)[w] for w, p in zip(want, plain))       # the mask moved both picks
    ref = _sample_reference(zs, step, 50, 0.9)
    assert min(r[3] for r in ref) >= GAP and min(r[4] for r in ref) > 1e-4
    sw = ops.sample_workspace(B, "cuda")
    nk, mk = torch.zeros(B, dtype=I32, device="cuda"), torch.zeros(B, dtype=F32, device="cuda")
    s = _pick_state(B, gen, step)
    ops.sample_pick(dl, s["work"], s["gen"], s["st"], s["fin"], 1.3, 2, None, PAD, s["nxt"], V, TEMP, 50, 0.9, SEED, sw, n_kept=nk, min_kept=mk,
                    mask=mask)
    assert nk.cpu().tolist() == [r[0] for r in ref] and s["nxt"].cpu().tolist() == [r[2] for r in ref]
    assert all(abs(a - r[1]) <= 2e-7 * max(1.0, abs(r[1])) for a, r in zip(mk.cpu().double().tolist(), ref))
    assert int(sw.view(B, ops.SAMPLE_WORK_PER_ROW)[:, :65536].abs().sum()) == 0


def test_allowed_set_distribution(ops):
    """An allowed set of 4 ids, 4000 seeds: the draws pass a chi-square test against the softmax over those 4 at the significance of
    tests/test_sample_gpu.py (the 1 - 1e-6 quantile, 3 degrees of freedom) and fail it against the softmax at another temperature."""
    from tests.test_sample_gpu import _chi2_quantile
    V, B, N = 2051, 8, 4000
    rng = np.random.default_rng(44)
    row = torch.from_numpy((2 * rng.standard_normal(V)).astype(np.float32)).to(BF16)
    allowed = [31, 32, 1040, V - 1]
    row[allowed] = torch.tensor([1.0, 0.5, 0.0, -0.25]).to(BF16)             # none of them near the row's best: the mask does the work
    s = row.float().numpy()[allowed].astype(np.float64) / float(np.float32(TEMP))
    prob = np.exp(s - s.max()) / np.exp(s - s.max()).sum()
    s1 = row.float().numpy()[allowed].astype(np.float64)
    prob1 = np.exp(s1 - s1.max()) / np.exp(s1 - s1.max()).sum()
    assert N * prob.min() >= 5
    dl = row[None].repeat(B, 1).contiguous().cuda()
    mask = _device_mask(ops, V, 0, allowed_token_ids=allowed)
    gen = np.zeros((B, 8), np.int64)
    st = _pick_state(B, gen, 0)
    sw = ops.sample_workspace(B, "cuda")
    nk = torch.zeros(B, dtype=I32, device="cuda")
    out = torch.zeros((N // B, B), dtype=I32, device="cuda")
    for i in range(N // B):
        ops.sample_pick(dl, st["work"], st["gen"], st["st"], st["fin"], 1.0, 0, None, 0, st["nxt"], V, TEMP, 50, 1.0, 1000 + i, sw, n_kept=nk,
                        mask=mask)
        out[i] = st["nxt"]
    assert nk.cpu().tolist() == [4] * B
    draws = out.cpu().numpy()
    assert np.isin(draws, allowed).all()
    counts = np.array([(draws == i).sum() for i in allowed])
    bound = _chi2_quantile(1e-6, 3)
    x = float(((counts - N * prob) ** 2 / (N * prob)).sum())
    x1 = float(((counts - N * prob1) ** 2 / (N * prob1)).sum())
    print(f"chi2 {x:.2f}, against the T = 1 probabilities {x1:.2f}, bound {bound:.2f}")
    assert x < bound and x1 > bound


# ================================================================================================ B. end to end on the tiny model
from tests.test_generate_gpu import TIE_TOL, _tiny_model          # noqa: E402

KEYS = ("suppress_tokens", "begin_suppress_tokens", "min_new_tokens", "allowed_token_ids", "bad_words_ids")


@pytest.fixture(scope="module")
def tiny():
    return _tiny_model()


def _eos_list(kw):
    e = kw.get("eos_token_id")
    return [] if e is None else ([e] if isinstance(e, int) else list(e))


def _ckw(kw):
    return dict({k: kw[k] for k in KEYS if k in kw}, eos_token_id=kw.get("eos_token_id"))


def _assert_constraints_held(new, kw, V, what):
    """new: the emitted ids [rows, steps]. No id is a masked id at its step and no eos comes before min_new_tokens; after a row's eos
    only pad follows (pad does not go through the logits)."""
    eos, pad = _eos_list(kw), kw.get("pad_token_id")
    for b, row in enumerate(new.tolist()):
        done = False
        for t, tok in enumerate(row):
            if done:
                assert tok == (pad if pad is not None else eos[0]), (what, b, t, tok)
                continue
            assert not masked_ids(V, t, **_ckw(kw))[tok], (what, b, t, tok)
            if tok in eos:
                assert t >= kw.get("min_new_tokens", 0), (what, b, t, tok)
                done = True


def _check_greedy_case(model, sd, cfg, z, case, use_graph):
    """tests/test_generate_gpu.py's _check_case under constraints: ids equal to transformers' until a step where the emitted id lies
    within TIE_TOL of the best CONSTRAINED score of a cache-free forward over the reference's own sequence; that row's comparison ends
    there. -> (verified steps, exact)."""
    from oracle import generate as og
    from oracle import qwen3 as oq
    name, kw = case["name"], case["kw"]
    ocfg = oq.Qwen3Cfg(**cfg)
    ref = torch.from_numpy(z[f"{name}:out"])
    mask = torch.from_numpy(z[f"{name}:attention_mask"])
    if case["input"] == "input_ids":
        ids = torch.from_numpy(z[f"{name}:input_ids"])
        out, stats = model.generate(input_ids=ids.cuda(), attention_mask=mask.cuda(), return_stats=True, use_graph=use_graph, **kw)
        embeds, n_prompt = torch.nn.functional.embedding(ids, sd["model.embed_tokens.weight"]), ids.shape[1]
    else:
        embeds, n_prompt, ids = bf16(z[f"{name}:inputs_embeds"]), 0, None
        out, stats = model.generate(inputs_embeds=embeds.cuda(), attention_mask=mask.cuda(), return_stats=True, use_graph=use_graph, **kw)
    assert stats["graph"] == (use_graph and kw["max_new_tokens"] > 2)
    out = out.cpu()
    V = sd["model.embed_tokens.weight"].shape[0]
    _assert_constraints_held(out[:, n_prompt:], kw, V, name)
    matched, exact = 0, True
    for b in range(ref.shape[0]):
        n = min(out.shape[1], ref.shape[1])
        diff = (out[b, :n] != ref[b, :n]).nonzero().flatten()
        if diff.numel() == 0:
            matched += n - n_prompt
            continue
        exact = False
        t = int(diff[0])
        matched += t - n_prompt
        row = embeds[b][mask[b] != 0]
        seen = ([] if ids is None else ids[b].tolist()) + ref[b, n_prompt:t].tolist()
        x = torch.cat([row, sd["model.embed_tokens.weight"][ref[b, n_prompt:t]]], 0)[None]
        h = oq.model_forward(x, torch.ones(1, x.shape[1], dtype=torch.long), sd, ocfg)
        sc = torch.nn.functional.linear(h[0, -1], sd["model.embed_tokens.weight"]).float()
        og.repetition_penalty_(sc, seen, kw.get("repetition_penalty", 1.0))
        og.no_repeat_ngram_(sc, seen, kw.get("no_repeat_ngram_size", 0))
        sc = constrain(sc, seen, t - n_prompt, **_ckw(kw))
        gap = float(sc.max() - sc[out[b, t]])
        print(f"{name} row {b} step {t - n_prompt}: emitted {int(out[b, t])}, transformers {int(ref[b, t])}, {gap:.4f} below the best")
        assert sc[out[b, t]] >= sc.max() - TIE_TOL, (name, b, t, int(out[b, t]), int(ref[b, t]), gap)
    if exact:
        assert out.shape == ref.shape, (name, out.shape, ref.shape)
    return matched, exact


@pytest.mark.parametrize("use_graph", [True, False], ids=["graph", "eager"])
def test_generate_vs_transformers_golden(tiny, use_graph):
    """Every recorded greedy case. The strong cases (one per keyword; recorded with a top-2 margin of at least 4 x TIE_TOL at every
    step) are demanded in full. Floor on the verified steps: all steps of the strong cases and, of the other cases' 12 rows, one step
    per row on average - those rows' own margins are a few hundredths, any of them may end at its first step, not all of them."""
    model, sd, cfg = tiny
    z = load("constrain_tiny.npz")
    assert meta(z)["tie_tol"] == TIE_TOL
    cases = [c for c in meta(z)["cases"] if "num_beams" not in c["kw"]]
    total, strong_steps, strong_names = 0, 0, set()
    for case in cases:
        m, exact = _check_greedy_case(model, sd, cfg, z, case, use_graph)
        total += m
        if case["strong"]:
            assert case["margin"] >= 4 * TIE_TOL
            assert exact, case["name"]
            strong_steps += m
            strong_names.add(case["name"])
    assert strong_names == {k + "_strong" for k in ("suppress", "begin", "min_new", "allowed", "bad_words")}
    rows_other = sum(z[f"{c['name']}:out"].shape[0] for c in cases if not c["strong"])
    print(f"verified {total} steps, {strong_steps} of them in strong cases")
    assert rows_other == 12 and total >= strong_steps + rows_other


def _sample_kw(V):
    return dict(suppress_tokens=[3, 15, 244, 112], begin_suppress_tokens=[113, 234], eos_token_id=[256, 148], min_new_tokens=5, pad_token_id=318,
                allowed_token_ids=sorted(set(range(0, V, 3)) | {256, 148, 15, 234}), bad_words_ids=[[9]], repetition_penalty=1.1,
                no_repeat_ngram_size=2, temperature=1.5, top_k=40, top_p=0.95, seed=1234)


def _prompts(cfg, B, L, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, L, cfg["hidden_size"], generator=g) * 0.5).to(BF16).cuda(), torch.ones(B, L, dtype=torch.long).cuda()


def test_sample_under_constraints(tiny):
    """sample(): num_return_sequences=3, graph replay and eager stepping give the same bits, nothing masked is ever drawn; max_rows=16
    on 12 rows (the MFMA decode route); two turns on a KV cache."""
    from vggt_qwen3_amd import generate as G
    model, sd, cfg = tiny
    V = model.vocab
    kw = _sample_kw(V)
    emb, mask = _prompts(cfg, 2, 9, 3)
    outs = [model.sample(inputs_embeds=emb, attention_mask=mask, max_new_tokens=12, num_return_sequences=3, use_graph=ug, output_logprobs=True,
                         **kw) for ug in (True, False)]
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1].view(I32), outs[1][1].view(I32))
    assert outs[0][0].shape[0] == 6
    _assert_constraints_held(outs[0][0].cpu(), kw, V, "sample x3")
    free = model.sample(inputs_embeds=emb, attention_mask=mask, max_new_tokens=12, num_return_sequences=3,
                        **{k: v for k, v in kw.items() if k not in KEYS})
    assert not torch.equal(free[:, :outs[0][0].shape[1]], outs[0][0][:, :free.shape[1]])     # the keywords are not ignored
    # 12 rows under max_rows=16
    emb12, mask12 = _prompts(cfg, 12, 7, 4)
    for ug in (True, False):
        out = model.sample(inputs_embeds=emb12, attention_mask=mask12, max_new_tokens=8, max_rows=16, use_graph=ug, **kw)
        assert out.shape[0] == 12
        _assert_constraints_held(out.cpu(), kw, V, "sample 12 rows")
    # two turns on one cache: begin_suppress_tokens and min_new_tokens count from the start of each call
    kw2 = dict(kw, eos_token_id=None)
    cache = G.KVCache(model, 2, 64)
    t1 = model.sample(inputs_embeds=emb, attention_mask=mask, max_new_tokens=6, kv_cache=cache, **kw2)
    _assert_constraints_held(t1.cpu(), kw2, V, "turn 1")
    more, _ = _prompts(cfg, 2, 4, 5)
    emb2 = torch.cat([emb, model.get_input_embeddings()(t1), more], dim=1)
    t2 = model.sample(inputs_embeds=emb2, attention_mask=torch.ones(emb2.shape[:2], dtype=torch.long).cuda(), max_new_tokens=6, kv_cache=cache,
                      **kw2)
    assert t2.shape == (2, 6)
    _assert_constraints_held(t2.cpu(), kw2, V, "turn 2")


def test_greedy_with_kv_cache_max_rows_and_logprobs(tiny):
    """generate() under constraints with kv_cache= on two turns, with max_rows=16 on 12 rows, and output_logprobs: the log-probability
    stays that of the RAW logits - it equals what the unconstrained call reports wherever both emit the same id after the same ids."""
    from vggt_qwen3_amd import generate as G
    model, sd, cfg = tiny
    V = model.vocab
    kw = {k: v for k, v in _sample_kw(V).items() if k not in ("temperature", "top_k", "top_p", "seed")}
    emb12, mask12 = _prompts(cfg, 12, 7, 4)
    for ug in (True, False):
        out = model.generate(inputs_embeds=emb12, attention_mask=mask12, max_new_tokens=8, max_rows=16, use_graph=ug, **kw)
        _assert_constraints_held(out.cpu(), kw, V, "generate 12 rows")
    emb, mask = _prompts(cfg, 2, 9, 3)
    kw2 = dict(kw, eos_token_id=None)
    cache = G.KVCache(model, 2, 64)
    t1 = model.generate(inputs_embeds=emb, attention_mask=mask, max_new_tokens=6, kv_cache=cache, **kw2)
    emb2 = torch.cat([emb, model.get_input_embeddings()(t1), _prompts(cfg, 2, 4, 5)[0]], dim=1)
    t2 = model.generate(inputs_embeds=emb2, attention_mask=torch.ones(emb2.shape[:2], dtype=torch.long).cuda(), max_new_tokens=6, kv_cache=cache,
                        **kw2)
    for t, what in ((t1, "turn 1"), (t2, "turn 2")):
        _assert_constraints_held(t.cpu(), kw2, V, what)
    # raw log-probabilities: suppressing ids that would never have been picked changes nothing, log-probabilities included
    ids0, lp0 = model.generate(inputs_embeds=emb, attention_mask=mask, max_new_tokens=8, output_logprobs=True)
    unused = sorted(set(range(V)) - set(ids0.reshape(-1).tolist()))[:20]
    ids1, lp1 = model.generate(inputs_embeds=emb, attention_mask=mask, max_new_tokens=8, output_logprobs=True, suppress_tokens=unused)
    assert torch.equal(ids0, ids1) and torch.equal(lp0.view(I32), lp1.view(I32))
    # suppressing the first pick: the id changes, its log-probability is lower under the raw row and is not -inf or 0
    ids2, lp2 = model.generate(inputs_embeds=emb, attention_mask=mask, max_new_tokens=8, output_logprobs=True,
                               begin_suppress_tokens=ids0[:, 0].tolist())
    assert bool((ids2[:, 0] != ids0[:, 0]).all()) and bool((lp2[:, 0] <= lp0[:, 0]).all()) and bool(torch.isfinite(lp2).all())


def test_unconstrained_calls_are_untouched_by_a_constrained_one(tiny):
    """generate() without a constraint keyword: bit-equal ids, log-probabilities and stats before and after a constrained call in the
    same process, and the call owns no mask."""
    from vggt_qwen3_amd import generate as G
    model, sd, cfg = tiny
    emb, mask = _prompts(cfg, 2, 9, 3)
    kw = dict(inputs_embeds=emb, attention_mask=mask, max_new_tokens=10, repetition_penalty=1.1, no_repeat_ngram_size=2, eos_token_id=319,
              output_logprobs=True, return_stats=True)
    seen = []
    real = G.DecodeState

    class Spy(real):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            seen.append(self.mask is not None)

    ids0, lp0, st0 = model.generate(**kw)
    G.DecodeState = Spy
    try:
        con = model.generate(**dict(kw, suppress_tokens=ids0[:, 1].tolist(), min_new_tokens=4, begin_suppress_tokens=ids0[:, 0].tolist()))
        ids1, lp1, st1 = model.generate(**kw)
    finally:
        G.DecodeState = real
    assert seen == [True, False]
    assert not torch.equal(con[0], ids0)
    assert torch.equal(ids0, ids1) and torch.equal(lp0.view(I32), lp1.view(I32)) and st0 == st1
