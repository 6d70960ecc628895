"""Host-side reference of the sampling pick (include/vq3_hip.h: vq3_sample_pick) and what can be checked without a GPU: a NumPy
Philox4x32-10 against the published Random123 known-answer vectors, the fp64 reference kept set against plain torch restatements of
transformers' TopKLogitsWarper / TopPLogitsWarper, sample()'s argument errors, and the header constants. tests/test_sample_gpu.py
imports philox4x32_10, gumbel, ref_prepare, ref_cut and ref_pick from here.

Should a known-answer vector ever disagree with an implementation that follows the constants of the contract (multipliers 0xD2511F53 /
0xCD9E8D57, key increments 0x9E3779B9 / 0xBB67AE85, ten rounds), the definition of Philox (Salmon, Moraes, Dror, Shaw: "Parallel
random numbers: as easy as 1, 2, 3", SC'11) is what counts, not the table."""
import re
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key):
    """counter: four arrays (or ints) of 32-bit words, key: two ints. Returns uint32 [..., 4]."""
    c = [np.asarray(x, dtype=np.uint64) & MASK for x in np.broadcast_arrays(*[np.asarray(v, dtype=np.uint64) for v in counter])]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]                  # 32 x 32 -> 64 bits: no overflow in uint64
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & MASK, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & MASK]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return np.stack(c, axis=-1).astype(np.uint32)


def gumbel(r):
    """g = -log(-log(u)), u = ((r >> 8) + 0.5) * 2^-24, in fp64 (u is exact there)."""
    u = ((np.asarray(r, dtype=np.uint64) >> np.uint64(8)).astype(np.float64) + 0.5) * 2.0 ** -24
    return -np.log(-np.log(u))


def noise(ids, seed, t, row):
    """g_i for the given ids: word i & 3 of the Philox block with counter (i >> 2, t, row, 0) and key (seed low, seed high)."""
    ids = np.asarray(ids, dtype=np.int64)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    blocks, inv = np.unique(ids >> 2, return_inverse=True)          # one Philox block serves four consecutive ids
    words = philox4x32_10((blocks, t, row, 0), (seed & 0xFFFFFFFF, seed >> 32))
    return gumbel(words[inv, ids & 3])


def processed_logits(logits, history, penalty, ngram):
    """z: the f32 logits after the repetition penalty and the n-gram ban, as vq3_greedy_pick applies them (f32 arithmetic: a
    penalised value is z * penalty for z < 0, else z / penalty, once per distinct id; then every id that would complete a repeat of an
    n-gram already in `history` is -inf)."""
    z = np.array(logits, dtype=np.float32)
    history = [int(x) for x in history]
    if penalty != 1.0:
        pen = np.float32(penalty)
        for tok in dict.fromkeys(history):
            if 0 <= tok < z.size:
                z[tok] = z[tok] * pen if z[tok] < 0 else z[tok] / pen
    if ngram > 0 and len(history) + 1 >= ngram:
        pre = history[len(history) - (ngram - 1):] if ngram > 1 else []
        for i in range(len(history) - ngram + 1):
            if history[i:i + ngram - 1] == pre and 0 <= history[i + ngram - 1] < z.size:
                z[history[i + ngram - 1]] = -np.inf
    return z


def ref_prepare(z, temperature):
    """Everything about a row that does not depend on (top_k, top_p): s = z / temperature in fp64 (temperature as the f32 the entry
    receives), its distinct finite values in descending order with their counts, the count of ids above each and exp(s - max)."""
    T = float(np.float32(temperature))
    z = np.asarray(z)
    s = z.astype(np.float64) / T
    fin = np.isfinite(s)
    zv, counts = np.unique(z[fin], return_counts=True)      # (sorted in the dtype given: dividing by T > 0 keeps order and distinctness)
    vals, counts = zv[::-1].astype(np.float64) / T, counts[::-1]
    above = np.concatenate([[0], np.cumsum(counts)[:-1]])
    w = counts * np.exp(vals - vals[0]) if vals.size else np.zeros(0)
    return dict(s=s, fin=fin, vals=vals, counts=counts, above=above, w=w)


def ref_cut(prep, top_k, top_p):
    """(n_kept, smallest kept s, margin): top-k keeps a value iff fewer than top_k ids lie above it; top-p then keeps it iff the
    softmax mass (over the top-k set) of the values above it is < top_p, top_p = 1 keeping the whole top-k set. margin is the
    distance from top_p of the mass above the last kept value (unless that is the maximum, whose mass above is exactly 0) and above the
    first dropped one; inf where top-p cuts nothing."""
    vals, counts, above, w = prep["vals"], prep["counts"], prep["above"], prep["w"]
    if vals.size == 0:
        return 0, np.inf, np.inf
    in_k = np.ones(vals.size, bool) if top_k == 0 else above < top_k
    nk = int(in_k.sum())                                   # a prefix of the descending values
    p = float(np.float32(top_p))
    margin = np.inf
    if p < 1.0:
        wk = w[:nk]
        mass_above = np.concatenate([[0.0], np.cumsum(wk)[:-1]]) / wk.sum()
        keep = mass_above < p
        n_groups = int(keep.sum())
        assert keep[:n_groups].all()
        if n_groups > 1:                                   # (the mass above the maximum is exactly 0 in any arithmetic: no boundary there)
            margin = p - mass_above[n_groups - 1]
        if n_groups < nk:
            margin = min(margin, mass_above[n_groups] - p)
    else:
        n_groups = nk
    return int(counts[:n_groups].sum()), float(vals[n_groups - 1]), float(margin)


def ref_pick(logits, history, opts, seed, t, row):
    """The fp64 reference pick of one row: (kept mask [V], perturbed scores s + g [V] (-inf outside the kept set), id).
    opts: penalty, ngram, temperature, top_k, top_p."""
    z = processed_logits(logits, history, opts.get("penalty", 1.0), opts.get("ngram", 0))
    prep = ref_prepare(z, opts.get("temperature", 1.0))
    n_kept, s_min, _ = ref_cut(prep, opts.get("top_k", 0), opts.get("top_p", 1.0))
    kept = prep["fin"] & (prep["s"] >= s_min)
    assert int(kept.sum()) == n_kept
    score = np.full(z.size, -np.inf)
    ids = np.nonzero(kept)[0]
    score[ids] = prep["s"][ids] + noise(ids, seed, t, row)
    return kept, score, (int(score.argmax()) if ids.size else 0)


# ------------------------------------------------------------------------------------------------------------------------------------
def test_philox_known_answer_vectors():
    """Random123's kat_vectors for philox4x32-10."""
    cases = [((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
             ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
             ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1")]
    for ctr, key, want in cases:
        got = philox4x32_10(ctr, key)
        assert " ".join(f"{int(x):08x}" for x in got) == want, (ctr, key)
    # vectorised over the first counter word, as the reference pick uses it
    many = philox4x32_10((np.arange(5), 7, 3, 0), (11, 13))
    for i in range(5):
        assert np.array_equal(many[i], philox4x32_10((i, 7, 3, 0), (11, 13)))


def test_gumbel_range_of_a_24_bit_uniform():
    g = gumbel(np.array([0, 0xFFFFFFFF], dtype=np.uint64))
    assert -2.9 < g[0] < -2.8 and 17.3 < g[1] < 17.4


def _torch_warpers(s, top_k, top_p):
    """TopKLogitsWarper then TopPLogitsWarper (transformers.generation.logits_process), restated on one fp64 row."""
    s = s.clone()
    if top_k > 0:
        kth = torch.topk(s, min(top_k, s.numel()))[0][-1]
        s[s < kth] = -float("inf")
    if top_p < 1.0:
        sorted_s, order = torch.sort(s, descending=False)
        cum = sorted_s.softmax(dim=-1).cumsum(dim=-1)
        remove = cum <= (1 - top_p)
        remove[-1:] = False                                  # min_tokens_to_keep = 1
        s[order[remove]] = -float("inf")
    return torch.isfinite(s)


@pytest.mark.parametrize("top_k,top_p", [(0, 1.0), (1, 1.0), (50, 1.0), (0, 0.9), (50, 0.9), (7, 0.5), (0, 1e-6), (50, 1e-6), (400, 0.99)])
def test_reference_kept_set_matches_the_transformers_warpers(top_k, top_p):
    rng = np.random.default_rng(100 + top_k)
    for trial in range(4):
        T = [1.0, 0.7, 1.9, 0.3][trial]
        z = rng.normal(0, 3, 500)                           # fp64, tie-free
        assert np.unique(z).size == z.size
        prep = ref_prepare(z, T)
        n_kept, s_min, margin = ref_cut(prep, top_k, top_p)
        assert margin > 1e-9                               # fp64 against fp64: the boundary is not within rounding of top_p
        kept = prep["s"] >= s_min
        want = _torch_warpers(torch.from_numpy(z) / float(np.float32(T)), top_k, float(np.float32(top_p)))
        assert np.array_equal(kept, want.numpy()) and int(kept.sum()) == n_kept, (top_k, top_p, T)
        if top_k == 1 or top_p == 1e-6:
            assert n_kept == 1 and kept[z.argmax()]
        if top_p == 1.0:
            assert n_kept == (500 if top_k == 0 else top_k)


def test_reference_ties_stand_or_fall_together_and_banned_ids_are_never_kept():
    z = np.array([2.0, 5.0, 5.0, 1.0, 5.0, -np.inf, 2.0], dtype=np.float32)
    prep = ref_prepare(z, 1.0)
    assert ref_cut(prep, 1, 1.0)[0] == 3                   # three ids tie at the top: fewer than 1 id lies above each
    assert ref_cut(prep, 3, 1.0)[0] == 3 and ref_cut(prep, 4, 1.0)[0] == 5
    assert ref_cut(prep, 0, 1.0)[0] == 6                   # -inf is never kept
    assert ref_cut(prep, 0, 0.5)[0] == 3                   # the mass above the maximum is 0 < top_p: all three stay
    kept, score, pick = ref_pick(z, [], dict(top_k=0, top_p=1.0), 1, 0, 0)
    assert kept.tolist() == [True] * 5 + [False, True] and score[5] == -np.inf and kept[pick]
    # processors: the penalty divides positive logits once per distinct id, the ban removes the id that would repeat the bigram
    z2 = processed_logits(np.array([4.0, -2.0, 3.0, 1.0], dtype=np.float32), [0, 1, 0, 2, 0], 2.0, 2)
    assert z2.tolist() == [2.0, -np.inf, -np.inf, 1.0]      # id 1 and id 2 both followed an earlier 0


def test_sample_argument_errors_need_no_gpu():
    from vggt_qwen3_amd import generate as G
    e = torch.zeros(2, 4, 8)
    for kw in (dict(temperature=0.0), dict(temperature=-1.0), dict(temperature=float("nan")), dict(top_p=0.0), dict(top_p=1.5),
               dict(top_p=-0.1), dict(top_k=-1), dict(num_return_sequences=0), dict(num_return_sequences=-2),
               dict(num_return_sequences=5), dict(num_return_sequences=2, inputs_embeds=torch.zeros(5, 4, 8))):
        with pytest.raises(ValueError, match="sample"):
            G.sample(None, **dict(dict(inputs_embeds=e), **kw))
    with pytest.raises(ValueError, match="sample"):
        G.sample(None, input_ids=torch.zeros(3, 4, dtype=torch.long), num_return_sequences=3)
    from vggt_qwen3_amd.qwen3 import Qwen3ForCausalLM
    assert callable(Qwen3ForCausalLM.sample)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from vggt_qwen3_amd import _lib
    return _lib.load()


def test_sample_workspace_constant_matches_the_header():
    from vggt_qwen3_amd import ops
    text = (ROOT / "include" / "vq3_hip.h").read_text()
    m = re.search(r"#define\s+VQ3_SAMPLE_WORK_PER_ROW\s+(\d+)", text)
    assert m and int(m.group(1)) == ops.SAMPLE_WORK_PER_ROW
    assert ops.SAMPLE_WORK_PER_ROW >= 65536 + 1 and ops.SAMPLE_WORK_PER_ROW % 4 == 0      # the bins and the threshold; rows stay 16-byte aligned


def test_sample_pick_rejects_bad_arguments_without_a_launch(lib):
    import ctypes
    keep = ctypes.create_string_buffer(64 + 16)
    p = (ctypes.addressof(keep) + 15) & ~15                   # a non-null, 16-byte aligned host address: validation fails before any use
    good = dict(logits=p, ld=1024, work=p, B=2, V=1000, gen=p, max_new=16, step=p, fin=p, pen=1.0, ngram=0, eos=None, n_eos=0, pad=0,
                nxt=p, T=1.0, k=50, p=1.0, seed=1, sw=p, nk=None, mk=None)

    def call(**kw):
        a = dict(good, **kw)
        return lib.vq3_sample_pick(a["logits"], a["ld"], a["work"], a["B"], a["V"], a["gen"], a["max_new"], a["step"], a["fin"], a["pen"],
                                   a["ngram"], a["eos"], a["n_eos"], a["pad"], a["nxt"], a["T"], a["k"], a["p"], a["seed"], a["sw"], a["nk"],
                                   a["mk"], None)

    for name in ("logits", "work", "gen", "step", "fin", "nxt", "sw"):
        assert call(**{name: None}) != 0
        assert b"sample_pick" in lib.vq3_last_error() and b"null" in lib.vq3_last_error()
    for kw in (dict(ld=999), dict(B=0), dict(V=0), dict(max_new=0)):
        assert call(**kw) != 0 and b"shape" in lib.vq3_last_error()
    assert call(max_new=513) != 0 and b"512" in lib.vq3_last_error()
    for kw, word in ((dict(T=0.0), b"temperature"), (dict(T=-1.0), b"temperature"), (dict(k=-1), b"top_k"), (dict(p=0.0), b"top_p"),
                     (dict(p=1.5), b"top_p"), (dict(pen=0.0), b"repetition_penalty"), (dict(sw=p + 4), b"aligned")):
        assert call(**kw) != 0 and word in lib.vq3_last_error(), (kw, lib.vq3_last_error())
