"""What the decoding constraints can show without a GPU: tests/constrain_ref.py - the restatement the device code is held to in
tests/test_constrain_gpu.py - replayed on the raw logits transformers recorded (tests/golden/constrain_tiny.npz,
tools/make_golden_constrain.py) reproduces the -inf pattern of transformers' own processed scores and its sequences; the argument
errors of generate() / sample(); the bit planes the host builds. (The recorded beam cases are replayed here on the restatement alone:
beam_search() does not take the keywords.)"""
import ctypes
import types

import numpy as np
import pytest
import torch

from tests import beam_ref
from tests.constrain_ref import constrain, masked_ids
from tests.golden_io import load, meta
from tests.test_sample_host import processed_logits

Z = load("constrain_tiny.npz")
CASES = meta(Z)["cases"]
KEYS = ("suppress_tokens", "begin_suppress_tokens", "min_new_tokens", "allowed_token_ids", "bad_words_ids")


def _eos_list(kw):
    e = kw.get("eos_token_id")
    return [] if e is None else ([e] if isinstance(e, int) else list(e))


def _constraints(kw):
    return dict({k: kw[k] for k in KEYS if k in kw}, eos_token_id=kw.get("eos_token_id"))


@pytest.mark.parametrize("case", [c for c in CASES if "num_beams" not in c["kw"]], ids=lambda c: c["name"])
def test_restatement_replays_transformers_greedy(case):
    name, kw = case["name"], case["kw"]
    raw, scores, out = Z[f"{name}:logits"], Z[f"{name}:scores"], Z[f"{name}:out"]
    prompt = Z[f"{name}:input_ids"] if case["input"] == "input_ids" else np.zeros((out.shape[0], 0), np.int64)
    P, eos = prompt.shape[1], _eos_list(kw)
    assert np.array_equal(out[:, :P], prompt)
    bit = False
    for t in range(raw.shape[0]):
        for b in range(raw.shape[1]):
            history = out[b, :P + t].tolist()                      # (a finished row's pads included: transformers processes those rows too)
            z = processed_logits(raw[t, b], history, kw.get("repetition_penalty", 1.0), kw.get("no_repeat_ngram_size", 0))
            got = constrain(z, history, t, **_constraints(kw))
            assert np.array_equal(np.isneginf(got), np.isneginf(scores[t, b])), (name, t, b)
            fin = np.isfinite(got)
            np.testing.assert_allclose(got[fin], scores[t, b][fin], rtol=1e-6, atol=0)
            bit |= bool((np.isneginf(got) & ~np.isneginf(z)).any() and int(np.argmax(z)) != int(np.argmax(got)))
            if not any(x in eos for x in out[b, P:P + t].tolist()):           # a live row emits the first argmax of the constrained row
                assert int(np.argmax(got)) == int(out[b, P + t]), (name, t, b)
                assert not masked_ids(raw.shape[2], t, **_constraints(kw))[out[b, P + t]]
            else:
                assert int(out[b, P + t]) == kw["pad_token_id"]
    assert bit, f"{name}: the constraint never changed a pick"


@pytest.mark.parametrize("case", [c for c in CASES if "num_beams" in c["kw"]], ids=lambda c: c["name"])
def test_restatement_replays_transformers_beam(case):
    """The processed scores of beam search are log-probabilities: beam_ref.process, then the constraint per row. The search itself is
    stepped on transformers' own scores (tests/test_beam_host.py's replay), which the restated ones equal in their -inf pattern."""
    name, kw = case["name"], case["kw"]
    raw, scores = torch.from_numpy(Z[f"{name}:logits"]), torch.from_numpy(Z[f"{name}:scores"])
    B = Z[f"{name}:inputs_embeds"].shape[0]
    eos, fill = _eos_list(kw), kw["pad_token_id"]
    ref = beam_ref.BeamRef(torch.zeros((B, 0), dtype=torch.int64), kw["num_beams"], kw["max_new_tokens"], eos, kw.get("length_penalty", 1.0),
                           kw.get("early_stopping", False), fill=fill, dtype=torch.float32)
    t, masked_finite = 0, 0
    while not ref.done:
        rows = ref.rows()
        lp = beam_ref.process(raw[t], rows, kw.get("repetition_penalty", 1.0), kw.get("no_repeat_ngram_size", 0), dtype=torch.float32)
        for r in range(lp.shape[0]):
            got = constrain(lp[r], rows[r], t, **_constraints(kw))
            masked_finite += int((torch.isneginf(got) & ~torch.isneginf(lp[r])).sum())
            assert torch.equal(torch.isneginf(got), torch.isneginf(scores[t, r])), (name, t, r)
            fin = torch.isfinite(got)
            assert torch.allclose(got[fin], scores[t, r][fin], rtol=1e-5, atol=1e-5)
        ref.step(scores[t])
        t += 1
    assert t == scores.shape[0] and masked_finite > 0
    seqs, seq_scores, _ = ref.outputs(kw.get("num_return_sequences", 1))
    assert torch.equal(seqs, torch.from_numpy(Z[f"{name}:out"]))
    np.testing.assert_allclose(seq_scores.numpy(), Z[f"{name}:sequences_scores"], rtol=0, atol=1e-6)


def test_golden_covers_what_it_should():
    names = {c["name"]: c for c in CASES}
    tie_tol = meta(Z)["tie_tol"]
    assert meta(Z)["transformers"].startswith("5.")
    for key, case in (("suppress_tokens", "suppress"), ("begin_suppress_tokens", "begin"), ("min_new_tokens", "min_new"),
                      ("allowed_token_ids", "allowed"), ("bad_words_ids", "bad_words")):
        assert key in names[case]["kw"]
        strong = names[case + "_strong"]
        assert key in strong["kw"] and strong["strong"] and strong["margin"] >= 4 * tie_tol
    c = names["combined_ids"]["kw"]
    assert c["repetition_penalty"] == 1.1 and c["no_repeat_ngram_size"] == 2 and all(k in c for k in KEYS)
    beams = [c for c in CASES if "num_beams" in c["kw"]]
    assert len(beams) >= 2 and all(c["kw"]["num_beams"] == 3 and "suppress_tokens" in c["kw"] and "min_new_tokens" in c["kw"]
                                   and "begin_suppress_tokens" in c["kw"] for c in beams)
    # min_new_tokens holds back an eos the unconstrained pick would have emitted early
    kw = names["min_new"]["kw"]
    out = Z["min_new:out"]
    for b in range(out.shape[0]):
        hits = [t for t in range(out.shape[1]) if out[b, t] in _eos_list(kw)]
        assert not hits or hits[0] >= kw["min_new_tokens"]
    assert any(int(np.argmax(Z["min_new:logits"][t, b])) in _eos_list(kw) for t in range(kw["min_new_tokens"]) for b in range(out.shape[0]))


# ------------------------------------------------------------------------------------------------------------------------------------
def test_argument_errors_need_no_gpu():
    from vggt_qwen3_amd import generate as G
    tm = types.SimpleNamespace(vocab=320)                   # host arithmetic only: nothing else of the model is looked at
    e = torch.zeros(2, 4, 8)
    bad = (dict(suppress_tokens=[320]), dict(suppress_tokens=[-1]), dict(begin_suppress_tokens=[5, 1000]), dict(allowed_token_ids=[3, 320]),
           dict(bad_words_ids=[[320]]), dict(suppress_tokens=[1.5]), dict(min_new_tokens=-1), dict(min_new_tokens=7, max_new_tokens=6),
           dict(min_new_tokens=21), dict(allowed_token_ids=[]), dict(allowed_token_ids=[4, 5], suppress_tokens=[5, 4]),
           dict(allowed_token_ids=[4], bad_words_ids=[[4]]), dict(min_new_tokens=2, eos_token_id=400))
    for fn, who in ((G.generate, "generate"), (G.sample, "sample")):
        for kw in bad:
            with pytest.raises(ValueError, match=who):
                fn(tm, inputs_embeds=e, **kw)
        with pytest.raises(NotImplementedError, match=r"\[7, 8\]"):
            fn(tm, inputs_embeds=e, bad_words_ids=[[3], [7, 8]])
    # the plan itself
    plan = G._plan_constraints("generate", 320, 10, [5, 6], [1, 2, 2], [3], 4, None, [[7]])
    assert plan == dict(always=[1, 2, 7], until_min=[5, 6], at_begin=[3], min_new=4)
    plan = G._plan_constraints("generate", 10, 10, None, [1], None, 0, [1, 2, 3], None)
    assert plan["always"] == [0, 1, 4, 5, 6, 7, 8, 9] and plan["min_new"] == 0 and not plan["until_min"]
    # nothing to constrain: the call takes the unmasked entries
    assert G._plan_constraints("generate", 320, 10, 5) is None
    assert G._plan_constraints("generate", 320, 10, None, [], [], 3, None, []) is None          # min_new_tokens without an eos does nothing
    assert G._plan_constraints("generate", 320, 10, 5, None, None, 0, range(320)) is None


def test_the_keywords_are_named_parameters():
    """They used to disappear into **unused."""
    import inspect
    from vggt_qwen3_amd import generate as G
    for fn in (G.generate, G.sample):
        params = inspect.signature(fn).parameters
        assert all(k in params for k in ("suppress_tokens", "begin_suppress_tokens", "min_new_tokens", "allowed_token_ids", "bad_words_ids"))
    with pytest.raises(TypeError, match="suppress_tokens"):          # beam_search() has no **unused: an unknown keyword is an error
        G.beam_search(None, inputs_embeds=torch.zeros(1, 4, 8), suppress_tokens=[1])


def test_bit_planes():
    from vggt_qwen3_amd import ops
    for V in (320, 2051, 33, 151936):
        words = (V + 31) // 32
        p = ops.mask_planes(V, always=[0, 31, 32, V - 1], until_min=[V - 1], at_begin=[31, 31, 0])
        assert p.dtype == np.uint32 and p.shape == (3, words)
        want = np.zeros((3, words * 32), bool)
        want[0, [0, 31, 32, V - 1]] = True
        want[1, V - 1] = True
        want[2, [0, 31]] = True
        bits = ((p[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1).astype(bool).reshape(3, -1)
        assert np.array_equal(bits, want)
        assert not bits[:, V:].any()                              # V not a multiple of 32: the tail of the last word stays clear
    assert ops.mask_planes(33, [32]).tolist() == [[0, 1], [0, 0], [0, 0]]
    assert ops.mask_planes(64, [31, 32]).tolist()[0] == [0x80000000, 1]
    assert not ops.mask_planes(100).any()
    for ids in ([100], [-1], [2 ** 31]):
        with pytest.raises(ValueError):
            ops.mask_planes(100, ids)
    # the planes agree with the restatement at every gate
    kw = dict(eos_token_id=[7, 9], suppress_tokens=[1, 40], begin_suppress_tokens=[2], min_new_tokens=3, allowed_token_ids=list(range(60)),
              bad_words_ids=[[41]])
    from vggt_qwen3_amd import generate as G
    plan = G._plan_constraints("generate", 70, 8, **kw)
    p = ops.mask_planes(70, plan["always"], plan["until_min"], plan["at_begin"])
    bits = ((p[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1).astype(bool).reshape(3, -1)[:, :70]
    for n_new in range(6):
        eff = bits[0] | (bits[1] if n_new < plan["min_new"] else False) | (bits[2] if n_new == 0 else False)
        assert np.array_equal(eff, masked_ids(70, n_new, **kw)), n_new


def test_masked_entries_reject_bad_arguments_without_a_launch():
    import __graft_entry__ as g
    g.build()
    from vggt_qwen3_amd import _lib
    lib = _lib.load()
    keep = ctypes.create_string_buffer(64 + 16)
    p = (ctypes.addressof(keep) + 15) & ~15                       # a non-null, aligned host address: validation fails before any use

    def mask(**kw):
        m = _lib.PickMask()
        m.planes, m.words, m.min_new, m.prompt_cols = p, 32, 0, 0
        for k, v in kw.items():
            setattr(m, k, v)
        return m

    def greedy(m, V=1000):
        return lib.vq3_greedy_pick_masked(p, 1024, p, 2, V, p, 16, p, p, 1.0, 0, None, 0, 0, p, m, None)

    def sample(m, V=1000):
        return lib.vq3_sample_pick_masked(p, 1024, p, 2, V, p, 16, p, p, 1.0, 0, None, 0, 0, p, 1.0, 0, 1.0, 0, p, None, None, m, None)

    for fn, who in ((greedy, b"greedy_pick_masked"), (sample, b"sample_pick_masked")):
        for m, word in ((None, b"null"), (ctypes.byref(mask(planes=None)), b"null"), (ctypes.byref(mask(words=31)), b"shorter"),
                        (ctypes.byref(mask(min_new=-1)), b">= 0"), (ctypes.byref(mask(prompt_cols=-2)), b">= 0")):
            assert fn(m) != 0
            assert who in lib.vq3_last_error() and word in lib.vq3_last_error(), (who, lib.vq3_last_error())
