"""What beam search can show without a GPU: tests/beam_ref.py - the reference the device code is held to in tests/test_beam_gpu.py -
replayed on the per-step scores transformers recorded (tests/golden/beam_tiny.npz, tools/make_golden_beam.py) reproduces transformers'
own sequences, beam indices and scores; beam_search()'s argument errors; the header constant."""
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import beam_ref
from tests.golden_io import load, meta

ROOT = Path(__file__).resolve().parents[1]
Z = load("beam_tiny.npz")
CASES = meta(Z)["cases"]


def _eos_list(kw):
    e = kw.get("eos_token_id")
    return [] if e is None else ([e] if isinstance(e, int) else list(e))


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_reference_replays_transformers(case):
    """Both sides call torch.topk on the same CPU values, so this is exact even where scores tie."""
    name, kw = case["name"], case["kw"]
    scores = torch.from_numpy(Z[f"{name}:scores"])                      # [steps, B * num_beams, 320] f32, after the processors
    prompt = torch.from_numpy(Z["input_ids"]) if case["input"] == "input_ids" else torch.zeros((Z["embeds"].shape[0], 0), dtype=torch.int64)
    eos = _eos_list(kw)
    pad = kw.get("pad_token_id")
    fill = pad if pad is not None else eos[0]
    ref = beam_ref.BeamRef(prompt, kw["num_beams"], prompt.shape[1] + kw["max_new_tokens"], eos, kw.get("length_penalty", 1.0),
                           kw.get("early_stopping", False), fill=fill, dtype=torch.float32)
    steps = 0
    while not ref.done:
        ref.step(scores[steps])
        steps += 1
    assert steps == scores.shape[0]                                      # the loop condition stopped where transformers stopped
    seqs, seq_scores, bi = ref.outputs(kw.get("num_return_sequences", 1))
    assert torch.equal(seqs, torch.from_numpy(Z[f"{name}:sequences"]))
    assert torch.equal(bi, torch.from_numpy(Z[f"{name}:beam_indices"]))
    np.testing.assert_allclose(seq_scores.numpy(), Z[f"{name}:sequences_scores"], rtol=0, atol=1e-6)
    # the assembly on its own, from the finished slots, gives the same ids
    out = beam_ref.assemble(ref.sequences, ref.finished_lengths(), kw.get("num_return_sequences", 1), fill)
    assert torch.equal(out, seqs)


def test_golden_covers_what_it_should():
    names = {c["name"]: c for c in CASES}
    assert meta(Z)["transformers"].startswith("5.")
    assert {c["kw"].get("early_stopping", False) for c in CASES} >= {False, True, "never"}
    assert {c["kw"].get("length_penalty", 1.0) for c in CASES} >= {0.0, 1.0, 2.0}
    assert any(len(_eos_list(c["kw"])) == 2 for c in CASES)
    assert names["ids"]["kw"]["repetition_penalty"] == 1.1 and names["ids"]["kw"]["no_repeat_ngram_size"] == 2
    # some beam finished early somewhere: a returned hypothesis shorter than the longest
    assert len(_eos_list(names["es_true_lp0"]["kw"])) == 2 and (Z["es_true_lp0:sequences"] == 317).any()


def test_process_applies_the_processors_to_log_probabilities():
    logits = torch.tensor([[2.0, 1.0, 0.0, -1.0]])
    lp0 = torch.log_softmax(logits.double(), -1)
    lp = beam_ref.process(logits, [[0, 1, 0, 2, 0]], penalty=2.0, ngram=2)
    assert lp[0, 0] == lp0[0, 0] * 2.0                                   # log-probabilities are negative: multiplied, once per distinct id
    assert lp[0, 1] == -float("inf") and lp[0, 2] == -float("inf")      # both followed an earlier 0
    assert lp[0, 3] == lp0[0, 3]


def test_beam_search_argument_errors_need_no_gpu():
    from vggt_qwen3_amd import generate as G
    e = torch.zeros(2, 4, 8)
    for kw in (dict(num_beams=1), dict(num_beams=9), dict(num_beams=2.5), dict(num_beams=5), dict(num_beams=3, inputs_embeds=torch.zeros(3, 4, 8)),
               dict(num_return_sequences=0), dict(num_return_sequences=5), dict(num_beams=2, num_return_sequences=3),
               dict(eos_token_id=[1, 2, 3, 4]), dict(early_stopping="always"), dict(early_stopping=1), dict(early_stopping=None),
               dict(length_penalty=float("inf")), dict(length_penalty=float("nan")),
               dict(inputs_embeds=None), dict(input_ids=torch.zeros(2, 4, dtype=torch.long))):
        with pytest.raises(ValueError, match="beam_search"):
            G.beam_search(None, **dict(dict(inputs_embeds=e), **kw))
    from vggt_qwen3_amd.qwen3 import Qwen3ForCausalLM
    assert callable(Qwen3ForCausalLM.beam_search)


def test_generate_names_beam_search_when_it_refuses_beams():
    from vggt_qwen3_amd import generate as G
    with pytest.raises(NotImplementedError, match=r"beam_search\(\)"):
        G.generate(None, inputs_embeds=torch.zeros(1, 4, 8), num_beams=4)


def test_beam_constants_match_the_header():
    from vggt_qwen3_amd import ops
    text = (ROOT / "include" / "vq3_hip.h").read_text()
    m = re.search(r"#define\s+VQ3_BEAM_WORK_PER_ROW\s+(\d+)", text)
    assert m and int(m.group(1)) == ops.BEAM_WORK_PER_ROW == 64 * (2 + 2 * 32)


def test_beam_entries_reject_bad_arguments_without_a_launch():
    import ctypes
    import __graft_entry__ as g
    g.build()
    from vggt_qwen3_amd import _lib
    lib = _lib.load()
    keep = ctypes.create_string_buffer(64 + 16)
    p = (ctypes.addressof(keep) + 15) & ~15                   # a non-null, 16-byte aligned host address: validation fails before any use

    def desc(**kw):
        d = _lib.BeamStepDesc()
        for f in ("logits_bf16", "step", "run_seq", "run_score", "fin_seq", "fin_score", "fin_len", "fin_flag", "heur", "all_done",
                  "next_ids", "src_row", "work"):
            setattr(d, f, p)
        d.ld_logits, d.V, d.n_prompts, d.num_beams, d.max_len, d.prompt_len = 1024, 1000, 2, 3, 32, 0
        d.repetition_penalty, d.length_penalty = 1.0, 1.0
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    for kw, word in ((dict(work=None), b"null"), (dict(all_done=None), b"null"), (dict(num_beams=1), b"num_beams"), (dict(num_beams=9), b"num_beams"),
                     (dict(n_prompts=3), b"rows"), (dict(n_prompts=5, num_beams=2), b"rows"), (dict(n_eos=4), b"eos"), (dict(ld_logits=999), b"shape"),
                     (dict(V=1 << 19, ld_logits=1 << 19), b"shape"), (dict(max_len=513), b"512"), (dict(prompt_len=32), b"prompt_len"),
                     (dict(repetition_penalty=0.0), b"repetition_penalty"), (dict(early_stopping=3), b"early_stopping"),
                     (dict(length_penalty=float("inf")), b"length_penalty"), (dict(trace_parent=p), b"trace")):
        assert lib.vq3_beam_step(ctypes.byref(desc(**kw)), None) != 0
        assert b"beam_step" in lib.vq3_last_error() and word in lib.vq3_last_error(), (kw, lib.vq3_last_error())
    good = [p, p, p, p, None, 2, 2, 3, 2, 128, 128, None]
    for at, bad, word in ((0, None, b"null"), (2, None, b"null"), (10, 64, b"head_dim"), (7, 9, b"beams"), (0, p + 2, b"aligned"), (9, 0, b"shape")):
        a = list(good)
        a[at] = bad
        assert lib.vq3_beam_reorder(*a) != 0
        assert b"beam_reorder" in lib.vq3_last_error() and word in lib.vq3_last_error(), (at, lib.vq3_last_error())
