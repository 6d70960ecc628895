"""Host-side checks of the per-token log-probability entries (vq3_token_logprob, vq3_token_logprob_step) and of score()'s label
alignment: argument validation fails before any launch and names the entry; Qwen3ForCausalLM.score_rows on CPU tensors."""
import ctypes

import pytest
import torch


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from vggt_qwen3_amd import _lib
    return _lib.load()


def _buf():
    """A non-null host address: validation must fail before anything dereferences it."""
    b = ctypes.create_string_buffer(64)
    return b, ctypes.addressof(b)


def test_token_logprob_rejects_bad_arguments_without_a_launch(lib):
    keep, p = _buf()
    good = dict(logits=p, ld=16, n=2, V=9, targets=p, logprob=p, lse=p, rank=p, work=p, slices=0)

    def call(**kw):
        a = dict(good, **kw)
        return lib.vq3_token_logprob(a["logits"], a["ld"], a["n"], a["V"], a["targets"], a["logprob"], a["lse"], a["rank"], a["work"],
                                     a["slices"], None)

    for name in ("logits", "targets", "logprob"):
        assert call(**{name: None}) != 0
        msg = lib.vq3_last_error()
        assert b"token_logprob" in msg and b"null" in msg, msg
    assert call(work=None, slices=64) != 0 and b"token_logprob" in lib.vq3_last_error() and b"null" in lib.vq3_last_error()
    for kw in (dict(ld=8), dict(n=0), dict(n=-3), dict(V=0)):
        assert call(**kw) != 0
        msg = lib.vq3_last_error()
        assert b"token_logprob" in msg and b"shape" in msg, msg
    assert call(slices=65) != 0 and b"slices" in lib.vq3_last_error()
    assert call(slices=-1) != 0 and b"slices" in lib.vq3_last_error()


def test_token_logprob_step_rejects_bad_arguments_without_a_launch(lib):
    keep, p = _buf()
    good = dict(logits=p, ld=1024, B=4, V=1000, next_ids=p, step=p, off=0, finished=p, done=p, logprob=p, rank=None, cols=8, work=p)

    def call(**kw):
        a = dict(good, **kw)
        return lib.vq3_token_logprob_step(a["logits"], a["ld"], a["B"], a["V"], a["next_ids"], a["step"], a["off"], a["finished"],
                                          a["done"], a["logprob"], a["rank"], a["cols"], a["work"], None)

    for name in ("logits", "next_ids", "step", "finished", "done", "logprob", "work"):
        assert call(**{name: None}) != 0
        msg = lib.vq3_last_error()
        assert b"token_logprob_step" in msg and b"null" in msg, msg
    for kw in (dict(ld=999), dict(B=0), dict(V=0), dict(cols=0), dict(off=-1)):
        assert call(**kw) != 0
        msg = lib.vq3_last_error()
        assert b"token_logprob_step" in msg and b"shape" in msg, msg


def test_ops_wrappers_refuse_cpu_tensors():
    from vggt_qwen3_amd import _lib, ops
    with pytest.raises(_lib.Vq3Error, match="token_logprob"):
        ops.token_logprob(torch.zeros(2, 8, dtype=torch.bfloat16), torch.zeros(2, dtype=torch.int32), 8)


def test_score_rows_is_the_shift_of_label_rows():
    from vggt_qwen3_amd.qwen3 import Qwen3ForCausalLM as Q
    g = torch.Generator().manual_seed(0)
    B, L, Lp = 3, 13, 16
    labels = torch.randint(0, 50, (B, L), generator=g)
    labels[torch.rand(B, L, generator=g) < 0.5] = -100
    labels[0, 0], labels[1, 0] = 7, -100                 # position 0 is never predicted
    labels[2, L - 1] = 9                                 # the last column is predicted by row L - 2
    labels[1, 3:] = -100
    idx, tgt, dest = Q.score_rows(labels, Lp)
    # the same rows and targets as label_rows on the labels padded to the hidden rows' length
    padded = torch.cat([labels, torch.full((B, Lp - L), -100)], 1)
    idx2, tgt2 = Q.label_rows(padded)
    assert torch.equal(idx, idx2) and torch.equal(tgt, tgt2) and idx.dtype == torch.int32 and tgt.dtype == torch.int32
    # each result lands on the label it scores; everything else stays ignored
    out = torch.full((B * L,), -100, dtype=torch.long)
    out[dest] = tgt.long()
    want = labels.clone()
    want[:, 0] = -100
    assert torch.equal(out.view(B, L), want)
    b, t = idx.long() // Lp, idx.long() % Lp
    assert torch.equal(dest, b * L + t + 1) and int(t.max()) <= L - 2
    # nothing labelled: empty, not an error
    idx, tgt, dest = Q.score_rows(torch.full((2, 5), -100), 8)
    assert idx.numel() == 0 and tgt.numel() == 0 and dest.numel() == 0
