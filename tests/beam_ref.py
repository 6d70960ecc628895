"""Reference beam search for the tests: transformers 5.15 GenerationMixin._beam_search (do_sample=False) restated in plain torch, one
step at a time, with the state open so that a test can start it anywhere. It shares nothing with the product. torch.topk is called
exactly where transformers calls it (the top K continuations, the next running beams, the finished-slot merge).

dtype: torch.float32 repeats transformers' own arithmetic (tests/test_beam_host.py replays recorded scores and must reproduce its
outputs bit for bit in the integers); torch.float64 is the reference the device code is compared against."""
from typing import List, Optional, Sequence

import torch

NEG = -1.0e9


def process(logits: torch.Tensor, seqs: Sequence[Sequence[int]], penalty: float = 1.0, ngram: int = 0, dtype=torch.float64) -> torch.Tensor:
    """Steps 1-2: log_softmax of the logits [R, V], then - on the LOG-PROBABILITIES, as transformers applies its processors in beam
    search - RepetitionPenaltyLogitsProcessor and NoRepeatNGramLogitsProcessor over each row's ids so far."""
    lp = torch.log_softmax(logits.to(dtype), dim=-1)
    V = lp.shape[1]
    for r, seq in enumerate(seqs):
        seq = [int(t) for t in seq]
        if penalty != 1.0:
            for t in set(seq):
                if 0 <= t < V:
                    lp[r, t] = lp[r, t] * penalty if lp[r, t] < 0 else lp[r, t] / penalty
        if ngram > 0 and len(seq) + 1 >= ngram:
            pre = seq[len(seq) - (ngram - 1):] if ngram > 1 else []
            for i in range(len(seq) - ngram + 1):
                if seq[i:i + ngram - 1] == pre and 0 <= seq[i + ngram - 1] < V:
                    lp[r, seq[i + ngram - 1]] = -float("inf")
    return lp


def _gather(t: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
    while idx.dim() < t.dim():
        idx = idx.unsqueeze(-1)
    return torch.take_along_dim(t, idx, dim=1)


class BeamRef:
    """The state of _beam_search between two steps. Fresh: the start of a search over `prompt` (i64 [B, prompt_len]; [B, 0] for the
    inputs_embeds path)."""

    def __init__(self, prompt: torch.Tensor, num_beams: int, max_length: int, eos_ids: Optional[Sequence[int]] = None,
                 length_penalty: float = 1.0, early_stopping=False, fill: int = 0, dtype=torch.float64):
        B, P = prompt.shape
        self.B, self.nb, self.max_length, self.prompt_len, self.cur_len = B, num_beams, max_length, P, P
        self.eos = [] if eos_ids is None else [int(e) for e in eos_ids]
        self.K = max(2, 1 + len(self.eos)) * num_beams
        self.length_penalty, self.early_stopping, self.dtype, self.fill = float(length_penalty), early_stopping, dtype, fill
        self.running_sequences = torch.full((B, num_beams, max_length), fill, dtype=torch.int64)
        self.running_sequences[:, :, :P] = prompt[:, None, :]
        self.sequences = self.running_sequences.clone()
        self.running_beam_scores = torch.zeros((B, num_beams), dtype=dtype)
        self.running_beam_scores[:, 1:] = NEG
        self.beam_scores = torch.full((B, num_beams), NEG, dtype=dtype)
        self.is_sent_finished = torch.zeros((B, num_beams), dtype=torch.bool)
        self.heuristic = torch.ones((B, 1), dtype=torch.bool)
        self.running_beam_indices = torch.full((B, num_beams, max_length - P), -1, dtype=torch.int32)
        self.beam_indices = self.running_beam_indices.clone()
        self.done = False
        self.last = {}

    def rows(self) -> List[List[int]]:
        """The ids so far of every running row (what the processors see)."""
        return self.running_sequences[:, :, :self.cur_len].reshape(self.B * self.nb, self.cur_len).tolist()

    def step(self, log_probs: torch.Tensor) -> None:
        """Steps 3-9 on the processed log-probabilities [B * num_beams, V]. Leaves what it decided in self.last."""
        B, nb, K, cur, P = self.B, self.nb, self.K, self.cur_len, self.prompt_len
        V = log_probs.shape[1]
        acc = log_probs.to(self.dtype).reshape(B, nb, V) + self.running_beam_scores[:, :, None]
        acc = acc.reshape(B, nb * V)
        topk_log_probs, topk_indices = torch.topk(acc, k=K)
        parent = topk_indices // V
        topk_running_beam_indices = _gather(self.running_beam_indices, parent)
        topk_running_sequences = _gather(self.running_sequences, parent)
        tokens = topk_indices % V
        topk_running_sequences[:, :, cur] = tokens
        topk_running_beam_indices[:, :, cur - P] = (parent + torch.arange(B).view(-1, 1) * nb).to(torch.int32)
        hit = torch.zeros((B, K), dtype=torch.bool)
        for e in self.eos:
            hit |= tokens == e
        if cur + 1 >= self.max_length:
            hit[:] = True
        # the running beams of the next step
        running_lp = topk_log_probs + hit.to(self.dtype) * NEG
        nxt = torch.topk(running_lp, k=nb)[1]
        self.running_sequences = _gather(topk_running_sequences, nxt)
        self.running_beam_scores = _gather(running_lp, nxt)
        self.running_beam_indices = _gather(topk_running_beam_indices, nxt)
        # _update_finished_beams
        top_mask = torch.cat((torch.ones(nb, dtype=torch.bool), torch.zeros(K - nb, dtype=torch.bool)))
        just = hit & top_mask[None, :]
        fin_lp = topk_log_probs / ((cur + 1 - P) ** self.length_penalty)
        full = torch.all(self.is_sent_finished, dim=-1, keepdim=True) & (self.early_stopping is True)
        fin_lp = fin_lp + full.to(self.dtype) * NEG
        fin_lp = fin_lp + (~self.heuristic).to(self.dtype) * NEG
        fin_lp = fin_lp + (~just).to(self.dtype) * NEG
        merged_scores = torch.cat((self.beam_scores, fin_lp), dim=1)
        pick = torch.topk(merged_scores, k=nb)[1]
        self.sequences = _gather(torch.cat((self.sequences, topk_running_sequences), dim=1), pick)
        self.beam_scores = _gather(merged_scores, pick)
        self.beam_indices = _gather(torch.cat((self.beam_indices, topk_running_beam_indices), dim=1), pick)
        self.is_sent_finished = _gather(torch.cat((self.is_sent_finished, just), dim=1), pick)
        self.cur_len = cur + 1
        # _check_early_stop_heuristic
        if self.early_stopping == "never" and self.length_penalty > 0.0:
            hyp = self.max_length - P
        else:
            hyp = self.cur_len - P
        best_running = self.running_beam_scores[:, :1] / (hyp ** self.length_penalty)
        worst = torch.where(self.is_sent_finished, torch.min(self.beam_scores, dim=1, keepdim=True)[0],
                            torch.tensor(NEG, dtype=self.dtype))
        self.heuristic = self.heuristic & torch.any(best_running > worst, dim=-1, keepdim=True)
        # _beam_search_has_unfinished_sequences
        unfinished = bool(torch.any(self.heuristic)) and not (bool(torch.all(self.is_sent_finished)) and self.early_stopping is True) \
            and not bool(torch.all(hit))
        self.done = not unfinished
        self.last = dict(acc=acc, topk_log_probs=topk_log_probs, topk_indices=topk_indices, hit=hit, running_lp=running_lp, next=nxt,
                         merged_scores=merged_scores, merged_pick=pick, best_running=best_running, worst=worst,
                         parents=(_gather(parent, nxt) + torch.arange(B).view(-1, 1) * nb).reshape(-1),
                         tokens=_gather(tokens, nxt).reshape(-1))

    def finished_lengths(self) -> torch.Tensor:
        """Ids (prompt included) of every finished slot [B, num_beams]: the entries of beam_indices that were written."""
        return self.prompt_len + (self.beam_indices >= 0).sum(-1)

    def outputs(self, num_return_sequences: int):
        """Step 5 of _beam_search: (sequences, sequences_scores, beam_indices), cropped."""
        n = num_return_sequences
        seqs = self.sequences[:, :n].reshape(self.B * n, -1)
        scores = self.beam_scores[:, :n].reshape(self.B * n)
        bi = self.beam_indices[:, :n].reshape(self.B * n, -1)
        longest = int((bi >= 0).sum(1).max())
        return seqs[:, :self.prompt_len + longest], scores, bi[:, :longest]


def assemble(fin_seq: torch.Tensor, fin_len: torch.Tensor, num_return_sequences: int, fill: int) -> torch.Tensor:
    """The output assembly alone, from finished slots given as (ids [B, num_beams, max_length], ids per slot [B, num_beams], prompt
    included): the best num_return_sequences slots of every prompt, prompt-major, cropped to the longest returned hypothesis, `fill`
    past each one's own end."""
    B, nb, _ = fin_seq.shape
    n = num_return_sequences
    lens = fin_len[:, :n].reshape(B * n)
    longest = int(lens.max())
    out = fin_seq[:, :n].reshape(B * n, -1)[:, :longest].clone().to(torch.int64)
    cols = torch.arange(longest)[None, :]
    out[cols >= lens[:, None]] = fill
    return out
