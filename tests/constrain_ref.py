"""Reference restatement of the decoding constraints for the tests: transformers' SuppressTokensLogitsProcessor,
SuppressTokensAtBeginLogitsProcessor (begin_index = prompt length), MinNewTokensLengthLogitsProcessor, PrefixConstrainedLogitsProcessor
with a fixed allowed set and one-token NoBadWordsLogitsProcessor entries, on one row of scores. It shares nothing with the product.
Every one of them only writes -inf, so their order among themselves and after the repetition penalty / n-gram ban does not matter; a
caller composes: tests/test_sample_host.py's processed_logits() -> constrain() -> ref_prepare / ref_cut / ref_pick for the picks,
tests/beam_ref.py's process() -> constrain() per row -> BeamRef.step() for beam search (there the scores are log-probabilities)."""
from typing import Optional, Sequence

import numpy as np


def masked_ids(V: int, n_new: int, eos_token_id=None, suppress_tokens: Optional[Sequence[int]] = None,
               begin_suppress_tokens: Optional[Sequence[int]] = None, min_new_tokens: int = 0,
               allowed_token_ids: Optional[Sequence[int]] = None, bad_words_ids: Optional[Sequence[Sequence[int]]] = None) -> np.ndarray:
    """bool [V]: the ids that score -inf when n_new new ids have been emitted so far."""
    m = np.zeros(V, dtype=bool)
    for t in (suppress_tokens or []):
        m[int(t)] = True
    for entry in (bad_words_ids or []):
        entry = list(entry)
        if len(entry) != 1:
            raise NotImplementedError(f"bad_words_ids entry {entry}: only one-token entries")
        m[int(entry[0])] = True
    if n_new == 0:
        for t in (begin_suppress_tokens or []):
            m[int(t)] = True
    if eos_token_id is not None and n_new < int(min_new_tokens or 0):
        for e in ([eos_token_id] if isinstance(eos_token_id, int) else list(eos_token_id)):
            m[int(e)] = True
    if allowed_token_ids is not None:
        keep = np.zeros(V, dtype=bool)
        keep[[int(t) for t in allowed_token_ids]] = True
        m |= ~keep
    return m


def constrain(scores, ids_so_far, n_new: int, **keywords):
    """The masked row: a copy of `scores` (a 1-d numpy array or torch tensor of any float dtype, f32 in the tests) with -inf at every
    masked id. ids_so_far (what a prefix_allowed_tokens_fn would be shown) does not enter: the allowed set is fixed."""
    del ids_so_far
    m = masked_ids(int(scores.shape[-1]), n_new, **keywords)
    if isinstance(scores, np.ndarray):
        out = scores.copy()
        out[m] = -np.inf
        return out
    import torch
    out = scores.clone()
    out[torch.from_numpy(m)] = -float("inf")
    return out
