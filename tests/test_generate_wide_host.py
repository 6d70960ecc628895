"""max_rows=, the caller's cap on the rows generate() / sample() decode per call: what can be checked without a GPU. Every error is
raised from host arithmetic before the model (None here) or the device is touched, as tests/test_sample_host.py checks for sample()'s
other arguments."""
import pytest
import torch


def _embeds(rows):
    return torch.zeros(rows, 4, 8)


@pytest.mark.parametrize("bad", [0, 65, -1, 2.5])
def test_max_rows_outside_1_to_64_raises(bad):
    from vggt_qwen3_amd import generate as G
    with pytest.raises(ValueError, match="generate: max_rows must be an integer in 1..64"):
        G.generate(None, inputs_embeds=_embeds(2), max_rows=bad)
    with pytest.raises(ValueError, match="sample: max_rows must be an integer in 1..64"):
        G.sample(None, inputs_embeds=_embeds(2), max_rows=bad)
    with pytest.raises(ValueError, match="max_rows"):
        G.generate(None, input_ids=torch.zeros(2, 4, dtype=torch.long), max_rows=bad)


def test_the_default_cap_is_8_rows():
    from vggt_qwen3_amd import generate as G
    with pytest.raises(ValueError, match="generate: at most 8 rows per call"):
        G.generate(None, inputs_embeds=_embeds(9))
    with pytest.raises(ValueError, match="generate: at most 8 rows per call"):
        G.generate(None, input_ids=torch.zeros(9, 4, dtype=torch.long))
    with pytest.raises(ValueError, match="sample: at most 8 rows per call"):
        G.sample(None, inputs_embeds=_embeds(9))
    with pytest.raises(ValueError, match=r"sample: at most 8 rows per call .* got 2 prompts x 5 draws"):
        G.sample(None, inputs_embeds=_embeds(2), num_return_sequences=5)


def test_rows_above_a_raised_cap_raise():
    from vggt_qwen3_amd import generate as G
    with pytest.raises(ValueError, match=r"sample: at most 16 rows per call .* got 3 prompts x 6 draws"):
        G.sample(None, inputs_embeds=_embeds(3), num_return_sequences=6, max_rows=16)
    with pytest.raises(ValueError, match="generate: at most 64 rows per call"):
        G.generate(None, inputs_embeds=_embeds(65), max_rows=64)
    with pytest.raises(ValueError, match="sample: at most 64 rows per call"):
        G.sample(None, inputs_embeds=_embeds(65), max_rows=64)
    with pytest.raises(ValueError, match="generate: at most 9 rows per call"):
        G.generate(None, inputs_embeds=_embeds(10), max_rows=9)


def test_the_constants():
    from vggt_qwen3_amd import ops
    assert ops.DECODE_MAX_ROWS == 64 and ops.SKINNY_MAX_ROWS == 8
