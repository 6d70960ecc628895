"""KV-cache sessions, the host side: which columns extend() computes for every kind of mask (generate._plan_extend over
generate._row_spans), the errors raised before anything is launched, KVCache.truncate's arithmetic, and the argument checks of the two
C entry points (vq3_qwen_append_qkprep / vq3_qwen_append_attn) - all without a GPU."""
import ctypes

import pytest
import torch

from vggt_qwen3_amd import generate as G


def _spans(mask):
    return G._row_spans(torch.tensor(mask))


def test_plan_extend_left_right_and_unpadded_masks():
    left = _spans([[0, 0, 0, 1, 1, 1, 1, 1], [0, 1, 1, 1, 1, 1, 1, 1]])
    assert left == [(3, 5), (1, 7)]
    assert G._plan_extend(left, [0, 0], 64) == [(3, 5), (1, 7)]                 # cached = 0: the whole attended run
    assert G._plan_extend(left, [2, 6], 64) == [(5, 3), (7, 1)]                 # ragged cached lengths: each row's own suffix
    right = _spans([[1, 1, 1, 1, 1, 0, 0, 0], [1, 1, 1, 1, 1, 1, 1, 0]])
    assert G._plan_extend(right, [4, 0], 64) == [(4, 1), (0, 7)]
    full = _spans([[1] * 8, [1] * 8])
    assert G._plan_extend(full, [7, 3], 64) == [(7, 1), (3, 5)]
    both = _spans([[0, 0, 1, 1, 1, 1, 0, 0]])                                    # padding on both sides
    assert G._plan_extend(both, [1], 64) == [(3, 3)]
    # a row may fill the cache to its last position, with and without tokens to decode after it
    assert G._plan_extend(_spans([[1] * 64]), [60], 64) == [(60, 4)]
    assert G._plan_extend(_spans([[1] * 60]), [0], 64, 4) == [(0, 60)]


def test_plan_extend_errors():
    spans = _spans([[0, 1, 1, 1, 1, 1], [1, 1, 1, 1, 1, 1]])
    with pytest.raises(ValueError, match="nothing new"):
        G._plan_extend(spans, [5, 2], 64)                                       # row 0: all 5 attended positions cached
    with pytest.raises(ValueError, match="nothing new"):
        G._plan_extend(spans, [2, 9], 64)                                       # row 1: the cache holds more than the row has
    with pytest.raises(ValueError, match="capacity"):
        G._plan_extend(_spans([[1] * 65]), [0], 64)
    with pytest.raises(ValueError, match="capacity"):
        G._plan_extend(_spans([[1] * 60]), [0], 64, 5)                          # 60 + 5 tokens to decode > 64
    with pytest.raises(ValueError, match="contiguous"):
        _spans([[1, 1, 0, 1, 1, 1]])
    with pytest.raises(ValueError, match="rows"):
        G._plan_extend(spans, [0], 64)                                          # cache batch != rows
    with pytest.raises(ValueError, match="rows"):
        G._plan_extend(spans, [0, 0, 0], 64)


def _host_cache(batch, capacity, lengths):
    """A KVCache without device tensors: truncate() is host arithmetic and one small copy into `lens`."""
    c = object.__new__(G.KVCache)
    c.batch, c.capacity = batch, capacity
    c.K = c.V = None
    c.lens = torch.tensor(lengths, dtype=torch.int32)
    c.lengths = list(lengths)
    return c


def test_truncate_only_shrinks():
    c = _host_cache(2, 64, [29, 19])
    c.truncate([11, 19])
    assert c.lengths == [11, 19] and c.lens.tolist() == [11, 19]
    c.truncate(7)                                                               # an int: every row
    assert c.lengths == [7, 7] and c.lens.tolist() == [7, 7]
    c.truncate([0, 7])
    assert c.lengths == [0, 7]
    for bad in ([1, 7], [0, 8], [0, -1], [0], [0, 0, 0]):
        with pytest.raises(ValueError):
            c.truncate(bad)
    assert c.lengths == [0, 7] and c.lens.tolist() == [0, 7]                    # a refused call changes nothing


def test_append_entry_points_reject_bad_arguments_without_gpu():
    """Argument validation runs on the host before any launch: null pointers, head_dim, heads per kv head, cache capacity (a multiple
    of 64 in [64, 12288], the decode attention's limits) and chunk length (1..8192)."""
    from vggt_qwen3_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)                                                   # non-null; never dereferenced: every call fails its checks

    def qkprep(B=1, Ln=8, Hq=4, Hkv=1, Dh=128, Lmax=64, ptr=p):
        return lib.vq3_qwen_append_qkprep(ptr, p, p, p, p, p, p, p, p, p, B, Ln, Hq, Hkv, Dh, Lmax, 1e-6, None)

    def attn(B=1, Ln=8, Hq=4, Hkv=1, Dh=128, Lmax=64, ldo=512, ptr=p):
        return lib.vq3_qwen_append_attn(ptr, p, p, p, p, p, B, Ln, Hq, Hkv, Dh, Lmax, ldo, 0.1, None)

    for fn in (qkprep, attn):
        assert fn(ptr=None) != 0 and b"null" in lib.vq3_last_error()
        assert fn(Dh=64) != 0 and b"head_dim" in lib.vq3_last_error()
        assert fn(Hq=8, Hkv=1) != 0 and b"query heads per kv head" in lib.vq3_last_error()
        assert fn(Hq=3, Hkv=2) != 0 and b"query heads per kv head" in lib.vq3_last_error()
        assert fn(B=0) != 0
        for Lmax in (0, 63, 96, 12352):
            assert fn(Lmax=Lmax) != 0 and b"capacity" in lib.vq3_last_error(), Lmax
        for Ln in (0, -1, 8193):
            assert fn(Ln=Ln) != 0 and b"chunk length" in lib.vq3_last_error(), Ln
    assert attn(ldo=511) != 0 and b"stride" in lib.vq3_last_error()
    assert attn(ldo=256) != 0 and b"stride" in lib.vq3_last_error()              # narrower than Hq * 128
