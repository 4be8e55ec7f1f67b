"""pack_feature_lists: the pure host helper that turns S per-stream id lists into the CSR pair EngineStream.update takes.  No GPU."""
import numpy as np
import pytest
import torch

from nnue_hip.engine import pack_feature_lists


def _unpack(ids, offsets):
    return [ids[int(offsets[b]):int(offsets[b + 1])].tolist() for b in range(offsets.numel() - 1)]


def test_csr_of_mixed_lists_with_empty_ones():
    lists = [[5, 1, 5], [], torch.tensor([7, 0], dtype=torch.int64), np.array([3], dtype=np.int16), (), torch.zeros(0, dtype=torch.int32),
             range(2, 4)]
    ids, offsets = pack_feature_lists(lists, 7)
    assert ids.dtype == torch.int32 and offsets.dtype == torch.int32
    assert not ids.is_cuda and not offsets.is_cuda
    assert offsets.tolist() == [0, 3, 3, 5, 6, 6, 6, 8]
    assert _unpack(ids, offsets) == [[5, 1, 5], [], [7, 0], [3], [], [], [2, 3]]  # order and duplicates are kept


def test_all_lists_empty():
    ids, offsets = pack_feature_lists([[], (), torch.zeros(0, dtype=torch.int64)], 3)
    assert ids.dtype == torch.int32 and ids.numel() == 0
    assert offsets.tolist() == [0, 0, 0, 0]
    ids, offsets = pack_feature_lists([[]], 1)
    assert ids.numel() == 0 and offsets.tolist() == [0, 0]


def test_ids_outside_int32_become_minus_one():
    big = [2 ** 31, -2 ** 31 - 1, 2 ** 40, 2 ** 31 - 1, -2 ** 31, -1]
    ids, offsets = pack_feature_lists([big, torch.tensor(big, dtype=torch.int64), np.array([2 ** 63], dtype=np.uint64)], 3)
    want = [-1, -1, -1, 2 ** 31 - 1, -2 ** 31, -1]
    assert _unpack(ids, offsets) == [want, want, [-1]]


def test_offsets_are_monotone_and_cover_the_ids():
    gen = np.random.default_rng(0)
    lists = [gen.integers(0, 1000, size=int(n)) for n in gen.integers(0, 50, size=33)]
    ids, offsets = pack_feature_lists(lists, 33)
    off = offsets.numpy()
    assert off[0] == 0 and off[-1] == ids.numel() and (np.diff(off) >= 0).all()
    assert _unpack(ids, offsets) == [a.tolist() for a in lists]


def test_wrong_list_count_is_refused():
    with pytest.raises(ValueError, match="expected 3 id lists"):
        pack_feature_lists([[1], [2]], 3)
    with pytest.raises(ValueError, match="expected 1 id lists"):
        pack_feature_lists([], 1)
    with pytest.raises(ValueError):
        pack_feature_lists(torch.zeros(3, 2, dtype=torch.int32), 3)  # a tensor is not a sequence of lists
    with pytest.raises(ValueError):
        pack_feature_lists(5, 1)


def test_non_integer_ids_are_refused():
    with pytest.raises(ValueError, match="integer ids"):
        pack_feature_lists([[1.0, 2.0]], 1)
    with pytest.raises(ValueError, match="integer ids"):
        pack_feature_lists([[1], torch.tensor([1.0])], 2)
    with pytest.raises(ValueError, match="integer ids"):
        pack_feature_lists([[1], np.array([0.5], dtype=np.float32)], 2)
    with pytest.raises(ValueError, match="integer ids"):
        pack_feature_lists([["a"]], 1)
    with pytest.raises(ValueError, match="integer ids"):
        pack_feature_lists([torch.tensor([True, False])], 1)
    with pytest.raises(ValueError, match="one dimension"):
        pack_feature_lists([[[1, 2], [3, 4]]], 1)
