"""The mock backend's Embedding backward follows the header's rule for ids outside [0, V) (include/tnt_hip.h: every entry
point treats an id as clip(id, 0, V-1)): its dense and sparse forms agree with each other and with the float64 scatter over
the clamped ids, and the sparse form's cleanup covers the rows that stray ids of the previous step wrote.  CPU only."""
import numpy as np
import pytest
import torch

from mock_backend import MockBackend

I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1


def stray_layouts(V):
    """layout (e) of tests/test_gpu_embedding_paths.py: stray ids mixed with genuine 0 and V-1, once with the stray
    occurrence of a row first and once with the in-range one first"""
    return {"stray-first": [-1, 0, -7, I32_MIN, V, V - 1, V + 5, I32_MAX, 0, V - 1, -1, V, 3, 4, 3],
            "in-range-first": [0, V - 1, -1, -7, I32_MIN, V, V + 5, I32_MAX, 0, V - 1, 4, 3, 4, 2, 1]}


@pytest.mark.parametrize("order", ["stray-first", "in-range-first"])
def test_mock_dense_and_sparse_agree_on_stray_ids(order):
    B, T, E, V = 5, 3, 8, 9
    rng = np.random.default_rng(3)
    be = MockBackend()
    ids = np.array(stray_layouts(V)[order], np.int64).reshape(B, T)
    rows = rng.integers(-3, 4, (T, B, E)).astype(np.float32)                       # exact in any order
    want = np.zeros((V, E))
    np.add.at(want, np.clip(ids, 0, V - 1).reshape(-1), rows.transpose(1, 0, 2).reshape(B * T, E).astype(np.float64))
    idt, dr = torch.tensor(ids.astype(np.int32)), torch.from_numpy(rows.reshape(T * B, E).copy())
    dense, sq = torch.full((V, E), 9.0), torch.zeros(1)
    be.embedding_bwd(dr, idt, dense, sq, torch.zeros(B * T), B, T, E, E, V)
    assert np.array_equal(dense.numpy(), want.astype(np.float32)) and float(sq) == float((rows.astype(np.float64) ** 2).sum())
    # sparse, behind a step whose stray ids wrote rows 0 and V-1 and whose id 5 vanishes: the three rows are cleaned
    sparse = torch.zeros(V, E)
    sparse[0], sparse[V - 1], sparse[5] = 1.0, 2.0, 3.0
    other = ids.copy()
    other[ids == 0] = 6
    other[ids == V - 1] = 7                                                        # a step without genuine 0 and V-1
    for cur in (ids, other[::-1].copy(), np.full((B, T), 4)):                      # the last one writes none of the three
        prev = torch.tensor([I32_MIN, V + 2, 5] + [-1] * (B * T - 3), dtype=torch.int32)
        tab = sparse.clone()
        parts = torch.full((be.embedding_bwd_parts(B, T, E),), float("nan"))
        be.embedding_bwd_sparse(dr, torch.tensor(cur.astype(np.int32)), prev, tab, parts, B, T, E, E, V)
        ref = torch.full((V, E), 9.0)
        be.embedding_bwd(dr, torch.tensor(cur.astype(np.int32)), ref, None, None, B, T, E, E, V)
        assert torch.equal(tab, ref), order
        assert float(parts.sum()) == float(sq)
