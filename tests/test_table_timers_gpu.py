"""The two table-aligner timers no other test runs, local_time_device and semiglobal_full_time_device, on torch device
buffers: the average time is positive and finite, and what the timed calls left in the buffers is what local_align and
semiglobal_full return for the same inputs (those are pinned to the C restatements by test_local_gpu.py and
test_sgfull_gpu.py)."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N, LEN1, LEN2 = 3, 5, 7
SM = np.array([5, -4, -3, -4, -4, 6, -4, -2, -3, -4, 7, -4, -4, -2, -4, 8], np.int8)
GAP = 3


def _device_buffers(a, b, ends_width, move_words):
    dev = torch.device("cuda:0")
    t = dict(a=torch.from_numpy(a).to(dev), b=torch.from_numpy(b).to(dev), sc=torch.zeros(N, dtype=torch.int32, device=dev),
             ends=torch.zeros((N, ends_width), dtype=torch.int32, device=dev),
             mv=torch.zeros((N, move_words), dtype=torch.int64, device=dev), ct=torch.zeros(N, dtype=torch.int32, device=dev))
    torch.cuda.synchronize()
    return t


def _assert_same(t, want, steps_of):
    """The buffers against a host entry's (scores, ends, moves, counts); moves up to each alignment's last step."""
    torch.cuda.synchronize()
    scores, ends, moves, counts = want
    assert np.array_equal(t["sc"].cpu().numpy(), scores) and np.array_equal(t["ends"].cpu().numpy(), ends)
    assert np.array_equal(t["ct"].cpu().numpy().view(np.uint32), counts)
    got = t["mv"].cpu().numpy().view(np.uint64)
    for k in range(N):
        for step in range(steps_of(int(counts[k]))):
            assert (int(got[k, step // 32]) >> 2 * (step % 32)) & 3 == (int(moves[k, step // 32]) >> 2 * (step % 32)) & 3, (k, step)


def test_local_time_device(gpu):
    rng = np.random.default_rng(11)
    a, b = rng.integers(0, 4, (N, LEN1), dtype=np.uint8), rng.integers(0, 4, (N, 128), dtype=np.uint8)
    b[0, 40:45] = a[0]                                            # one alignment with a run of five matches
    t = _device_buffers(a, b, 4, gpu.local_move_words(LEN1))
    ms = gpu.local_time_device(t["a"].data_ptr(), LEN1, t["b"].data_ptr(), N, SM, GAP, t["sc"].data_ptr(), t["ends"].data_ptr(),
                               t["mv"].data_ptr(), t["ct"].data_ptr(), iters=2)
    assert type(ms) is float and math.isfinite(ms) and ms > 0
    _assert_same(t, gpu.local_align(a, b, SM, GAP), lambda steps: steps)


def test_semiglobal_full_time_device(gpu):
    rng = np.random.default_rng(12)
    a, b = rng.integers(0, 4, (N, LEN1), dtype=np.uint8), rng.integers(0, 4, (N, LEN2), dtype=np.uint8)
    b[0, :LEN1] = a[0]
    t = _device_buffers(a, b, 2, gpu.semiglobal_full_move_words(LEN1, LEN2))
    ms = gpu.semiglobal_full_time_device(t["a"].data_ptr(), LEN1, t["b"].data_ptr(), LEN2, N, SM, GAP, t["sc"].data_ptr(),
                                         t["ends"].data_ptr(), t["mv"].data_ptr(), t["ct"].data_ptr(), iters=2)
    assert type(ms) is float and math.isfinite(ms) and ms > 0
    _assert_same(t, gpu.semiglobal_full(a, b, SM, GAP), lambda length: length - 1)
