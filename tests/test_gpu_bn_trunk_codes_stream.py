"""GPU: slfp_bn_res_codes_train_fwd runs on the current stream (the rest of its tests: test_gpu_bn_res_codes_train.py).
In a file of its own that sorts behind test_gpu_bn_train.py: this test draws streams from the process's pool, and the stream tests
of test_gpu_bn_res_train.py and test_gpu_bn_train.py take the first stream the pool hands them -- which hardware queue that one
shares depends on how many streams were drawn before it.  Drawn in front of them, this file's streams made
test_gpu_bn_train.py::test_runs_on_the_current_stream serialise behind the default stream."""
import pytest
import torch

import _bn_cases as B
from _bn_calls import _same
from _bn_res_codes_calls import res_codes_fwd
from test_gpu_bn_codes_train import KAS
from test_gpu_bn_res_codes_train import _res

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _side_stream(cycles):
    """The first of four new streams on which work completes while a sleep of `cycles` holds the default stream (HIP puts streams
    on a few hardware queues, and a stream that shares the default stream's serialises behind it: the rule of
    test_gpu_headline._concurrent_streams)."""
    for s in [torch.cuda.Stream(device=DEV) for _ in range(4)]:
        torch.cuda.synchronize()
        held, done = torch.cuda.Event(), torch.cuda.Event()
        torch.cuda._sleep(cycles)
        held.record()
        with torch.cuda.stream(s):
            done.record()
        done.synchronize()
        free = not held.query()
        torch.cuda.synchronize()
        if free:
            return s
    raise AssertionError("none of four new streams runs beside the default stream")


def test_runs_on_the_current_stream():
    """The default stream is held by a sleep; a call on another stream completes meanwhile, with the same bits."""
    case = (B.ragged(32), False)
    shape = case[0]
    d = B.inputs(*case)
    res = _res(case, KAS[0])

    def run():
        return res_codes_fwd(shape, d, 1, res, KAS[0], 8)

    want = run()
    from test_gpu_headline import _sleep_cycles
    cycles = _sleep_cycles(200)
    torch.cuda.synchronize()
    side = _side_stream(cycles // 10)
    side.wait_stream(torch.cuda.current_stream())
    held, done = torch.cuda.Event(), torch.cuda.Event()
    torch.cuda._sleep(cycles)               # 0.2 s on the default stream
    held.record()
    with torch.cuda.stream(side):
        got = run()
        done.record()
    done.synchronize()
    still_held = not held.query()
    torch.cuda.synchronize()
    assert still_held, "the side stream's work waited for the default stream (or the sleep was too short to tell)"
    for a, b in zip(got, want):
        assert torch.equal(a, b) if a.dtype == torch.uint8 else _same(a, b)
