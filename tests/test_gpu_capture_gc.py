"""GPU: no finaliser runs inside a stream capture (hmse_amd/stream_common.py PhaseGraphs.run).  A dropped stream front end is cyclic
garbage that holds device buffers and captured graphs; the cycle collector runs whenever an allocation count trips it, and inside a
capture its finalisers (graph destruction, pool release) are calls the runtime does not allow there."""
import gc
import weakref

import pytest

pytestmark = pytest.mark.gpu


def test_cyclic_garbage_is_collected_before_a_capture_and_never_inside_it():
    import torch
    from hmse_amd import stream_common
    assert torch.cuda.is_available()
    dev = torch.device("cuda:0")
    x = torch.zeros(1024, dtype=torch.int32, device=dev)
    seen = []                                                        # (label, was a capture under way when the finaliser ran)

    class Node:
        pass

    def garbage(label):
        a = Node()
        a.me = a                                                     # a cycle: only the collector frees it
        weakref.finalize(a, lambda: seen.append((label, torch.cuda.is_current_stream_capturing())))

    def fn():
        if torch.cuda.is_current_stream_capturing():
            garbage("inside")
            churn = [[] for _ in range(200_000)]                     # far more container allocations than any collector threshold
            del churn
        x.add_(1)

    pg = stream_common.PhaseGraphs(True, lambda size: stream_common.SizeEntry(None))
    assert gc.isenabled()
    old = gc.get_threshold()
    gc.set_threshold(50, 2, 2)
    try:
        pg.run(8, "A", fn)                                           # first use: eager
        pg.end_batch(8)
        garbage("before")
        pg.run(8, "A", fn)                                           # second use: captured, then replayed
        pg.end_batch(8)
        assert gc.isenabled() and pg.captured(8) == {"A"}
        assert ("before", False) in seen and not any(inside for _, inside in seen)
        gc.collect()
        assert ("inside", False) in seen                             # freed once the capture had ended
        pg.run(8, "A", fn)
        torch.cuda.synchronize()
        assert int(x[0]) == 3                                        # eager, the captured graph's first replay, a second replay
    finally:
        gc.set_threshold(*old)
