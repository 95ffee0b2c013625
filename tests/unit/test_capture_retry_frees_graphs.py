"""``StepGraphs._capture``: when an overlapped capture fails on some rank and every rank retries in
split mode, whatever the failed capture still held (its HIP graphs, through the caught error's
traceback) must be gone BEFORE the retry starts capturing.  Left to the cyclic collector it is freed
at some later allocation, possibly inside a capture, where HIP refuses to destroy a graph and the
graph's destructor aborts the process.  No GPU: the capture itself is replaced by stand-ins."""

import gc
import types
import weakref

import torch

from rocket_amd.runtime import comm, graphs


class _Graph:
    """Stands in for the failed capture's graph objects."""


def test_failed_capture_is_freed_before_the_retry(monkeypatch):
    sg = object.__new__(graphs.StepGraphs)
    sg.mod = types.SimpleNamespace(_accelerator=types.SimpleNamespace(sync_gradients=True, num_processes=2))
    rep = types.SimpleNamespace(capture_mode="overlap", force_split=False)
    alive_at_retry = []
    held = []

    def capture_inner(attrs, tens, pend):
        if not held:
            g = _Graph()  # a local of the raising frame: reachable only through the error's traceback
            held.append(weakref.ref(g))
            raise RuntimeError("capture failed on this rank")
        alive_at_retry.append(held[0]() is not None)
        return types.SimpleNamespace(graphs=[])

    answers = iter([False, True])
    monkeypatch.setattr(sg, "_bind_pending", lambda attrs, tens, run: (None, []), raising=False)
    monkeypatch.setattr(sg, "_replica", lambda: rep, raising=False)
    monkeypatch.setattr(sg, "_side_effects", lambda pend: None, raising=False)
    monkeypatch.setattr(sg, "_restore_side_effects", lambda pend, side: None, raising=False)
    monkeypatch.setattr(sg, "_capture_inner", capture_inner, raising=False)
    monkeypatch.setattr(comm, "all_ranks_agree", lambda ok: next(answers))
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)
    gc.disable()  # the automatic collector must not be what frees it
    try:
        v = sg._capture(None, [], run=False)
    finally:
        gc.enable()
    assert rep.force_split and v is not None
    assert alive_at_retry == [False]
