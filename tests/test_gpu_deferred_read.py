"""gflow_amd.pinned.DeferredRead alone: a few device words copied to page-locked memory behind the queued work and looked at
later (``-m gpu``).  FitEngine's two watches and the batched rasteriser's flags are instances of it."""
import pytest
import torch

from gflow_amd.pinned import DeferredRead

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _words(values):
    return torch.tensor(values, dtype=torch.int32).to(DEV)


def test_a_read_returns_the_words_of_the_moment_of_the_watch():
    src = _words([7, 1, 0, 3, -2])
    r = DeferredRead(5)
    assert not r.armed and r.ready() and r.read() is None and r.poll() is None
    r.watch(src)
    src.fill_(99)                        # (same stream, behind the copy)
    assert r.armed
    assert r.read() == [7, 1, 0, 3, -2]
    assert not r.armed and r.read() is None
    assert src.tolist() == [99] * 5


def test_poll_after_the_device_is_idle_returns_the_words_and_drop_disarms():
    src = _words([4, 5, 6, 7, 8])
    r = DeferredRead(5)
    r.watch(src)
    torch.cuda.synchronize()
    assert r.ready()
    assert r.poll() == [4, 5, 6, 7, 8]
    assert not r.armed and r.poll() is None
    r.watch(src)
    assert r.armed
    r.drop()
    assert not r.armed and r.ready() and r.read() is None and r.poll() is None


def test_a_second_watch_supersedes_the_first():
    src = _words([1, 2, 3, 4, 5])
    r = DeferredRead(5)
    r.watch(src)
    src.add_(10)
    r.watch(src)
    src.add_(10)
    assert r.read() == [11, 12, 13, 14, 15]
    assert r.read() is None
    # fewer words than the buffer holds: a view of one word lands in front
    one = DeferredRead(1)
    one.watch(src[2:3])
    assert one.read() == [23]
