"""Page-locked staging memory and the side stream that fills it: where images leave the device without stopping the host
(the snapshots and part images of trainer.train_steps, the trajectory images of fit_video.fit_clip)."""
import threading
import weakref

import torch


class PinnedPool:
    """Page-locked staging blocks for the snapshots, re-used across train() calls.  Pinning costs ~0.15 ms per MB
    (hipHostMalloc of the 110-180 MB a stage's snapshots need: 16-43 ms, five times per later frame in a HIP API
    trace of a clip fit), so a block goes back to the pool as soon as the arrays handed out of it are gone."""

    MAX_BYTES = 4 << 30         # beyond this much page-locked memory the snapshots are handed out as pageable copies

    def __init__(self):
        self.blocks = []                                # [uint8 pinned tensor, arrays still alive, event of the last copy INTO it]
        # re-entrant: the finalizers below take it too, and a garbage collection that runs them can start inside take()
        # (which allocates while it holds the lock) on the same thread
        self.lock = threading.RLock()                   # several fits may run in one process (fit_clips_concurrent)

    def total_bytes(self):
        return sum(b[0].numel() for b in self.blocks)

    def take(self, nbytes):
        """a free block of at least ``nbytes``; it counts as taken (one reference) until ``release``"""
        with self.lock:
            for b in self.blocks:
                if b[1] == 0 and b[0].numel() >= nbytes:
                    b[1] = 1
                    break
            else:
                step = 32 << 20
                b = [torch.empty((nbytes + step - 1) // step * step, dtype=torch.uint8, pin_memory=True), 1, None]
                self.blocks.append(b)
                return b
        # a caller that did not wait for its images (lazy_images) may have dropped them while the device-to-host copy
        # into this block was still queued: the next user must not be given the block before that copy has landed
        if b[2] is not None:
            b[2].synchronize()
            b[2] = None
        return b

    def copied(self, block, stream):
        """a device-to-host copy into ``block`` has just been queued on ``stream``"""
        ev = torch.cuda.Event()
        ev.record(stream)
        block[2] = ev

    def release(self, block):
        """drop the reference ``take`` left (after ``hold`` / ``hand_out`` have added theirs)"""
        with self.lock:
            block[1] -= 1

    def _gone(self, block):
        with self.lock:
            block[1] -= 1

    def hold(self, block, owner):
        """the block stays taken while ``owner`` is alive"""
        with self.lock:
            block[1] += 1
        return weakref.finalize(owner, self._gone, block)   # call it to let go early

    def hand_out(self, block, tensors):
        """numpy views of ``tensors`` (views of the block); the block is free again when all of them are collected."""
        if self.total_bytes() > self.MAX_BYTES:
            # a caller that keeps every frame's snapshot lists (the reference's fit_video does, to write its videos)
            # would otherwise hold one 110-180 MB page-locked block per train() call: tens of GB over a 60-frame clip.
            # Pageable copies then -- taken only once the device has filled the block (lazy_images callers included)
            if block[2] is not None:
                block[2].synchronize()
            return [t.numpy().copy() for t in tensors]
        out = []
        for t in tensors:
            a = t.numpy()
            with self.lock:
                block[1] += 1
            weakref.finalize(a, self._gone, block)
            out.append(a)
        return out


class DeferredRead:
    """A few device int32 words, looked at later without stopping the host: ``watch`` copies them to page-locked memory behind
    the work queued so far and records an event behind the copy.  The one place where this idiom exists (the overflow words of
    FitEngine and of the batched rasteriser)."""

    def __init__(self, words):
        self.words = int(words)
        self._host = self._event = None     # the pinned buffer (allocated by the first watch); the event of an armed watch

    def watch(self, src):
        """``src``: a device view of at most ``words`` int32, copied on the current stream; supersedes a watch nobody has read"""
        if self._host is None:
            self._host = torch.zeros(self.words, dtype=torch.int32, pin_memory=True)
        self._host[:src.numel()].copy_(src, non_blocking=True)
        self._event = torch.cuda.Event()
        self._event.record()

    armed = property(lambda self: self._event is not None)

    def ready(self):
        """False while a watched copy has not landed yet (``read`` would wait)."""
        return self._event is None or self._event.query()

    def read(self):
        """The watched words as a list of ints (None without a watch); waits for exactly that copy -- never for work queued
        after it -- and disarms."""
        if self._event is None:
            return None
        self._event.synchronize()
        self._event = None
        return self._host.tolist()

    def poll(self):
        """``read`` if that would not wait, else None."""
        return self.read() if self.ready() else None

    def drop(self):
        """forget a watch nobody has read"""
        self._event = None


PINNED = PinnedPool()
_COPY_STREAMS = {}


def copy_stream(dev):
    """one side stream per device and FIT stream for the snapshot copies (creating a stream per train() call cost
    1.4 ms each; several fits on one device -- fit_clips_concurrent -- must not queue behind each other's copies)"""
    key = (dev.type, dev.index, torch.cuda.current_stream(dev).cuda_stream)
    if key not in _COPY_STREAMS:
        _COPY_STREAMS[key] = torch.cuda.Stream(device=dev)
    return _COPY_STREAMS[key]
