"""Copies of device rings to the host that queue behind the launches and are
read once they have landed, so that no loop step waits for the device.

``copy_ring_cells`` queues the copy of a range of ring cells and returns the
host tensor with the event that marks its arrival; ``PendingCopies`` keeps such
copies in order and hands over those that have arrived.  The episode ring
(``sac.device_envs.DeviceVectorEnv.episode_cells``, ``EpisodeDrain``) and both
Q-value logs (``sac.agent.QValueLog``, ``sac.device_envs.DeviceQValueLog``) are
written on these two.  Imports without a GPU; on CPU tensors a copy is
complete when the call returns.
"""
from __future__ import annotations

from collections import deque
from contextlib import nullcontext
from typing import Any, Callable, Optional, Tuple

import torch


def copy_ring_cells(ring: torch.Tensor, first: int, n: int) -> Tuple[torch.Tensor, Optional[torch.cuda.Event]]:
    """Copy ``n`` consecutive cells of the ring ``[S, ...]``, starting at cell
    ``first % S`` and wrapping past cell S - 1, into a fresh host tensor
    ``[n, ...]``: one copy, or two when the range wraps.  Returns (host, event).
    A device ring is copied without blocking into pinned memory on the current
    stream of its device, and the event is recorded there behind the copies:
    the host tensor is valid once the event has completed, and later launches
    that write the cells queue behind the copy.  A CPU ring is copied at once;
    the event is None.  ValueError unless 1 <= n <= S."""
    S = ring.shape[0]
    if n < 1 or n > S:
        raise ValueError(f"copy_ring_cells: {n} cells do not fit the ring of {S}")
    cuda = ring.is_cuda
    host = torch.empty((n,) + tuple(ring.shape[1:]), dtype=ring.dtype, pin_memory=cuda)
    a = first % S
    k = min(n, S - a)  # cells before the ring's end
    ev = None
    with torch.cuda.device(ring.device) if cuda else nullcontext():
        if k == n:
            host.copy_(ring[a:a + n], non_blocking=cuda)
        else:  # the range wraps the ring
            host[:k].copy_(ring[a:], non_blocking=cuda)
            host[k:].copy_(ring[:n - k], non_blocking=cuda)
        if cuda:
            ev = torch.cuda.Event()
            ev.record()
    return host, ev


class PendingCopies(deque):
    """FIFO of copies in flight: (host tensor, event, tag) in the order they
    were queued.  An event of None counts as completed.  Empty is falsy, so a
    loop step can skip ``consume`` without a call."""

    def push(self, host: torch.Tensor, event: Any, tag: Any) -> None:
        self.append((host, event, tag))

    def consume(self, block: bool, fn: Callable[[torch.Tensor, Any], None]) -> None:
        """Hand entries to ``fn(host, tag)`` strictly in the order pushed, each
        once.  Without ``block`` it stops at the first entry whose event has not
        completed and leaves every later one, landed or not; with ``block`` it
        waits for each entry in turn (the only place that synchronises)."""
        while self:
            host, ev, tag = self[0]
            if ev is not None:
                if not block and not ev.query():
                    return
                ev.synchronize()
            fn(host, tag)
            self.popleft()


__all__ = ["PendingCopies", "copy_ring_cells"]
