"""The parts the three training loops share, without a GPU: the ring copy and
the FIFO of copies in flight (sac/copy_behind.py) and the episode statistics
(sac.agent.EpisodeStats)."""
import builtins
import collections
import random

import numpy as np
import pytest
import torch


def test_ring_copy_takes_consecutive_cells_and_wraps():
    from sac.copy_behind import copy_ring_cells

    S = 5
    ring = torch.arange(S, dtype=torch.float32).reshape(S, 1, 1).expand(S, 3, 2).contiguous()  # cell i holds i
    for first, n, want in ((1, 3, [1, 2, 3]), (3, 4, [3, 4, 0, 1]), (0, 5, [0, 1, 2, 3, 4]), (4, 1, [4]),
                           (9, 2, [4, 0])):
        host, event = copy_ring_cells(ring, first, n)
        assert event is None
        assert host.shape == (n, 3, 2) and host.dtype == ring.dtype and not host.is_pinned()
        assert host[:, 0, 0].tolist() == want, (first, n)
        assert torch.equal(host, ring[want])
        host.fill_(-1.0)  # a fresh tensor: the ring keeps its cells
        assert ring[:, 0, 0].tolist() == list(range(S))
    for n in (0, 6, -1):
        with pytest.raises(ValueError):
            copy_ring_cells(ring, 0, n)


class FakeEvent:
    def __init__(self, name, landed, calls):
        self.name, self.landed, self.calls = name, landed, calls

    def query(self):
        self.calls.append(("query", self.name))
        return self.landed

    def synchronize(self):
        self.calls.append(("synchronize", self.name))
        self.landed = True


def test_pending_copies_hand_over_in_order_and_stop_at_the_first_unlanded():
    from sac.copy_behind import PendingCopies

    calls, got = [], []
    fn = lambda host, tag: got.append((host, tag))  # noqa: E731
    hosts = [torch.full((1,), float(i)) for i in range(3)]
    q = PendingCopies()
    for i, landed in enumerate((True, False, True)):
        q.push(hosts[i], FakeEvent(i, landed, calls), f"tag{i}")
    q.consume(False, fn)
    assert [(h is hosts[0], t) for h, t in got] == [(True, "tag0")]  # the third stays behind the second
    assert ("query", 2) not in calls and ("synchronize", 1) not in calls and ("synchronize", 2) not in calls
    q.consume(False, fn)  # nothing landed since: nothing handed over, nothing waited for
    assert len(got) == 1 and not [c for c in calls if c[0] == "synchronize" and c[1] != 0]
    del calls[:]
    q.consume(True, fn)
    assert [c for c in calls if c[0] == "synchronize"] == [("synchronize", 1), ("synchronize", 2)]
    assert [t for _, t in got] == ["tag0", "tag1", "tag2"] and all(h is w for (h, _), w in zip(got, hosts))
    q.consume(True, fn)
    assert len(got) == 3 and not q  # each exactly once

    q.push(hosts[0], None, "a")  # no event: the copy was complete when it was queued
    q.push(hosts[1], None, "b")
    del got[:]
    q.consume(False, fn)
    assert [t for _, t in got] == ["a", "b"] and not q


def test_episode_stats_window_best_index_and_order(monkeypatch):
    from sac.agent import EpisodeStats

    rng = random.Random(1234)
    returns = [rng.uniform(-50.0, 50.0) - abs(i - 120) for i in range(250)]  # the best window is not the last
    lengths = [rng.randrange(1, 400) for _ in returns]
    seen = []  # ("log", index, return, length) and ("print", text) in the order they happened

    class Logger:
        def log_episode_metrics(self, episode_idx, reward, length):
            seen.append(("log", episode_idx, reward, length))

    monkeypatch.setattr(builtins, "print", lambda *a, **k: seen.append(("print", " ".join(map(str, a)))))
    stats = EpisodeStats(Logger(), print_rewards=True)
    assert stats.count == 0 and stats.avg != stats.avg and stats.best == -float("inf")
    window, best, avg = collections.deque(maxlen=100), -float("inf"), float("nan")
    for i, (ret, length) in enumerate(zip(returns, lengths)):
        stats.episode(ret, length)
        window.append(ret)
        avg = float(np.mean(window))
        best = max(best, avg)
        assert (stats.avg, stats.best, stats.count) == (avg, best, i + 1)
    monkeypatch.undo()
    assert stats.avg == float(np.mean(returns[-100:])) and stats.best == best > stats.avg
    assert stats.counters(7, 3) == {"env_steps": 7, "gradient_steps": 3, "episodes": 250, "avg_return": avg}
    assert len(seen) == 500
    for i in range(250):  # the logger first, then the line, both under the index before it is counted
        assert seen[2 * i] == ("log", i, returns[i], lengths[i])
        kind, text = seen[2 * i + 1]
        assert kind == "print" and text.startswith(f"Episode {i}, Return: {returns[i]:.2f}, ")

    quiet = EpisodeStats()  # no logger, no line
    quiet.episode(1.0, 1)
    assert (quiet.count, quiet.avg, quiet.best) == (1, 1.0, 1.0)
