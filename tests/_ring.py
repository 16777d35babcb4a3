"""Host model of the replay ring and the ring states the gradient step's
in-step gathers are tested on (tests/test_gpu_ring.py, tests/test_ring_cpu.py).

RingModel is the reference's deque (replay_buffer.py:11-30): a list of pushed
rows, truncated to the last `capacity`; logical index 0 is the oldest row.  It
also keeps what every physical slot of a ring written in push order holds, so
a test can say what a gather with a wrong slot rule would have read.

Ring drives a model and, when given one, a real sac.replay_buffer.ReplayBuffer
through the same pushes; fill() brings it into one of STATES:
  partial  n < capacity rows pushed: size = pos = n;
  wrapped  capacity + w rows pushed (two push_batch calls and three single
           push calls, w no multiple of 16): size = capacity, pos = w;
  cleared  filled, `between` called (the GPU tests train two steps there, so a
           staged batch is pending), clear(), refilled to a partial state;
twin() is a second ring of capacity = size holding the same logical rows
pushed in order: full with write slot 0, the state every other oracle test of
the step runs in.  No GPU is needed without a buffer."""
import numpy as np

STATES = ("partial", "wrapped", "cleared")
F32 = np.float32
ROWS = 16  # rows per row tile of the phase kernels (SAC_ROWS) and per gather workgroup of the stage path (WGR)

# Ring geometry per case of cases(): capacity (no power of two), rows of the
# partial state (more than half the capacity, so the logical neighbours
# capacity - pos - 1 and capacity - pos exist and a gather that applied pos to
# a partly filled ring would wrap), w of the wrapped state, rows of the refill
# after clear() (fewer than half)
GEOMETRY = {"split": (131, 77, 21), "obs40": (299, 170, 45)}
DEFAULT_GEOMETRY = (203, 120, 37)
BATCH = 40


def geometry(case):
    cap, n, w = GEOMETRY.get(case, DEFAULT_GEOMETRY)
    return dict(capacity=cap, partial=n, w=w, refill=BATCH + 17)


def cases():
    """case -> (shape, layout overrides, the layout it must run): LAYOUTS of
    tests/test_gpu_activations.py and obs 40 on [256, 256] nets, past the
    O <= 32 branch of the hidden-split kernels' staged-record read."""
    from test_gpu_activations import LAYOUTS

    out = {k: (shape, lay, k) for k, (shape, lay) in LAYOUTS.items()}
    out["obs40"] = (dict(obs=40, act=4, hidden=[256, 256], batch=BATCH, capacity=512), None, "split")
    return out


COLUMNS = ("obs", "act", "rew", "next_obs", "done")


class RingModel:
    def __init__(self, capacity, obs, act):
        self.capacity, self.obs, self.act = int(capacity), obs, act
        self.rows = []  # the deque: (obs, act, rew, next_obs, done) per row, oldest first
        self.pushed = 0  # since the last clear()
        self.phys = dict(obs=np.zeros((capacity, obs), F32), act=np.zeros((capacity, act), F32),
                         rew=np.zeros(capacity, F32), next_obs=np.zeros((capacity, obs), F32),
                         done=np.zeros(capacity, F32))

    def push(self, rows):
        n = rows["rew"].shape[0]
        for i in range(n):
            self.rows.append(tuple(np.asarray(rows[k][i], F32) for k in COLUMNS))
            for k in COLUMNS:
                self.phys[k][(self.pushed + i) % self.capacity] = rows[k][i]
        self.rows = self.rows[-self.capacity:]
        self.pushed += n

    def clear(self):
        """ReplayBuffer.clear(): size and write slot back to 0; the storage keeps its old rows."""
        self.rows = []
        self.pushed = 0

    @property
    def size(self):
        return len(self.rows)

    @property
    def pos(self):
        return self.pushed % self.capacity

    def slot(self, li):
        """Physical slot of logical index li (array or int)."""
        li = np.asarray(li, np.int64)
        assert np.all((0 <= li) & (li < self.size))
        return li if self.size < self.capacity else (self.pos + li) % self.capacity

    def logical(self):
        """The logical rows in order, one array per column."""
        return {k: np.stack([r[j] for r in self.rows]) for j, k in enumerate(COLUMNS)}


def id_rows(obs, act, seed):
    """rows(n, first): random obs, act and next_obs, every row terminal, rew =
    1 + the row's push counter (exact in fp32, never 0): y == r bit for bit, so
    a step's targets name the rows it gathered."""
    def rows(n, first):
        g = np.random.default_rng([seed, first])
        return dict(obs=g.standard_normal((n, obs), dtype=F32), act=g.uniform(-1, 1, (n, act)).astype(F32),
                    rew=(1 + first + np.arange(n)).astype(F32), next_obs=g.standard_normal((n, obs), dtype=F32),
                    done=np.ones(n, F32))
    return rows


def mixed_rows(obs, act, seed, done_p=0.3):
    """rows(n, first): ordinary rows (N(0, 1) rewards and observations), a share done_p of them terminal."""
    def rows(n, first):
        g = np.random.default_rng([seed, first])
        return dict(obs=g.standard_normal((n, obs), dtype=F32), act=g.uniform(-1, 1, (n, act)).astype(F32),
                    rew=g.standard_normal(n, dtype=F32), next_obs=g.standard_normal((n, obs), dtype=F32),
                    done=(g.random(n) < done_p).astype(F32))
    return rows


class Ring:
    """A RingModel and, with `buffer`, a real ReplayBuffer fed the same pushes.
    rows_fn(n, first) makes the next n rows; `first` counts every row ever
    pushed (clear() does not reset it)."""

    def __init__(self, capacity, obs, act, rows_fn, buffer=None):
        self.model = RingModel(capacity, obs, act)
        self.rows_fn, self.rb, self.count = rows_fn, buffer, 0
        self.calls = dict(push_batch=0, push=0)
        assert buffer is None or (buffer.capacity == capacity and len(buffer) == 0)

    def _next(self, n):
        rows = self.rows_fn(n, self.count)
        self.count += n
        return rows

    def push_batch(self, n, rows=None):
        rows = self._next(n) if rows is None else rows
        self.model.push(rows)
        self.calls["push_batch"] += 1
        if self.rb is not None:
            self.rb.push_batch(*(rows[k] for k in COLUMNS))

    def push_rows(self, n):
        """n single push() calls (staged on the host until the next read)."""
        rows = self._next(n)
        self.model.push(rows)
        self.calls["push"] += n
        if self.rb is not None:
            for i in range(n):
                self.rb.push(rows["obs"][i], rows["act"][i], float(rows["rew"][i]), rows["next_obs"][i],
                             bool(rows["done"][i]))

    def clear(self):
        self.model.clear()
        if self.rb is not None:
            self.rb.clear()

    def check_buffer(self):
        """The real buffer's host and device (size, pos) are the model's."""
        self.rb.flush()
        assert (len(self.rb), self.rb._pos) == (self.model.size, self.model.pos)
        assert self.rb.state[:2].cpu().tolist() == [self.model.size, self.model.pos]


def fill(ring, state, geo, between=None):
    """Bring an empty ring into `state` (geo: geometry(case))."""
    cap = ring.model.capacity
    assert cap == geo["capacity"] and ring.model.size == 0
    if state == "partial":
        ring.push_batch(geo["partial"] - 3)
        ring.push_rows(3)
        want = (geo["partial"], geo["partial"])
    elif state == "wrapped":
        assert geo["w"] % 16 and 3 < geo["w"] < cap
        first = cap // 2 + 5
        ring.push_batch(first)
        ring.push_batch(cap + geo["w"] - 3 - first)
        ring.push_rows(3)
        want = (cap, geo["w"])
    elif state == "cleared":
        ring.push_batch(cap)
        if between:
            between(ring)
        ring.clear()
        ring.push_batch(geo["refill"] - 3)
        ring.push_rows(3)
        want = (geo["refill"], geo["refill"])
    else:
        raise ValueError(state)
    assert (ring.model.size, ring.model.pos) == want, (state, ring.model.size, ring.model.pos, want)
    return ring


def twin(ring, make_buffer=None):
    """A ring of capacity = size with the same logical rows pushed in order:
    full, write slot 0 (logical index = physical slot)."""
    m = ring.model
    t = Ring(m.size, m.obs, m.act, None, make_buffer(m.size) if make_buffer else None)
    t.push_batch(m.size, m.logical())
    assert (t.model.size, t.model.pos) == (m.size, 0)
    return t


def edge_indices(model, batch, g):
    """[batch] int32 logical indices, drawn with replacement, with the ring's
    edges -- 0, size - 1 and the neighbours capacity - pos - 1 and capacity -
    pos that straddle the physical wrap, where they are rows of the ring -- in
    the first row tile, in the last (ragged) row tile, and one at row batch - 1."""
    size = model.size
    edges = [e for e in (0, size - 1, model.capacity - model.pos - 1, model.capacity - model.pos) if 0 <= e < size]
    idx = g.integers(0, size, batch)
    last = (batch - 1) // ROWS * ROWS
    assert last >= ROWS and batch - last > len(edges), (batch, last)
    idx[1:1 + len(edges)] = edges
    idx[last:last + len(edges)] = edges[::-1]
    idx[batch - 1] = edges[-1]
    return idx.astype(np.int32)


def wrong_slots(model, li):
    """The slots a gather would read under the slot rule that is wrong for
    this state: the logical index alone on a full ring whose write slot moved,
    (pos + li) % capacity on a partly filled one."""
    li = np.asarray(li, np.int64)
    return li if model.size == model.capacity else (model.pos + li) % model.capacity


def sampled_indices(size, batch, seed, step):
    """The device sampler's logical rows for (seed, step) on a ring of `size`
    rows (oracle/sampler_oracle.py, equal to sac_debug_sample_indices_host:
    tests/test_gpu_engine.py::test_device_sampler_equals_host)."""
    from oracle import sampler_oracle as S

    return np.asarray(S.sample_indices(size, batch, seed, step), np.int64)


ANCHOR_SEED = 5


def anchor_inputs(case, make_buffer=None):
    """The oracle anchor's inputs for a case of cases(): its config dict (with
    the ring's capacity), the wrapped ring holding mixed rows (with a real
    buffer from make_buffer(capacity), if given), injected indices and the two
    eps draws."""
    shape, lay, expect = cases()[case]
    geo = geometry(case)
    c = dict(shape, capacity=geo["capacity"], name=f"ring_{case}")
    ring = Ring(geo["capacity"], c["obs"], c["act"], mixed_rows(c["obs"], c["act"], ANCHOR_SEED),
                make_buffer(geo["capacity"]) if make_buffer else None)
    fill(ring, "wrapped", geo)
    g = np.random.default_rng(ANCHOR_SEED + 1)
    idx = edge_indices(ring.model, c["batch"], g)
    et = g.standard_normal((c["batch"], c["act"])).astype(F32)
    ea = g.standard_normal((c["batch"], c["act"])).astype(F32)
    return c, ring, idx, et, ea


def batch_of(rows, idx):
    from oracle import sac_oracle as O

    return O.Batch(*(rows[k][idx] for k in COLUMNS))
