"""The update tile of phases B and D (csrc/sac_phases.h, dw_adam_tile) as named
stages: geometry and loads, dW on the single-round or the multi-round path, the
batch-part hand-off, Adam + Polyak, the packed copies.  The split moves no
float operation, load, store or barrier, so every case is bit-identical to the
parent commit's build: tests/golden/update_tile_parent_digests.json holds the
SHA-256 of every array of state_tensors() and of the stats buffer after two
injected steps, made from that build by
tests/golden/make_update_tile_parent_digests.py; the digests are recomputed
here.  Every case asserts the kernel layout of phases A and C;
tests/test_update_tile_stages_cpu.py holds the update kernels' block size and
slots of every case to the case table.

The cases are the smallest shapes that reach every instance and path of the
tile (obs 24, act 4, hidden [256, 256], capacity 1024 unless stated; most are
the shapes tests/test_gpu_update_single_round.py argues for):

  b16   fp32, bf16  split layout, single round, one partial slot, summed dY
                    parts (gsum 2, and 4 for pi in fp32), no batch parts
  b40   fp32        the smallest batch with layer-0 batch-part halves: producer
                    and consumer through the hand-off, bias sums handed over
  b144  fp32        slot 0 full, slot 1 partial (the masked trip counts)
  b256  fp32, bf16  every slot full (the compile-time trip counts): two fp32
                    slots, the one bf16 slot the planner gives this batch
  b272  fp32        full-batch tiles on the multi-round path with the seeds
                    handed over through LDS; the halves still single-round
  b528  bf16        past two bf16 slots: multi-round, per-piece seeds
  small48  fp32     obs 5, act 3, q [72, 40], pi [40, 72], batch 48: masked N
                    and K tile edges, no summed parts, roles layout
  ut512_b48  fp32, bf16  small48 with upd_threads = 512: phase B's 512-thread,
                    one-slot, two-pairs-per-wave instance (always multi-round)
  parts_b1040  fp32, bf16  obs 4, act 1, [64, 64], batch 1040, capacity 2048
                    (Bp > 1024): four batch parts per tile off the split, at
                    the default block size and with upd_threads = 512,
                    upd_parts = 4 (the 512-thread consumer that takes three
                    producer parts)
"""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_update_tile_parent_digests as G  # noqa: E402

pytestmark = pytest.mark.gpu

with open(G.OUT) as _f:
    GOLDEN = json.load(_f)


def test_the_committed_digests_cover_the_cases():
    assert sorted(GOLDEN["cases"]) == sorted(G.CASES) and GOLDEN["steps"] == G.STEPS
    with open(G.OUT) as f:
        assert f.read() == G.render(GOLDEN)


@pytest.mark.parametrize("case", list(G.CASES))
def test_state_is_bit_identical_to_the_parent_build(case):
    """Two injected steps: every state array and the stats buffer hash to the
    parent build's digests."""
    got = G.digests(case)
    want = GOLDEN["cases"][case]
    assert sorted(got) == sorted(want)
    differ = [k for k in want if got[k] != want[k]]
    assert not differ, (case, differ)
