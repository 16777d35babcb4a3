"""Generate tests/golden/update_tile_parent_digests.json: SHA-256 digests of the
engine state after two injected steps on every instance and path of the update
tile (phases B and D), taken from a build of the commit BEFORE the tile was
split into named stages (csrc/sac_phases.h, dw_adam_tile).

    SAC_ENGINE_LIB=/path/to/parent/libsac_engine.so \
        python tests/golden/make_update_tile_parent_digests.py --parent <commit>

How the file is made and what a digest covers: tests/golden/_parent_digests.py.
The change moves no float operation, load, store or barrier, so
tests/test_gpu_update_tile_stages.py recomputes every digest on the build
under test and asks for equality; tests/test_update_tile_stages_cpu.py holds
every case to the plan fields of its row here.
"""
from __future__ import annotations

import os

import _parent_digests as P
from _parent_digests import STEPS, render  # noqa: F401  (the tests read them from here)

OUT = os.path.join(P.HERE, "update_tile_parent_digests.json")


def _split(batch):
    return dict(obs=24, act=4, hidden=[256, 256], batch=batch, capacity=1024)


SMALL48 = dict(obs=5, act=3, q_hidden=[72, 40], pi_hidden=[40, 72], batch=48, capacity=1024)
UT512_B48 = dict(SMALL48, layout=dict(upd_threads=512))
PARTS = dict(obs=4, act=1, hidden=[64, 64], batch=1040, capacity=2048)
PARTS_UT512 = dict(PARTS, layout=dict(upd_threads=512, upd_parts=4))

# name -> (config dict, precision, the plan's path, upd_threads_b, upd_slots).  A slot is one 512-B chunk per
# operand row: 128 batch columns in fp32, 256 in bf16; Bp is the batch padded to whole 32-column K-steps.
CASES = {
    # one partial slot; summed dY parts (gsum 2, and 4 for pi in fp32), no batch parts
    "b16_fp32": (_split(16), "fp32", "split", 1024, 1),
    "b16_bf16": (_split(16), "bf16", "split", 1024, 1),
    # the smallest batch with layer-0 batch-part halves: producer and consumer, bias sums handed over
    "b40_fp32": (_split(40), "fp32", "split", 1024, 1),
    "b144_fp32": (_split(144), "fp32", "split", 1024, 2),   # slot 0 full, slot 1 partial: the masked trip counts
    "b256_fp32": (_split(256), "fp32", "split", 1024, 2),   # both slots full: the compile-time trip counts
    "b256_bf16": (_split(256), "bf16", "split", 1024, 1),   # bf16: its one slot full
    # full-batch tiles multi-round with the seeds handed over through LDS; the halves still single-round
    "b272_fp32": (_split(272), "fp32", "split", 1024, 2),
    "b528_bf16": (_split(528), "bf16", "roles", 1024, 2),   # bf16 past two slots: multi-round, per-piece seeds
    "small48_fp32": (SMALL48, "fp32", "roles", 1024, 1),    # masked N and K tile edges, GS 1
    # phase B's 512-thread, one-slot, two-pairs-per-wave instance: always multi-round
    "ut512_b48_fp32": (UT512_B48, "fp32", "roles", 512, 1),
    "ut512_b48_bf16": (UT512_B48, "bf16", "roles", 512, 1),
    # Bp > 1024: four batch parts per tile off the split (a consumer and three producers) ...
    "parts_b1040_fp32": (PARTS, "fp32", "pairs", 1024, 2),
    "parts_b1040_bf16": (PARTS, "bf16", "pairs", 1024, 2),
    # ... and phase B's 512-thread consumer taking three producer parts
    "parts_b1040_ut512_fp32": (PARTS_UT512, "fp32", "pairs", 512, 2),
    "parts_b1040_ut512_bf16": (PARTS_UT512, "bf16", "pairs", 512, 2),
}


def digests(name):
    """{array name: sha256 hex} of case `name` on the loaded engine library."""
    c, precision, path, _, _ = CASES[name]
    return P.state_digests(dict(c, name="update_tile_" + name), precision, path)


if __name__ == "__main__":
    P.main(OUT, CASES, digests)
