"""The schedule of K1's loader waves (csrc/k1_loader.h), walked on the host: no GPU.  tests/emul/k1_loader_emul.cpp hands
out the values the kernel compiles (k1_body.inc, LDW > 0); this file plays the two roles of one workgroup against
each other, barrier by barrier, and asks of every iteration what the hardware needs for the bytes to be right.

The model.  The workgroup's barriers are numbered in program order; epoch e is the code between barrier e - 1 and
barrier e, and every wave is in the same epoch at any moment (all of them arrive at every barrier).  A loader's LDS-DMA
pieces complete in issue order, so a counted wait `n` retires all but its newest n pieces, and nothing else says a
piece has landed: a piece that no wait retired is treated as still in flight (the late extreme), and a piece is treated
as overwriting its slot the moment it is issued (the early extreme).  Bytes retired by a wait in epoch e may be read
from epoch e + 1 on (the barrier publishes them); a slot read in epoch e may be refilled from epoch e + 1 on (a compute
wave arrives at the barrier only after its reads have returned).

The compute side is the kernel's frame loop as written: one barrier after the twiddle table is filled, then per
iteration the unpack, the top-of-frame barrier, pass 1, the pass-1 exchange barrier; then the flush, one barrier
before the accumulators are staged and one after (per plane with statistics)."""
import ctypes
import os

import pytest

from helpers import ROOT

GRID, FPW = 256, 2                 # N = 4096: one 512-thread workgroup per CU, two frames side by side
COMPUTE_WAVES, PIECES = 8, 2       # eight compute waves, two 1-KiB pieces per wave and frame (cu8, P = 16)
_emul = None


def emul():
    global _emul
    if _emul is None:
        _emul = ctypes.CDLL(os.path.join(ROOT, "tests", "emul", "librpf_emul_k1_loader.so"))
    return _emul


def k(name, *args):
    return getattr(emul(), "rpf_emul_k1_loader_" + name)(*args)


def iterations_of_workgroup(frames, wg):
    """How often workgroup `wg` goes round the kernel's frame loop: fb = wg FPW, += grid FPW while fb < frames."""
    stride = GRID * FPW
    fb, n = wg * FPW, 0
    while fb < frames:
        fb += stride
        n += 1
    return n


class Loader:
    """One loader wave: the queue of its pieces in flight, (iteration, slot, epoch issued), in issue order."""

    def __init__(self):
        self.flight = []
        self.landed = {}            # slot -> (iteration, epoch of the wait that retired it)
        self.issued = []            # (iteration, slot, epoch)
        self.waits = []

    def issue(self, iteration, slot, ppi, epoch):
        self.flight += [(iteration, slot)] * ppi
        self.landed.pop(slot, None)                 # early extreme: the slot's old bytes are gone at once
        self.issued.append((iteration, slot, epoch))

    def wait(self, n, epoch):
        self.waits.append(n)
        while len(self.flight) > n:
            iteration, slot = self.flight.pop(0)
            if (iteration, slot) not in self.flight:            # the last piece of that iteration's frames
                self.landed[slot] = (iteration, epoch)


def walk(iters, rawd, ldw, stats=False):
    """Plays one workgroup that runs `iters` iterations; returns what the assertions below look at."""
    ppi = k("pieces_per_iteration", COMPUTE_WAVES, ldw, PIECES)
    pro, per_it = k("prologue_barriers"), k("barriers_per_iteration")
    refill_b, landed_b = k("refill_barrier"), k("landed_barrier")
    ld = Loader()
    reads = []                       # (iteration, slot, epoch, what the slot held: (iteration, retired in epoch) or None)
    loader_barriers = compute_barriers = 0

    # epoch 0: the prologue
    if iters > 0:
        for d in range(rawd):
            ld.issue(d, k("slot_of", d, rawd), ppi, 0)
        ld.wait(k("prologue_wait", rawd, ppi), 0)
    loader_barriers += pro
    compute_barriers += 1            # after fill_twlds
    for it in range(iters):
        first = pro + per_it * it    # the barrier index of this iteration's barrier 0
        # compute: the unpack, in the epoch that ends at the top-of-frame barrier
        slot = k("slot_of", it, rawd)
        reads.append((it, slot, first, ld.landed.get(slot)))
        compute_barriers += 2        # top of frame, pass-1 exchange
        # loader: arrives at the iteration's barriers; the refill and the wait lie between two of them
        assert 0 <= refill_b < landed_b < per_it
        epoch = first + refill_b + 1
        ld.issue(k("refill_iteration", it, rawd), slot, ppi, epoch)
        ld.wait(k("loop_wait", rawd, ppi), epoch)
        assert epoch <= first + landed_b          # the wait is over before the loader arrives at the landed barrier
        loader_barriers += per_it
    flush_epoch = pro + per_it * iters
    ld.wait(k("flush_wait"), flush_epoch)
    outstanding_at_flush = len(ld.flight)
    loader_barriers += k("flush_barriers", int(stats))
    compute_barriers += 6 if stats else 2
    return {"reads": reads, "issued": ld.issued, "waits": ld.waits, "loader_barriers": loader_barriers,
            "compute_barriers": compute_barriers, "outstanding_at_flush": outstanding_at_flush, "ppi": ppi}


# frame counts that give workgroup 0 exactly 1, 2, 3, 4 and 20 iterations (the last workgroups then run one fewer
# where the count is ragged: both are walked)
FRAMES = {1: 3, 2: GRID * FPW + 7, 3: 2 * GRID * FPW + 1, 4: 4 * GRID * FPW - 1, 20: 20 * GRID * FPW - 5}


@pytest.mark.parametrize("ldw", [1, 2])
@pytest.mark.parametrize("rawd", [2, 3])
@pytest.mark.parametrize("iters", sorted(FRAMES))
def test_schedule(iters, rawd, ldw):
    frames = FRAMES[iters]
    assert iterations_of_workgroup(frames, 0) == iters
    for wg in (0, GRID - 1):
        n = iterations_of_workgroup(frames, wg)
        w = walk(n, rawd, ldw)
        # every slot read at iteration `it` holds iteration `it`'s frames, retired by a wait in an EARLIER epoch
        for it, slot, epoch, held in w["reads"]:
            assert held is not None, (it, slot, "read while its pieces may be in flight")
            assert held[0] == it, (it, slot, held)
            assert held[1] < epoch, (it, slot, held, epoch)
        # no refill is issued before the barrier that follows the slot's last read
        last_read = {}
        events = [(e, 0, "read", s, i) for i, s, e, _ in w["reads"]] + [(e, 1, "issue", s, i) for i, s, e in w["issued"]]
        for epoch, _, what, slot, iteration in sorted(events):
            if what == "read":
                last_read[slot] = epoch
            elif iteration >= rawd:                        # a refill (the prologue fills empty slots)
                assert slot in last_read and epoch > last_read[slot], (iteration, slot, epoch, last_read.get(slot))
        # counted waits fit the 6-bit field
        assert all(0 <= c < 64 for c in w["waits"]), w["waits"]
        assert max(w["waits"]) <= k("max_counted_wait")
        # the two roles arrive at the same number of barriers, flush included
        assert w["loader_barriers"] == w["compute_barriers"] == 1 + 2 * n + 2
        # nothing is in flight when the flush starts to reuse the LDS
        assert w["outstanding_at_flush"] == 0


def test_barrier_count_with_statistics():
    w = walk(3, 2, 1, stats=True)
    assert w["loader_barriers"] == w["compute_barriers"] == 1 + 2 * 3 + 6


def test_the_shipped_counts():
    # N = 4096, cu8, ring of two: one loader issues sixteen pieces per iteration and waits for all but the newest sixteen
    assert k("pieces_per_iteration", COMPUTE_WAVES, 1, PIECES) == 16
    assert k("prologue_wait", 2, 16) == 16 and k("loop_wait", 2, 16) == 16 and k("flush_wait") == 0
    assert k("pieces_per_iteration", COMPUTE_WAVES, 2, PIECES) == 8 and k("loop_wait", 2, 8) == 8


def test_a_short_wait_is_caught():
    """The model is not vacuous: with one piece too many allowed in flight the first read is flagged."""
    ld = Loader()
    for d in range(2):
        ld.issue(d, d, 16, 0)
    ld.wait(17, 0)
    assert ld.landed.get(0) is None
