"""Device-side step meter: per-step loss terms, gradient norm and clip coefficient without a host sync per step.

mmcv's TextLoggerHook reads every logged value with ``.item()`` at every iteration; on a step that is one hipGraph
replay that read is the only thing that would make the host wait.  Here one small launch per step
(``demf_step_meter``, csrc/meter.hip) writes a 64-byte record into a device-resident ring, row ``t % rows``, stamped
with the optimizer's step count ``t``.  The host copies the whole ring into pinned memory now and then
(``snapshot``: one copy + one event, returns at once) and decodes it once the event has completed (``collect``).
The stamps tell which rows are new, so nothing has to be counted on the host - a step that is a node of a captured
graph is metered by the replay itself.
"""
import numpy as np
import torch

from . import ops

ROW_WORDS, HEAD_WORDS, MAX_SCALARS = ops.METER_ROW_WORDS, ops.METER_HEAD_WORDS, ops.METER_MAX_SCALARS
FLAG_GRAD_NORM = ops.METER_FLAG_GRAD_NORM


def loss_names():
    """The scalars ``engine.Trainer`` meters: the head's seven loss terms, the vote loss and their sum."""
    return tuple(ops.HEAD_LOSS_NAMES) + ("vote_loss", "_total")


def empty_ring(rows):
    """A host ring as ``StepMeter`` initialises the device one: every stamp -1, every other word 0."""
    ring = np.zeros((int(rows), ROW_WORDS), np.int32)
    ring[:, :2].view(np.int64)[:, 0] = -1
    return ring


def decode_ring(ring, names, next_t):
    """The steps ``next_t .. newest stamp`` of a ring snapshot ((rows, 16) int32, layout in include/demf_hip.h), in
    ``t`` order -> (list of row dicts, the next ``t`` to expect).  A row dict has ``t``, ``lr_factor``,
    ``grad_norm``, ``clip``, ``nonfinite`` (the names whose flag bit is set, ``"grad_norm"`` included; empty when
    all is finite) and one float per name.  A row of that range carrying another stamp has been overwritten by a
    later step or never written: the ring was overrun (more steps between two snapshots than it has rows)."""
    ring = np.ascontiguousarray(ring, dtype=np.int32)
    if ring.ndim != 2 or ring.shape[1] != ROW_WORDS or ring.shape[0] < 1:
        raise ValueError("a meter ring is (rows >= 1, %d) int32, got %s" % (ROW_WORDS, ring.shape))
    if not 1 <= len(names) <= MAX_SCALARS:
        raise ValueError("a meter row holds 1..%d scalars, got %d names" % (MAX_SCALARS, len(names)))
    R = ring.shape[0]
    stamps = ring[:, :2].view(np.int64)[:, 0]
    flags = ring[:, 2].view(np.uint32)
    f32 = ring.view(np.float32)
    newest = int(stamps.max())
    out = []
    for t in range(int(next_t), newest + 1):
        r = t % R
        if int(stamps[r]) != t:
            raise RuntimeError("step meter ring overrun: step %d was expected in row %d, which holds step %d (%d "
                               "steps since the last snapshot, the ring has %d rows)"
                               % (t, r, int(stamps[r]), newest + 1 - int(next_t), R))
        bits = int(flags[r])
        bad = tuple(n for i, n in enumerate(names) if bits >> i & 1)
        if bits & FLAG_GRAD_NORM:
            bad += ("grad_norm",)
        row = dict(t=t, lr_factor=float(f32[r, 3]), grad_norm=float(f32[r, 4]), clip=float(f32[r, 5]), nonfinite=bad)
        for i, n in enumerate(names):
            row[n] = float(f32[r, HEAD_WORDS + i])
        out.append(row)
    return out, max(int(next_t), newest + 1)


class StepMeter:
    """The ring on ``device`` plus its host side.  ``names``: what the scalars of ``record`` are called."""

    def __init__(self, names, ring_rows=128, device=None):
        self.names = tuple(names)
        if not 1 <= len(self.names) <= MAX_SCALARS:
            raise ValueError("StepMeter takes 1..%d names, got %d" % (MAX_SCALARS, len(self.names)))
        if int(ring_rows) < 1:
            raise ValueError("StepMeter: ring_rows must be positive")
        self.rows = int(ring_rows)
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.ring = torch.from_numpy(empty_ring(self.rows)).to(self.device)
        self.next_t = 0                   # the first step the host has not been handed yet
        self._pending = []                # (pinned copy of the ring, event behind the copy), oldest first
        self._free = []                   # pinned buffers to use again

    def record(self, scalars, opt_state, grad_scale, max_norm):
        """Launch the meter on the current stream (or into the capture in progress)."""
        if len(scalars) != len(self.names):
            raise ValueError("StepMeter.record: %d scalars for %d names" % (len(scalars), len(self.names)))
        ops.step_meter(list(scalars), opt_state, grad_scale, max_norm, self.ring)

    def snapshot(self):
        """Enqueue one device -> pinned copy of the ring and an event behind it; does not wait.  In a process group
        of more than one rank the ring copied is the merge of every rank's (``ranks.merge_rings``: one collective of
        ``rows * 64`` bytes per rank, then ``ops.meter_merge`` on the current stream), so every rank decodes the same
        rows - the loss terms averaged over ranks; every rank has to take its snapshots at the same steps."""
        from . import ranks
        buf = self._free.pop() if self._free else torch.empty((self.rows, ROW_WORDS), dtype=torch.int32,
                                                              pin_memory=True)
        buf.copy_(ranks.merge_rings(self.ring) if ranks.world() > 1 else self.ring, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self._pending.append((buf, ev))

    def collect(self, wait=False):
        """Rows of the snapshots whose copy has completed (``wait``: of all snapshots, blocking on their events):
        every step once, in ``t`` order.  Raises on a ring overrun (``decode_ring``)."""
        out = []
        while self._pending:
            buf, ev = self._pending[0]
            if wait:
                ev.synchronize()
            elif not ev.query():
                break
            self._pending.pop(0)
            rows, self.next_t = decode_ring(buf.numpy(), self.names, self.next_t)
            self._free.append(buf)
            out += rows
        return out

    def state_dict(self):
        return dict(next_t=int(self.next_t))

    def load_state_dict(self, sd):
        """Continue at the checkpoint's position: snapshots in flight are dropped and the ring starts empty."""
        self.next_t = int(sd["next_t"])
        self._free += [b for b, _ in self._pending]
        self._pending = []
        self.ring.copy_(torch.from_numpy(empty_ring(self.rows)))
