"""Training-step engine for the DeMF hot path on MI355X.

The reference trains with mmcv's EpochBasedRunner + MMDistributedDataParallel over NCCL
(train.py:56-63,140-147; tools/dist_train.sh:8-9): replicas only, gradients all-reduced,
AdamW with 'decoder' lr_mult 0.05 and grad-clip 10 (configs/demf/demf_votenet.py:16-24,
configs/_base_/schedules/schedule_3x.py:6).  MI355X-first restatement:

  * one process per GPU, torch.distributed backend "nccl" (= RCCL over xGMI);
  * the 2.19 M trainable parameters' gradients live in ONE flat fp32 buffer (8.76 MB):
    every p.grad is a view into it, so a step issues exactly one RCCL all-reduce - at this
    size the collective is latency-bound on xGMI, so one call beats DDP's bucket stream -
    and one fused clip + AdamW over the flat buffers;
  * no model sharding (the reference has none).
"""
import contextlib
import os

import torch
import torch.distributed as dist

from . import switches


def init_distributed():
    """Reads RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* from the environment (torchrun)."""
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if switches.env_on("DEMF_SHARE_DEVICE"):
        # test hook: several ranks on ONE GPU (with DEMF_DIST_BACKEND=gloo), to exercise the
        # multi-rank code path of bench.py on a single-GPU box
        local = 0
    if world > 1 and not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29500")
        backend = switches.env_str("DEMF_DIST_BACKEND") or \
            ("nccl" if torch.cuda.is_available() else "gloo")
        if torch.cuda.is_available():
            torch.cuda.set_device(local)
        dist.init_process_group(backend=backend, rank=rank, world_size=world)
    elif torch.cuda.is_available():
        torch.cuda.set_device(local)
    return rank, local, world


def cu_masked_streams(side_cus):
    """(main, side) torch streams on disjoint CU sets: ``side`` runs only on ``side_cus``, ``main``
    on every other CU (hipExtStreamCreateWithCUMask through libdemf_hip.so)."""
    import ctypes
    from . import _ffi
    arr = (ctypes.c_int * len(side_cus))(*side_cus)
    out = []
    for invert in (1, 0):
        h = ctypes.c_void_p()
        _ffi.call("demf_stream_create_cu_masked", ctypes.cast(arr, ctypes.c_void_p), len(side_cus),
                  invert, ctypes.cast(ctypes.byref(h), ctypes.c_void_p))
        out.append(torch.cuda.ExternalStream(h.value))
    return out[0], out[1]


_REJECTED_STREAMS = []      # streams found to share the main stream's hardware queue (kept: the pool must move on)


def concurrent_stream(main=None, tries=8, spin_us=300):
    """A new torch stream that really runs CONCURRENTLY with ``main`` (default: the current stream).
    HIP multiplexes streams onto a few hardware queues (4 by default); a side stream that lands on the main
    stream's queue is serialised with it, and the pipelined FPS pre-pass - 2.1 ms meant to run underneath the
    step - then runs in front of it (measured: 4.84 -> 7.45 ms per step for one unlucky stream of torch's pool,
    bench.py's clustered leg after another stream had been created).  Each candidate is probed with two spin
    kernels of known length (demf_spin_us), one per stream: together they take one length if the streams are
    concurrent, two if they share a queue."""
    from . import _ffi
    main = main if main is not None else torch.cuda.current_stream()
    if torch.cuda.is_current_stream_capturing():
        return torch.cuda.Stream()
    last = None
    for _ in range(tries):
        cand = torch.cuda.Stream()
        last = cand
        cand.wait_stream(main)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(main)
        _ffi.call("demf_spin_us", spin_us, main.cuda_stream)
        with torch.cuda.stream(cand):
            _ffi.call("demf_spin_us", spin_us, cand.cuda_stream)
        main.wait_stream(cand)
        e1.record(main)
        e1.synchronize()
        if e0.elapsed_time(e1) * 1e3 < 1.5 * spin_us:
            return cand
        _REJECTED_STREAMS.append(cand)
    return last


class FlatGrads:
    """All trainable gradients as views of one contiguous buffer; one all-reduce per step."""

    def __init__(self, params):
        self.params = [p for p in params if p.requires_grad]
        n = sum(p.numel() for p in self.params)
        dev, dt = self.params[0].device, self.params[0].dtype
        self.flat = torch.zeros(n, dtype=dt, device=dev)
        self.views = []
        self._pending_tables, self._tables = [], []     # address tables of captured pack launches
        self.captured_pack = False      # set inside ``capturing`` (Trainer.capture, which calls finish_capture)
        self.sumsq_state = None         # FlatAdamW.state while a capture wants the pack to take the clip norm
        self.mode = None                # gradient accumulation (Trainer(accumulate > 1)): "accumulate" / "last" - the
        #                                 pack ADDS into the buffer; None: it overwrites (one pass per optimizer step)
        self._reserved_table = None
        off = 0
        for p in self.params:
            k = p.numel()
            p.grad = self.flat[off:off + k].view_as(p)
            self.views.append(p.grad)
            off += k

    def backward_into(self, loss):
        """d(loss)/d(params) straight into the flat buffer: one autograd.grad + multi-tensor
        copies, instead of 119 per-parameter accumulate kernels (and no zero-fill dependence)."""
        if self.flat.is_cuda:
            from . import ops
            with ops.deferred_weight_grads():       # the few-row stacks' dW products as one grouped launch at the end
                grads = torch.autograd.grad(loss, self.params, allow_unused=True)
        else:
            grads = torch.autograd.grad(loss, self.params, allow_unused=True)
        if self.mode is not None:
            return self._add_into(grads)
        dst = [v for v, g in zip(self.views, grads) if g is not None]
        src = [g for g in grads if g is not None]
        if len(src) != len(grads):
            self.flat.zero_()
        if self.captured_pack and self.flat.is_cuda and torch.cuda.is_current_stream_capturing() and src:
            # Under capture the gradients live at fixed addresses of the graph's pool: one
            # demf_multi_copy launch over an address table (two multi-tensor launches of 37 us each
            # otherwise).  The table cannot be uploaded while capturing; the recorded launch only
            # holds its device address, ``finish_capture`` fills it before the first replay.
            from . import _ffi
            src = [g if g.is_contiguous() else g.contiguous() for g in src]
            tab = [[g.data_ptr() for g in src], [d.data_ptr() for d in dst],
                   [d.numel() for d in dst]]
            # (allocated by Trainer.capture BEFORE capturing: memory of the graphs' shared pool is
            # scratch that the forward graph rewrites on every replay)
            table = self._reserved_table.view(-1)[:3 * len(src)].view(3, len(src))
            blocks = max(1, min(64, max(tab[2]) // 4096))
            if self.sumsq_state is not None:
                # + the squared norm of everything packed, for the clip of the in-graph update
                _ffi.call("demf_multi_copy_sumsq", len(src), table.data_ptr(), blocks,
                          self.sumsq_state.data_ptr(), torch.cuda.current_stream().cuda_stream)
            else:
                _ffi.call("demf_multi_copy", len(src), table.data_ptr(), blocks,
                          torch.cuda.current_stream().cuda_stream)
            self._pending_tables.append((table, tab))
            return
        torch._foreach_copy_(dst, src)

    def _add_into(self, grads):
        """One pass of a group of micro-steps: flat += grads.  The buffer is zero at the start of a group
        (Trainer's invariant), nothing is zero-filled here - a ``None`` gradient leaves the earlier passes' sum
        alone.  Captured: one demf_multi_add launch; the last pass's table covers EVERY parameter (null sources
        for ``None`` gradients) so that demf_multi_add_sumsq takes the norm of the whole accumulated buffer."""
        if self.captured_pack and self.flat.is_cuda and torch.cuda.is_current_stream_capturing():
            from . import _ffi
            with_sum = self.mode == "last" and self.sumsq_state is not None
            pairs = [(g, d) for g, d in zip(grads, self.views) if g is not None or with_sum]
            if not pairs:
                return
            src = [g if g is None or g.is_contiguous() else g.contiguous() for g, _ in pairs]
            tab = [[0 if g is None else g.data_ptr() for g in src], [d.data_ptr() for _, d in pairs],
                   [d.numel() for _, d in pairs]]
            table = self._reserved_table.view(-1)[:3 * len(src)].view(3, len(src))
            blocks = max(1, min(64, max(tab[2]) // 4096))
            stream = torch.cuda.current_stream().cuda_stream
            if with_sum:
                _ffi.call("demf_multi_add_sumsq", len(src), table.data_ptr(), blocks, self.sumsq_state.data_ptr(),
                          stream)
            else:
                _ffi.call("demf_multi_add", len(src), table.data_ptr(), blocks, stream)
            self._pending_tables.append((table, tab))
            return
        dst = [v for v, g in zip(self.views, grads) if g is not None]
        if dst:
            torch._foreach_add_(dst, [g for g in grads if g is not None])

    @contextlib.contextmanager
    def capturing(self, mode, sumsq_state):
        """Around a stream capture of a backward: the pack is ONE launch over an address table, in ``mode``, and
        takes the clip norm into ``sumsq_state`` (or ``None``); all three are cleared however the capture ends."""
        self.captured_pack, self.mode, self.sumsq_state = True, mode, sumsq_state
        try:
            yield
        finally:
            self.captured_pack, self.mode, self.sumsq_state = False, None, None

    def reserve_table(self):
        """Room for the address table of one captured pack launch, from the ordinary allocator."""
        self._reserved_table = torch.empty((3, len(self.params)), dtype=torch.int64,
                                           device=self.flat.device)

    def finish_capture(self):
        """Upload the address tables of the pack launches recorded while capturing (call once the
        capture has ended, before the first replay)."""
        for table, tab in self._pending_tables:
            table.copy_(torch.tensor(tab, dtype=torch.int64))
            self._tables.append(table)                 # the graphs hold its address
        self._reserved_table = None
        self._pending_tables = []

    def zero_(self):
        self.flat.zero_()

    def all_reduce_mean(self):
        if dist.is_initialized() and dist.get_world_size() > 1:
            dist.all_reduce(self.flat, op=dist.ReduceOp.SUM)
            self.flat.div_(dist.get_world_size())

    def clip_(self, max_norm):
        """clip_grad_norm_(max_norm) on the flat buffer (one norm, one scale)."""
        norm = torch.linalg.vector_norm(self.flat)
        self.flat.mul_(torch.clamp(max_norm / (norm + 1e-6), max=1.0))
        return norm


class FlatAdamW:
    """torch.optim.AdamW over parameter groups whose parameters are re-homed into ONE flat fp32
    buffer (each p.data becomes a view of it, in FlatGrads order), with flat moment buffers: a
    step is ONE demf_adamw_state_f32 launch over all groups (csrc/optim.hip) with the clip coefficient
    and the 1/world_size of the gradient mean folded in, instead of 22 multi-tensor launches + a
    scaling pass.  Step count, learning-rate factor and the squared gradient norm live in a 64-byte
    DEVICE state block, so the launch takes no host argument that changes from step to step and the
    whole update can be a node of the step's hipGraph (Trainer.capture).  Group semantics as the
    reference's config (demf_votenet.py:16-24)."""

    def __init__(self, groups, flat_grads, betas=(0.9, 0.999), eps=1e-8):
        import ctypes
        from ._ffi import OptState
        params = flat_grads.params
        assert [id(p) for g in groups for p in g["params"] if p.requires_grad] == [id(p) for p in params]
        self.grads = flat_grads.flat
        self.flat = torch.empty_like(self.grads)
        off, self.segments = 0, []
        for g in groups:
            start = off
            for p in g["params"]:
                if not p.requires_grad:
                    continue
                k = p.numel()
                self.flat[off:off + k].copy_(p.data.reshape(-1))
                p.data = self.flat[off:off + k].view_as(p)
                off += k
            if off > start:
                self.segments.append((start, off - start, float(g["lr"]), float(g["weight_decay"])))
        if not 1 <= len(self.segments) <= 4:
            raise ValueError("FlatAdamW: %d parameter groups (demf_adamw_state_f32 takes 1..4)" % len(self.segments))
        n = len(self.segments)
        self._seg = ((ctypes.c_longlong * n)(*[s[0] for s in self.segments]),
                     (ctypes.c_longlong * n)(*[s[1] for s in self.segments]),
                     (ctypes.c_float * n)(*[s[2] for s in self.segments]),
                     (ctypes.c_float * n)(*[s[3] for s in self.segments]))
        self.params = params
        self.exp_avg = torch.zeros_like(self.flat)
        self.exp_avg_sq = torch.zeros_like(self.flat)
        self.betas, self.eps = betas, eps
        self.state = torch.zeros(ctypes.sizeof(OptState), dtype=torch.uint8, device=self.flat.device)
        self._t_word, self._lr_word = OptState.t.offset // 8, OptState.lr_factor.offset // 4    # of int64 / fp32 views
        self._lr_factor = 1.0
        self.state.view(torch.float32)[self._lr_word] = 1.0

    @property
    def t(self):
        """Completed optimizer steps (read from the device: synchronises)."""
        return int(self.state.view(torch.int64)[self._t_word].item())

    @t.setter
    def t(self, value):
        self.state.view(torch.int64)[self._t_word] = int(value)

    @property
    def lr_factor(self):
        return self._lr_factor

    def set_lr_factor(self, factor):
        """Multiplies every group's base learning rate (the reference's step schedule:
        lr_config step=[24, 32], x0.1 each - configs/_base_/schedules/schedule_3x.py:7-9).
        Written into the device state: captured steps pick it up at their next replay."""
        self._lr_factor = float(factor)
        self.state.view(torch.float32)[self._lr_word] = float(factor)

    def check_aliasing(self):
        """Every parameter must still be a view of the flat buffer: ``model.to()`` / ``.float()`` /
        ``.half()`` after the optimizer was built re-allocates ``p.data`` and would silently detach
        the parameter from the update."""
        lo = self.flat.data_ptr()
        hi = lo + 4 * self.flat.numel()
        for p in self.params:
            if not (lo <= p.data_ptr() < hi):
                raise RuntimeError("a parameter no longer lives in FlatAdamW's flat buffer (was the "
                                   "model moved or cast after the Trainer was built?)")

    def state_dict(self):
        """Moments + step count + lr factor (resume: mmcv CheckpointHook saves the optimizer too)."""
        return dict(exp_avg=self.exp_avg.clone(), exp_avg_sq=self.exp_avg_sq.clone(), t=self.t,
                    lr_factor=self.lr_factor, numel=self.flat.numel())

    def load_state_dict(self, sd):
        if int(sd["numel"]) != self.flat.numel():
            raise ValueError("optimizer state is for %d parameters, this model has %d"
                             % (int(sd["numel"]), self.flat.numel()))
        self.exp_avg.copy_(sd["exp_avg"])
        self.exp_avg_sq.copy_(sd["exp_avg_sq"])
        self.t = int(sd["t"])
        self.set_lr_factor(float(sd.get("lr_factor", 1.0)))

    def step(self, max_norm=0.0, grad_scale=1.0, norm_taken=False, meter=None, scalars=None):
        """One update of every group from the flat gradient buffer.  ``norm_taken``: the squared norm
        of the gradients is already in the device state (the captured pack took it,
        demf_multi_copy_sumsq); otherwise one reduction launch over the flat buffer comes first.
        ``meter`` (meter.StepMeter) with the step's loss ``scalars``: one more launch, between the point
        where the norm is complete in the state and the AdamW launch that clears it."""
        import ctypes
        from . import _ffi
        self.check_aliasing()
        stream = torch.cuda.current_stream().cuda_stream
        if max_norm > 0.0 and not norm_taken:
            _ffi.call("demf_sumsq_f32", self.grads.numel(), self.grads.data_ptr(), self.state.data_ptr(), stream)
        if meter is not None:
            meter.record(scalars, self.state, grad_scale, max_norm)
        a = [ctypes.cast(x, ctypes.c_void_p) for x in self._seg]
        _ffi.call("demf_adamw_state_f32", len(self.segments), a[0], a[1], a[2], a[3], self.flat.data_ptr(),
                  self.grads.data_ptr(), self.exp_avg.data_ptr(), self.exp_avg_sq.data_ptr(),
                  self.state.data_ptr(), float(max_norm), float(grad_scale), self.betas[0], self.betas[1],
                  self.eps, stream)


@contextlib.contextmanager
def _gc_paused():
    """No garbage collection inside a stream capture.  A collection that reaches an unreachable CUDAGraph (the trainer of
    an earlier phase, kept alive by a reference cycle until now) releases that graph's memory pool, and a hipFree under
    capture aborts the process (seen in the test suite: `Fatal Python error: Aborted`, "Garbage-collecting" on the
    stack of a capture).  Collect once before the capture begins, then keep the collector off until it has ended."""
    import gc
    gc.collect()
    was = gc.isenabled()
    gc.disable()
    try:
        yield
    finally:
        if was:
            gc.enable()


# Replay orders that measured slower than the default and were taken out; ``Trainer.capture`` refuses their
# switches instead of silently measuring the default order under their name (DESIGN_LOG section 5).
RETIRED_ORDERS = {
    "DEMF_GEO_AT_BWD": "forward and backward as two graphs with the pre-pass launched in between measured 6.49 "
                       "against 6.39 ms per step, later 4.95 against 4.88 ms",
    "DEMF_GEO_TWO_DEEP": "the pre-pass two steps ahead measured 7.80 against 7.67 ms per step",
}
_OVERLAP_REFUSAL = "the overlapped (deferred) update is not available with accumulate = %d > 1: unset " \
                   "DEMF_AR_OVERLAP / allreduce_overlap"


def _capture_plan(accumulate, micro, role, dry, update_in_graph, fused, world, stub, overlap, graph_update,
                  graph_allreduce, retired_set):
    """What ``Trainer.capture`` decides before it touches anything -> (role, dry, update_in_graph), or a refusal.
    No torch and no environment in here: ``overlap`` is ``allreduce_config()[2]``, ``graph_update`` /
    ``graph_allreduce`` are the values of DEMF_GRAPH_UPDATE / DEMF_GRAPH_ALLREDUCE and ``retired_set`` holds the
    names of RETIRED_ORDERS found in the environment.  In this order: a retired switch is refused whatever else
    was asked; with accumulate = 1 the role is ``None`` (asked as ``None`` or "last"); with W > 1 it defaults from
    ``micro``, the warm-up is dry and the overlapped update is refused; the update goes into the graph only on the
    fused path, without an all-reduce stub, and on one rank unless the collective is captured too."""
    if retired_set:
        name = min(retired_set)
        raise RuntimeError("%s is set, and the replay order it selected was retired (%s): capture() records the "
                           "default order only; unset it" % (name, RETIRED_ORDERS[name]))
    if accumulate == 1:
        if role not in (None, "last"):
            raise ValueError("capture(role=%r): with accumulate = 1 every step is the last of its group" % (role,))
        role = None
    else:
        if role is None:
            role = "last" if micro == accumulate - 1 else "accumulate"
        if role not in ("accumulate", "last"):
            raise ValueError("capture(role=%r): 'accumulate' or 'last'" % (role,))
        if fused and overlap:
            raise RuntimeError(_OVERLAP_REFUSAL % accumulate)
        dry = True
    if update_in_graph is None:
        update_in_graph = bool(graph_update)
    update_in_graph = bool(update_in_graph) and fused and stub == 0 and (world == 1 or bool(graph_allreduce))
    return role, dry, update_in_graph


class Trainer:
    """fwd -> loss -> bwd -> one all-reduce -> clip -> AdamW, as one callable step."""

    _accumulate, micro, _loss_acc = 1, 0, None        # (gradient accumulation off: the plain step)

    def __init__(self, model, lr=0.008, weight_decay=0.01, max_grad_norm=10.0, forward=None, accumulate=1):
        """``forward``: called instead of ``model.forward_train`` with the same arguments (a detector whose own
        ``forward_train`` takes the image runs its hot path through this: demf_amd/train.py).
        ``accumulate`` = W: one optimizer step is formed from W micro-steps (``step`` / a replay = ONE forward +
        backward on one batch), AdamW on the mean of their gradients - the reference's 8 ranks x 16 scenes
        (tools/dist_train.sh:4) on one GPU with W = 8.  ``micro`` (0 .. W-1, host side) is the position in the open
        group.  Between optimizer steps the flat gradient buffer, the loss accumulator, the state's ``sumsq`` and
        its ticket are all zero; the last micro-step clears them after AdamW has consumed them.  W = 1 is the plain
        step."""
        self._accumulate = self._check_accumulate(accumulate)
        self.micro = 0
        self._loss_acc = None              # with a meter and W > 1: the group's mean loss scalars, on the device
        self.model = model
        self._forward = forward
        self.meter = None
        self._loss_scalars = None          # with a meter: the loss dict's device scalars of the last forward
        self._pending_scalars = None       # ... of the step whose deferred update is still owed
        self._pending_update = False       # an overlapped step's norm + AdamW are still owed (flush)
        self.side_stream = None            # the pre-pass stream of the next capture (default: a probed concurrent one)
        self._comm_stream = None           # the collective's stream, made on first use
        self.allreduce_stub_us = 0         # > 0: a spin kernel of that length in the collective's place
        self.allreduce_overlap = None      # None: DEMF_AR_OVERLAP decides
        self.allreduce_events = None       # a list: HIP event pairs around every collective are appended (bench.py)
        self._graph = None                 # the hipGraph of the last capture
        groups = model.param_groups(lr=lr, weight_decay=weight_decay)
        self.flat = FlatGrads([p for g in groups for p in g["params"]])
        self.max_grad_norm = max_grad_norm
        if dist.is_initialized() and dist.get_world_size() > 1:
            for p in model.parameters():           # identical replicas at step 0
                dist.broadcast(p.data, src=0)
            for b in model.buffers():
                dist.broadcast(b.data, src=0)
        # device path: flat fused AdamW (HIP); the torch optimizer serves the CPU/gloo host-logic
        # tests only
        self.fused = self.flat.flat.is_cuda
        if self.fused:
            from . import fused
            rank = dist.get_rank() if dist.is_initialized() else 0
            fused.rng_state(self.flat.flat.device, seed=torch.initial_seed() + 7919 * rank)
        self.opt = FlatAdamW(groups, self.flat) if self.fused else \
            torch.optim.AdamW(groups, lr=lr, weight_decay=weight_decay, foreach=True)
        self._base_lrs = [float(g["lr"]) for g in groups]

    # ---- gradient accumulation ------------------------------------------------------------------------
    @staticmethod
    def _check_accumulate(value):
        if isinstance(value, bool) or not isinstance(value, int) or value < 1:
            raise ValueError("accumulate must be a positive integer, got %r" % (value,))
        return int(value)

    @property
    def accumulate(self):
        return self._accumulate

    @accumulate.setter
    def accumulate(self, value):
        value = self._check_accumulate(value)
        if value == self._accumulate:
            return
        if self.micro:
            raise RuntimeError("accumulate cannot change inside a group (micro = %d of %d): finish it or call "
                               "reset_accumulation()" % (self.micro, self._accumulate))
        if self.fused:
            self.flush()
        self._accumulate = value
        self._ensure_acc()
        self.reset_accumulation()          # (the plain step overwrites the buffer and may leave anything in it)

    def _ensure_acc(self):
        if self._accumulate > 1 and self.meter is not None and self._loss_acc is None:
            from . import ops
            self._loss_acc = torch.zeros(ops.METER_MAX_SCALARS, dtype=torch.float32, device=self.flat.flat.device)

    def _acc_scalars(self):
        return [self._loss_acc[i:i + 1] for i in range(len(self.meter.names))]

    def reset_accumulation(self):
        """Abandon the open group: gradient buffer, loss accumulator, ``sumsq`` and ticket back to zero,
        ``micro = 0``.  Runs by itself when a forward + backward raises (outside capture), in ``load_state_dict``
        and whenever the runner drops an incomplete group."""
        self.micro = 0
        if self._accumulate == 1:
            return
        self.flat.flat.zero_()
        if self._loss_acc is not None:
            self._loss_acc.zero_()
        if self.fused:
            self.opt.state[0:8].zero_()
            self.opt.state[16:20].zero_()

    def _mid_group(self, what):
        if self.micro:
            raise RuntimeError("%s in the middle of a group of micro-steps (micro = %d of accumulate = %d): finish "
                               "the group or call reset_accumulation()" % (what, self.micro, self._accumulate))

    def _refuse_overlap(self):
        if self._accumulate > 1 and self.fused and self.allreduce_config()[2]:
            raise RuntimeError(_OVERLAP_REFUSAL % self._accumulate)

    def _clear_group(self):
        """The clears of a group's last micro-step, behind the AdamW launch that consumed the buffers (kernel
        launches: in the stream of an eager step, nodes of a captured one)."""
        from . import _ffi
        stream = torch.cuda.current_stream().cuda_stream
        _ffi.call("demf_zero_f32", self.flat.flat.numel(), self.flat.flat.data_ptr(), stream)
        if self.meter is not None:
            _ffi.call("demf_zero_f32", self._loss_acc.numel(), self._loss_acc.data_ptr(), stream)

    def _accumulate_scalars(self, scalars=None):
        """acc += loss scalars / W (one demf_scalars_accum launch); without a meter there is no launch."""
        if self.meter is not None:
            from . import ops
            ops.scalars_accum(self._loss_scalars if scalars is None else scalars,
                              self._loss_acc, 1.0 / self._accumulate)

    def attach_meter(self, meter):
        """Meter every optimizer step from now on (meter.StepMeter over ``meter.loss_names()``): one
        ``demf_step_meter`` launch per step in front of the AdamW launch - in the stream of an eager update, as a
        node of a step captured with its update.  Attach BEFORE capturing: a captured step is metered or not for
        good, and its replay refuses to run if that no longer matches the trainer.  Without a meter nothing
        changes.  ``None`` detaches."""
        if meter is not None and not self.fused:
            raise RuntimeError("attach_meter: the step meter is a device kernel; this trainer runs the CPU / gloo "
                               "path (torch.optim.AdamW), which has nothing to meter")
        self._mid_group("attach_meter()")
        if meter is not None:
            self.flush()
            meter.next_t = self.opt.t
        self.meter = meter
        self._loss_scalars = self._pending_scalars = None
        self._ensure_acc()

    def set_epoch(self, epoch, steps=(24, 32), gamma=0.1):
        """The reference's step schedule (configs/_base_/schedules/schedule_3x.py:7-9:
        lr_config = dict(policy='step', step=[24, 32]), 36 epochs): lr x gamma at each milestone."""
        self._mid_group("set_epoch()")
        factor = gamma ** sum(1 for s in steps if epoch >= s)
        if self.fused:
            self.flush()                 # (an overlapped step's owed update still uses the old rate)
            self.opt.set_lr_factor(factor)
        else:
            for g, base in zip(self.opt.param_groups, self._base_lrs):
                g["lr"] = base * factor
        return factor

    def state_dict(self):
        """Model + optimizer state for resume (mmcv CheckpointHook, cfg:280), plus the dropout
        counter [seed, step] of the fused decoder layer so that a resumed run continues the mask
        sequence instead of replaying it from step 0."""
        self._mid_group("state_dict()")
        if self.fused:
            self.flush()
        sd = dict(model=self.model.state_dict(), optimizer=self.opt.state_dict())
        if self.fused:
            from . import fused
            sd["dropout_rng"] = fused.get_rng_state(self.flat.flat.device)
        return sd

    def load_state_dict(self, sd):
        # copies INTO the existing (flat-buffer-resident) parameters: the views stay intact
        if self.fused:
            self.flush()                 # (never apply an owed update of the OLD gradients to the loaded state)
        self.model.load_state_dict(sd["model"])
        self.opt.load_state_dict(sd["optimizer"])
        if self.fused and sd.get("dropout_rng") is not None:
            from . import fused
            fused.set_rng_state(self.flat.flat.device, sd["dropout_rng"])
        self.reset_accumulation()

    def _fwd(self, batch, geometry=None):
        kw = {} if geometry is None else dict(geometry=geometry)
        # (the fused decoder layer advances its counter-based dropout state by itself, inside the
        # forward and therefore inside the captured graph: demf_amd/fused.py)
        fwd = self.model.forward_train if self._forward is None else self._forward
        if "img_features" in batch:
            losses = fwd(batch["points"], batch["img_features"], batch["img_metas"], batch["gt_bboxes_3d"],
                         batch["gt_labels_3d"], **kw)
        else:
            # a points-only batch (modules.VoteNet: no image stream, nothing to stage or refresh per batch)
            losses = fwd(batch["points"], batch.get("img_metas"), batch["gt_bboxes_3d"], batch["gt_labels_3d"], **kw)
        if self.meter is not None:
            missing = [k for k in self.meter.names if k not in losses]
            if missing:
                raise RuntimeError("the step meter expects the loss terms %s; this forward did not produce %s (the "
                                   "fused loss path hands out all of them)" % (list(self.meter.names), missing))
            self._loss_scalars = [losses[k].detach() for k in self.meter.names]
        # the head hands out the sum of its losses directly (one node instead of 8 selects)
        return losses["_total"] if "_total" in losses else torch.stack(list(losses.values())).sum()

    def _arena(self, begin):
        """Bracket forward + backward with the step's zero arena (ops._ZeroArena) on the device path."""
        if self.fused:
            from . import ops
            if begin:
                ops.ARENA.begin(self.flat.flat.device)
            else:
                ops.ARENA.end()

    def _fwd_bwd(self, batch, geometry=None):
        self._arena(True)
        try:
            total = self._fwd(batch, geometry)
            self.flat.backward_into(total)
        except BaseException:
            if self.fused and not torch.cuda.is_current_stream_capturing():
                from . import ops
                ops.reset_accumulators()          # (a step that raised half-way leaves BatchNorm sums behind)
            if self._accumulate > 1 and not (self.fused and torch.cuda.is_current_stream_capturing()):
                self.reset_accumulation()         # (the group this pass belonged to is abandoned)
            raise
        finally:
            self._arena(False)
        return total.detach()

    # ---- gradient all-reduce + clip + AdamW ------------------------------------------------------------
    # The collective is latency-bound at 8.76 MB and nothing after it in the step can start
    # before it ends (the clip needs the norm of the reduced gradients) - but the NEXT batch's input path can:
    # ``replay.load`` (token conversion of the image pyramid, target padding, constants) and the launch of the
    # coordinate pre-pass touch neither the gradients nor the parameters.  With ``overlap`` the collective is issued
    # on a communication stream when the step's graph has been enqueued, ``replay()`` returns, and norm + AdamW
    # are enqueued at the start of the next ``replay()`` (or by ``flush()``), behind the collective: it runs
    # underneath whatever the caller enqueues in between.  The RCCL call itself stays an ordinary eager call on a
    # stream - nothing is captured, so the multi-GPU path is the one the gloo / shared-GPU tests exercise.
    def _comm(self):
        if self._comm_stream is None:
            self._comm_stream = concurrent_stream()
        return self._comm_stream

    def allreduce_config(self):
        """(world, stub_us, overlap): ``stub_us`` > 0 replaces the collective by a spin kernel of that length
        (bench.py --allreduce-stub-us: the overlap measured on one GPU); overlap is opt-in (DEMF_AR_OVERLAP=1 or
        ``trainer.allreduce_overlap = True``)."""
        world = dist.get_world_size() if dist.is_initialized() else 1
        stub = int(self.allreduce_stub_us or 0)
        ov = self.allreduce_overlap
        if ov is None:
            # default OFF: measured on MI355X / ROCm 7.2 with a spin kernel in the collective's place
            # (bench.py secondary.allreduce_stub100us_*; profiles/r05_allreduce_overlap_probe.log) the extra
            # cross-queue dependencies of the deferred order cost 0.23 ms per step - more than a 100 us collective
            # takes on the step's own stream
            ov = bool(switches.env_int("DEMF_AR_OVERLAP"))
        return world, stub, bool(ov) and (world > 1 or stub > 0)

    def _collective(self, world, stub):
        ev = self.allreduce_events                     # bench.py: HIP events around the collective
        if ev is not None:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
        if stub > 0:
            from . import _ffi
            _ffi.call("demf_spin_us", stub, torch.cuda.current_stream().cuda_stream)
        if world > 1:
            dist.all_reduce(self.flat.flat, op=dist.ReduceOp.SUM)
        if ev is not None:
            e1.record()
            ev.append((e0, e1))

    def _finish_update(self, norm_taken=False, scalars=None):
        world = dist.get_world_size() if dist.is_initialized() else 1
        # (the norm is that of the SUM over ranks; 1/world is applied in-kernel)
        if self._accumulate > 1:
            # ... and over the W passes of the group: 1 / (W * world); the meter reads the accumulated means
            self.opt.step(self.max_grad_norm, 1.0 / (self._accumulate * world), norm_taken=norm_taken,
                          meter=self.meter, scalars=None if self.meter is None else self._acc_scalars())
            self._clear_group()
            return
        if self.meter is None:
            self.opt.step(self.max_grad_norm, 1.0 / world, norm_taken=norm_taken)
            return
        # metered: ``scalars`` are the loss tensors of the step this update belongs to - a captured step's own
        # (its CapturedStep owns them), else those of the last forward
        self.opt.step(self.max_grad_norm, 1.0 / world, norm_taken=norm_taken, meter=self.meter,
                      scalars=self._loss_scalars if scalars is None else scalars)

    def _captured_update(self, world):
        """The update as nodes of the step's graph (called while capturing, behind the gradient pack).  One
        rank: the pack has taken the squared norm.  More ranks (DEMF_GRAPH_ALLREDUCE=1): the flat SUM
        all-reduce is captured too (torch's NCCL / RCCL process group records the collective into the
        capturing stream), then one reduction launch for the norm of the reduced gradients."""
        if world > 1:
            dist.all_reduce(self.flat.flat, op=dist.ReduceOp.SUM)
        self._finish_update(norm_taken=(world == 1))

    def flush(self):
        """Enqueue the update a deferred (overlapped) step still owes: call before reading parameters,
        gradients or optimizer state.  ``replay()``, ``step()`` and ``state_dict()`` do it themselves."""
        if self._pending_update:
            self._pending_update = False
            torch.cuda.current_stream().wait_stream(self._comm())
            scalars, self._pending_scalars = self._pending_scalars, None
            self._finish_update(scalars=scalars)

    def _update(self, defer=False, scalars=None):
        if self.fused:
            self.flush()
            world, stub, overlap = self.allreduce_config()
            if (world > 1 or stub > 0) and overlap and defer:
                comm = self._comm()
                comm.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(comm):
                    self._collective(world, stub)
                self._pending_update = True
                if self.meter is not None:
                    self._pending_scalars = self._loss_scalars if scalars is None else scalars
                return
            if world > 1 or stub > 0:
                self._collective(world, stub)
            self._finish_update(scalars=scalars)
            return
        self.flat.all_reduce_mean()
        if self._accumulate > 1:
            self.flat.flat.mul_(1.0 / self._accumulate)
        self.flat.clip_(self.max_grad_norm)
        self.opt.step()
        if self._accumulate > 1:
            self.flat.flat.zero_()

    def step(self, batch):
        """One micro-step: forward + backward on ``batch`` -> its loss.  With ``accumulate`` = 1 that is the whole
        optimizer step.  With W > 1 micro-steps 0 .. W-2 only add into the flat gradient buffer (no norm, no
        collective, no meter row, no AdamW); micro-step W-1 adds, takes the norm of the sum (over ranks too - the
        collective runs only here), clips, runs AdamW with grad_scale = 1 / (W * world) and clears the group."""
        if self.fused:
            self.flush()
        if self._accumulate == 1:
            total = self._fwd_bwd(batch)
            self._update()
            return total
        self._refuse_overlap()
        self._ensure_acc()
        last = self.micro == self._accumulate - 1
        self.flat.mode = "last" if last else "accumulate"
        try:
            total = self._fwd_bwd(batch)
        finally:
            self.flat.mode = None
        if self.fused:
            self._accumulate_scalars()
        if last:
            self._update()
        self.micro = 0 if last else self.micro + 1
        return total

    @staticmethod
    def pad_targets(gt_boxes, gt_labels, G, device):
        """list of (n_i,7) / (n_i,) -> static-shape (B,G,7) float32, (B,G) int64 with label -1 on
        padding slots; an empty scene gets the reference's single all-zero fake box with label 0
        (class_agnostic_vote_head.py:766-773)."""
        B = len(gt_boxes)
        first = gt_boxes[0].tensor if hasattr(gt_boxes[0], "tensor") else gt_boxes[0]
        if first.is_cuda:
            # device-resident lists: padded on the device (one concatenation + one row gather per tensor,
            # DeMFVoteHead.pad_gt) - a `.cpu()` here would make the host wait for the step in flight and
            # serialise the input path with the GPU (measured: 6.66 instead of 5.6 ms per step)
            from .modules.head import DeMFVoteHead
            gt, lab, _ = DeMFVoteHead.pad_gt(gt_boxes, gt_labels, device, with_slot_labels=True, G=G)
            return gt, lab
        gt = torch.zeros((B, G, 7), dtype=torch.float32)
        lab = torch.full((B, G), -1, dtype=torch.int64)
        for i, (b, l) in enumerate(zip(gt_boxes, gt_labels)):
            b = b.tensor if hasattr(b, "tensor") else b
            n = int(b.shape[0])
            if n > G:
                raise ValueError(f"scene {i} has {n} ground-truth boxes, the captured step holds {G}")
            if n:
                gt[i, :n] = b.detach().float().cpu()
                lab[i, :n] = l.detach().cpu()
            else:
                lab[i, 0] = 0
        return gt.to(device), lab.to(device)

    def _snapshot_state(self):
        """What a forward + backward WITHOUT an optimizer update still changes: BatchNorm running
        statistics / counters and the dropout counter.  (-> restore closure)"""
        bufs = [(b, b.clone()) for b in self.model.buffers()]
        rng = None
        if self.fused:
            from . import fused
            rng = fused.get_rng_state(self.flat.flat.device)
        if self._accumulate > 1:
            # ... and, inside a group, what the earlier passes have accumulated: the warm-up passes ADD their
            # gradients into the flat buffer (StepCache captures lazily, possibly at micro >= 1)
            bufs.append((self.flat.flat, self.flat.flat.clone()))
            if self._loss_acc is not None:
                bufs.append((self._loss_acc, self._loss_acc.clone()))
            if self.fused:
                bufs.append((self.opt.state, self.opt.state.clone()))

        def restore():
            for b, c in bufs:
                b.copy_(c)
            if rng is not None:
                from . import fused
                fused.set_rng_state(self.flat.flat.device, rng)
        return restore

    def capture(self, batch, warmup=3, prefetch_geometry=True, max_gt=None, dry=False, geo_pipe=None,
                update_in_graph=None, role=None):
        """Capture forward + loss + backward of ``batch`` (static shapes, device-resident inputs) into one
        hipGraph; returns a ``CapturedStep``: ``replay(next_points=None)`` = graph launch (+ the eager all-reduce /
        clip / AdamW where the update is not in the graph).  The path issues no host sync or host->device copy
        after warm-up (targets are batched, metas are cached), which is what makes it capturable.

        The graph reads STATIC input buffers owned by the returned object: ``replay.load(batch)`` copies another
        batch (same shapes; at most ``max_gt`` boxes per scene, default the largest count in the captured batch)
        into them and refreshes the cached per-image constants in place, so a training loop is

            replay = trainer.capture(batch_0)
            for k in range(steps):
                if k: replay.load(batch_k)
                loss = replay(next_points=batch_{k+1}["points"])

        Batches whose SHAPES differ (padded image size, point count, batch size) need their own graph:
        ``Trainer.bucketed()`` keeps one per shape.

        ``prefetch_geometry``: the coordinate-only pre-pass of the NEXT batch (every FPS level, the backbone ball
        queries, 3-NN - ``DeMFHotPath.index_geometry``) is issued on a side HIP stream in front of the current
        batch's graph, so the latency-bound FPS chain (B workgroups on 256 CUs) runs underneath the current step's
        forward instead of in front of the next step.  Every step still computes one full pre-pass; the graph reads
        it from static buffers that are refreshed by ONE ~6 MB multi-copy launch at the step boundary.  This is the
        only replay order: two slower ones (``DEMF_GEO_AT_BWD``, ``DEMF_GEO_TWO_DEEP``) were retired and are
        refused here, their figures are in DESIGN_LOG section 5.
        ``dry``: the warm-up passes run forward + backward only (no optimizer update) and the state they touch
        (BatchNorm running statistics, dropout counter) is restored afterwards - a capture in the middle of
        training leaves the model exactly as it found it.
        ``geo_pipe``: the pre-pass pipeline (``replay.geo``) of another capture with the same cloud shape
        (B, N, channels): both graphs then read the same index buffers and share one pipelined pre-pass.
        ``update_in_graph`` (default: on one rank, ``DEMF_GRAPH_UPDATE=0`` turns it off): gradient norm (taken by
        the gradient pack on its way), clip and AdamW are nodes of the graph too - the optimizer's step count /
        learning-rate factor / norm live on the device (FlatAdamW.state), so a replay is the WHOLE step and nothing
        eager follows it.  With more than one rank the collective sits between backward and update and stays an
        eager RCCL call (``DEMF_GRAPH_ALLREDUCE=1``: captured as well, where the runtime allows it).
        ``role`` (``accumulate`` > 1 only; default: from ``trainer.micro``): ``"accumulate"`` - the graph of a
        micro-step 0 .. W-2: forward + backward + ONE demf_multi_add pack (+ one demf_scalars_accum node with a
        meter); ``"last"`` - the graph of micro-step W-1: forward + backward + demf_multi_add_sumsq,
        demf_scalars_accum, demf_step_meter reading the accumulator, demf_adamw_state_f32, the clears.  With
        ``update_in_graph=False`` or more ranks the eager tail (norm, collective, meter, AdamW, clears) follows a
        ``"last"`` replay only.  A replay refuses to run when its role does not match ``trainer.micro`` or when
        ``accumulate`` has changed since the capture, and advances ``micro``.  Warm-up passes are always ``dry``
        with W > 1: they must not touch the open group."""
        world, stub, overlap = self.allreduce_config()
        role, dry, update_in_graph = _capture_plan(
            self._accumulate, self.micro, role, dry, update_in_graph, self.fused, world, stub, overlap,
            switches.env_int("DEMF_GRAPH_UPDATE"), switches.env_int("DEMF_GRAPH_ALLREDUCE"),
            {name for name in RETIRED_ORDERS if switches.env_on(name)})
        if role is not None:
            self._ensure_acc()
        step = CapturedStep(self, batch, max_gt, role, update_in_graph, world)
        dev = batch["points"].device
        side = self.side_stream if self.side_stream is not None else \
            (concurrent_stream() if dev.type == "cuda" else torch.cuda.Stream())
        if geo_pipe is not None:
            side = geo_pipe.side
        restore = self._snapshot_state() if dry else None
        self._warm_up(step.static, warmup, dry, role, side)
        if prefetch_geometry and hasattr(self.model, "index_geometry"):
            step.geo = self._geo_pipe(step.static["points"], geo_pipe, side)
        torch.cuda.synchronize()
        try:
            self._record(step)
        except Exception:
            if restore is not None and role is not None:
                restore()                 # (the warm-up passes added into the open group)
            if update_in_graph and world > 1:
                # the runtime refused to capture the collective: fall back to the eager update
                # (a second capture: the failed one left nothing behind)
                return self.capture(step.static, warmup=0, prefetch_geometry=prefetch_geometry, max_gt=max_gt,
                                    dry=dry, geo_pipe=step.geo if step.geo is not None else geo_pipe,
                                    update_in_graph=False, role=role)
            raise
        self.flat.finish_capture()
        if restore is not None:
            restore()
            torch.cuda.synchronize()
        self._graph = step.graph
        return step

    def _warm_up(self, batch, warmup, dry, role, side):
        """``warmup`` passes over the static inputs on the side stream: real steps, or forward + backward only."""
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            self.flat.mode = role
            try:
                for _ in range(warmup):
                    if dry:
                        self._fwd_bwd(batch)
                    else:
                        self.step(batch)
            finally:
                self.flat.mode = None
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()

    def _geo_pipe(self, points, geo_pipe, side):
        """The pre-pass pipeline of the static cloud ``points``: a new one, or ``geo_pipe`` adopted."""
        if geo_pipe is None:
            return _GeoPipe(self.model, points, side)
        if tuple(geo_pipe.static_pts.shape) != tuple(points.shape):
            raise ValueError("geo_pipe was built for clouds of shape %s, this batch has %s"
                             % (tuple(geo_pipe.static_pts.shape), tuple(points.shape)))
        # the shared index buffers must describe THIS batch's cloud while it is being captured
        # (values do not matter to a capture, but the eager bookkeeping of the replays assumes them)
        geo_pipe.ensure(torch.cuda.current_stream(), points, points)
        return geo_pipe

    def _record(self, step):
        """Forward + loss + backward of ``step``'s static inputs, and the update where it belongs to the graph,
        as ONE hipGraph."""
        in_graph = step.update_in_graph and step.role != "accumulate"
        self.flat.reserve_table()
        step.graph = torch.cuda.CUDAGraph()
        with self.flat.capturing(step.role, self.opt.state if in_graph and step.world == 1 else None), \
                _gc_paused(), torch.cuda.graph(step.graph):
            step.loss = self._fwd_bwd(step.static, step.geo.static_geo if step.geo is not None else None)
            if step.role is not None:
                self._accumulate_scalars()
            if in_graph:
                self._captured_update(step.world)
        # A metered step: the loss tensors the meter launch reads live in THIS graph's pool and belong to this
        # step (StepCache keeps several graphs alive; the trainer's own reference moves on with every forward).
        # In the graph, the captured launch holds their addresses; outside, the eager update gets them.
        step.scalars = self._loss_scalars if step.metered else None

    def capture_double(self, batch_a, batch_b, **kw):
        """Two captured steps over two sets of static input buffers (``DoubleBufferedStep``): the next batch is
        loaded into the idle set on an input stream WHILE the current step runs.  Not available with
        ``accumulate`` > 1 (it would need two sets per role)."""
        if self._accumulate > 1:
            raise RuntimeError("capture_double is not available with accumulate = %d > 1: use capture() per role "
                               "or bucketed()" % self._accumulate)
        return DoubleBufferedStep(self, batch_a, batch_b, **kw)

    def bucketed(self, **kw):
        """A step that keeps one captured graph per input SHAPE (``StepCache``)."""
        return StepCache(self, **kw)


def _flat_tensors(g):
    """Every tensor of the (nested) geometry structure, in a deterministic order."""
    if torch.is_tensor(g):
        return [g]
    if isinstance(g, dict):
        return [t for k in sorted(g) for t in _flat_tensors(g[k])]
    return [t for v in g for t in _flat_tensors(v)]


def _batch_tensors(batch):
    """Every tensor of a batch dict (points, pyramid maps / token dict, GT lists or padded GT)."""
    out = []

    def walk(v):
        if torch.is_tensor(v):
            out.append(v)
        elif hasattr(v, "tensor") and torch.is_tensor(v.tensor):
            out.append(v.tensor)
        elif isinstance(v, dict):
            for k, x in v.items():
                if k != "img_metas":
                    walk(x)
        elif isinstance(v, (list, tuple)):
            for x in v:
                walk(x)
    walk({k: v for k, v in batch.items() if k != "img_metas"})
    return out


class _Cloud:
    """Which cloud a set of index buffers describes.  Identity is the tensor OBJECT handed in (held
    here, so the caching allocator cannot hand its address to the next batch) plus its version
    counter; an address / shape tag would match a recycled buffer and silently pair new points with
    old indices."""
    __slots__ = ("t", "v")

    def __init__(self, t):
        self.t, self.v = t, t._version

    def holds(self, t):
        return self.t is t and self.v == t._version


class _GeoPipe:
    """The pipelined coordinate pre-pass of ONE cloud shape (B, N, channels): static index buffers that
    captured step graphs read, a small hipGraph that recomputes them for another cloud on a side stream
    (``DeMFHotPath.index_geometry``: every FPS level, ball queries + inverse lists, 3-NN, the head's seed
    FPS), and the one-launch refresh that moves a finished pre-pass into the static buffers.  Shared by
    every step graph captured for that cloud shape (graphs for different padded image sizes read the
    same index buffers)."""

    def __init__(self, model, points, side):
        from . import ops
        self.side = side
        self.static_geo = model.index_geometry(points)
        torch.cuda.synchronize()
        # the pre-pass is its own (small) hipGraph, replayed on the side stream: one launch
        # call instead of ~30, so the main graph is not held up behind host launch latency
        self.static_pts = points.clone()
        torch.cuda.synchronize()
        self.graph = torch.cuda.CUDAGraph()
        with _gc_paused(), torch.cuda.graph(self.graph, stream=side):
            fresh = _flat_tensors(model.index_geometry(self.static_pts))
        torch.cuda.synchronize()
        static_flat = _flat_tensors(self.static_geo)
        # one launch instead of one copy per index tensor (~30 of them)
        pairs = [(d, s) for d, s in zip(static_flat, fresh) if d.numel()]
        self.refresh = ops.MultiCopy([d for d, _ in pairs], [s for _, s in pairs])
        # Which cloud the static geometry buffers hold, which cloud's pre-pass sits in `fresh` (in flight or
        # finished; None: consumed) and which cloud static_pts holds: the captured one, three times.
        self.in_static = self.in_pts = _Cloud(points)
        self.in_fresh = None

    def take_fresh(self, main):
        """fresh -> static (one launch), after the pre-pass that filled `fresh` has finished."""
        main.wait_stream(self.side)
        self.refresh()
        self.in_static, self.in_fresh = self.in_fresh, None

    def launch_prepass(self, main, next_points):
        if next_points is not None:
            self.static_pts.copy_(next_points)
            self.in_pts = _Cloud(next_points)
        self.side.wait_stream(main)                # the cloud is in place, `fresh` has been consumed
        with torch.cuda.stream(self.side):
            self.graph.replay()
        self.in_fresh = self.in_pts

    def ensure(self, main, points, static_points=None):
        """Make the static index buffers describe ``points``: already there, taken from the finished /
        in-flight pre-pass (waiting for it), or recomputed here."""
        if self.in_static.holds(points) or (static_points is not None and self.in_static.holds(static_points)
                                            and points is static_points):
            return
        if self.in_fresh is not None and self.in_fresh.holds(points):
            self.take_fresh(main)
        else:
            # (an unrelated pre-pass in flight is left to finish; its result is dropped)
            self.launch_prepass(main, points)
            self.take_fresh(main)


class CapturedStep:
    """One captured training step (``Trainer.capture``): the static input buffers its hipGraph reads, ``load`` to
    fill them with another batch, and the call that runs it.  ``role`` / ``accumulate`` / ``update_in_graph`` /
    ``metered`` are what it was captured as, ``max_gt`` the ground-truth slots per scene (``None``: the targets
    came padded), ``geo`` the pre-pass pipeline (``None``: the graph computes its geometry itself), ``graph`` the
    hipGraph and ``loss`` the tensor every replay writes the step's loss into."""

    def __init__(self, trainer, batch, max_gt, role, update_in_graph, world):
        """Builds the static inputs out of ``batch``; the trainer warms up on them and sets ``geo``, ``graph``,
        ``loss`` and ``scalars`` (with a meter: the loss terms in the graph's pool)."""
        self.trainer, self.world = trainer, world
        self.role, self.accumulate, self.update_in_graph = role, trainer._accumulate, update_in_graph
        self.metered = trainer.meter is not None
        self.geo = self.graph = self.loss = self.scalars = None
        dev = batch["points"].device
        if isinstance(batch["gt_bboxes_3d"], (list, tuple)) and dev.type == "cuda":
            G = max_gt or max(1, max(int((b.tensor if hasattr(b, "tensor") else b).shape[0])
                                     for b in batch["gt_bboxes_3d"]))
            gt, lab = trainer.pad_targets(batch["gt_bboxes_3d"], batch["gt_labels_3d"], G, dev)
        else:
            G, gt, lab = None, batch["gt_bboxes_3d"], batch["gt_labels_3d"]
        self.max_gt = G
        feats = batch.get("img_features")            # None: a points-only batch - every image block is skipped
        self.has_image = feats is not None
        self.head = head = getattr(trainer.model, "pts_bbox_head", None) if feats is not None else None
        # A pyramid handed over as the reference's list of (B,C,H_l,W_l) maps: the captured step reads TOKENS
        # (channels-last rows, padding zeroed) from a static buffer, and ``load`` converts every new batch
        # straight out of the caller's maps into that buffer (one tiled-transpose launch) - instead of copying
        # the 152 MB pyramid into static maps and transposing those inside the graph.
        self.tok_static = tok = None
        if (feats is not None and not isinstance(feats, dict) and dev.type == "cuda" and hasattr(head, "pyramid_tokens")
                and switches.env_int("DEMF_ZERO_COPY_TOKENS")):
            self.tok_static = tok = head.pyramid_tokens(feats, batch["img_metas"])
        if feats is None:
            self.static = dict(points=batch["points"].clone(), gt_bboxes_3d=gt, gt_labels_3d=lab)
        else:
            self.static = dict(points=batch["points"].clone(),
                               img_features=(tok if tok is not None else
                                             dict(feats, tokens=feats["tokens"].clone())
                                             if isinstance(feats, dict) else [f.clone() for f in feats]),
                               img_metas=batch["img_metas"], gt_bboxes_3d=gt, gt_labels_3d=lab)
        if head is not None and hasattr(head, "pin_metas"):
            head.pin_metas(self.static["img_metas"])     # the graph holds raw pointers into its cache entry

    def __call__(self, next_points=None):
        """One training step behind the gradient-accumulation checks: the role this step was captured in must be
        the one ``trainer.micro`` asks for (last <=> micro == W-1) and ``accumulate`` must be what it was at the
        capture; nothing has been touched when it refuses.  Advances ``micro``.  ``next_points``: see ``_run``."""
        tr, W = self.trainer, self.accumulate
        if tr._accumulate != W:
            raise RuntimeError("this step was captured with accumulate = %d and the trainer now has accumulate "
                               "= %d: capture again" % (W, tr._accumulate))
        if self.role is None:
            return self._run(next_points)
        if (self.role == "last") != (tr.micro == W - 1):
            raise RuntimeError("this step was captured in the '%s' role and the trainer is at micro = %d of "
                               "accumulate = %d, which takes the '%s' role"
                               % (self.role, tr.micro, W, "last" if tr.micro == W - 1 else "accumulate"))
        tr._refuse_overlap()
        out = self._run(next_points)
        tr.micro = 0 if self.role == "last" else tr.micro + 1
        return out

    def _run(self, next_points):
        """``next_points`` is the cloud of the NEXT batch: its coordinate pre-pass is launched on the side stream
        in front of the step's graph (enqueueing the ~900-node graph takes the host about a millisecond) and runs
        underneath the forward; the result is moved into the static buffers at the end of the call.  Any other
        usage stays correct: ``load`` checks whether the static / in-flight geometry belongs to the very tensor
        object it is given (same object, same version) and otherwise recomputes it.  ``next_points=None``
        recomputes the pre-pass of the cloud last given (every step still pays for one full pre-pass)."""
        tr, geo = self.trainer, self.geo
        main = torch.cuda.current_stream()
        if (tr.meter is not None) != self.metered:
            raise RuntimeError("this step was captured %s a step meter and the trainer now has %s: capture again"
                               % (("with", "none") if self.metered else ("without", "one")))
        if self.update_in_graph:
            w_now, stub_now, _ = tr.allreduce_config()
            if w_now != self.world or stub_now:
                raise RuntimeError("this step was captured with its optimizer update inside the graph "
                                   "(world %d, no all-reduce stub); capture again with update_in_graph=False"
                                   % self.world)
        # the owed update - norm + AdamW behind an overlapped collective - goes in front of the pre-pass launch
        # (behind it the step measured 0.17 ms slower, profiles/r05_allreduce_overlap_probe.log).  This one call
        # serves the whole step: ``flush`` clears ``_pending_update`` and only ``_update`` below sets it again -
        # ``launch_prepass`` touches nothing of the trainer - so a second one in front of the graph would do nothing.
        tr.flush()
        if geo is not None and switches.env_on("DEMF_SKIP_GEO"):     # measurement only: the step alone
            self.graph.replay()
            self._update()
            return self.loss
        if geo is not None:
            geo.launch_prepass(main, next_points)
        self.graph.replay()
        self._update(defer=True)
        if geo is not None:
            geo.take_fresh(main)
        return self.loss

    def _update(self, defer=False):
        """The eager tail of a replay whose graph does not hold the update: collective, norm, meter, AdamW."""
        if not (self.update_in_graph or self.role == "accumulate"):
            self.trainer._update(defer, scalars=self.scalars)

    def load(self, new, skip_geo=False):
        """Copy another batch into the static input buffers of the captured step.  The captured forward reads its
        FPS / ball-query / 3-NN indices from the static geometry buffers; if they do not hold THIS cloud's
        geometry, it is fetched from the finished / in-flight pre-pass (waiting for it) or recomputed here, so
        geometry and targets can never belong to different batches.  ``skip_geo``: the caller has done that
        already (DoubleBufferedStep: on the main stream, while this call runs on its input stream)."""
        static, head, tok_static, G = self.static, self.head, self.tok_static, self.max_gt
        if self.geo is not None and not skip_geo:
            self.geo.ensure(torch.cuda.current_stream(), new["points"], static["points"])
        static["points"].copy_(new["points"])
        if ("img_features" in new) != self.has_image:
            raise ValueError("load(): the captured step %s an image pyramid, the new batch %s"
                             % (("has", "has none") if self.has_image else ("has no", "brings one")))
        nf = new.get("img_features")
        metas_done = nf is None
        if nf is None:
            pass
        elif tok_static is not None and not isinstance(nf, dict):
            # the padding mask the conversion zeroes by is the NEW batch's: constants first
            head.refresh_metas(static["img_metas"], new["img_metas"])
            metas_done = True
            if head.pyramid_tokens(nf, static["img_metas"], out=tok_static) is None:
                # (non-contiguous / non-fp32 maps or maps that require grad: the conversion did not run and
                # the static token buffer would silently keep the previous batch's image features)
                raise ValueError("load(): the new pyramid cannot be converted in place (it must be contiguous "
                                 "fp32 NCHW maps without requires_grad, as the captured batch's)")
        elif isinstance(nf, dict):
            if tok_static is not None and not nf.get("padding_zeroed"):
                raise ValueError("this step was captured on a pyramid of feature maps: load() takes maps "
                                 "(or tokens built by DeMFVoteHead.pyramid_tokens)")
            static["img_features"]["tokens"].copy_(nf["tokens"])
        else:
            for d, f in zip(static["img_features"], nf):
                d.copy_(f)
        if G is not None:
            nb = [b.tensor if hasattr(b, "tensor") else b for b in new["gt_bboxes_3d"]]
            if len(nb) <= 32 and all(b.is_cuda for b in nb) and all(l.is_cuda for l in new["gt_labels_3d"]):
                # device lists: padded straight into the static buffers (one launch, no copies)
                if max(int(b.shape[0]) for b in nb) > G:
                    raise ValueError("a scene has more ground-truth boxes than the captured step's %d slots" % G)
                from . import ops
                ops.pad_gt_lists(nb, list(new["gt_labels_3d"]), G,
                                 out=(static["gt_bboxes_3d"], static["gt_labels_3d"]))
            else:
                g2, l2 = self.trainer.pad_targets(new["gt_bboxes_3d"], new["gt_labels_3d"], G,
                                                  static["points"].device)
                static["gt_bboxes_3d"].copy_(g2)
                static["gt_labels_3d"].copy_(l2)
        else:
            static["gt_bboxes_3d"].copy_(new["gt_bboxes_3d"])
            static["gt_labels_3d"].copy_(new["gt_labels_3d"])
        if not metas_done and head is not None and hasattr(head, "refresh_metas"):
            head.refresh_metas(static["img_metas"], new["img_metas"])


class DoubleBufferedStep:
    """The captured step with DOUBLE-BUFFERED static inputs: two hipGraphs of the same step (same model, optimizer,
    pre-pass pipeline) reading two sets of static input buffers.  ``load(batch)`` fills the set the NEXT call will
    read, on an input stream, so the per-batch input path - the pyramid's conversion to tokens (63 us of HBM traffic),
    the copies of points / padded targets / constants - runs underneath the step in flight instead of between two
    steps (the host runs about one step ahead of the GPU, so ``load(k+1)`` is enqueued while step k executes).
    Same calling convention as ``Trainer.capture``'s replay:

        step = trainer.capture_double(batch_0, batch_1)
        for k in range(steps):
            if k: step.load(batch_k)            # k = 0: batch_0 is in place
            loss = step(next_points=batch_{k+1}["points"])

    Ordering: a set is overwritten only after the last step that read it has finished (event), and a step waits for
    its set's load (event).  The reference's loader does the same thing with pinned-memory prefetch threads
    (mmcv's DataLoader workers feeding MMDistributedDataParallel, /root/reference/train.py:140-147)."""

    def __init__(self, trainer, batch_a, batch_b, **kw):
        if "img_features" in batch_a and batch_a["img_metas"] is batch_b["img_metas"]:
            raise ValueError("capture_double: the two batches must carry their own img_metas objects (each set of "
                             "static buffers owns the device constants cached for its metas)")
        self.trainer = trainer
        first = trainer.capture(batch_a, **kw)
        kw2 = dict(kw)
        kw2.update(dry=True, geo_pipe=first.geo)
        second = trainer.capture(batch_b, **kw2)
        self.slots = [first, second]
        self.geo, self.max_gt = first.geo, first.max_gt
        self.input_stream = concurrent_stream()
        self.loaded = [None, None]           # event: the set's load has finished
        self.done = [None, None]             # event: the last step that read the set has finished
        self.nxt = 0                         # the set the next call replays (set 0 holds batch_a)
        # the shared pre-pass pipeline must describe batch_a's cloud for the first call
        if self.geo is not None:
            self.geo.ensure(torch.cuda.current_stream(), batch_a["points"])

    @property
    def static(self):
        return self.slots[self.nxt].static

    def load(self, new):
        s = self.nxt
        main = torch.cuda.current_stream()
        if self.slots[s].geo is not None:
            # geometry bookkeeping (normally a no-op: the pre-pass of this cloud was launched under the previous step
            # and moved into the static index buffers at its end) belongs to the main stream
            self.slots[s].geo.ensure(main, new["points"])
        ins = self.input_stream
        if self.done[s] is not None:
            ins.wait_event(self.done[s])
        else:
            ins.wait_stream(main)            # first use of the set: behind its capture
        # The tensors of ``new`` (H2D copies, image-stream outputs, GT lists) are normally produced on the
        # caller's current stream: the input stream must not read them before they are written, and the
        # caching allocator must not hand their memory out again while the input stream still reads it.
        ready = torch.cuda.Event()
        ready.record(main)
        ins.wait_event(ready)
        for t in _batch_tensors(new):
            if t.is_cuda:
                t.record_stream(ins)
        with torch.cuda.stream(ins):
            self.slots[s].load(new, skip_geo=True)
            ev = torch.cuda.Event()
            ev.record(ins)
        self.loaded[s] = ev

    def __call__(self, next_points=None):
        s = self.nxt
        main = torch.cuda.current_stream()
        if self.loaded[s] is not None:
            main.wait_event(self.loaded[s])
            self.loaded[s] = None
        out = self.slots[s](next_points=next_points)
        ev = torch.cuda.Event()
        ev.record(main)
        self.done[s] = ev
        self.nxt = 1 - s
        return out


class StepCache:
    """Training step over batches of VARYING shape: one captured hipGraph per shape key

        (scenes, points, point channels, image-pyramid shapes, GT slots)

    in an LRU of ``max_graphs``, an eager step for shapes seen fewer than ``capture_on`` times.  The
    reference rebuilds its masks and shapes per batch from ``img_metas[0]['batch_input_shape']``
    (demf/modeling/heads/class_agnostic_vote_head.py:556-568) and its pipeline pads every batch to a
    multiple of 32 after ``Resize((1333, 800), keep_ratio)`` (configs/demf/demf_votenet.py:194-197): SUN
    RGB-D's four sensors give four padded image sizes, so a single static-shape graph would only ever
    serve one of them.  GT slots are bucketed (8 / 16 / 32 / 64) so that box counts do not multiply the
    graphs.  Graphs of the same cloud shape share one pipelined coordinate pre-pass (``_GeoPipe``).
    Captures are ``dry``: they leave parameters, optimizer state, BatchNorm statistics and the dropout
    counter untouched, so the sequence of updates equals that of eager steps.

    With ``trainer.accumulate`` > 1 a call is one MICRO-step and the role it plays in its group ("accumulate" /
    "last", ``Trainer.capture``) joins the key: ``max_graphs`` still counts shapes, so up to ``2 * max_graphs``
    graphs live, and both graphs of a shape share its pre-pass pipeline.  A capture may fall in the middle of a
    group; being dry it leaves the group's accumulated gradients as they were.  ``captures`` records
    (shape key, role, micro) of every capture."""

    GT_BUCKETS = (8, 16, 32, 64)

    def __init__(self, trainer, max_graphs=4, capture_on=2, warmup=2, prefetch_geometry=True):
        import collections
        self.trainer, self.max_graphs, self.capture_on = trainer, int(max_graphs), int(capture_on)
        self.warmup, self.prefetch = int(warmup), prefetch_geometry
        self.graphs = collections.OrderedDict()       # key -> replay
        self.pipes = {}                               # cloud shape -> _GeoPipe
        self.seen = collections.Counter()
        self.stats = dict(eager=0, replayed=0, captured=0, evicted=0)
        self.captures = []                            # (shape key, role or None, trainer.micro) per capture

    @classmethod
    def gt_slots(cls, gt_boxes):
        if not isinstance(gt_boxes, (list, tuple)):
            return int(gt_boxes.shape[1])
        n = max(1, max(int((b.tensor if hasattr(b, "tensor") else b).shape[0]) for b in gt_boxes))
        for g in cls.GT_BUCKETS:
            if n <= g:
                return g
        raise ValueError("a scene has %d ground-truth boxes; the target kernels hold %d" % (n, cls.GT_BUCKETS[-1]))

    @classmethod
    def key(cls, batch):
        f = batch.get("img_features")
        if f is None:
            img = None                             # a points-only batch: the pyramid is no part of the shape
        elif isinstance(f, dict):
            img = (tuple(f["tokens"].shape), tuple(tuple(s) for s in f["spatial"]))
        else:
            img = tuple(tuple(t.shape) for t in f)
        return (tuple(batch["points"].shape), img, cls.gt_slots(batch["gt_bboxes_3d"]))

    def step(self, batch, next_points=None):
        """One optimizer step on ``batch``.  ``next_points``: the cloud of the next batch (its
        coordinate pre-pass then runs underneath this step if the next batch replays a graph of the
        same cloud shape)."""
        key = self.key(batch)
        tr = self.trainer
        role = None
        if tr.accumulate > 1:
            role = "last" if tr.micro == tr.accumulate - 1 else "accumulate"
        gkey = key if role is None else key + (role,)
        r = self.graphs.get(gkey)
        if r is not None and r.accumulate != tr.accumulate:
            raise RuntimeError("StepCache holds graphs captured with accumulate = %d and the trainer now has "
                               "accumulate = %d: build a new StepCache" % (r.accumulate, tr.accumulate))
        if r is None:
            self.seen[key] += 1
            if self.seen[key] < self.capture_on:
                self.stats["eager"] += 1
                return self.trainer.step(batch)
            # (room is counted in SHAPES: the graphs of the other role of this shape do not count against it)
            while key not in {k[:3] for k in self.graphs} and len({k[:3] for k in self.graphs}) >= self.max_graphs:
                oldest = next(iter(self.graphs))[:3]
                for old in [k for k in self.graphs if k[:3] == oldest]:
                    dead = self.graphs.pop(old)
                    self.stats["evicted"] += 1
                    # (the pipe - static index buffers + the pre-pass hipGraph - of a cloud shape survives while any
                    # graph of that shape does, INCLUDING the one about to be captured)
                    if old[0] != key[0] and not any(k[0] == old[0] for k in self.graphs):
                        self.pipes.pop(old[0], None)
                    head = getattr(self.trainer.model, "pts_bbox_head", None)
                    if head is not None and hasattr(head, "unpin_metas"):
                        head.unpin_metas(dead.static["img_metas"])
                    del dead
            pipe = self.pipes.get(key[0]) if self.prefetch else None
            self.captures.append((key, role, tr.micro))
            r = self.trainer.capture(batch, warmup=self.warmup, prefetch_geometry=self.prefetch,
                                     max_gt=key[2] if isinstance(batch["gt_bboxes_3d"], (list, tuple)) else None,
                                     dry=True, geo_pipe=pipe, role=role)
            if self.prefetch and r.geo is not None:
                self.pipes[key[0]] = r.geo
            self.graphs[gkey] = r
            self.stats["captured"] += 1
        else:
            self.graphs.move_to_end(gkey)
        r.load(batch)
        self.stats["replayed"] += 1
        if next_points is not None and tuple(next_points.shape) != key[0]:
            next_points = None                      # another cloud shape: its own pipeline fetches it
        return r(next_points=next_points)

    __call__ = step
