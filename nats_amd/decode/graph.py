"""hipGraph-captured beam-decode step.

The reference's beam loop calls a compiled f_next per step (nats.py:960);
our f_next is itself a chain of ~15 kernel launches (embedding, fused
cond-GRU step, readout GEMMs, softmax). Capturing that chain into a
hipGraph (torch.cuda.CUDAGraph on ROCm) collapses per-step launch
overhead into one graph replay.

Shapes are static: the stepper is captured for a fixed (row budget, source
length Ts); the beam keeps that many rows alive (dead/padded rows carry
copies of row 0, harmless — callers slice [:live]). Host-side feedback
between replays (parent gather after rank selection) writes the static
input buffers with index copies.

Both steppers have a ``shared_ctx`` mode: the context is kept once per
source, rounded to bf16 when it is set, and the captured f_next reads it
through a static int32 row -> source table (ops.cond_gru_step_shared), so
no per-row copy of ctx / pctx / mask exists inside or outside the graph.
"""

import weakref

import torch

from ..ops import weights_version

_STEPPER_CACHE = weakref.WeakKeyDictionary()
_MAX_PER_FAMILY = 8


def _cached_stepper(cls, model, shape, context, rows, **mode):
    """One stepper of class ``cls`` per (model, shape): the captured graph
    is reused across inputs of the same shape — a hit only refreshes the
    static context buffers. Packed weights are baked into the graph at
    capture (ops/cond_gru.py _step_packed), so any weight update drops
    every stepper of the model. Capture memory is bounded per class: the
    oldest of its steppers makes room for a new shape."""
    ver = weights_version(model.P.values())
    per_model = _STEPPER_CACHE.setdefault(model, {})
    if per_model.get("__ver__") != ver:
        per_model.clear()
        per_model["__ver__"] = ver
    key = (cls,) + shape
    st = per_model.get(key)
    if st is None:
        family = [kk for kk in per_model if kk[0] is cls]
        if len(family) >= _MAX_PER_FAMILY:
            per_model.pop(family[0])
        st = per_model[key] = cls(model, *context, rows, **mode)
    else:
        st.set_context(*context)
    return st


def get_stepper(model, ctx0, pctx0, k, shared_ctx=False):
    """Cached GraphDecodeStepper per (model, Ts, k, shared_ctx)."""
    return _cached_stepper(GraphDecodeStepper, model,
                           (int(ctx0.shape[0]), int(k), bool(shared_ctx)),
                           (ctx0, pctx0), k, shared_ctx=bool(shared_ctx))


def get_batched_stepper(model, ctx_pad, ctx_mask, pctx_pad, R,
                        shared_ctx=False):
    """Cached BatchedGraphStepper per (model, Ts, S, R, shared_ctx) —
    reused across same-shaped micro-batches (serving)."""
    return _cached_stepper(
        BatchedGraphStepper, model,
        (int(ctx_pad.shape[0]), int(ctx_pad.shape[1]), int(R),
         bool(shared_ctx)),
        (ctx_pad, ctx_mask, pctx_pad), R, shared_ctx=bool(shared_ctx))


class _GraphStepper:
    """Replayable f_next (argmax/beam mode, no sampling) over a static
    budget of ``rows`` hypothesis rows. Subclasses own the context buffers,
    refresh them in ``set_context`` and call f_next in ``_run``; they list
    the static per-row input buffers, in ``step`` argument order, in
    ``self.inputs``."""

    def __init__(self, model, rows, Ts, C, device):
        self.model = model
        self.rows = rows
        H = model.options["dim"]
        self.y_in = torch.zeros(rows, dtype=torch.int64, device=device)
        self.state_in = torch.zeros(rows, H, device=device)
        self.accC_in = torch.zeros(rows, C, device=device)
        self.accA_in = torch.zeros(rows, Ts, device=device)
        self.inputs = (self.y_in, self.state_in, self.accC_in, self.accA_in)
        self.graph = None
        self.outs = None

    def capture(self):
        # warmup (allocator + kernels) on a side stream, then capture
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(2):
                self._run()
        torch.cuda.current_stream().wait_stream(s)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            outs = self._run()
            # keep stable output storage across replays
            self.outs = tuple(o.clone() if isinstance(o, torch.Tensor) else o
                              for o in outs)
        return self

    def step(self, *values):
        """One decode step for live = len(values[0]) (<= rows) hypothesis
        rows, one value per buffer of ``self.inputs``; returns (probs,
        state, alpha, ctx_t, acc_ctx, acc_alpha), each ``rows`` rows —
        callers slice [:live]."""
        _fill_rows(self.inputs, values, self.rows)
        return self.replay()

    def replay(self, live=None):
        """Replay the captured graph on the input buffers as they stand
        (``step`` or ops.beam_reorder wrote them); captures on first use.
        Same returns as ``step``. ``live`` is not needed here: all ``rows``
        rows run (RowStepper, the graph-less twin, runs the live ones)."""
        if self.graph is None:
            self.capture()
        self.graph.replay()
        probs, _, h2, alpha, ctx_t, accC, accA = self.outs
        return probs, h2, alpha, ctx_t, accC, accA


def _fill_rows(inputs, values, rows):
    """Write ``values`` (live rows each) into the static buffers and pad the
    tail with copies of row 0."""
    live = values[0].shape[0]
    for buf, v in zip(inputs, values):
        buf[:live] = v
    if live < rows:
        for buf, v in zip(inputs, values):
            buf[live:] = v[0]


class GraphDecodeStepper(_GraphStepper):
    """Single-sentence beam: step(y, state, acc_ctx, acc_alpha) against the
    sentence's context expanded to all k rows, no mask. ``shared_ctx``: the
    context stays (Ts,1,C) in bf16 and all k rows read its one column."""

    def __init__(self, model, ctx0, pctx0, k, shared_ctx=False):
        """ctx0 (Ts,1,C), pctx0 (Ts,1,A) from f_init/project_ctx."""
        Ts, _, C = ctx0.shape
        super().__init__(model, k, Ts, C, ctx0.device)
        self.shared_ctx = shared_ctx
        if shared_ctx:
            self.ctx = ctx0.to(torch.bfloat16).contiguous().clone()
            self.pctx = pctx0.float().contiguous().clone()
            self.row_src = torch.zeros(k, dtype=torch.int32,
                                       device=ctx0.device)
        else:
            self.ctx = ctx0.expand(Ts, k, C).contiguous()
            self.pctx = pctx0.expand(Ts, k, pctx0.shape[2]).contiguous()
            self.row_src = None

    def set_context(self, ctx0, pctx0):
        """Refresh the static context buffers for a new source sequence
        (same Ts) without recapturing the graph."""
        self.ctx.copy_(ctx0.expand_as(self.ctx))
        self.pctx.copy_(pctx0.expand_as(self.pctx))

    def _run(self):
        return self.model.f_next(self.y_in, self.ctx, None, self.pctx,
                                 self.state_in, self.accC_in, self.accA_in,
                                 sample_draw=False, row_src=self.row_src)


class BatchedGraphStepper(_GraphStepper):
    """Batched multi-sentence beam (decode/batched.py — the production
    serving path): step(sent_idx, y, state, acc_ctx, acc_alpha) with a
    static row budget R (= S*k). The per-step context gather
    ctx_pad[:, sent_idx] happens INSIDE the graph from a static sent_idx
    buffer, so hypothesis->sentence routing changes never force
    recapture. ``shared_ctx``: no gather at all — ctx_pad is held in bf16
    and ``step`` writes its sent_idx argument into ``row_src``, the static
    int32 row -> source table the attention kernel reads the per-sentence
    context through (``sent_idx``, the gather's int64 buffer, is then
    None)."""

    def __init__(self, model, ctx_pad, ctx_mask, pctx_pad, R,
                 shared_ctx=False):
        Ts, S, C = ctx_pad.shape
        super().__init__(model, R, Ts, C, ctx_pad.device)
        self.shared_ctx = shared_ctx
        # own the static buffers (a caller's tensor may alias freed memory
        # by the next micro-batch)
        if shared_ctx:
            self.ctx_pad = ctx_pad.to(torch.bfloat16).contiguous().clone()
        else:
            self.ctx_pad = ctx_pad.contiguous().clone()
        self.ctx_mask = ctx_mask.float().contiguous().clone()
        self.pctx_pad = pctx_pad.float().contiguous().clone() if shared_ctx \
            else pctx_pad.contiguous().clone()
        # step() writes the caller's sent_idx into this buffer; in shared
        # mode it is the kernel's int32 row -> source table (the write
        # converts)
        self.sent_idx = self.row_src = None
        if shared_ctx:
            self.row_src = torch.zeros(R, dtype=torch.int32,
                                       device=ctx_pad.device)
            self.inputs = (self.row_src,) + self.inputs
        else:
            self.sent_idx = torch.zeros(R, dtype=torch.int64,
                                        device=ctx_pad.device)
            self.inputs = (self.sent_idx,) + self.inputs

    def set_context(self, ctx_pad, ctx_mask, pctx_pad):
        self.ctx_pad.copy_(ctx_pad)
        self.ctx_mask.copy_(ctx_mask)
        self.pctx_pad.copy_(pctx_pad)

    def resident_buffers(self):
        """What ops.beam_reorder writes between two ``replay`` calls:
        ((state_in, accC_in, accA_in), y_in, route buffer), the route
        buffer being ``sent_idx`` (int64) or, in shared mode, ``row_src``
        (int32)."""
        return self.inputs[2:], self.y_in, self.inputs[0]

    def _run(self):
        if self.shared_ctx:
            return self.model.f_next(self.y_in, self.ctx_pad, self.ctx_mask,
                                     self.pctx_pad, self.state_in,
                                     self.accC_in, self.accA_in,
                                     sample_draw=False,
                                     row_src=self.row_src)
        ctx_b = self.ctx_pad.index_select(1, self.sent_idx)
        cmask_b = self.ctx_mask.index_select(1, self.sent_idx)
        pctx_b = self.pctx_pad.index_select(1, self.sent_idx)
        return self.model.f_next(self.y_in, ctx_b, cmask_b, pctx_b,
                                 self.state_in, self.accC_in, self.accA_in,
                                 sample_draw=False)


class RowStepper:
    """BatchedGraphStepper without the graph (CPU, or use_graph=False), for
    the resident-state decode: a plain holder of the same per-row buffers,
    with the same ``step`` / ``replay`` / ``resident_buffers``. f_next runs
    on the ``[:live]`` views, uncaptured, against the caller's context
    (not copied: the holder lives for one decode). ``shared_ctx``: ctx /
    ctx_mask / pctx are NatsModel.decode_context's per-source operands and
    the route buffer is the int32 row -> source table."""

    def __init__(self, model, ctx, ctx_mask, pctx, R, shared_ctx=False):
        Ts, _, C = ctx.shape
        device = ctx.device
        self.model = model
        self.rows = R
        self.shared_ctx = shared_ctx
        self.ctx, self.ctx_mask, self.pctx = ctx, ctx_mask, pctx
        self.route = torch.zeros(
            R, dtype=torch.int32 if shared_ctx else torch.int64,
            device=device)
        self.y_in = torch.zeros(R, dtype=torch.int64, device=device)
        self.state_in = torch.zeros(R, model.options["dim"], device=device)
        self.accC_in = torch.zeros(R, C, device=device)
        self.accA_in = torch.zeros(R, Ts, device=device)
        self.inputs = (self.route, self.y_in, self.state_in, self.accC_in,
                       self.accA_in)

    def resident_buffers(self):
        return self.inputs[2:], self.y_in, self.route

    def step(self, *values):
        """Fill the buffers from (sent_idx, y, state, acc_ctx, acc_alpha)
        and run the step; returns ``replay``'s six outputs."""
        _fill_rows(self.inputs, values, self.rows)
        return self.replay(values[0].shape[0])

    def replay(self, live):
        """f_next on the first ``live`` rows of the buffers as they stand:
        (probs, state, alpha, ctx_t, acc_ctx, acc_alpha), ``live`` rows
        each, none of them a view of a buffer."""
        route = self.route[:live]
        # the step kernels update fp32 contiguous accumulators in place:
        # they get copies, so that ops.beam_reorder can read the outputs
        # while it writes the buffers
        args = (self.state_in[:live], self.accC_in[:live].clone(),
                self.accA_in[:live].clone())
        if self.shared_ctx:
            outs = self.model.f_next(
                self.y_in[:live], self.ctx, self.ctx_mask, self.pctx, *args,
                sample_draw=False, row_src=route)
        else:
            outs = self.model.f_next(
                self.y_in[:live], self.ctx[:, route], self.ctx_mask[:, route],
                self.pctx[:, route], *args, sample_draw=False)
        probs, _, h2, alpha, ctx_t, accC, accA = outs
        return probs, h2, alpha, ctx_t, accC, accA
