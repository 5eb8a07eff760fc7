"""Op dispatch layer.

Every hot op has two implementations:

  * ``nats_amd.ops.eager`` — plain PyTorch, runs on CPU (and GPU), serves as
    the numerics oracle for the HIP kernels (the Theano graph equations at
    nats.py:336-372, 498-572, 753-770 are the spec),
  * ``nats_amd.ops.hip`` (built from ``nats_amd/ops/hip/*.hip``) — the
    hand-written CDNA4 kernels used on MI355X.

Dispatch rule: CUDA tensors use the HIP kernels; if the extension is not
importable on a GPU machine the op RAISES (no silent eager fallback — set
``NATS_AMD_ALLOW_EAGER_GPU=1`` to override for debugging). CPU tensors use
eager. ``NATS_AMD_FORCE_EAGER=1`` forces eager everywhere (used in tests to
A/B the kernels).
"""

import os

import torch

from . import eager

_HIP = None
_HIP_TRIED = False


def _hip_ext():
    """Import the compiled HIP extension lazily (built in-tree by setup or
    __graft_entry__.build())."""
    global _HIP, _HIP_TRIED
    if not _HIP_TRIED:
        _HIP_TRIED = True
        try:
            from . import hip_ext as m  # thin loader module
            _HIP = m.load()
        except Exception:
            _HIP = None
    return _HIP


def _use_hip(*tensors):
    if os.environ.get("NATS_AMD_FORCE_EAGER"):
        return False
    if not any(t.is_cuda for t in tensors if isinstance(t, torch.Tensor)):
        return False
    ext = _hip_ext()
    if ext is None:
        if os.environ.get("NATS_AMD_ALLOW_EAGER_GPU"):
            return False
        raise RuntimeError(
            "nats_amd HIP extension is not built but tensors are on GPU. "
            "Run `python -c 'import __graft_entry__; __graft_entry__.build()'` "
            "or set NATS_AMD_ALLOW_EAGER_GPU=1 to run the (slow) eager path.")
    return True


def weights_version(params):
    """Monotone tag over ``params``, the key of every cache derived from
    weights (packed decoder operands, captured decode graphs): in-place
    torch updates bump tensor _version; updates through raw pointers (the
    fused adadelta kernel, graph replays) never do, so their callers
    advance an explicit epoch with ``bump_update_epoch``."""
    return tuple((p._version, getattr(p, "_nats_update_epoch", 0))
                 for p in params)


def bump_update_epoch(params):
    for p in params:
        p._nats_update_epoch = getattr(p, "_nats_update_epoch", 0) + 1


MAX_KERNEL_BATCH = 32  # MFMA M-tiling of the step kernels (2x 16-row tiles)


def _batch_chunks(B):
    return [(b0, min(b0 + MAX_KERNEL_BATCH, B))
            for b0 in range(0, B, MAX_KERNEL_BATCH)]


_CHUNK_STREAMS = {}


def _chunk_streams(device, n):
    """Per-device side streams for concurrent batch-chunk chains."""
    key = device.index or 0
    pool = _CHUNK_STREAMS.setdefault(key, [])
    while len(pool) < n:
        pool.append(torch.cuda.Stream(device=device))
    return pool[:n]


def _opt_slice(t, a, b, dim):
    return None if t is None else t.narrow(dim, a, b - a)


def _run_chunks(call, B, cat_dims, concurrent):
    """Batches beyond the kernels' 32-row MFMA tiling run as exact per-chunk
    passes (batch rows are independent): ``call(a, b)`` returns the tuple of
    outputs for rows [a, b); output i is concatenated along ``cat_dims[i]``.

    ``concurrent`` runs the chunks as chains on separate HIP streams: the
    per-step decoder kernels occupy a fraction of the chip each, and the
    chains are independent (autograd replays each backward on its recorded
    stream, so the reverse chains overlap too; for beam batches it doubles
    the serving micro-batch row budget)."""
    chunks = _batch_chunks(B)
    if concurrent:
        cur = torch.cuda.current_stream()
        streams = _chunk_streams(cur.device, len(chunks))
        outs = []
        for (a, b), s in zip(chunks, streams):
            s.wait_stream(cur)
            with torch.cuda.stream(s):
                outs.append(call(a, b))
        for s in streams:
            cur.wait_stream(s)
        for o in outs:
            for t in o:
                t.record_stream(cur)
    else:
        outs = [call(a, b) for a, b in chunks]
    return tuple(torch.cat([o[i] for o in outs], dim=d)
                 for i, d in enumerate(cat_dims))


def gru_scan(x_gates, x_cand, mask, U, Ux, h0=None):
    """GRU scan over time. Returns hidden states (T, B, H).

    Semantics: nats.py:336-372 (gru_layer step). ``x_gates``/``x_cand`` are
    the hoisted input projections x@W+b (T,B,2H) and x@Wx+bx (T,B,H).
    """
    if _use_hip(x_gates, U):
        from .gru import gru_scan_hip
        B = x_gates.shape[1]
        if B <= MAX_KERNEL_BATCH:
            return gru_scan_hip(x_gates, x_cand, mask, U, Ux, h0)
        return _run_chunks(lambda a, b: (gru_scan_hip(
            x_gates[:, a:b], x_cand[:, a:b], _opt_slice(mask, a, b, 1), U, Ux,
            _opt_slice(h0, a, b, 0)),), B, (1,), concurrent=False)[0]
    return eager.gru_scan(x_gates, x_cand, mask, U, Ux, h0)


def gru_scan_bidir(xg0, xc0, mask0, U0, Ux0, xg1, xc1, mask1, U1, Ux1):
    """Both encoder directions (independent scans) in one fused launch
    sequence on GPU; two eager scans on CPU. Returns (h_fwd, h_bwd)."""
    if _use_hip(xg0, U0):
        from .gru import gru_scan_bidir_hip
        B = xg0.shape[1]
        # the persistent scans take up to 64 rows natively (two 32-row
        # chunk jobs concurrent in one launch — same barrier count as 32)
        direct_max = MAX_KERNEL_BATCH
        if _hip_ext().gru_persistent_ok(U0.shape[0], 2 * MAX_KERNEL_BATCH):
            direct_max = 2 * MAX_KERNEL_BATCH
        if B <= direct_max:
            return gru_scan_bidir_hip(xg0, xc0, mask0, U0, Ux0, xg1, xc1,
                                      mask1, U1, Ux1)
        return _run_chunks(lambda a, b: gru_scan_bidir_hip(
            xg0[:, a:b], xc0[:, a:b], _opt_slice(mask0, a, b, 1), U0, Ux0,
            xg1[:, a:b], xc1[:, a:b], _opt_slice(mask1, a, b, 1), U1, Ux1),
            B, (1, 1), concurrent=False)
    return (eager.gru_scan(xg0, xc0, mask0, U0, Ux0),
            eager.gru_scan(xg1, xc1, mask1, U1, Ux1))


def cond_gru_scan(y_gates, y_cand, mask, init_state, ctx, ctx_mask, pctx, P):
    """Conditional-GRU decoder scan (training). Returns
    (h2s, ctxs, alphas, acc_ctx, acc_alpha).

    Semantics: nats.py:498-608 (gru_cond_layer scan path).
    """
    if _use_hip(y_gates, ctx):
        from .cond_gru import cond_gru_scan_hip
        B = y_gates.shape[1]
        if B <= MAX_KERNEL_BATCH:
            return cond_gru_scan_hip(y_gates, y_cand, mask, init_state, ctx,
                                     ctx_mask, pctx, P)
        return _run_chunks(lambda a, b: cond_gru_scan_hip(
            y_gates[:, a:b], y_cand[:, a:b], _opt_slice(mask, a, b, 1),
            init_state[a:b], ctx[:, a:b], _opt_slice(ctx_mask, a, b, 1),
            pctx[:, a:b], P), B, (1, 1, 1, 0, 0), concurrent=True)
    return eager.cond_gru_scan(y_gates, y_cand, mask, init_state, ctx,
                               ctx_mask, pctx, P)


def cond_gru_step(h_prev, x_g, x_c, ctx, ctx_mask, pctx, acc_ctx, acc_alpha, P):
    """One decoder step (beam search / sampler one_step path).

    Semantics: nats.py:592-594 with mask == all-ones.
    """
    if _use_hip(h_prev, ctx):
        from .cond_gru import cond_gru_step_hip
        B = h_prev.shape[0]
        if B <= MAX_KERNEL_BATCH:
            return cond_gru_step_hip(h_prev, x_g, x_c, ctx, ctx_mask, pctx,
                                     acc_ctx, acc_alpha, P)
        return _run_chunks(lambda a, b: cond_gru_step_hip(
            h_prev[a:b], x_g[a:b], x_c[a:b], ctx[:, a:b],
            _opt_slice(ctx_mask, a, b, 1), pctx[:, a:b], acc_ctx[a:b],
            acc_alpha[a:b], P), B, (0,) * 5, concurrent=True)
    return eager.cond_gru_step(h_prev, x_g, x_c, ctx, ctx_mask, pctx,
                               acc_ctx, acc_alpha, P)


def _row_src_table(row_src, R, S, device):
    """The row -> source-column table of cond_gru_step_shared as an int64
    tensor for index_select (CPU / eager) or an int32 device tensor for the
    kernel. A list or a CPU tensor is validated here (length R, entries in
    [0, S)) and uploaded in one copy; a device tensor is taken on trust:
    reading it would sync."""
    if torch.is_tensor(row_src):
        if row_src.dtype not in (torch.int32, torch.int64) or \
                row_src.dim() != 1:
            raise TypeError("cond_gru_step_shared: row_src must be a 1-d "
                            "integer tensor, got %s %s"
                            % (row_src.dtype, tuple(row_src.shape)))
        if row_src.is_cuda:
            if row_src.dtype != torch.int32:
                raise TypeError("cond_gru_step_shared: a device row_src must "
                                "be int32, got %s" % row_src.dtype)
            if row_src.shape[0] != R:
                raise ValueError("cond_gru_step_shared: row_src has %d "
                                 "entries for %d rows"
                                 % (row_src.shape[0], R))
            return row_src
        vals = row_src.tolist()
    else:
        vals = list(row_src)
        if any(isinstance(v, bool) or not isinstance(v, int) for v in vals):
            raise TypeError("cond_gru_step_shared: row_src entries must be "
                            "integers")
    if len(vals) != R:
        raise ValueError("cond_gru_step_shared: row_src has %d entries for "
                         "%d rows" % (len(vals), R))
    for v in vals:
        if not 0 <= v < S:
            raise ValueError("cond_gru_step_shared: row_src entry %d outside "
                             "[0, S=%d)" % (v, S))
    if device.type == "cuda":
        return torch.tensor(vals, dtype=torch.int32).to(device,
                                                        non_blocking=True)
    return torch.tensor(vals, dtype=torch.int64, device=device)


def cond_gru_step_shared(h_prev, x_g, x_c, ctx_src, ctx_mask_src, pctx_src,
                         row_src, acc_ctx, acc_alpha, P):
    """One decoder step against a context kept once per source: row r
    attends to column ``row_src[r]`` of ctx_src (Ts,S,C), ctx_mask_src
    (Ts,S) or None, pctx_src (Ts,S,A). Same returns and semantics as
    ``cond_gru_step`` on ``ctx_src[:, row_src]``, ``ctx_mask_src[:,
    row_src]``, ``pctx_src[:, row_src]``, without making those copies on
    the GPU, and bit for bit its results there.

    ``row_src``: a list or CPU int tensor (validated, one upload) or an
    int32 device tensor (taken on trust). ``ctx_src`` is best passed in
    bf16 (NatsModel.decode_context): the kernel then reads it in place;
    any other dtype is cast on every call.
    """
    R = h_prev.shape[0]
    if ctx_src.dim() != 3 or pctx_src.dim() != 3 or \
            pctx_src.shape[:2] != ctx_src.shape[:2]:
        raise ValueError("cond_gru_step_shared: ctx_src (Ts,S,C) and "
                         "pctx_src (Ts,S,A) disagree: %s %s"
                         % (tuple(ctx_src.shape), tuple(pctx_src.shape)))
    S = ctx_src.shape[1]
    if ctx_mask_src is not None and \
            tuple(ctx_mask_src.shape) != tuple(ctx_src.shape[:2]):
        raise ValueError("cond_gru_step_shared: ctx_mask_src must be (Ts,S)")
    tab = _row_src_table(row_src, R, S, h_prev.device)
    if _use_hip(h_prev, ctx_src):
        from .cond_gru import cond_gru_step_hip
        tab = tab.to(device=h_prev.device, dtype=torch.int32).contiguous()
        if R <= MAX_KERNEL_BATCH:
            return cond_gru_step_hip(h_prev, x_g, x_c, ctx_src, ctx_mask_src,
                                     pctx_src, acc_ctx, acc_alpha, P, tab)
        ctx_bf = ctx_src.to(torch.bfloat16).contiguous()  # once, not per chunk
        return _run_chunks(lambda a, b: cond_gru_step_hip(
            h_prev[a:b], x_g[a:b], x_c[a:b], ctx_bf, ctx_mask_src, pctx_src,
            acc_ctx[a:b], acc_alpha[a:b], P, tab[a:b]), R, (0,) * 5,
            concurrent=True)
    idx = tab.to(device=ctx_src.device, dtype=torch.int64)
    if ctx_src.dtype != pctx_src.dtype:
        # a context already rounded for the kernel (a shared-mode graph
        # stepper with the kernels switched off): eager runs in one dtype
        ctx_src = ctx_src.to(pctx_src.dtype)
    return eager.cond_gru_step_shared(h_prev, x_g, x_c, ctx_src,
                                      ctx_mask_src, pctx_src, idx, acc_ctx,
                                      acc_alpha, P)


def _autocast_bf16():
    return (torch.is_autocast_enabled("cuda")
            and torch.get_autocast_dtype("cuda") == torch.bfloat16)


def linear_bias(x, W, b):
    """x (..., K) @ W (K, N) + b (N,): the hoisted input projections and
    the training vocab projection.

    Under bf16 autocast on GPU the result is bf16: the value
    ``(x @ W + b).to(bfloat16)``, which is what the scan and softmax
    kernels round the fp32 sum to anyway, from one bias+round pass over the
    GEMM output; the backward column-sums the bf16 gradient in place.
    Everywhere else this is the plain expression.
    """
    if _use_hip(x, W) and _autocast_bf16():
        from .io_fusion import linear_bias_hip
        return linear_bias_hip(x, W, b)
    return eager.linear_bias(x, W, b)


def encoder_head(h_f, h_r, x_mask, Wc_att, b_att):
    """Context assembly after the last encoder layer, for training:
    (ctx (T,B,2H) = [h_f | flip(h_r)], ctx_mean (B,2H), pctx (T,B,A)).
    ``h_r`` is in the reverse scan's own time order.

    Under bf16 autocast on GPU ctx is returned in bf16 (the only form the
    decoder scan and the key projection read) from one pass over the scan
    outputs, and the backward sums the three gradient terms of ctx
    straight into the tensors the scan backward consumes. ctx_mean is
    torch's own fp32 reduction, bit for bit the value of the expression.
    """
    if _use_hip(h_f, Wc_att) and _autocast_bf16():
        from .io_fusion import encoder_head_hip
        return encoder_head_hip(h_f, h_r, x_mask, Wc_att, b_att)
    return eager.encoder_head(h_f, h_r, x_mask, Wc_att, b_att)


def embed_gather(Wemb, ids, shift=False):
    """Embedding gather, optionally fused with the decoder's
    shift-right-by-one (BOS row = zeros). Semantics: nats.py:700-701
    (plain) and 730-734 (shifted target embedding).
    """
    if (Wemb.dtype == torch.float32
            and not os.environ.get("NATS_EMBED_EAGER")
            and _use_hip(Wemb)):
        from .embed import embed_gather_hip
        return embed_gather_hip(Wemb, ids, shift=shift)
    emb = Wemb[ids.clamp_min(0)]
    if shift and ids.dim() == 2:
        shifted = torch.zeros_like(emb)
        shifted[1:] = emb[:-1]
        return shifted
    return emb


BEAM_SELECT_MAX_K = 32  # winners a selection block keeps (beam_select.hip)


def _host_ints(t):
    """Values of a segment table the host can read for free: a list, or a
    CPU tensor. None for a device tensor (reading it would sync)."""
    if not torch.is_tensor(t):
        return [int(v) for v in t]
    if t.dtype != torch.int32 or t.dim() != 1:
        raise TypeError("beam_select: seg_off and want must be 1-d int32, "
                        "got %s %s" % (t.dtype, tuple(t.shape)))
    return None if t.is_cuda else t.tolist()


def beam_select(probs, prev_cost, seg_off, want, penalty=None, use_unk=True,
                K=None):
    """Per-sentence beam candidate selection in one call: the ``want[s]``
    smallest ``(prev_cost[r] - log(probs[r, w])) + penalty[r]`` over the
    rows ``[seg_off[s], seg_off[s+1])`` of sentence ``s``, ascending, ties
    to the lower flat index ``local_row*V + w``, NaN after +inf.

    probs (R,V) fp32 contiguous; prev_cost (R,) fp32; seg_off (S+1,) and
    want (S,) int32; penalty (R,) fp32 or None. ``seg_off``/``want`` may be
    lists or CPU tensors (validated here, then moved to ``probs.device`` in
    one copy) or tensors already on the device; the latter cannot be read
    without a sync, so ``K = max(want)`` must then be passed and the caller
    vouches for ``1 <= want[s] <= min(K, live_s*V)`` and ``live_s*V < 2**31``.

    Returns (ranks (S,K) int64, -1 beyond want[s]; costs (S,K) fp32, +inf
    beyond want[s]). costs are the UN-reranked candidate costs, recomputed
    from prev_cost and probs (nats.py:1004 cand_flat[ranks]).
    Semantics: nats.py:1001-1004 per sentence; use_unk=False pins word 1 to
    log-probability log(1e-20).
    """
    if probs.dim() != 2 or probs.dtype != torch.float32:
        raise TypeError("beam_select: probs must be (R, V) float32, got %s %s"
                        % (probs.dtype, tuple(probs.shape)))
    R, V = probs.shape
    for name, t in (("prev_cost", prev_cost), ("penalty", penalty)):
        if t is not None and (t.dtype != torch.float32 or t.shape != (R,)):
            raise TypeError("beam_select: %s must be (R,) float32, got %s %s"
                            % (name, t.dtype, tuple(t.shape)))
    offs, wants = _host_ints(seg_off), _host_ints(want)
    S = len(want)
    if len(seg_off) != S + 1 or S < 1:
        raise ValueError("beam_select: seg_off must have len(want)+1 entries")
    if K is None:
        if wants is None:
            raise ValueError("beam_select: pass K=max(want) when want is a "
                             "device tensor (deriving it would sync)")
        K = max(wants)
    K = int(K)
    if K > BEAM_SELECT_MAX_K:
        raise ValueError("beam_select: K=%d exceeds the kernel's %d winners "
                         "per sentence" % (K, BEAM_SELECT_MAX_K))
    if offs is not None:
        if offs[0] != 0 or offs[-1] != R:
            raise ValueError("beam_select: seg_off must run from 0 to R=%d"
                             % R)
        for s in range(S):
            live = offs[s + 1] - offs[s]
            if live < 0 or live * V >= 2 ** 31:
                raise ValueError("beam_select: sentence %d has %d x %d "
                                 "candidates; the flat index needs live*V "
                                 "in [0, 2**31)" % (s, live, V))
    if wants is not None:
        for s in range(S):
            if not 1 <= wants[s] <= K:
                raise ValueError("beam_select: want[%d]=%d outside [1, K=%d]"
                                 % (s, wants[s], K))
            if offs is not None and wants[s] > (offs[s + 1] - offs[s]) * V:
                raise ValueError("beam_select: want[%d]=%d exceeds the "
                                 "sentence's %d candidates" % (
                                     s, wants[s],
                                     (offs[s + 1] - offs[s]) * V))
    if not probs.is_contiguous():
        raise ValueError("beam_select: probs must be contiguous (row stride "
                         "V)")
    if _use_hip(probs):
        if offs is not None and wants is not None:
            tab = torch.tensor(offs + wants, dtype=torch.int32).to(
                probs.device, non_blocking=True)
            seg_off, want = tab[:S + 1], tab[S + 1:]
        else:
            seg_off = torch.as_tensor(seg_off, dtype=torch.int32,
                                      device=probs.device)
            want = torch.as_tensor(want, dtype=torch.int32,
                                   device=probs.device)
        ranks, costs = _hip_ext().beam_select(
            probs, prev_cost.contiguous(), seg_off.contiguous(),
            want.contiguous(),
            None if penalty is None else penalty.contiguous(), K,
            bool(use_unk), eager.NEG_UNK)
        return ranks, costs
    return eager.beam_select(probs, prev_cost, seg_off, want, penalty,
                             use_unk, K)


BEAM_REORDER_MAX_BUFFERS = 4  # pointer slots of ReorderArgs (beam_reorder.hip)


def _reorder_table(table, L_max, n_prev, device):
    """The (3, L) int64 [parent | word | sentence] table of beam_reorder on
    ``device``. A nested list or a CPU integer tensor is validated and
    uploaded in one copy; an int64 device tensor is taken on trust (reading
    it would sync)."""
    op = "beam_reorder"
    if torch.is_tensor(table):
        if table.dtype not in (torch.int32, torch.int64) or \
                table.dim() != 2 or table.shape[0] != 3:
            raise TypeError("%s: table must be a (3, L) integer tensor, got "
                            "%s %s" % (op, table.dtype, tuple(table.shape)))
        if table.is_cuda:
            if table.dtype != torch.int64:
                raise TypeError("%s: a device table must be int64, got %s"
                                % (op, table.dtype))
            if not 1 <= table.shape[1] <= L_max:
                raise ValueError("%s: L=%d rows outside [1, Rmax=%d]"
                                 % (op, table.shape[1], L_max))
            return table.contiguous()
        rows = table.tolist()
    else:
        rows = [list(r) for r in table]
        if len(rows) != 3 or len({len(r) for r in rows}) != 1:
            raise ValueError("%s: table must be three rows of one length "
                             "[parent | word | sentence]" % op)
        if any(isinstance(v, bool) or not isinstance(v, int)
               for r in rows for v in r):
            raise TypeError("%s: table entries must be integers" % op)
    L = len(rows[0])
    if not 1 <= L <= L_max:
        raise ValueError("%s: L=%d rows outside [1, Rmax=%d]"
                         % (op, L, L_max))
    for r in range(L):
        if not 0 <= rows[0][r] < n_prev:
            raise ValueError("%s: parent[%d]=%d outside the previous step's "
                             "%d rows" % (op, r, rows[0][r], n_prev))
        if rows[1][r] < -1:
            raise ValueError("%s: word[%d]=%d below -1"
                             % (op, r, rows[1][r]))
        if rows[2][r] < 0:
            raise ValueError("%s: sentence[%d]=%d is negative"
                             % (op, r, rows[2][r]))
    return torch.tensor(rows, dtype=torch.int64).to(device,
                                                    non_blocking=True)


def _byte_range(t):
    return t.data_ptr(), t.data_ptr() + t.numel() * t.element_size()


def beam_reorder(table, src, dst, y_out, route_out, n_prev=None):
    """Move the beam rows the host selected from a decode step's outputs
    into the next step's input buffers, in one call (one kernel launch on
    the GPU): for r < L ``dst_j[r] = src_j[parent[r]]``, ``y_out[r] =
    word[r]``, ``route_out[r] = sentence[r]``; every row ``L <= r < Rmax``
    becomes a copy of the new row 0 (the padding rule of the decode
    steppers).

    table (3, L) = [parent | word | sentence], 1 <= L <= Rmax: a nested list
    or CPU integer tensor (validated: parent in [0, n_prev), word >= -1,
    sentence >= 0; one upload) or an int64 device tensor (taken on trust; a
    parent outside [0, n_prev) is never dereferenced: that row's dst_j
    become NaN, its y_out and route_out 0). src: up to four (>= n_prev, D_j)
    fp32 contiguous tensors, n_prev defaults to ``src[0].shape[0]``; dst:
    the matching (Rmax, D_j) fp32 contiguous buffers, none overlapping a
    src; y_out (Rmax,) int64; route_out (Rmax,) int64 or int32.

    Returns the table as the (3, L) int64 tensor on the buffers' device:
    its row 0 is the ``parent`` of RerankHistory.step.
    """
    op = "beam_reorder"
    src, dst = tuple(src), tuple(dst)
    if not 1 <= len(src) <= BEAM_REORDER_MAX_BUFFERS or len(dst) != len(src):
        raise ValueError("%s: need 1 to %d src buffers and as many dst "
                         "buffers, got %d and %d" % (
                             op, BEAM_REORDER_MAX_BUFFERS, len(src),
                             len(dst)))
    for name, t in (("y_out", y_out), ("route_out", route_out)):
        if (not torch.is_tensor(t) or t.dim() != 1 or t.dtype not in
                ((torch.int64,) if name == "y_out"
                 else (torch.int64, torch.int32))):
            raise TypeError("%s: %s must be a 1-d int64%s tensor, got %s %s"
                            % (op, name,
                               "" if name == "y_out" else " or int32",
                               getattr(t, "dtype", type(t)),
                               tuple(getattr(t, "shape", ()))))
        if not t.is_contiguous():
            raise ValueError("%s: %s must be contiguous" % (op, name))
    Rmax, device = y_out.shape[0], y_out.device
    if route_out.shape[0] != Rmax:
        raise ValueError("%s: route_out has %d entries, y_out %d"
                         % (op, route_out.shape[0], Rmax))
    for j, (s, d) in enumerate(zip(src, dst)):
        for name, t in (("src", s), ("dst", d)):
            if (not torch.is_tensor(t) or t.dtype != torch.float32
                    or t.dim() != 2):
                raise TypeError("%s: %s[%d] must be a 2-d float32 tensor, "
                                "got %s %s" % (
                                    op, name, j, getattr(t, "dtype", type(t)),
                                    tuple(getattr(t, "shape", ()))))
            if not t.is_contiguous():
                raise ValueError("%s: %s[%d] must be contiguous"
                                 % (op, name, j))
            if t.device != device:
                raise ValueError("%s: %s[%d] is on %s, y_out on %s"
                                 % (op, name, j, t.device, device))
        if s.shape[1] != d.shape[1] or s.shape[1] < 1:
            raise ValueError("%s: src[%d] %s and dst[%d] %s disagree in row "
                             "width" % (op, j, tuple(s.shape), j,
                                        tuple(d.shape)))
        if d.shape[0] != Rmax:
            raise ValueError("%s: dst[%d] has %d rows, y_out %d"
                             % (op, j, d.shape[0], Rmax))
    n_prev = src[0].shape[0] if n_prev is None else int(n_prev)
    if n_prev < 1 or any(s.shape[0] < n_prev for s in src):
        raise ValueError("%s: n_prev=%d does not fit src buffers of %s rows"
                         % (op, n_prev, [s.shape[0] for s in src]))
    for j, s in enumerate(src):
        s0, s1 = _byte_range(s)
        for i, d in enumerate(dst):
            d0, d1 = _byte_range(d)
            if s0 < d1 and d0 < s1:
                raise ValueError("%s: src[%d] and dst[%d] overlap: rows "
                                 "would be read after they are written"
                                 % (op, j, i))
    if route_out.device != device or (torch.is_tensor(table) and table.is_cuda
                                      and table.device != device):
        raise ValueError("%s: table, y_out and route_out must share the "
                         "buffers' device" % op)
    table = _reorder_table(table, Rmax, n_prev, device)
    if _use_hip(y_out, *dst):
        _hip_ext().beam_reorder(table, list(src), list(dst), y_out,
                                route_out, n_prev)
    else:
        eager.beam_reorder(table, src, dst, y_out, route_out, n_prev)
    return table


def softmax_xent(logits, targets):
    """Per-position NLL of a softmax over the vocabulary.

    logits (N, V) float, targets (N,) int64 -> (N,) float32.
    Semantics: nats.py:763-768 (softmax + categorical_crossentropy).
    """
    if _use_hip(logits):
        from .softmax_ce import softmax_xent_hip
        return softmax_xent_hip(logits, targets)
    return eager.softmax_xent(logits, targets)


# paged distraction-rerank histories (ops defined next to their container)
from .rerank import (RerankHistory, rerank_advance,  # noqa: E402,F401
                     rerank_penalties_paged)
