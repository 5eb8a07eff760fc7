"""Paged distraction-rerank histories for batched beam decode.

A beam's history is a tree: the hypotheses that continue one row share that
row's whole past. So every decode step's rows are stored once, in slabs
``hist_* (Tmax, Rmax, dim)`` that are never moved, and a small int32
ancestor table ``anc (Tmax, Rmax)`` says, for each current batch row ``r``
and each earlier step ``t``, which slot of ``hist_*[t]`` is row ``r``'s
history entry. A reshuffle of the beam rewrites only that table
(``rerank_advance``); the penalties of all rows of all sentences come from
one call (``rerank_penalties_paged``, kernels in hip/rerank.hip).
"""

import torch

from . import _hip_ext, _use_hip, eager


def _check_tables(op, *tables):
    for t in tables:
        if (not torch.is_tensor(t) or t.dtype != torch.int32
                or t.dim() != 2):
            raise TypeError("%s: ancestor tables must be (Tmax, Rmax) int32 "
                            "tensors, got %s %s" % (
                                op, getattr(t, "dtype", type(t)),
                                tuple(getattr(t, "shape", ()))))
        if not t.is_contiguous():
            raise ValueError("%s: ancestor tables must be contiguous (row "
                             "stride Rmax)" % op)


def rerank_advance(anc_old, anc_new, parent, n, prev_rows):
    """Reshuffle the ancestor table for a decode step with ``n`` history
    steps: batch row ``r`` continues row ``parent[r]`` of the previous
    step, which had ``prev_rows`` rows. Writes, for r < len(parent),
    ``anc_new[t, r] = anc_old[t, parent[r]]`` (t < n-1) and
    ``anc_new[n-1, r] = parent[r]``; returns ``anc_new``.

    anc_old / anc_new: two distinct contiguous (Tmax, Rmax) int32 tables.
    ``parent`` is a list or CPU tensor (checked against ``prev_rows``, then
    moved to the tables' device in one copy) or an int64 tensor already on
    the device, which is taken on trust: reading it would sync.
    """
    op = "rerank_advance"
    _check_tables(op, anc_old, anc_new)
    if anc_old.shape != anc_new.shape or anc_old.device != anc_new.device:
        raise ValueError("%s: anc_old %s and anc_new %s must have one shape "
                         "and device" % (op, tuple(anc_old.shape),
                                         tuple(anc_new.shape)))
    if anc_old.data_ptr() == anc_new.data_ptr():
        raise ValueError("%s: anc_old and anc_new must be two tables" % op)
    Tmax, Rmax = anc_old.shape
    n, prev_rows = int(n), int(prev_rows)
    if not 1 <= n <= Tmax:
        raise ValueError("%s: n=%d outside [1, Tmax=%d]" % (op, n, Tmax))
    if not 1 <= prev_rows <= Rmax:
        raise ValueError("%s: prev_rows=%d outside [1, Rmax=%d]"
                         % (op, prev_rows, Rmax))
    on_device = torch.is_tensor(parent) and parent.is_cuda
    if torch.is_tensor(parent) and (parent.dim() != 1 or parent.dtype not in
                                    (torch.int32, torch.int64)):
        raise TypeError("%s: parent must be 1-d int32/int64, got %s %s"
                        % (op, parent.dtype, tuple(parent.shape)))
    if on_device and parent.dtype != torch.int64:
        raise TypeError("%s: a device parent must be int64, got %s"
                        % (op, parent.dtype))
    R = len(parent)
    if not 1 <= R <= Rmax:
        raise ValueError("%s: R=%d rows outside [1, Rmax=%d]" % (op, R, Rmax))
    if not on_device:
        vals = [int(v) for v in (parent.tolist() if torch.is_tensor(parent)
                                 else parent)]
        for r, p in enumerate(vals):
            if not 0 <= p < prev_rows:
                raise ValueError("%s: parent[%d]=%d outside the previous "
                                 "step's %d rows" % (op, r, p, prev_rows))
        parent = torch.tensor(vals, dtype=torch.int64).to(
            anc_old.device, non_blocking=True)
    if _use_hip(anc_old):
        _hip_ext().rerank_advance(anc_old, anc_new, parent.contiguous(), n)
        return anc_new
    return eager.rerank_advance(anc_old, anc_new, parent, n)


def rerank_penalties_paged(hist_a, hist_c, hist_s, anc, n, cur_a, cur_c,
                           cur_s, kl_factor, ctx_factor, state_factor):
    """Distraction rerank penalties (nats.py:981-999) of the R current
    batch rows against their ``n`` history steps, read in place:
    ``hist_*[t, anc[t, r]]`` is row r's entry for step t < n.

    hist_a/c/s (Tmax, Rmax, Ts/C/H) fp32 contiguous; anc (Tmax, Rmax) int32
    contiguous; cur_a/c/s (R, Ts/C/H) fp32 contiguous (the leading rows of
    a larger buffer are). Returns (R,) fp32, zeros when n == 0, and bit for
    bit what ``rerank_penalties`` gives on the densely gathered history.
    """
    op = "rerank_penalties_paged"
    for name, t, rank in (("hist_a", hist_a, 3), ("hist_c", hist_c, 3),
                          ("hist_s", hist_s, 3), ("cur_a", cur_a, 2),
                          ("cur_c", cur_c, 2), ("cur_s", cur_s, 2)):
        if (not torch.is_tensor(t) or t.dtype != torch.float32
                or t.dim() != rank):
            raise TypeError("%s: %s must be a %d-d float32 tensor, got %s %s"
                            % (op, name, rank, getattr(t, "dtype", type(t)),
                               tuple(getattr(t, "shape", ()))))
        if not t.is_contiguous():
            raise ValueError("%s: %s must be contiguous" % (op, name))
    _check_tables(op, anc)
    Tmax, Rmax = anc.shape
    R = cur_a.shape[0]
    for h, c, name in ((hist_a, cur_a, "a"), (hist_c, cur_c, "c"),
                       (hist_s, cur_s, "s")):
        if tuple(h.shape[:2]) != (Tmax, Rmax):
            raise ValueError("%s: hist_%s %s does not match the (%d, %d) "
                             "table" % (op, name, tuple(h.shape), Tmax, Rmax))
        if tuple(c.shape) != (R, h.shape[2]):
            raise ValueError("%s: cur_%s must be (%d, %d), got %s"
                             % (op, name, R, h.shape[2], tuple(c.shape)))
    if not 1 <= R <= Rmax:
        raise ValueError("%s: R=%d rows outside [1, Rmax=%d]" % (op, R, Rmax))
    n = int(n)
    if not 0 <= n <= Tmax:
        raise ValueError("%s: n=%d outside [0, Tmax=%d]" % (op, n, Tmax))
    args = (hist_a, hist_c, hist_s, anc, n, cur_a, cur_c, cur_s,
            float(kl_factor), float(ctx_factor), float(state_factor))
    if _use_hip(hist_a):
        return _hip_ext().rerank_penalties_paged(*args)
    return eager.rerank_penalties_paged(*args)


class RerankHistory:
    """Slabs, the two ping-pong ancestor tables and the step count of one
    batched decode. All sentences of the batch start together, so every
    row alive at step ``n`` has exactly ``n`` history steps."""

    def __init__(self, Tmax, Rmax, Ts, C, H, device):
        self.hist_a = torch.empty(Tmax, Rmax, Ts, device=device)
        self.hist_c = torch.empty(Tmax, Rmax, C, device=device)
        self.hist_s = torch.empty(Tmax, Rmax, H, device=device)
        # only written slots are ever read
        self.anc = [torch.empty(Tmax, Rmax, dtype=torch.int32, device=device)
                    for _ in range(2)]
        self.n = 0
        self.rows = 0

    def step(self, parent, cur_a, cur_c, cur_s, factors):
        """One decode step. ``cur_*`` (R, dim) fp32 are the step outputs of
        the R batch rows, ``parent`` (ignored at step 0) names the row of
        the previous step each continues, ``factors`` = (kl, ctx, state).
        Advances the table, returns the (R,) penalties (zeros at step 0)
        and stores the current rows as this step's history entries."""
        n, R = self.n, cur_a.shape[0]
        if n == 0:
            pen = torch.zeros(R, device=cur_a.device)
        else:
            rerank_advance(self.anc[0], self.anc[1], parent, n, self.rows)
            self.anc.reverse()
            pen = rerank_penalties_paged(
                self.hist_a, self.hist_c, self.hist_s, self.anc[0], n,
                cur_a, cur_c, cur_s, *factors)
        self.hist_a[n, :R] = cur_a
        self.hist_c[n, :R] = cur_c
        self.hist_s[n, :R] = cur_s
        self.n, self.rows = n + 1, R
        return pen
