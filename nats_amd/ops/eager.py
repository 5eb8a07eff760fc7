"""Eager (plain PyTorch) reference implementations of the hot ops.

These are the numerics oracles for the HIP kernels. Each function's
semantics are the Theano graph equations of the reference, cited per-op.
They are deliberately written as straight-line tensor code (no custom
autograd) so torch autograd provides the exact BPTT the reference got from
``tensor.grad`` (nats.py:1340).
"""

import math

import torch


def gru_scan(x_gates, x_cand, mask, U, Ux, h0=None):
    """GRU over time (nats.py:336-372).

    x_gates: (T,B,2H) = x@W + b     (hoisted, nats.py:328-329)
    x_cand:  (T,B,H)  = x@Wx + bx   (nats.py:331-332)
    mask:    (T,B) float or None (None = all ones, nats.py:317-318)
    U: (H,2H), Ux: (H,H); h0: (B,H) or None (zeros, nats.py:360)

    Per step (nats.py:336-356):
      preact = h_{t-1} @ U + x_t ;  r = sigmoid(preact[:, :H]),
      u = sigmoid(preact[:, H:]) ;  hbar = tanh((h_{t-1} @ Ux) * r + xx_t)
      h_t = u * h_{t-1} + (1-u) * hbar ;  h_t = m*h_t + (1-m)*h_{t-1}
    """
    T, B = x_gates.shape[0], x_gates.shape[1]
    H = Ux.shape[1]
    h = h0 if h0 is not None else x_gates.new_zeros(B, H)
    out = []
    for t in range(T):
        preact = torch.sigmoid(h @ U + x_gates[t])
        r, u = preact[:, :H], preact[:, H:]
        hbar = torch.tanh((h @ Ux) * r + x_cand[t])
        h_new = u * h + (1.0 - u) * hbar
        if mask is not None:
            m = mask[t].unsqueeze(1)
            h_new = m * h_new + (1.0 - m) * h
        h = h_new
        out.append(h)
    return torch.stack(out, dim=0)


def _attention(h1, ctx, ctx_mask, pctx, acc_ctx, acc_alpha, P):
    """Bahdanau attention + the two distraction terms (nats.py:527-546).

    Returns (alpha (Ts,B), ctx_t (B,C)). The softmax is computed with
    max-subtraction for stability; because the reference normalises
    exp(e)*mask / sum(exp(e)*mask) (nats.py:537-540), subtracting the
    per-column max before exp yields the identical result.
    """
    pstate = h1 @ P["decoder_W_att"]                       # (B,A)
    pc = pctx + pstate.unsqueeze(0)                        # (Ts,B,A)
    # distraction over the attention-weight history (nats.py:532):
    # (Ts,B,1) @ (1,A) -> (Ts,B,A)
    pc = pc + acc_alpha.t().unsqueeze(-1) * P["decoder_D_wei"].reshape(-1)
    pc = torch.tanh(pc)
    e = (pc @ P["decoder_U_att"]).squeeze(-1) + P["decoder_c_att"]  # (Ts,B)
    e = e - e.max(dim=0, keepdim=True).values
    alpha = torch.exp(e)
    if ctx_mask is not None:
        alpha = alpha * ctx_mask
    alpha = alpha / alpha.sum(dim=0, keepdim=True)
    ctx_t = (ctx * alpha.unsqueeze(-1)).sum(dim=0)         # (B,C)
    # distraction over input content vectors (nats.py:545-546)
    ctx_t = torch.tanh(P["decoder_U_con"].reshape(-1) * ctx_t +
                       acc_ctx * P["decoder_W_con"].reshape(-1))
    return alpha, ctx_t


def cond_gru_step(h_prev, x_g, x_c, ctx, ctx_mask, pctx, acc_ctx, acc_alpha,
                  P, m=None):
    """One conditional-GRU step (nats.py:498-572).

    h_prev (B,H); x_g (B,2H) = emb@W+b; x_c (B,H) = emb@Wx+bx;
    ctx (Ts,B,C); ctx_mask (Ts,B) or None; pctx (Ts,B,A) = ctx@Wc_att+b_att;
    acc_ctx (B,C); acc_alpha (B,Ts); m (B,) mask or None.

    Returns (h2, ctx_t, alpha_T, new_acc_ctx, new_acc_alpha) where
    alpha_T is (B,Ts) (the reference returns alpha.T, nats.py:572).

    NOTE GRU_2 applies sigmoid to the FULL 2H preactivation then slices
    (nats.py:505-510) — mathematically identical to slicing first.
    """
    H = h_prev.shape[1]
    # GRU_2 (nats.py:503-519)
    preact1 = torch.sigmoid(h_prev @ P["decoder_U"] + x_g)
    r1, u1 = preact1[:, :H], preact1[:, H:]
    h1 = torch.tanh((h_prev @ P["decoder_Ux"]) * r1 + x_c)
    h1 = u1 * h_prev + (1.0 - u1) * h1
    if m is not None:
        mm = m.unsqueeze(1)
        h1 = mm * h1 + (1.0 - mm) * h_prev

    alpha, ctx_t = _attention(h1, ctx, ctx_mask, pctx, acc_ctx, acc_alpha, P)

    # GRU_1 (nats.py:551-565)
    preact2 = torch.sigmoid(h1 @ P["decoder_U_1"] + P["decoder_b_1"] +
                            ctx_t @ P["decoder_W_1"])
    r2, u2 = preact2[:, :H], preact2[:, H:]
    h2 = torch.tanh((h1 @ P["decoder_Ux_1"] + P["decoder_bx_1"]) * r2 +
                    ctx_t @ P["decoder_Wx_1"])
    h2 = u2 * h1 + (1.0 - u2) * h2
    if m is not None:
        h2 = mm * h2 + (1.0 - mm) * h1

    # accumulate histories (nats.py:569-570)
    if m is not None:
        new_acc_ctx = mm * ctx_t + acc_ctx
        new_acc_alpha = mm * alpha.t() + acc_alpha
    else:
        new_acc_ctx = ctx_t + acc_ctx
        new_acc_alpha = alpha.t() + acc_alpha
    return h2, ctx_t, alpha.t(), new_acc_ctx, new_acc_alpha


def cond_gru_step_shared(h_prev, x_g, x_c, ctx_src, ctx_mask_src, pctx_src,
                         row_src, acc_ctx, acc_alpha, P):
    """cond_gru_step for rows that read column ``row_src[r]`` (int64
    tensor) of a context kept once per source: gather, then the plain
    step. The definition the shared-context kernel path is held to."""
    return cond_gru_step(
        h_prev, x_g, x_c, ctx_src.index_select(1, row_src),
        (None if ctx_mask_src is None
         else ctx_mask_src.index_select(1, row_src)),
        pctx_src.index_select(1, row_src), acc_ctx, acc_alpha, P)


def cond_gru_scan(y_gates, y_cand, mask, init_state, ctx, ctx_mask, pctx, P):
    """Decoder scan over target time (nats.py:596-608).

    Returns (h2s (T,B,H), ctxs (T,B,C), alphas (T,B,Ts),
    acc_ctx (B,C), acc_alpha (B,Ts)) — the final accumulators.
    """
    T, B = y_gates.shape[0], y_gates.shape[1]
    Ts = ctx.shape[0]
    C = ctx.shape[2]
    h = init_state
    acc_ctx = ctx.new_zeros(B, C)
    acc_alpha = ctx.new_zeros(B, Ts)
    h2s, ctxs, alphas = [], [], []
    for t in range(T):
        m = mask[t] if mask is not None else None
        h, ctx_t, alpha_t, acc_ctx, acc_alpha = cond_gru_step(
            h, y_gates[t], y_cand[t], ctx, ctx_mask, pctx, acc_ctx, acc_alpha,
            P, m=m)
        h2s.append(h)
        ctxs.append(ctx_t)
        alphas.append(alpha_t)
    return (torch.stack(h2s, 0), torch.stack(ctxs, 0), torch.stack(alphas, 0),
            acc_ctx, acc_alpha)


def softmax_xent(logits, targets):
    """Per-position negative log-likelihood (nats.py:763-768).

    logits (N,V), targets (N,) -> (N,) in logits.dtype's accumulation
    precision (fp32; fp64 logits stay fp64, for use as a test oracle).
    """
    if logits.dtype != torch.float64:
        logits = logits.float()
    logp = torch.log_softmax(logits, dim=-1)
    return -logp.gather(1, targets.unsqueeze(1)).squeeze(1)


def linear_bias(x, W, b):
    """Hoisted input / vocab projection x @ W + b."""
    return x @ W + b


def context_mean(ctx, x_mask):
    """Masked time-mean of the context (nats.py:717); the plain mean
    without a mask (the sampler, nats.py:810)."""
    if x_mask is not None:
        return ((ctx * x_mask.unsqueeze(-1)).sum(0) /
                x_mask.sum(0).unsqueeze(-1))
    return ctx.mean(0)


def encoder_head(h_f, h_r, x_mask, Wc_att, b_att):
    """Context assembly from the two scan outputs (h_r in the reverse
    scan's own time order): ctx = [h_f | flip(h_r)] (nats.py:713), its
    masked mean and the attention keys ctx @ Wc_att + b_att
    (nats.py:493-494). Returns (ctx, ctx_mean, pctx)."""
    ctx = torch.cat([h_f, h_r.flip(0)], dim=-1)
    return ctx, context_mean(ctx, x_mask), ctx @ Wc_att + b_att


NEG_UNK = math.log(1e-20)  # log-probability UNK is pinned to (nats.py:1001)


def beam_select(probs, prev_cost, seg_off, want, penalty=None, use_unk=True,
                K=None):
    """Segmented beam candidate selection (nats.py:1001-1004 per sentence).

    probs (R,V) fp32; prev_cost (R,); seg_off (S+1,) / want (S,) int32
    tensors or lists: rows [seg_off[s], seg_off[s+1]) are sentence s's live
    hypotheses; penalty (R,) or None. Candidate cost c = prev_cost[:, None]
    - log(probs) (word 1 pinned to -log(1e-20) unless use_unk), selection
    key c + penalty[:, None]. Per sentence the want[s] smallest keys in
    ascending order, ties to the lower flat index local_row*V + w, NaN
    after +inf — a stable sort of the flattened keys gives all three.

    Returns (ranks (S,K) int64 padded with -1, costs (S,K) fp32 padded
    with +inf); costs are the UN-reranked c at the selected candidates.
    """
    offs = [int(v) for v in (seg_off.tolist() if torch.is_tensor(seg_off)
                             else seg_off)]
    wants = [int(v) for v in (want.tolist() if torch.is_tensor(want)
                              else want)]
    S = len(wants)
    K = max(wants) if K is None else int(K)
    logp = probs.log()
    if not use_unk:
        logp[:, 1] = NEG_UNK
    cand = prev_cost[:, None] - logp
    key = cand if penalty is None else cand + penalty[:, None]
    ranks = torch.full((S, K), -1, dtype=torch.int64, device=probs.device)
    costs = torch.full((S, K), float("inf"), dtype=probs.dtype,
                       device=probs.device)
    for s in range(S):
        sl = slice(offs[s], offs[s + 1])
        order = torch.sort(key[sl].flatten(), stable=True).indices[:wants[s]]
        ranks[s, :wants[s]] = order
        costs[s, :wants[s]] = cand[sl].flatten()[order]
    return ranks, costs


def rerank_penalties(hist_a, hist_c, hist_s, cur_a, cur_c, cur_s,
                     kl_factor, ctx_factor, state_factor):
    """Distraction rerank penalties (nats.py:981-999), vectorised over
    (history step, hypothesis): hist_* (n, k, dim), cur_* (k, dim) ->
    (k,) = -kl_factor * min_t KL(hist_a[t] || cur_a) + ctx_factor * max_t
    cosine_dist(hist_c[t], cur_c) + state_factor * max_t
    cosine_dist(hist_s[t], cur_s); KL in scipy's entropy convention (both
    sides normalised, 0 log 0 = 0), cosine distance 0 at a zero norm."""
    p = hist_a / hist_a.sum(-1, keepdim=True)
    q = (cur_a / cur_a.sum(-1, keepdim=True)).unsqueeze(0)
    logterm = torch.where(p > 0, p * (torch.log(p) - torch.log(q)),
                          torch.zeros_like(p))
    a_pen = -kl_factor * logterm.sum(-1).min(dim=0).values

    def cosd(h, c):
        num = (h * c.unsqueeze(0)).sum(-1)
        den = h.norm(dim=-1) * c.norm(dim=-1).unsqueeze(0)
        d = 1.0 - num / den
        return torch.where(den == 0, torch.zeros_like(d), d)

    c_pen = ctx_factor * cosd(hist_c, cur_c).max(dim=0).values
    s_pen = state_factor * cosd(hist_s, cur_s).max(dim=0).values
    return a_pen + c_pen + s_pen


def rerank_advance(anc_old, anc_new, parent, n):
    """Ancestor-table reshuffle of a decode step: row r of the new batch
    continues row parent[r] of the previous one, so it inherits that row's
    n-1 earlier slots and gets the parent row itself as the slot of step
    n-1. Tables are (Tmax, Rmax) int32; writes anc_new[:n, :len(parent)]."""
    parent = torch.as_tensor(parent, dtype=torch.int64,
                             device=anc_old.device)
    R = parent.shape[0]
    anc_new[:n - 1, :R] = anc_old[:n - 1].index_select(1, parent)
    anc_new[n - 1, :R] = parent.to(anc_new.dtype)
    return anc_new


def rerank_gather(hist, anc, n, R):
    """Dense (n, R, dim) history of the R current rows, read from a slab
    hist (Tmax, Rmax, dim) through the ancestor table."""
    steps = torch.arange(n, device=hist.device)[:, None]
    return hist[steps, anc[:n, :R].long()]


def rerank_penalties_paged(hist_a, hist_c, hist_s, anc, n, cur_a, cur_c,
                           cur_s, kl_factor, ctx_factor, state_factor):
    """rerank_penalties on the histories gathered through ``anc``; zeros
    when there is no history yet."""
    R = cur_a.shape[0]
    if n == 0:
        return torch.zeros(R, dtype=cur_a.dtype, device=cur_a.device)
    return rerank_penalties(
        rerank_gather(hist_a, anc, n, R), rerank_gather(hist_c, anc, n, R),
        rerank_gather(hist_s, anc, n, R), cur_a, cur_c, cur_s,
        kl_factor, ctx_factor, state_factor)


def beam_reorder(table, src, dst, y_out, route_out, n_prev):
    """Beam-row reshuffle of a batched decode step, as index_selects.
    table (3, L) int64 on the buffers' device = [parent | word | sentence];
    for r < L: dst_j[r] = src_j[parent[r]], y_out[r] = word[r],
    route_out[r] = sentence[r]; rows L <= r < Rmax repeat the new row 0. A
    parent outside [0, n_prev) is not dereferenced: NaN rows, y and route 0
    (the kernel's poison convention)."""
    L, Rmax = table.shape[1], y_out.shape[0]
    cols = torch.arange(Rmax, device=table.device)
    tab = table.index_select(1, torch.where(cols < L, cols,
                                            torch.zeros_like(cols)))
    parent = tab[0]
    ok = (parent >= 0) & (parent < n_prev)
    safe = torch.where(ok, parent, torch.zeros_like(parent))
    for s, d in zip(src, dst):
        rows = s.index_select(0, safe)
        d.copy_(torch.where(ok[:, None], rows,
                            torch.full_like(rows, float("nan"))))
    zero = torch.zeros_like(parent)
    y_out.copy_(torch.where(ok, tab[1], zero))
    route_out.copy_(torch.where(ok, tab[2], zero))
