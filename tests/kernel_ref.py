"""Shared input builders, oracle runs and comparison helpers of the kernel
tests (tests/test_gpu_kernels.py, tests/test_gpu_kernel_edges.py,
tests/test_gru_kloop_edges.py).

The oracle is always nats_amd.ops.eager. It is run in three ways:
  * fp64: the reference every comparison is made against,
  * fp32 with the operands the kernels read as bf16 rounded to bf16 first
    ("bf16-operand run"): a model of the error the kernels are entitled to,
    used to check on the CPU that a bound is not within reference noise and
    to derive the relative bound on the attention weights,
  * through the HIP op on the GPU, by passing ``fn``/``dev``.
"""

import torch


def assert_grad_close(a, b, name="", rel=0.06, floor_frac=1e-3,
                      global_scale=None):
    """Scale-aware gradient comparison.

    Global-max normalization (rel = max|a-b| / max|a|) lets a large
    relative error on a small-magnitude COLUMN hide under the tensor's
    largest column. Instead: normalize per output column (last axis —
    each column of a weight grad is an independent sum over (T,B)), with
    a small absolute floor of floor_frac * global_max covering bf16
    swamping where large contributions cancel. floor_frac=1e-3 is ~60x
    tighter than the old global-max bound for the smallest columns.
    """
    a2 = a.reshape(-1, a.shape[-1]) if a.dim() > 1 else a.reshape(1, -1)
    b2 = b.reshape(-1, b.shape[-1]) if b.dim() > 1 else b.reshape(1, -1)
    col_scale = a2.abs().amax(dim=0)
    # global_scale: the MODEL's gradient magnitude — reduce-to-scalar
    # grads (c_att = sum of thousands of cancelling de terms) carry fp32
    # accumulation noise proportional to the contributions, not to their
    # near-zero sum; floor such tensors at 1e-3 of the model scale
    floor_base = a2.abs().max().clamp_min(1e-6)
    if global_scale is not None:
        floor_base = max(float(floor_base), 1e-2 * float(global_scale))
    floor = floor_frac * floor_base
    col_err = (a2 - b2).abs().amax(dim=0)
    bound = rel * col_scale + floor
    bad = col_err > bound
    if bool(bad.any()):
        worst = int((col_err - bound)[bad].argmax())
        idx = bad.nonzero().flatten()[worst]
        raise AssertionError(
            "%s: %d/%d columns out of bound; worst col %d err %.3e vs "
            "bound %.3e (col scale %.3e, floor %.3e)" % (
                name, int(bad.sum()), bad.numel(), int(idx),
                float(col_err[idx]), float(bound[idx]),
                float(col_scale[idx]), float(floor)))


def grad_err_ratio(a, b, rel=0.06, floor_frac=1e-3, global_scale=None):
    """max over columns of err / bound, with err and bound exactly as in
    assert_grad_close (which passes iff this is <= 1). For reporting."""
    a2 = a.reshape(-1, a.shape[-1]) if a.dim() > 1 else a.reshape(1, -1)
    b2 = b.reshape(-1, b.shape[-1]) if b.dim() > 1 else b.reshape(1, -1)
    col_scale = a2.abs().amax(dim=0)
    floor_base = a2.abs().max().clamp_min(1e-6)
    if global_scale is not None:
        floor_base = max(float(floor_base), 1e-2 * float(global_scale))
    floor = floor_frac * floor_base
    col_err = (a2 - b2).abs().amax(dim=0)
    return float((col_err / (rel * col_scale + floor)).max())


def _gru_inputs(T=13, B=5, H=48, E=20, seed=0, with_mask=True):
    g = torch.Generator().manual_seed(seed)
    xg = torch.randn(T, B, 2 * H, generator=g)
    xc = torch.randn(T, B, H, generator=g)
    U = 0.3 * torch.randn(H, 2 * H, generator=g)
    Ux = 0.3 * torch.randn(H, H, generator=g)
    mask = None
    if with_mask:
        lens = torch.randint(2, T + 1, (B,), generator=g)
        mask = (torch.arange(T).unsqueeze(1) < lens.unsqueeze(0)).float()
    return xg, xc, U, Ux, mask


def _cond_inputs(T=7, B=5, H=32, Ts=9, A=12, E=10, seed=5, with_masks=True):
    from nats_amd.models.distraction import NatsModel, default_options
    torch.manual_seed(seed)
    g = torch.Generator().manual_seed(seed)
    C = 2 * H
    opts = default_options(dim_word=E, dim=H, dim_att=A, n_words=50)
    model = NatsModel(opts, seed=seed)
    # inflate the 0.01-scale attention/distraction weights so alpha is far
    # from uniform and the gate far from linear — otherwise a broken
    # pstate/gate path can hide inside a near-uniform attention pattern
    with torch.no_grad():
        for k in ("decoder_W_att", "decoder_Wc_att", "decoder_U_att",
                  "decoder_D_wei", "decoder_W_con", "decoder_U_con"):
            model.P[k].mul_(40.0)
    yg = torch.randn(T, B, 2 * H, generator=g)
    yc = torch.randn(T, B, H, generator=g)
    init = torch.randn(B, H, generator=g) * 0.1
    ctx = torch.randn(Ts, B, C, generator=g)
    mask = ctx_mask = None
    if with_masks:
        lens = torch.randint(2, T + 1, (B,), generator=g)
        mask = (torch.arange(T).unsqueeze(1) < lens.unsqueeze(0)).float()
        slens = torch.randint(2, Ts + 1, (B,), generator=g)
        ctx_mask = (torch.arange(Ts).unsqueeze(1) < slens.unsqueeze(0)).float()
    return model, yg, yc, mask, init, ctx, ctx_mask


def round_bf16(x):
    """x rounded to bf16, kept in x's dtype, gradient passed straight
    through (a plain cast pair would round the gradient to bf16 as well)."""
    xd = x.detach()
    return x + (xd.to(torch.bfloat16).to(x.dtype) - xd)


def weighted_loss(outs, dev, dtype):
    """sum_i (out_i * w_i).sum() with w_i ~ N(0,1) drawn on the CPU from
    seed 0 in output order, so every device optimises the SAME loss."""
    g = torch.Generator().manual_seed(0)
    loss = 0
    for o in outs:
        w = torch.randn(o.shape, generator=g).to(device=dev, dtype=dtype)
        loss = loss + (o.to(dtype) * w).sum()
    return loss


# the sixteen decoder parameters: the fourteen the scan takes, plus the two
# that reach it through pctx = ctx @ Wc_att + b_att
DECODER_GRAD_KEYS = (
    "decoder_U", "decoder_Ux", "decoder_U_1", "decoder_W_1", "decoder_b_1",
    "decoder_Wx_1", "decoder_Ux_1", "decoder_bx_1", "decoder_W_att",
    "decoder_U_att", "decoder_c_att", "decoder_W_con", "decoder_U_con",
    "decoder_D_wei", "decoder_Wc_att", "decoder_b_att")
# the weight matrices cond_gru.hip reads as packed bf16 GEMM operands
DECODER_BF16_KEYS = ("decoder_U", "decoder_Ux", "decoder_U_1", "decoder_W_1",
                     "decoder_Wx_1", "decoder_Ux_1", "decoder_W_att")
COND_OUT_NAMES = ("h2s", "ctxs", "alphas", "acc_ctx", "acc_alpha")
COND_IN_NAMES = ("yg", "yc", "init", "ctx")


def run_cond_scan(fn, case, dev="cpu", dtype=torch.float32,
                  bf16_operands=False):
    """Decoder scan ``fn`` on ``case`` (a _cond_inputs tuple) with the loss
    of weighted_loss over all five outputs. Returns (outs, grads): outs maps
    COND_OUT_NAMES and grads maps DECODER_GRAD_KEYS + COND_IN_NAMES to
    detached CPU tensors of ``dtype``.

    bf16_operands rounds what the HIP decoder reads as bf16 (yg, yc, ctx as
    the attention-sum operand, DECODER_BF16_KEYS); pctx is computed from the
    unrounded ctx and stays in ``dtype``, like the small vectors."""
    model, yg, yc, mask, init, ctx, ctx_mask = case
    P = {k: v.detach().clone().to(device=dev, dtype=dtype).requires_grad_(
        k in DECODER_GRAD_KEYS) for k, v in model.P.items()}
    ins = [t.clone().to(device=dev, dtype=dtype).requires_grad_(True)
           for t in (yg, yc, init, ctx)]
    m_ = mask.to(device=dev, dtype=dtype)
    cm = ctx_mask.to(device=dev, dtype=dtype)
    pctx = ins[3] @ P["decoder_Wc_att"] + P["decoder_b_att"]
    Pe, (yg_, yc_, init_, ctx_) = P, ins
    if bf16_operands:
        Pe = dict(P)
        for k in DECODER_BF16_KEYS:
            Pe[k] = round_bf16(P[k])
        yg_, yc_, ctx_ = round_bf16(yg_), round_bf16(yc_), round_bf16(ctx_)
    outs = fn(yg_, yc_, m_, init_, ctx_, cm, pctx, Pe)
    weighted_loss(outs, dev, dtype).backward()
    grads = {k: P[k].grad for k in DECODER_GRAD_KEYS}
    grads.update(zip(COND_IN_NAMES, (t.grad for t in ins)))
    return ({n: o.detach().cpu().to(dtype)
             for n, o in zip(COND_OUT_NAMES, outs)},
            {k: v.detach().cpu().to(dtype) for k, v in grads.items()})


def alphas_rel_err(alphas, ref_alphas, ctx_mask):
    """Largest relative deviation of ``alphas`` (T,B,Ts) from ``ref_alphas``
    over the entries that are unmasked and >= 1e-6 in the reference."""
    sel = (ctx_mask.t().unsqueeze(0) > 0) & (ref_alphas >= 1e-6)
    rel = (alphas.double() - ref_alphas.double()).abs() / ref_alphas.double()
    return float(rel[sel.expand_as(rel)].max())


def _gru_kloop_inputs(T, B, H, seed):
    """GRU scan inputs for hidden sizes up to the production ones. U and Ux
    are N(0,1) * 2 * H^-0.5: H^-0.5 keeps the gates out of saturation at
    H = 1000, the factor 2 keeps the recurrent term large enough that one
    missing 32-wide K slice of it is visible. Lengths lie in [2, T].
    Returns ((xg, xc, U, Ux, mask), h0)."""
    g = torch.Generator().manual_seed(seed)
    xg = torch.randn(T, B, 2 * H, generator=g)
    xc = torch.randn(T, B, H, generator=g)
    U = 2 * H ** -0.5 * torch.randn(H, 2 * H, generator=g)
    Ux = 2 * H ** -0.5 * torch.randn(H, H, generator=g)
    lens = torch.randint(2, T + 1, (B,), generator=g)
    mask = (torch.arange(T).unsqueeze(1) < lens.unsqueeze(0)).float()
    h0 = 0.5 * torch.randn(B, H, generator=g)
    return (xg, xc, U, Ux, mask), h0


GRU_GRAD_NAMES = ("xg", "xc", "U", "Ux", "h0")
GRU_BIDIR_GRAD_NAMES = ("xg0", "xc0", "U0", "Ux0", "xg1", "xc1", "U1", "Ux1")


def run_gru_scan(fn, inputs, h0, dev="cpu", dtype=torch.float32,
                 bf16_operands=False):
    """GRU scan ``fn`` from the initial state ``h0`` with the loss
    (h * w).sum(), w ~ N(0,1) from seed 0. Returns (h, grads) as detached
    CPU tensors of ``dtype``; grads maps GRU_GRAD_NAMES. bf16_operands
    rounds what gru_scan.hip reads as bf16: xg, xc, U and Ux."""
    xg, xc, U, Ux, mask = inputs
    leaves = [t.clone().to(device=dev, dtype=dtype).requires_grad_(True)
              for t in (xg, xc, U, Ux, h0)]
    a = [round_bf16(t) for t in leaves[:4]] if bf16_operands else leaves[:4]
    h = fn(a[0], a[1], mask.to(device=dev, dtype=dtype), a[2], a[3],
           leaves[4])
    weighted_loss([h], dev, dtype).backward()
    return (h.detach().cpu().to(dtype),
            {n: t.grad.detach().cpu().to(dtype)
             for n, t in zip(GRU_GRAD_NAMES, leaves)})


def run_gru_scan_bidir(fn, inputs0, inputs1, dev="cpu", dtype=torch.float32,
                       bf16_operands=False):
    """Bidirectional counterpart of run_gru_scan: ``fn(xg0, xc0, mask0, U0,
    Ux0, xg1, xc1, mask1, U1, Ux1)`` -> (h_fwd, h_bwd), both from a zero
    state, with the loss of weighted_loss over the two outputs. inputs0 and
    inputs1 are (xg, xc, U, Ux, mask) per direction; a mask may be None.
    Returns ((h_fwd, h_bwd), grads) as detached CPU tensors of ``dtype``;
    grads maps GRU_BIDIR_GRAD_NAMES."""
    leaves, args = [], []
    for xg, xc, U, Ux, mask in (inputs0, inputs1):
        lv = [t.clone().to(device=dev, dtype=dtype).requires_grad_(True)
              for t in (xg, xc, U, Ux)]
        a = [round_bf16(t) for t in lv] if bf16_operands else lv
        m = None if mask is None else mask.to(device=dev, dtype=dtype)
        leaves += lv
        args += [a[0], a[1], m, a[2], a[3]]
    hs = fn(*args)
    weighted_loss(hs, dev, dtype).backward()
    return (tuple(h.detach().cpu().to(dtype) for h in hs),
            {n: t.grad.detach().cpu().to(dtype)
             for n, t in zip(GRU_BIDIR_GRAD_NAMES, leaves)})
