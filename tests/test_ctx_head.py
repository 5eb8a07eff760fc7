"""GPU tests of the context head (ctx_head_fwd / ctx_head_bwd in
ops/hip/io_fusion.hip, ops.encoder_head on top of them) and of the
training forward that uses it, against the torch composition it replaces
and fp64 evaluations."""

import numpy
import pytest
import torch

from kernel_ref import assert_grad_close, grad_err_ratio

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
A = 12


@pytest.fixture(scope="module")
def ext():
    from nats_amd.ops import _hip_ext
    m = _hip_ext()
    assert m is not None, "HIP extension must build/load on a GPU box"
    return m


def _mask(kind, T, B):
    if kind == "none":
        return None
    if kind == "ones":
        return torch.ones(T, B)
    # ragged: lengths cycle through 1..T, every column keeps >= 1 token
    lens = torch.arange(B) % T + 1
    return (torch.arange(T).unsqueeze(1) < lens.unsqueeze(0)).float()


_CASES = {}


def _case(T, B, H, kind):
    """Inputs of one shape, drawn once. h_f and h_r carry a time ramp of
    opposite sign on top of the noise, so a missing or doubled time
    reversal moves every element."""
    key = (T, B, H, kind)
    if key not in _CASES:
        g = torch.Generator().manual_seed(1000 * T + 10 * B + H)
        ramp = torch.arange(T, dtype=torch.float32).view(T, 1, 1)
        h_f = torch.randn(T, B, H, generator=g) + 0.5 * ramp
        h_r = torch.randn(T, B, H, generator=g) - 0.25 * ramp
        Wc = 0.2 * torch.randn(2 * H, A, generator=g)
        b = torch.randn(A, generator=g)
        # gradients: dctx as the decoder hands it over, a permuted view of
        # a [B,T,C] bf16 buffer; dpctx and dmean in fp32
        dctx = torch.randn(B, T, 2 * H, generator=g).to(BF16)
        dpctx = torch.randn(T, B, A, generator=g)
        dmean = torch.randn(B, 2 * H, generator=g)
        _CASES[key] = tuple(t.cuda() for t in (h_f, h_r, Wc, b, dctx, dpctx,
                                               dmean)) + (_mask(kind, T, B),)
    return _CASES[key]


def _composition(h_f, h_r, mask, Wc, b):
    """What NatsModel.forward computed before ops.encoder_head."""
    ctx = torch.cat([h_f, h_r.flip(0)], dim=-1)
    if mask is not None:
        mean = (ctx * mask.unsqueeze(-1)).sum(0) / mask.sum(0).unsqueeze(-1)
    else:
        mean = ctx.mean(0)
    return ctx, mean, ctx @ Wc + b


SHAPES = [(T, B, H) for T in (1, 2, 17) for B in (1, 6, 33)
          for H in (4, 48, 50)]
KINDS = ("none", "ones", "ragged")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("T,B,H", SHAPES)
def test_encoder_head_forward(ext, T, B, H, kind):
    from nats_amd import ops
    h_f, h_r, Wc, b, _, _, _, mask = _case(T, B, H, kind)
    mask = mask.cuda() if mask is not None else None
    with torch.autocast("cuda", dtype=BF16):
        ctx_bf, mean, pctx = ops.encoder_head(h_f, h_r, mask, Wc, b)
        ctx_r, _, pctx_r = _composition(h_f, h_r, mask, Wc, b)
    assert ctx_bf.dtype == BF16 and ctx_bf.is_contiguous()
    assert torch.equal(ctx_bf, ctx_r.to(BF16))

    c64 = ctx_r.double()
    m64 = (mask.double() if mask is not None
           else torch.ones(T, B, dtype=torch.float64, device="cuda"))
    cnt = m64.sum(0).unsqueeze(-1)
    ref = (c64 * m64.unsqueeze(-1)).sum(0) / cnt
    bound = T * 2.0 ** -24 * (c64 * m64.unsqueeze(-1)).abs().sum(0) / cnt
    err = (mean.double() - ref).abs()
    assert mean.dtype == torch.float32 and mean.shape == (B, 2 * H)
    assert bool((err <= bound).all()), float((err - bound).max())

    # both run the same bf16 GEMM on the same operands and add the fp32
    # bias in fp32; only the GEMM result carries a bf16 rounding, so one
    # bf16 ulp (8 significand bits) of that part is the allowance
    assert pctx.dtype == pctx_r.dtype == torch.float32
    gemm = (pctx_r - b).abs().clamp_min(2.0 ** -126)
    ulp = torch.exp2(torch.floor(torch.log2(gemm)) - 7)
    assert bool(((pctx - pctx_r).abs() <= ulp).all())


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("T,B,H", SHAPES)
def test_encoder_head_backward(ext, T, B, H, kind):
    from nats_amd import ops
    h_f, h_r, Wc, b, dctx_bt, dpctx, dmean, mask = _case(T, B, H, kind)
    mask = mask.cuda() if mask is not None else None
    dctx = dctx_bt.permute(1, 0, 2)          # (T,B,C), strides (C, T*C, 1)

    def run(fn, dtype, ctx_grad, amp):
        leaves = [t.detach().clone().to(dtype).requires_grad_(True)
                  for t in (h_f, h_r, Wc, b)]
        m = mask.to(dtype) if mask is not None else None
        with torch.autocast("cuda", dtype=BF16, enabled=amp):
            outs = fn(leaves[0], leaves[1], m, leaves[2], leaves[3])
        torch.autograd.backward(
            list(outs), [ctx_grad, dmean.to(dtype), dpctx.to(dtype)])
        return [t.grad for t in leaves]

    new = run(ops.encoder_head, torch.float32, dctx, True)
    # the composition received the decoder's ctx gradient cast to fp32
    old = run(_composition, torch.float32, dctx.float(), True)
    ref = run(_composition, torch.float64, dctx.double(), False)
    for name, n, o, r in zip(("h_f", "h_r", "Wc_att", "b_att"), new, old,
                             ref):
        assert n.dtype == torch.float32 and n.shape == r.shape
        e_new = float((n.double() - r).abs().max())
        e_old = float((o.double() - r).abs().max())
        ulp = 2.0 ** -23 * float(r.abs().max())
        print("%s: err new %.3e old %.3e ulp %.3e" % (name, e_new, e_old,
                                                      ulp))
        # per tensor: at most twice the composition's own worst error
        # against fp64, plus one fp32 ulp at the tensor's scale
        assert e_new <= 2 * e_old + ulp, name


def _ragged_batch(n, seed):
    from nats_amd.data.prepare import prepare_data
    rng = numpy.random.RandomState(seed)
    xs = [list(rng.randint(2, 120, size=rng.randint(4, 12)))
          for _ in range(n)]
    ys = [list(rng.randint(2, 120, size=rng.randint(3, 8)))
          for _ in range(n)]
    return [torch.from_numpy(a) for a in prepare_data(xs, ys)]


@pytest.mark.parametrize("batch", [6, 33])
@pytest.mark.parametrize("dim", [48, 50])
def test_model_training_step_vs_cpu_fp32(ext, dim, batch):
    """One autocast forward+backward of a tiny model on the HIP path
    against the CPU fp32 model: cost to the 5 % of
    test_model_forward_gpu_vs_cpu, every parameter gradient to
    assert_grad_close at the rel=0.08 / model-scale floor of
    test_cond_gru_backward."""
    from nats_amd.models.distraction import NatsModel, default_options
    opts = default_options(dim_word=16, dim=dim, dim_att=8, n_words=120)
    model = NatsModel(opts, seed=9)
    arrs = _ragged_batch(batch, 0)
    cost_cpu = model(*arrs)
    cost_cpu.mean().backward()

    gmodel = NatsModel(opts, params=model.get_params()).cuda()
    with torch.autocast("cuda", dtype=BF16):
        cost_gpu = gmodel(*[a.cuda() for a in arrs])
    cost_gpu.mean().backward()
    rel = ((cost_cpu - cost_gpu.float().cpu()).abs() / cost_cpu.abs()).max()
    print("cost max rel err %.3e" % float(rel))
    assert rel < 0.05, float(rel)

    ref = {k: p.grad for k, p in model.P.items()}
    got = {k: p.grad.float().cpu() for k, p in gmodel.P.items()}
    gscale = max(float(v.abs().max()) for v in ref.values())
    for k in ref:
        print("%s err/bound %.3f" % (k, grad_err_ratio(
            ref[k], got[k], rel=0.08, global_scale=gscale)))
    for k in ref:
        assert_grad_close(ref[k], got[k], k, rel=0.08, global_scale=gscale)
