"""CPU: ops.linear_bias and ops.encoder_head are exactly the expressions
they replaced in the model, values and gradients bit for bit, and the
model's training forward still agrees with encode() + project_ctx()."""

import pytest
import torch


def _randn(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def _grads(fn, tensors, weights):
    leaves = [t.clone().requires_grad_(True) for t in tensors]
    outs = fn(*leaves)
    outs = outs if isinstance(outs, tuple) else (outs,)
    sum((o * w).sum() for o, w in zip(outs, weights)).backward()
    return [o.detach() for o in outs], [t.grad for t in leaves]


@pytest.mark.parametrize("xshape", [(7, 5), (4, 3, 5)])
def test_linear_bias_cpu_is_the_expression(xshape):
    from nats_amd import ops
    ins = (_randn(*xshape, seed=1), _randn(5, 9, seed=2), _randn(9, seed=3))
    w = [_randn(*xshape[:-1], 9, seed=4)]
    o1, g1 = _grads(ops.linear_bias, ins, w)
    o2, g2 = _grads(lambda x, W, b: x @ W + b, ins, w)
    for a, b in zip(o1 + g1, o2 + g2):
        assert a.dtype == b.dtype and torch.equal(a, b)


@pytest.mark.parametrize("masked", [True, False])
def test_encoder_head_cpu_is_the_expression(masked):
    from nats_amd import ops
    T, B, H, A = 6, 4, 5, 3
    mask = None
    if masked:
        lens = torch.tensor([6, 1, 3, 4])
        mask = (torch.arange(T).unsqueeze(1) < lens.unsqueeze(0)).float()
    ins = (_randn(T, B, H, seed=5), _randn(T, B, H, seed=6),
           _randn(2 * H, A, seed=7), _randn(A, seed=8))
    w = [_randn(T, B, 2 * H, seed=9), _randn(B, 2 * H, seed=10),
         _randn(T, B, A, seed=11)]

    def old(h_f, h_r, Wc, b):
        ctx = torch.cat([h_f, h_r.flip(0)], dim=-1)
        if mask is not None:
            mean = ((ctx * mask.unsqueeze(-1)).sum(0) /
                    mask.sum(0).unsqueeze(-1))
        else:
            mean = ctx.mean(0)
        return ctx, mean, ctx @ Wc + b

    o1, g1 = _grads(lambda h_f, h_r, Wc, b: ops.encoder_head(
        h_f, h_r, mask, Wc, b), ins, w)
    o2, g2 = _grads(old, ins, w)
    for a, b in zip(o1 + g1, o2 + g2):
        assert a.dtype == b.dtype and torch.equal(a, b)


@pytest.mark.parametrize("depth", [1, 2])
def test_training_forward_matches_encode_path(depth):
    """forward() goes through ops.encoder_head / ops.linear_bias; the
    pieces decode uses (encode, project_ctx, readout_logits) must give the
    same cost."""
    from nats_amd import ops
    from nats_amd.data.synthetic import synthetic_batch
    from nats_amd.models.distraction import NatsModel, default_options
    import numpy
    opts = default_options(dim_word=12, dim=20, dim_att=12, n_words=50,
                           enc_depth=depth)
    model = NatsModel(opts, seed=3)
    x, xm, y, ym = [torch.from_numpy(a) for a in synthetic_batch(
        numpy.random.RandomState(0), 3, 7, 4, 50)]
    xm[5:, 1] = 0.0
    cost = model(x, xm, y, ym)

    ctx, init = model.encode(x, xm)
    emb = model.embed(y, shift=True)
    yg, yc = model._dec_inputs(emb)
    h2s, ctxs, _, _, _ = ops.cond_gru_scan(
        yg, yc, ym, init, ctx, xm, model.project_ctx(ctx), model.P)
    logits = model.readout_logits(h2s, emb, ctxs)
    nll = ops.softmax_xent(logits.reshape(-1, 50), y.reshape(-1))
    assert torch.equal(cost, (nll.reshape(y.shape) * ym).sum(0))
