"""CPU tests of the Python layer between the model and the HIP kernels:
batch chunking, the decoder operand pack and its cache, the weight-version
protocol and the decode-graph stepper cache. No kernel runs here."""

import pytest
import torch


def _tiny_model(seed=3):
    # H=20, C=40, A=12: no multiple of the 16/32 tile sizes
    from nats_amd.models.distraction import NatsModel, default_options
    opts = default_options(dim_word=12, dim=20, dim_att=12, n_words=50)
    return NatsModel(opts, seed=seed)


def _bump(params):
    from nats_amd.ops import bump_update_epoch
    bump_update_epoch(params)


def test_run_chunks_serial_matches_unchunked():
    from nats_amd import ops
    B, T, H = 70, 3, 5
    g = torch.Generator().manual_seed(0)
    x_tm = torch.randn(T, B, H, generator=g)     # time-major, batch on dim 1
    x_bm = torch.randn(B, H, generator=g)        # batch-major, batch on dim 0
    W = torch.randn(H, generator=g)              # unsliced weight
    none_arg = None
    seen = []

    def rowwise(xt, xb, opt, W):
        # elementwise only: every output element sees the same arithmetic
        # whatever the batch extent, so chunked == unchunked bit for bit
        assert opt is None
        return xt * W + xb, (xt[0] * xb - xt[-1]) * W

    def call(a, b):
        seen.append((a, b))
        return rowwise(x_tm[:, a:b], x_bm[a:b],
                       ops._opt_slice(none_arg, a, b, 1), W)

    out_tm, out_bm = ops._run_chunks(call, B, (1, 0), concurrent=False)
    ref_tm, ref_bm = rowwise(x_tm, x_bm, None, W)
    assert seen == [(0, 32), (32, 64), (64, 70)]
    assert torch.equal(out_tm, ref_tm)
    assert torch.equal(out_bm, ref_bm)
    assert torch.equal(ops._opt_slice(x_tm, 32, 64, 1), x_tm[:, 32:64])
    assert torch.equal(ops._opt_slice(x_bm, 64, 70, 0), x_bm[64:70])


class _Recorded(Exception):
    pass


class _Recorder:
    def __init__(self):
        self.calls = []

    def cond_gru_fwd(self, *args):
        self.calls.append(args)
        raise _Recorded()


def test_decoder_paths_pack_same_operands(monkeypatch):
    """Training scan and one-step decode hand cond_gru_fwd the same ten
    packed weight operands (arguments 7..16)."""
    from nats_amd.ops import cond_gru as cg
    rec = _Recorder()
    monkeypatch.setattr(cg, "_hip_ext", lambda: rec)
    model = _tiny_model()
    H, A = 20, 12
    C = 2 * H
    T, B, Ts = 2, 3, 5
    g = torch.Generator().manual_seed(1)
    yg = torch.randn(T, B, 2 * H, generator=g)
    yc = torch.randn(T, B, H, generator=g)
    init = torch.randn(B, H, generator=g)
    ctx = torch.randn(Ts, B, C, generator=g)
    pctx = torch.randn(Ts, B, A, generator=g)
    with pytest.raises(_Recorded):
        cg.cond_gru_scan_hip(yg, yc, None, init, ctx, None, pctx, model.P)
    with pytest.raises(_Recorded):
        cg.cond_gru_step_hip(init, yg[0], yc[0], ctx, None, pctx,
                             torch.zeros(B, C), torch.zeros(B, Ts), model.P)
    scan_args, step_args = rec.calls
    assert len(scan_args) == len(step_args) == 19
    for i in range(7, 17):
        a, b = scan_args[i], step_args[i]
        assert a.dtype == b.dtype, i
        assert torch.equal(a, b), i


def test_step_pack_cache_follows_weight_version():
    from nats_amd.ops.cond_gru import _step_packed
    model = _tiny_model()
    first = _step_packed(model.P)
    assert len(first) == 10
    assert _step_packed(model.P) is first
    with torch.no_grad():
        model.P["decoder_W_att"].mul_(1.0)
    second = _step_packed(model.P)
    assert second is not first
    assert _step_packed(model.P) is second
    _bump([model.P["decoder_U_1"]])
    third = _step_packed(model.P)
    assert third is not second
    assert _step_packed(model.P) is third
    # a plain dict cannot carry the cache: packed afresh on every call
    plain = {k: v.detach() for k, v in model.P.items()}
    p1, p2 = _step_packed(plain), _step_packed(plain)
    assert p1 is not p2
    for a, b, c in zip(p1, p2, third):
        assert torch.equal(a, b) and torch.equal(a, c)


def test_stepper_cache_policy():
    """Steppers are built but never captured, so this needs no GPU."""
    from nats_amd.decode import graph
    model = _tiny_model()
    C, A, k = 40, 12, 3
    g = torch.Generator().manual_seed(2)

    def plain(Ts):
        ctx0 = torch.randn(Ts, 1, C, generator=g)
        pctx0 = torch.randn(Ts, 1, A, generator=g)
        return graph.get_stepper(model, ctx0, pctx0, k), ctx0, pctx0

    def batched(Ts, S=2):
        return graph.get_batched_stepper(
            model, torch.randn(Ts, S, C, generator=g), torch.ones(Ts, S),
            torch.randn(Ts, S, A, generator=g), S * k)

    def cached():
        return [v for kk, v in graph._STEPPER_CACHE[model].items()
                if kk != "__ver__"]

    # same (Ts, k): same object, context refreshed
    s1, _, _ = plain(4)
    s1b, ctx0, pctx0 = plain(4)
    assert s1b is s1
    assert torch.equal(s1.ctx, ctx0.expand(4, k, C))
    assert torch.equal(s1.pctx, pctx0.expand(4, k, A))

    # eight distinct Ts keep the first entry; a batched stepper does not
    # count against them; the ninth plain one evicts the oldest
    for Ts in range(5, 12):
        plain(Ts)
    assert len(cached()) == 8 and any(s is s1 for s in cached())
    b1 = batched(4)
    assert batched(4) is b1
    assert len(cached()) == 9 and any(s is s1 for s in cached())
    s12, _, _ = plain(12)
    assert len(cached()) == 9
    assert not any(s is s1 for s in cached())
    assert any(s is b1 for s in cached())

    # any in-place parameter update, or an epoch bump, drops everything
    with torch.no_grad():
        model.P["Wemb"].mul_(1.0)
    s2, _, _ = plain(12)
    assert s2 is not s12
    assert len(graph._STEPPER_CACHE[model]) == 2
    assert cached()[0] is s2
    _bump([model.P["ff_state_b"]])
    b2 = batched(4)
    assert b2 is not b1
    assert len(graph._STEPPER_CACHE[model]) == 2
    assert cached()[0] is b2
