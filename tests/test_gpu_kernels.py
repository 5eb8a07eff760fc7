"""GPU numerics tests: every HIP kernel vs the plain-PyTorch fp32 oracle
(nats_amd.ops.eager). All marked gpu; run with `pytest -m gpu` on MI355X."""

import numpy
import pytest
import torch

from kernel_ref import _cond_inputs, _gru_inputs, assert_grad_close

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ext():
    from nats_amd.ops import _hip_ext
    m = _hip_ext()
    assert m is not None, "HIP extension must build/load on a GPU box"
    return m


def test_mfma_fragment_layout(ext):
    """Transpose-detecting self-test of the MFMA lane maps (asymmetric B)."""
    torch.manual_seed(0)
    M, K, N = 32, 64, 48
    A = torch.randn(M, K, device="cuda").to(torch.bfloat16)
    B = torch.randn(K, N, device="cuda").to(torch.bfloat16)
    C = ext.mfma_gemm_bt(A.contiguous(), B.t().contiguous())
    ref = (A.float() @ B.float())
    torch.testing.assert_close(C, ref, rtol=2e-2, atol=2e-2)


@pytest.mark.parametrize("with_mask", [False, True])
@pytest.mark.parametrize("shape", [(13, 5, 48), (40, 20, 96), (7, 32, 16)])
def test_gru_scan_forward(ext, shape, with_mask):
    from nats_amd.ops import eager
    from nats_amd.ops.gru import gru_scan_hip
    T, B, H = shape
    xg, xc, U, Ux, mask = _gru_inputs(T, B, H, with_mask=with_mask)
    ref = eager.gru_scan(xg, xc, mask, U, Ux)
    out = gru_scan_hip(xg.cuda(), xc.cuda(),
                       mask.cuda() if mask is not None else None,
                       U.cuda(), Ux.cuda())
    # bf16 h-chain drift over long T puts a handful of near-zero elements
    # slightly past tight bounds; 0.06 absolute is ~15 bf16 ulps at |h|<=1
    torch.testing.assert_close(out.cpu(), ref, rtol=0.1, atol=6e-2)


def test_gru_scan_backward(ext):
    from nats_amd.ops import eager
    from nats_amd.ops.gru import gru_scan_hip
    T, B, H = 11, 6, 32
    xg, xc, U, Ux, mask = _gru_inputs(T, B, H, seed=3)

    # fp32 eager oracle
    ref_in = [t.clone().requires_grad_(True) for t in (xg, xc, U, Ux)]
    h_ref = eager.gru_scan(ref_in[0], ref_in[1], mask, ref_in[2], ref_in[3])
    loss_w = torch.randn_like(h_ref)
    (h_ref * loss_w).sum().backward()

    hip_in = [t.clone().cuda().requires_grad_(True) for t in (xg, xc, U, Ux)]
    h_hip = gru_scan_hip(hip_in[0], hip_in[1], mask.cuda(), hip_in[2],
                         hip_in[3])
    (h_hip * loss_w.cuda()).sum().backward()

    for r, h, name in zip(ref_in, hip_in, ["xg", "xc", "U", "Ux"]):
        assert_grad_close(r.grad, h.grad.cpu().float(), name, rel=0.06)


@pytest.mark.parametrize("V", [120, 3001, 30000])
def test_softmax_ce(ext, V):
    """V=120 regresses the small-vocab reduce (idle threads hold -inf)."""
    from nats_amd.ops import eager
    from nats_amd.ops.softmax_ce import softmax_xent_hip
    torch.manual_seed(1)
    N = 37
    logits = (5 * torch.randn(N, V)).to(torch.bfloat16)
    targets = torch.randint(0, V, (N,))
    ref_l = logits.float().clone().requires_grad_(True)
    ref = eager.softmax_xent(ref_l, targets)
    dn = torch.randn(N)
    (ref * dn).sum().backward()

    hip_l = logits.cuda().clone().requires_grad_(True)
    out = softmax_xent_hip(hip_l, targets.cuda())
    torch.testing.assert_close(out.cpu(), ref.detach(), rtol=2e-2, atol=2e-2)
    (out * dn.cuda()).sum().backward()
    a, b = ref_l.grad, hip_l.grad.cpu().float()
    assert (a - b).abs().max() < 2e-2


def test_model_forward_gpu_vs_cpu():
    """Full model: GPU (HIP gru + fused CE under autocast) vs CPU fp32."""
    from nats_amd.data.prepare import prepare_data
    from nats_amd.models.distraction import NatsModel, default_options
    opts = default_options(dim_word=16, dim=32, dim_att=8, n_words=120)
    model = NatsModel(opts, seed=9)
    rng = numpy.random.RandomState(0)
    xs = [list(rng.randint(2, 120, size=rng.randint(4, 12))) for _ in range(6)]
    ys = [list(rng.randint(2, 120, size=rng.randint(3, 8))) for _ in range(6)]
    arrs = [torch.from_numpy(a) for a in prepare_data(xs, ys)]
    cost_cpu = model(*arrs)

    gmodel = NatsModel(opts, params=model.get_params()).cuda()
    with torch.autocast("cuda", dtype=torch.bfloat16):
        cost_gpu = gmodel(*[a.cuda() for a in arrs])
    rel = ((cost_cpu - cost_gpu.float().cpu()).abs() / cost_cpu.abs()).max()
    assert rel < 0.05, float(rel)


def test_model_train_step_gpu():
    """One full train step (fwd+bwd+clip+fused adadelta) on the HIP path:
    finite cost, finite grads, params move."""
    from nats_amd.data.synthetic import synthetic_batch
    from nats_amd.engine.optim import build_optimizer
    from nats_amd.models.distraction import NatsModel, default_options
    opts = default_options(dim_word=24, dim=48, dim_att=12, n_words=500)
    model = NatsModel(opts, seed=2).cuda()
    opt = build_optimizer("adadelta", list(model.P.items()), clip_c=1.0)
    rng = numpy.random.RandomState(3)
    x, xm, y, ym = [torch.from_numpy(a).cuda()
                    for a in synthetic_batch(rng, 8, 30, 10, 500)]
    # watch a parameter with large gradients (encoder_U's first adadelta
    # step is ~1e-8 here — below fp32 ulp at its magnitude)
    before = model.P["ff_logit_b"].detach().clone()
    costs = []
    for _ in range(3):
        opt.zero_grad()
        with torch.autocast("cuda", dtype=torch.bfloat16):
            cost = model(x, xm, y, ym).mean()
        cost.backward()
        opt.step()
        costs.append(float(cost))
    assert all(numpy.isfinite(c) for c in costs), costs
    assert costs[-1] < costs[0], costs
    assert not torch.equal(before, model.P["ff_logit_b"].detach())


def test_native_extension_is_used_on_gpu():
    """Fail-loud contract: GPU tensors must NOT silently run eager."""
    import nats_amd.ops as ops
    assert ops._hip_ext() is not None
    import os
    assert not os.environ.get("NATS_AMD_FORCE_EAGER")


@pytest.mark.parametrize("with_masks", [False, True])
def test_cond_gru_forward(ext, with_masks):
    from nats_amd.ops import eager
    from nats_amd.ops.cond_gru import cond_gru_scan_hip
    model, yg, yc, mask, init, ctx, ctx_mask = _cond_inputs(
        with_masks=with_masks)
    P = {k: v.detach() for k, v in model.P.items()}
    pctx = ctx @ P["decoder_Wc_att"] + P["decoder_b_att"]
    ref = eager.cond_gru_scan(yg, yc, mask, init, ctx, ctx_mask, pctx, P)

    Pg = {k: v.cuda() for k, v in P.items()}
    out = cond_gru_scan_hip(
        yg.cuda(), yc.cuda(), mask.cuda() if mask is not None else None,
        init.cuda(), ctx.cuda(),
        ctx_mask.cuda() if ctx_mask is not None else None, pctx.cuda(), Pg)
    names = ["h2s", "ctxs", "alphas", "acc_ctx", "acc_alpha"]
    for r, o, n in zip(ref, out, names):
        torch.testing.assert_close(o.cpu(), r, rtol=5e-2, atol=5e-2,
                                   msg=lambda m, n=n: "%s: %s" % (n, m))


@pytest.mark.parametrize("with_masks", [True, False])
def test_cond_attn_softmax_all_16_waves(ext, with_masks):
    """Ts > 1024: every one of the 16 waves of the 1024-thread attention
    softmax block holds a partial max / sum. The kernel normalises in fp32
    by its own block sum, so a dropped or corrupted wave partial shows as a
    row-sum error of order 1/16."""
    from nats_amd.ops import eager
    from nats_amd.ops.cond_gru import cond_gru_scan_hip
    model, yg, yc, mask, init, ctx, ctx_mask = _cond_inputs(
        T=2, B=3, H=32, Ts=1100, A=12, with_masks=with_masks)
    P = {k: v.detach() for k, v in model.P.items()}
    pctx = ctx @ P["decoder_Wc_att"] + P["decoder_b_att"]
    ref = eager.cond_gru_scan(yg, yc, mask, init, ctx, ctx_mask, pctx, P)[2]
    Pg = {k: v.cuda() for k, v in P.items()}
    alphas = cond_gru_scan_hip(
        yg.cuda(), yc.cuda(), mask.cuda() if with_masks else None,
        init.cuda(), ctx.cuda(), ctx_mask.cuda() if with_masks else None,
        pctx.cuda(), Pg)[2].cpu().float()
    assert bool(torch.isfinite(alphas).all())
    keep = ctx_mask.t().unsqueeze(0) if with_masks else torch.ones(())
    rows = (alphas * keep).sum(-1)
    torch.testing.assert_close(rows, torch.ones_like(rows), rtol=0,
                               atol=1e-3)
    if with_masks:
        # Relative match with the eager oracle over entries >= 1e-6. The
        # build before the shared block reduction (right values, by luck of
        # LDS allocation granularity) measured a maximum relative error of
        # 2.996e-3 at this shape on MI355X; the bound is twice that.
        sel = ref >= 1e-6
        rel = ((alphas - ref).abs() / ref.clamp_min(1e-30))[sel]
        print("alphas max rel err vs eager: %.4e" % float(rel.max()))
        assert float(rel.max()) <= 5.99e-3


def test_cond_gru_backward(ext):
    from nats_amd.ops import eager
    from nats_amd.ops.cond_gru import cond_gru_scan_hip
    model, yg, yc, mask, init, ctx, ctx_mask = _cond_inputs(T=6, B=4, H=24,
                                                            Ts=8, A=10)
    keys = ["decoder_U", "decoder_Ux", "decoder_U_1", "decoder_W_1",
            "decoder_b_1", "decoder_Wx_1", "decoder_Ux_1", "decoder_bx_1",
            "decoder_W_att", "decoder_U_att", "decoder_c_att",
            "decoder_W_con", "decoder_U_con", "decoder_D_wei"]

    def run(dev, fn):
        P = {k: v.detach().clone().to(dev).requires_grad_(k in keys)
             for k, v in model.P.items()}
        ins = [t.clone().to(dev).requires_grad_(True)
               for t in (yg, yc, init, ctx)]
        m_ = mask.to(dev)
        cm = ctx_mask.to(dev)
        pctx = ins[3] @ P["decoder_Wc_att"] + P["decoder_b_att"]
        h2s, ctxs, alphas, accC, accA = fn(ins[0], ins[1], m_, ins[2],
                                           ins[3], cm, pctx, P)
        # loss weights drawn on CPU so both devices optimise the SAME loss
        g2 = torch.Generator().manual_seed(0)
        w1 = torch.randn(h2s.shape, generator=g2).to(dev)
        w2 = torch.randn(ctxs.shape, generator=g2).to(dev)
        ((h2s.float() * w1).sum() + (ctxs.float() * w2).sum()).backward()
        grads = {k: P[k].grad.cpu().float() for k in keys}
        gins = {n: t.grad.cpu().float()
                for n, t in zip(["yg", "yc", "init", "ctx"], ins)}
        return grads, gins

    rg, ri = run("cpu", eager.cond_gru_scan)
    hg, hi = run("cuda", cond_gru_scan_hip)

    gscale = max(float(v.abs().max()) for v in rg.values())
    for k in rg:
        assert_grad_close(rg[k], hg[k], k, rel=0.08, global_scale=gscale)
    for k in ri:
        assert_grad_close(ri[k], hi[k], k, rel=0.08, global_scale=gscale)


def test_cond_gru_one_step(ext):
    from nats_amd.ops import eager
    from nats_amd.ops.cond_gru import cond_gru_step_hip
    model, yg, yc, mask, init, ctx, ctx_mask = _cond_inputs(T=1, B=3, H=16,
                                                            Ts=6, A=8,
                                                            with_masks=False)
    P = {k: v.detach() for k, v in model.P.items()}
    pctx = ctx @ P["decoder_Wc_att"] + P["decoder_b_att"]
    C = ctx.shape[2]
    acc_c = torch.randn(3, C) * 0.1
    acc_a = torch.rand(3, 6)
    ref = eager.cond_gru_step(init, yg[0], yc[0], ctx, None, pctx,
                              acc_c, acc_a, P)
    Pg = {k: v.cuda() for k, v in P.items()}
    out = cond_gru_step_hip(init.cuda(), yg[0].cuda(), yc[0].cuda(),
                            ctx.cuda(), None, pctx.cuda(), acc_c.cuda(),
                            acc_a.cuda(), Pg)
    for r, o in zip(ref, out):
        torch.testing.assert_close(o.cpu(), r, rtol=5e-2, atol=5e-2)


@pytest.mark.parametrize("path", ["persistent", "per-step"])
def test_gru_scan_bidir(ext, path, monkeypatch):
    """Fused bidirectional scan vs two eager scans (fwd + grads), on the
    persistent kernels and on the per-step fallback bodies (otherwise only
    reached for H > 1504)."""
    from nats_amd.ops import eager
    from nats_amd.ops.gru import gru_scan_bidir_hip
    T, B, H = 15, 6, 48
    if path == "per-step":
        # the extension reads the variable on every call
        monkeypatch.setenv("NATS_NO_PERSISTENT", "1")
        assert not ext.gru_persistent_ok(H, B)
    else:
        assert ext.gru_persistent_ok(H, B)
    xg0, xc0, U0, Ux0, mask0 = _gru_inputs(T, B, H, seed=11)
    xg1, xc1, U1, Ux1, _ = _gru_inputs(T, B, H, seed=12)
    mask1 = mask0.flip(0)

    ref_in = [t.clone().requires_grad_(True)
              for t in (xg0, xc0, U0, Ux0, xg1, xc1, U1, Ux1)]
    r0 = eager.gru_scan(ref_in[0], ref_in[1], mask0, ref_in[2], ref_in[3])
    r1 = eager.gru_scan(ref_in[4], ref_in[5], mask1, ref_in[6], ref_in[7])
    g2 = torch.Generator().manual_seed(0)
    w0 = torch.randn(r0.shape, generator=g2)
    w1 = torch.randn(r1.shape, generator=g2)
    ((r0 * w0).sum() + (r1 * w1).sum()).backward()

    hip_in = [t.clone().cuda().requires_grad_(True)
              for t in (xg0, xc0, U0, Ux0, xg1, xc1, U1, Ux1)]
    h0, h1 = gru_scan_bidir_hip(hip_in[0], hip_in[1], mask0.cuda(), hip_in[2],
                                hip_in[3], hip_in[4], hip_in[5], mask1.cuda(),
                                hip_in[6], hip_in[7])
    ((h0 * w0.cuda()).sum() + (h1 * w1.cuda()).sum()).backward()

    torch.testing.assert_close(h0.cpu(), r0, rtol=0.1, atol=6e-2)
    torch.testing.assert_close(h1.cpu(), r1, rtol=0.1, atol=6e-2)
    for r, h, name in zip(ref_in, hip_in,
                          ["xg0", "xc0", "U0", "Ux0", "xg1", "xc1", "U1",
                           "Ux1"]):
        assert_grad_close(r.grad, h.grad.cpu().float(), name, rel=0.08)


@pytest.mark.parametrize("H,B,expected", [
    (1000, 64, True),    # 4 jobs x 63 tiles = 252 blocks of the 256 grid
    (1024, 64, True),    # 4 x 64 = 256: exactly the grid
    (1025, 64, False),   # 4 x 65 = 260 claim slots > 256 blocks
    (1025, 32, True),    # 2 jobs: 130 slots
    (1504, 32, True),    # 96*1504 + 6528 = 150912 B <= 150 KiB; 2*94 <= 192
    (1505, 32, False),   # Hpad 1536: 96*1536 + 6528 = 153984 B > 150 KiB
])
def test_gru_persistent_plan_truth_table(ext, H, B, expected):
    """Host-only: which (H, B) the persistent bidirectional scans accept.
    ngrp = ceil(H/16), jobs = 2*ceil(B/32); needs jobs*ngrp <= 256 (grid),
    2*ngrp <= 192, 96*Hpad + 6528 <= 150 KiB and 32*K3pad + 6528 <= 150 KiB."""
    assert ext.gru_persistent_ok(H, B) is expected


def test_gru_persistent_plan_rejects_bad_xpd(ext, monkeypatch):
    """Host-only: NATS_XPD (preferred XCDs per job) divides an XCC id in the
    claim, so anything but an integer in [1, 8] must raise, naming the
    variable; a valid value leaves the answer as without it."""
    expected = ext.gru_persistent_ok(1000, 20)
    for bad in ("0", "9", "two"):
        monkeypatch.setenv("NATS_XPD", bad)
        with pytest.raises(RuntimeError, match="NATS_XPD"):
            ext.gru_persistent_ok(1000, 20)
    monkeypatch.setenv("NATS_XPD", "2")
    assert ext.gru_persistent_ok(1000, 20) is expected


def test_gru_scan_bidir_wide_hidden_large_batch(ext):
    """B > 32 with H in (1024, 1504]: four persistent jobs would need more
    claim slots than the grid has blocks, so the dispatcher must take the
    sequential 32-row-chunk route (finite, matching eager)."""
    from nats_amd import ops
    from nats_amd.ops import eager
    T, B, H = 3, 40, 1040
    assert not ext.gru_persistent_ok(H, B)
    g = torch.Generator().manual_seed(21)
    ins = []
    for _ in range(2):
        ins += [torch.randn(T, B, 2 * H, generator=g),
                torch.randn(T, B, H, generator=g),
                torch.randn(H, 2 * H, generator=g) * H ** -0.5,
                torch.randn(H, H, generator=g) * H ** -0.5]
    lens = torch.randint(1, T + 1, (B,), generator=g)
    mask0 = (torch.arange(T).unsqueeze(1) < lens.unsqueeze(0)).float()
    mask1 = mask0.flip(0)
    r0 = eager.gru_scan(ins[0], ins[1], mask0, ins[2], ins[3])
    r1 = eager.gru_scan(ins[4], ins[5], mask1, ins[6], ins[7])
    c = [t.cuda() for t in ins]
    with torch.no_grad():
        h0, h1 = ops.gru_scan_bidir(c[0], c[1], mask0.cuda(), c[2], c[3],
                                    c[4], c[5], mask1.cuda(), c[6], c[7])
    for h, r in ((h0, r0), (h1, r1)):
        assert bool(torch.isfinite(h).all())
        torch.testing.assert_close(h.cpu(), r, rtol=0.1, atol=6e-2)


def test_graph_decode_matches_plain(ext):
    """hipGraph-captured beam decode must produce the same tokens as the
    plain per-step path."""
    from nats_amd.decode.beam import gen_sample
    from nats_amd.models.distraction import NatsModel, default_options
    opts = default_options(dim_word=24, dim=48, dim_att=12, n_words=300)
    model = NatsModel(opts, seed=4).cuda().eval()
    torch.manual_seed(0)
    x = torch.randint(2, 300, (15, 1), device="cuda")
    x[-1] = 0
    s_plain, c_plain, _ = gen_sample(model, x, k=4, maxlen=12,
                                     stochastic=False, use_unk=True)
    s_graph, c_graph, _ = gen_sample(model, x, k=4, maxlen=12,
                                     stochastic=False, use_unk=True,
                                     use_graph=True)
    assert s_plain == s_graph, (s_plain, s_graph)
    for a, b in zip(c_plain, c_graph):
        assert abs(a - b) < 1e-3


def test_gpu_rerank_matches_numpy(ext):
    """distraction_penalties_gpu vs the scipy-convention numpy oracle."""
    import numpy as np
    from nats_amd.decode.beam import (distraction_penalties,
                                      distraction_penalties_gpu)
    rng = np.random.RandomState(0)
    n, k, Ts, C, H = 4, 3, 7, 10, 6
    ha = rng.rand(n, k, Ts).astype("float32") + 1e-3
    hc = rng.randn(n, k, C).astype("float32")
    hs = rng.randn(n, k, H).astype("float32")
    ca = rng.rand(k, Ts).astype("float32") + 1e-3
    cc = rng.randn(k, C).astype("float32")
    cs = rng.randn(k, H).astype("float32")
    # numpy oracle expects per-hyp history lists
    la = [[ha[t, i] for t in range(n)] for i in range(k)]
    lc = [[hc[t, i] for t in range(n)] for i in range(k)]
    ls = [[hs[t, i] for t in range(n)] for i in range(k)]
    a_s, c_s, s_s = distraction_penalties(la, lc, ls, ca, cc, cs,
                                          1.3, 0.7, 2.1)
    ref = a_s + c_s + s_s
    got = distraction_penalties_gpu(
        torch.from_numpy(ha).cuda(), torch.from_numpy(hc).cuda(),
        torch.from_numpy(hs).cuda(), torch.from_numpy(ca).cuda(),
        torch.from_numpy(cc).cuda(), torch.from_numpy(cs).cuda(),
        1.3, 0.7, 2.1).cpu().numpy()
    np.testing.assert_allclose(got, ref, rtol=1e-4, atol=1e-5)


def test_beam_distraction_gpu_runs(ext):
    from nats_amd.decode.beam import gen_sample
    from nats_amd.models.distraction import NatsModel, default_options
    opts = default_options(dim_word=24, dim=48, dim_att=12, n_words=300)
    model = NatsModel(opts, seed=4).cuda().eval()
    torch.manual_seed(1)
    x = torch.randint(2, 300, (12, 1), device="cuda")
    x[-1] = 0
    s, c, al = gen_sample(model, x, k=4, maxlen=10, stochastic=False,
                          use_unk=True, kl_factor=0.6, ctx_factor=0.6,
                          state_factor=0.6)
    assert len(s) >= 1 and all(cc > 0 for cc in c)


def test_fused_adadelta_matches_cpu(ext):
    """fused clip+adadelta HIP kernel vs the CPU reference optimizer."""
    from nats_amd.engine.optim import Adadelta
    from nats_amd.ops.optim import FusedAdadelta
    torch.manual_seed(0)
    shapes = [(70000,), (123, 45), (7,), (300, 11)]
    cpu_params = [torch.nn.Parameter(torch.randn(*s)) for s in shapes]
    gpu_params = [torch.nn.Parameter(p.detach().clone().cuda())
                  for p in cpu_params]
    grads = [torch.randn(*s) for s in shapes]
    cpu_opt = Adadelta([("p%d" % i, p) for i, p in enumerate(cpu_params)],
                       clip_c=1.0)
    gpu_opt = FusedAdadelta([("p%d" % i, p)
                             for i, p in enumerate(gpu_params)], clip_c=1.0)
    for it in range(3):
        for p, g in zip(cpu_params, grads):
            p.grad = (g * (it + 1)).clone()
        for p, g in zip(gpu_params, grads):
            p.grad = (g * (it + 1)).clone().cuda()
        n_cpu = cpu_opt.step()
        n_gpu = gpu_opt.step()
        assert abs(float(n_cpu) - float(n_gpu)) < 1e-2 * float(n_cpu)
    for pc, pg in zip(cpu_params, gpu_params):
        torch.testing.assert_close(pg.detach().cpu(), pc.detach(),
                                   rtol=1e-4, atol=1e-6)


def test_train_entrypoint_gpu(tmp_path_factory):
    """End-to-end train() on the GPU HIP path: toy corpus, few updates,
    checkpoint written, finite validation error."""
    import os
    from nats_amd.data.synthetic import make_toy_corpus
    from nats_amd.engine.trainer import train
    d = str(tmp_path_factory.mktemp("toy_gpu"))
    make_toy_corpus(d, n_train=64, n_valid=16, n_test=8)
    saveto = os.path.join(d, "model.npz")
    err = train(dim_word=16, dim=32, dim_att=8, n_words=64, maxlen=50,
                batch_size=8, valid_batch_size=8, saveto=saveto,
                datasets=[os.path.join(d, "toy_train_input.txt"),
                          os.path.join(d, "toy_train_output.txt")],
                valid_datasets=[os.path.join(d, "toy_validation_input.txt"),
                                os.path.join(d, "toy_validation_output.txt")],
                dictionary=os.path.join(d, "toy_train_input.txt.pkl"),
                validFreq=1000, saveFreq=6, sampleFreq=4, dispFreq=2,
                finish_after=6, clip_c=1.0, device="cuda", seed=5)
    assert numpy.isfinite(err)
    assert os.path.exists(saveto)


def test_large_batch_chunking(ext):
    """B > 32 runs through exact per-chunk passes (full model fwd+bwd)."""
    from nats_amd.data.synthetic import synthetic_batch
    from nats_amd.models.distraction import NatsModel, default_options
    opts = default_options(dim_word=16, dim=32, dim_att=8, n_words=200)
    model = NatsModel(opts, seed=6)
    rng = numpy.random.RandomState(1)
    x, xm, y, ym = [torch.from_numpy(a)
                    for a in synthetic_batch(rng, 48, 12, 6, 200)]
    ref = model(x, xm, y, ym)  # CPU fp32 oracle
    gm = NatsModel(opts, params=model.get_params()).cuda()
    with torch.autocast("cuda", dtype=torch.bfloat16):
        cost = gm(x.cuda(), xm.cuda(), y.cuda(), ym.cuda())
    rel = ((cost.float().cpu() - ref).abs() / ref.abs()).max()
    assert cost.shape == (48,)
    assert float(rel) < 0.05, float(rel)
    cost.mean().backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all()
               for p in gm.parameters())


def test_cond_gru_large_dim_splitk_paths(ext):
    """H=1024 drives the split-K decoder paths (K1=3072 >= 2048 selects
    cond_gru1_gemm_splitk; Hpad=1024 selects nats_gru2_gemm_splitk; the
    pstate split-K + A-chunked escore/scatter run at every size) — the
    small-dim tests above only cover the fused variants."""
    from nats_amd.ops import eager
    from nats_amd.ops.cond_gru import cond_gru_scan_hip
    model, yg, yc, mask, init, ctx, ctx_mask = _cond_inputs(
        T=3, B=4, H=1024, Ts=16, A=16, E=8, seed=11, with_masks=True)
    P = {k: v.detach() for k, v in model.P.items()}
    pctx = ctx @ P["decoder_Wc_att"] + P["decoder_b_att"]
    ref = eager.cond_gru_scan(yg, yc, mask, init, ctx, ctx_mask, pctx, P)

    Pg = {k: v.cuda().requires_grad_() for k, v in P.items()}
    ygc = yg.cuda().requires_grad_()
    pctx_g = ctx.cuda() @ Pg["decoder_Wc_att"] + Pg["decoder_b_att"]
    out = cond_gru_scan_hip(ygc, yc.cuda(), mask.cuda(), init.cuda(),
                            ctx.cuda(), ctx_mask.cuda(), pctx_g, Pg)
    for o, r in zip(out[:3], ref[:3]):
        torch.testing.assert_close(o.float().cpu(), r, rtol=0.1, atol=6e-2)

    # backward parity on a weighted scalar (exercises the bwd chain at the
    # same large shape)
    w = torch.randn(out[0].shape)
    loss = (out[0] * w.cuda()).sum()
    loss.backward()
    P_ref = {k: v.detach().clone().requires_grad_() for k, v in P.items()}
    yg_ref = yg.detach().clone().requires_grad_()
    pctx_ref = ctx @ P_ref["decoder_Wc_att"] + P_ref["decoder_b_att"]
    ref2 = eager.cond_gru_scan(yg_ref, yc, mask, init, ctx, ctx_mask,
                               pctx_ref, P_ref)
    (ref2[0] * w).sum().backward()
    torch.testing.assert_close(ygc.grad.float().cpu(), yg_ref.grad,
                               rtol=0.1, atol=8e-2)
    for k in ("decoder_U_1", "decoder_W_att", "decoder_U", "decoder_D_wei"):
        torch.testing.assert_close(Pg[k].grad.float().cpu(), P_ref[k].grad,
                                   rtol=0.15, atol=0.1)


def test_batched_decode_matches_single_gpu(ext):
    """Device-resident batched beams == per-sentence gen_sample on the
    HIP kernel path (the CPU parity test covers eager; this pins the
    on-device top-k + index_select bookkeeping)."""
    from nats_amd.decode.batched import gen_sample_batched
    from nats_amd.decode.beam import gen_sample
    from nats_amd.models.distraction import NatsModel, default_options
    opts = default_options(dim_word=16, dim=32, dim_att=12, n_words=90)
    model = NatsModel(opts, seed=31).eval()
    with torch.no_grad():
        for key in ("ff_logit_lstm_W", "ff_logit_ctx_W", "ff_logit_prev_W",
                    "ff_logit_W"):
            model.P[key].mul_(50.0)
    model = model.cuda()
    g = torch.Generator().manual_seed(4)
    xs = []
    for n in (9, 13, 6):
        x = torch.randint(2, 90, (n, 1), generator=g)
        x[-1] = 0
        xs.append(x.cuda())
    batched = gen_sample_batched(model, xs, k=3, maxlen=8, use_unk=True)
    for x, (bs, bc, ba) in zip(xs, batched):
        ss, sc, sa = gen_sample(model, x, k=3, maxlen=8, stochastic=False,
                                use_unk=True)
        assert sorted(map(tuple, bs)) == sorted(map(tuple, ss))
        numpy.testing.assert_allclose(sorted(bc), sorted(sc), rtol=2e-3,
                                      atol=1e-3)


def test_stacked_encoder_gpu_matches_cpu(ext):
    """enc_depth=2 runs layer-2 scans over layer-1 outputs through the
    same HIP path (the longdoc config, BASELINE configs[4])."""
    from nats_amd.models.distraction import NatsModel, default_options
    opts = default_options(dim_word=16, dim=32, dim_att=12, n_words=80,
                           enc_depth=2)
    model = NatsModel(opts, seed=17).eval()
    g = torch.Generator().manual_seed(9)
    x = torch.randint(2, 80, (12, 5), generator=g)
    mask = torch.ones(12, 5)
    with torch.no_grad():
        ctx_cpu, init_cpu = model.encode(x, mask)
        mg = model.cuda()
        ctx_gpu, init_gpu = mg.encode(x.cuda(), mask.cuda())
    torch.testing.assert_close(ctx_gpu.float().cpu(), ctx_cpu,
                               rtol=0.05, atol=2e-2)
    torch.testing.assert_close(init_gpu.float().cpu(), init_cpu,
                               rtol=0.05, atol=2e-2)


def test_embed_gather_scatter(ext):
    """embed.hip gather (+fused shift) and scatter-add backward vs the
    torch indexing oracle (ref nats.py:700-701, 730-734)."""
    torch.manual_seed(4)
    V, E, T, B = 57, 20, 9, 5
    Wemb = torch.randn(V, E)
    ids = torch.randint(0, V, (T, B))
    from nats_amd.ops.embed import embed_gather_hip

    # plain gather + backward
    Wg = Wemb.cuda().requires_grad_(True)
    out = embed_gather_hip(Wg, ids.cuda(), shift=False)
    Wr = Wemb.clone().requires_grad_(True)
    ref = Wr[ids]
    torch.testing.assert_close(out.cpu(), ref.detach())
    dl = torch.randn(T, B, E)
    (ref * dl).sum().backward()
    (out * dl.cuda()).sum().backward()
    torch.testing.assert_close(Wg.grad.cpu(), Wr.grad, rtol=1e-5, atol=1e-5)

    # fused shift variant
    Wg2 = Wemb.cuda().requires_grad_(True)
    out_s = embed_gather_hip(Wg2, ids.cuda(), shift=True)
    Wr2 = Wemb.clone().requires_grad_(True)
    emb = Wr2[ids]
    ref_s = torch.zeros_like(emb)
    ref_s[1:] = emb[:-1]
    torch.testing.assert_close(out_s.cpu(), ref_s.detach())
    (ref_s * dl).sum().backward()
    (out_s * dl.cuda()).sum().backward()
    torch.testing.assert_close(Wg2.grad.cpu(), Wr2.grad, rtol=1e-5,
                               atol=1e-5)


def test_batched_decode_graph_matches_ungraphed(ext):
    """hipGraph-captured batched f_next == the uncaptured batched path
    (the production decode path is now captured)."""
    from nats_amd.decode.batched import gen_sample_batched
    from nats_amd.models.distraction import NatsModel, default_options
    opts = default_options(dim_word=16, dim=32, dim_att=12, n_words=90)
    model = NatsModel(opts, seed=13).eval()
    with torch.no_grad():
        for key in ("ff_logit_lstm_W", "ff_logit_ctx_W", "ff_logit_prev_W",
                    "ff_logit_W"):
            model.P[key].mul_(50.0)
    model = model.cuda()
    g = torch.Generator().manual_seed(8)
    xs = []
    for n in (11, 7, 14, 5):
        x = torch.randint(2, 90, (n, 1), generator=g)
        x[-1] = 0
        xs.append(x.cuda())
    plain = gen_sample_batched(model, xs, k=3, maxlen=9, use_unk=True,
                               use_graph=False)
    graphed = gen_sample_batched(model, xs, k=3, maxlen=9, use_unk=True,
                                 use_graph=True)
    for (ps, pc, _), (gs, gc, _) in zip(plain, graphed):
        assert sorted(map(tuple, ps)) == sorted(map(tuple, gs))
        numpy.testing.assert_allclose(sorted(pc), sorted(gc), rtol=2e-3,
                                      atol=1e-3)


def test_pack_kernels_match_torch(ext):
    """pack.hip fused packers vs the torch chains they replaced (the
    packed layouts are consumed by every MFMA kernel — a layout bug
    would corrupt training silently)."""
    from nats_amd.ops import gru as g
    from nats_amd.ops import cond_gru as cg
    torch.manual_seed(11)
    H, C, A = 72, 144, 20  # deliberately non-multiples of 32
    U = torch.randn(H, 2 * H, device="cuda")
    Ux = torch.randn(H, H, device="cuda")
    U_1 = torch.randn(H, 2 * H, device="cuda")
    W_1 = torch.randn(C, 2 * H, device="cuda")
    Ux_1 = torch.randn(H, H, device="cuda")
    Wx_1 = torch.randn(C, H, device="cuda")
    W_att = torch.randn(H, A, device="cuda")
    Hpad = (H + 31) // 32 * 32
    Cpad = (C + 31) // 32 * 32
    Apad = (A + 31) // 32 * 32

    # CPU inputs always take the torch pack path (reference)
    ref_fwd = g.pack_fwd_weights(U.cpu(), Ux.cpu())
    ref_bwd = g.pack_bwd_weights(U.cpu(), Ux.cpu())
    ref_g1 = cg.pack_gru1_weights(U_1.cpu(), W_1.cpu(), Ux_1.cpu(),
                                  Wx_1.cpu(), Hpad, Cpad)
    ref_att_t = cg._pack_rows(W_att.cpu().t(), (A + 15) // 16 * 16, Hpad)
    ref_att = cg._pack_rows(W_att.cpu(), (H + 15) // 16 * 16, Apad)

    torch.testing.assert_close(g.pack_fwd_weights(U, Ux).cpu(), ref_fwd)
    torch.testing.assert_close(g.pack_bwd_weights(U, Ux).cpu(), ref_bwd)
    torch.testing.assert_close(
        cg.pack_gru1_weights(U_1, W_1, Ux_1, Wx_1, Hpad, Cpad).cpu(), ref_g1)
    torch.testing.assert_close(
        cg._pack_rows(W_att.t(), (A + 15) // 16 * 16, Hpad).cpu(), ref_att_t)
    torch.testing.assert_close(
        cg._pack_rows(W_att, (H + 15) // 16 * 16, Apad).cpu(), ref_att)


@pytest.mark.parametrize("B", [48, 64])
def test_gru_scan_bidir_large_batch(ext, B):
    """B>32 bidirectional scans run as concurrent 32-row chunk jobs in
    ONE persistent launch (ragged batch chunking);
    parity vs the eager oracle, forward and grads."""
    from nats_amd.ops import eager, gru_scan_bidir
    T, H = 18, 96
    g = torch.Generator().manual_seed(21)
    xg0 = torch.randn(T, B, 2 * H, generator=g)
    xc0 = torch.randn(T, B, H, generator=g)
    xg1 = torch.randn(T, B, 2 * H, generator=g)
    xc1 = torch.randn(T, B, H, generator=g)
    U0 = 0.3 * torch.randn(H, 2 * H, generator=g)
    Ux0 = 0.3 * torch.randn(H, H, generator=g)
    U1 = 0.3 * torch.randn(H, 2 * H, generator=g)
    Ux1 = 0.3 * torch.randn(H, H, generator=g)
    lens = torch.randint(2, T + 1, (B,), generator=g)
    mask0 = (torch.arange(T).unsqueeze(1) < lens.unsqueeze(0)).float()
    mask1 = mask0.flip(0)

    ref_in = [t.clone().requires_grad_(True)
              for t in (xg0, xc0, U0, Ux0, xg1, xc1, U1, Ux1)]
    r0 = eager.gru_scan(ref_in[0], ref_in[1], mask0, ref_in[2], ref_in[3])
    r1 = eager.gru_scan(ref_in[4], ref_in[5], mask1, ref_in[6], ref_in[7])
    g2 = torch.Generator().manual_seed(1)
    w0 = torch.randn(r0.shape, generator=g2)
    w1 = torch.randn(r1.shape, generator=g2)
    ((r0 * w0).sum() + (r1 * w1).sum()).backward()

    hip_in = [t.clone().cuda().requires_grad_(True)
              for t in (xg0, xc0, U0, Ux0, xg1, xc1, U1, Ux1)]
    h0, h1 = gru_scan_bidir(hip_in[0], hip_in[1], mask0.cuda(), hip_in[2],
                            hip_in[3], hip_in[4], hip_in[5], mask1.cuda(),
                            hip_in[6], hip_in[7])
    ((h0 * w0.cuda()).sum() + (h1 * w1.cuda()).sum()).backward()

    torch.testing.assert_close(h0.cpu(), r0, rtol=0.1, atol=6e-2)
    torch.testing.assert_close(h1.cpu(), r1, rtol=0.1, atol=6e-2)
    for r, h, name in zip(ref_in, hip_in,
                          ["xg0", "xc0", "U0", "Ux0", "xg1", "xc1", "U1",
                           "Ux1"]):
        assert_grad_close(r.grad, h.grad.cpu().float(), name, rel=0.08)


def test_cond_gru_one_step_large_batch(ext):
    """B > 32 through the op layer: chunks of 32 + 8 rows on side streams,
    with per-column context lengths and per-row accumulators, so a chunk
    sliced along the wrong dim cannot pass."""
    from nats_amd import ops
    from nats_amd.ops import eager
    B, Ts = 40, 6
    model, yg, yc, _, init, ctx, _ = _cond_inputs(T=1, B=B, H=16, Ts=Ts, A=8,
                                                  with_masks=False)
    g = torch.Generator().manual_seed(9)
    slens = torch.randint(2, Ts + 1, (B,), generator=g)
    assert all(len(set(c.tolist())) > 1 for c in (slens[:32], slens[32:]))
    ctx_mask = (torch.arange(Ts).unsqueeze(1) < slens.unsqueeze(0)).float()
    P = {k: v.detach() for k, v in model.P.items()}
    pctx = ctx @ P["decoder_Wc_att"] + P["decoder_b_att"]
    acc_c = torch.randn(B, ctx.shape[2], generator=g) * 0.1
    acc_a = torch.rand(B, Ts, generator=g)
    ref = eager.cond_gru_step(init, yg[0], yc[0], ctx, ctx_mask, pctx,
                              acc_c, acc_a, P)
    Pg = {k: v.cuda() for k, v in P.items()}
    out = ops.cond_gru_step(init.cuda(), yg[0].cuda(), yc[0].cuda(),
                            ctx.cuda(), ctx_mask.cuda(), pctx.cuda(),
                            acc_c.cuda(), acc_a.cuda(), Pg)
    for r, o in zip(ref, out):
        assert o.shape == r.shape
        torch.testing.assert_close(o.cpu(), r, rtol=5e-2, atol=5e-2)
    alpha = out[2].cpu()
    assert alpha.shape == (B, Ts)
    assert bool((alpha[ctx_mask.t() == 0] == 0).all())


def test_gru_scan_large_batch(ext):
    """B > 32 through the op layer: serial chunks of 32 + 8 rows."""
    from nats_amd import ops
    from nats_amd.ops import eager
    xg, xc, U, Ux, mask = _gru_inputs(T=7, B=40, H=16)
    ref = eager.gru_scan(xg, xc, mask, U, Ux)
    out = ops.gru_scan(xg.cuda(), xc.cuda(), mask.cuda(), U.cuda(),
                       Ux.cuda())
    assert out.shape == ref.shape
    torch.testing.assert_close(out.cpu(), ref, rtol=0.1, atol=6e-2)
