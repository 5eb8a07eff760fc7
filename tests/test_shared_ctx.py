"""Shared-context decode: hypothesis row r attends to source column
row_src[r] of a context kept once per sentence (ops.cond_gru_step_shared,
NatsModel.f_next(row_src=...), the steppers' and beams' ``shared_ctx``).

The shared path loads the same bf16 context, fp32 pctx and mask values as
the gathered path and combines them in the same order under the same
chunking (it depends on the row count and Ts only), and rounding to bf16
commutes with the gather. So every comparison against the gathered path is
``torch.equal`` / ``==``: no tolerance. One case is also held to the fp64
eager oracle with the bounds of test_attn_fused_one_step, so that the new
path does not rest on the old one alone.
"""

import functools
import importlib.util
import os
import sys
import types

import numpy
import pytest
import torch

from kernel_ref import (DECODER_BF16_KEYS, _cond_inputs, alphas_rel_err,
                        round_bf16)
from nats_amd import ops
from nats_amd.decode.batched import gen_sample_batched
from nats_amd.decode.beam import gen_sample
from nats_amd.models.distraction import NatsModel, default_options
from nats_amd.ops import eager

gpu = pytest.mark.gpu

ALPHAS_MARGIN = 4.0         # the margin of test_attn_fused_one_step
STEP_OUT_NAMES = ("h2", "ctx_t", "alphas", "acc_ctx", "acc_alpha")


def chunk_len(B, Ts):
    """attn_chunk_len of cond_gru.hip: positions per (row, chunk) block."""
    per = (B * Ts + 255) // 256
    return (min(64, max(16, per)) + 7) // 8 * 8


# id -> (R, S, Ts, H, A, row_src, source lengths or None (generated) or
#        "nomask"). C = 2H.
SHARED_CASES = {
    # not monotone, repeats, source 1 unused; distinct length per source;
    # chunk 16 with a last chunk of 8; C = 36 takes the scalar column tail
    "r10_s3": (10, 3, 200, 18, 100, [2, 0, 0, 2, 2, 0, 2, 0, 0, 2],
               (200, 131, 57)),
    # production chunk 64 with a last chunk of one position; second MFMA
    # row tile; lengths 2 / 64 / 65 / 769 around the chunk edge
    "r19_s4": (19, 4, 769, 24, 100, [(3 * r) % 4 for r in range(19)],
               (2, 64, 65, 769)),
    # no mask: the single-sentence form, every row on the one column
    "r5_s1_nomask": (5, 1, 9, 18, 12, [0] * 5, "nomask"),
    # more sources than rows, as late in a decode
    "r2_s6": (2, 6, 129, 18, 36, [5, 3], None),
    # through _run_chunks (32 + 8 rows), all five sources in both chunks
    "r40_s5": (40, 5, 150, 18, 36, [(3 * r + 1) % 5 for r in range(40)],
               None),
}
SHARED_IDS = list(SHARED_CASES)


@functools.lru_cache(maxsize=None)
def _case(case_id):
    """(P, yg (R,2H), yc (R,H), init (R,H), ctx_src (Ts,S,C), mask_src
    (Ts,S) or None, pctx_src (Ts,S,A), row_src list, acc_c (R,C), acc_a
    (R,Ts)), all fp32 on the CPU; computed once and never written to."""
    R, S, Ts, H, A, row_src, lens = SHARED_CASES[case_id]
    B = max(R, S)
    # T = 2 only because _cond_inputs draws target lengths from [2, T]
    model, yg, yc, _, init, ctx, ctx_mask = _cond_inputs(
        T=2, B=B, H=H, Ts=Ts, A=A, seed=5, with_masks=True)
    ctx_src = ctx[:, :S].contiguous()
    if isinstance(lens, str):
        mask_src = None
    elif lens is None:
        mask_src = ctx_mask[:, :S].contiguous()
    else:
        mask_src = (torch.arange(Ts).unsqueeze(1) <
                    torch.tensor(lens).unsqueeze(0)).float()
    P = {k: v.detach() for k, v in model.P.items()}
    pctx_src = ctx_src @ P["decoder_Wc_att"] + P["decoder_b_att"]
    g = torch.Generator().manual_seed(11)
    acc_c = torch.randn(R, 2 * H, generator=g) * 0.3
    acc_a = torch.rand(R, Ts, generator=g) * 0.2
    if mask_src is not None:
        acc_a = acc_a * mask_src[:, row_src].t()
    return (P, yg[0, :R].contiguous(), yc[0, :R].contiguous(),
            init[:R].contiguous(), ctx_src, mask_src, pctx_src,
            list(row_src), acc_c, acc_a)


def _gathered(case):
    """The per-row ctx / mask / pctx that the table stands for."""
    P, yg, yc, init, ctx_src, mask_src, pctx_src, row_src, acc_c, acc_a = case
    idx = torch.tensor(row_src)
    return (ctx_src.index_select(1, idx),
            None if mask_src is None else mask_src.index_select(1, idx),
            pctx_src.index_select(1, idx))


@pytest.mark.parametrize("case_id", SHARED_IDS)
def test_shared_case_precondition(case_id):
    """Each SHARED_CASES line is what its comment claims."""
    R, S, Ts, H, A, row_src, lens = SHARED_CASES[case_id]
    case = _case(case_id)
    assert len(row_src) == R and all(0 <= v < S for v in row_src)
    assert float(case[8].abs().min()) > 0 and float(case[9].max()) > 0.1
    if case_id == "r10_s3":
        assert set(row_src) == {0, 2} and row_src != sorted(row_src)
        assert len(set(lens)) == S
        assert chunk_len(R, Ts) == 16 and Ts % 16 == 8 and (2 * H) % 8 != 0
    if case_id == "r19_s4":
        assert set(row_src) == set(range(S))
        assert chunk_len(R, Ts) == 64 and Ts % 64 == 1 and R > 16
        assert case[5].sum(0).long().tolist() == [2, 64, 65, 769]
    if case_id == "r5_s1_nomask":
        assert case[5] is None
    if case_id == "r2_s6":
        assert S > R
    if case_id == "r40_s5":
        assert R > ops.MAX_KERNEL_BATCH
        assert set(row_src[:32]) == set(row_src[32:]) == set(range(S))
    if case[5] is not None:
        assert float(case[5].sum(0).min()) >= 1


# ------------------------------------------------------------------ CPU: op

@pytest.mark.parametrize("case_id", ["r10_s3", "r5_s1_nomask", "r2_s6"])
@pytest.mark.parametrize("form", ["list", "int64", "int32"])
def test_shared_step_cpu_equals_gathered(case_id, form):
    case = _case(case_id)
    P, yg, yc, init, ctx_src, mask_src, pctx_src, row_src, acc_c, acc_a = case
    ctx_b, mask_b, pctx_b = _gathered(case)
    want = eager.cond_gru_step(init, yg, yc, ctx_b, mask_b, pctx_b, acc_c,
                               acc_a, P)
    tab = {"list": row_src, "int64": torch.tensor(row_src),
           "int32": torch.tensor(row_src, dtype=torch.int32)}[form]
    got = ops.cond_gru_step_shared(init, yg, yc, ctx_src, mask_src, pctx_src,
                                   tab, acc_c, acc_a, P)
    assert len(got) == len(want) == 5
    for g, w, n in zip(got, want, STEP_OUT_NAMES):
        assert torch.equal(g, w), n


def test_shared_step_validation():
    case = _case("r10_s3")
    P, yg, yc, init, ctx_src, mask_src, pctx_src, row_src, acc_c, acc_a = case
    S = ctx_src.shape[1]

    def call(tab, ctx=ctx_src, mask=mask_src, pctx=pctx_src):
        return ops.cond_gru_step_shared(init, yg, yc, ctx, mask, pctx, tab,
                                        acc_c, acc_a, P)

    assert len(call(row_src)) == 5
    with pytest.raises(ValueError, match="row_src"):
        call(row_src[:-1])                       # wrong length
    with pytest.raises(ValueError, match="row_src"):
        call(torch.tensor(row_src + [0]))
    with pytest.raises(ValueError, match="row_src"):
        call(row_src[:-1] + [S])                 # an entry == S
    with pytest.raises(ValueError, match="row_src"):
        call(torch.tensor(row_src[:-1] + [S]))
    with pytest.raises(ValueError, match="row_src"):
        call([-1] + row_src[1:])                 # an entry -1
    with pytest.raises(TypeError, match="row_src"):
        call(torch.tensor(row_src, dtype=torch.float32))
    with pytest.raises(TypeError, match="row_src"):
        call([float(v) for v in row_src])
    with pytest.raises(TypeError, match="row_src"):
        call(torch.tensor(row_src).reshape(2, 5))  # a 2-d shape
    with pytest.raises(ValueError, match="cond_gru_step_shared"):
        call(row_src, pctx=pctx_src[:, :2])
    with pytest.raises(ValueError, match="cond_gru_step_shared"):
        call(row_src, mask=mask_src[:, :2])


# --------------------------------------------------------------- CPU: beams

def _setup(seed=3):
    """The inflated-readout tiny model of tests/test_batched_decode.py."""
    opts = default_options(dim_word=12, dim=16, dim_att=8, n_words=80)
    model = NatsModel(opts, seed=seed).eval()
    with torch.no_grad():
        for key in ("ff_logit_lstm_W", "ff_logit_ctx_W", "ff_logit_prev_W",
                    "ff_logit_W"):
            model.P[key].mul_(50.0)
    g = torch.Generator().manual_seed(seed)
    xs = []
    for n in (7, 11, 5):
        x = torch.randint(2, 80, (n, 1), generator=g)
        x[-1] = 0
        xs.append(x)
    return model, xs


def _assert_same_beams(got, want):
    """Samples, scores and alignment rows identical, in the same order."""
    gs, gc, ga = got
    ws, wc, wa = want
    assert [list(map(int, s)) for s in gs] == [list(map(int, s)) for s in ws]
    assert [float(c) for c in gc] == [float(c) for c in wc]
    assert len(ga) == len(wa)
    for g_rows, w_rows in zip(ga, wa):
        assert len(g_rows) == len(w_rows)
        for g, w in zip(g_rows, w_rows):
            assert numpy.array_equal(numpy.asarray(g), numpy.asarray(w))


LAMBDAS = dict(kl_factor=0.7, ctx_factor=0.7, state_factor=0.7)
BEAM_MODES = {
    "plain": {},
    "rerank": LAMBDAS,
    "fused": dict(fused_select=True),
    "rerank_fused_paged": dict(fused_select=True, paged_rerank=True,
                               **LAMBDAS),
    "rerank_paged": dict(paged_rerank=True, **LAMBDAS),
    # sentences leave the batch at their own caps: the routing table
    # shrinks and shifts between steps
    "ragged_maxlen": dict(maxlen=[8, 3, 6]),
}


@pytest.mark.parametrize("mode", list(BEAM_MODES))
def test_batched_shared_ctx_cpu(mode):
    model, xs = _setup()
    kw = dict(k=3, maxlen=8, use_unk=True)
    kw.update(BEAM_MODES[mode])
    want = gen_sample_batched(model, xs, shared_ctx=False, **kw)
    got = gen_sample_batched(model, xs, shared_ctx=True, **kw)
    assert len(got) == len(want) == len(xs)
    assert sum(len(w[0]) for w in want) > 0
    for g, w in zip(got, want):
        _assert_same_beams(g, w)


def test_gen_sample_shared_ctx_cpu():
    model, xs = _setup()
    kw = dict(k=3, maxlen=8, stochastic=False, use_unk=True)
    for extra in ({}, LAMBDAS):
        want = gen_sample(model, xs[1], shared_ctx=False, **kw, **extra)
        got = gen_sample(model, xs[1], shared_ctx=True, **kw, **extra)
        _assert_same_beams(got, want)


def test_decode_context_cpu():
    model, xs = _setup()
    x = xs[1]
    _, ctx = model.f_init(x)
    mask = torch.ones(ctx.shape[0], 1, dtype=torch.float64)
    ctx_dec, m, pctx = model.decode_context(ctx, mask)
    assert ctx_dec is ctx
    assert m.dtype == torch.float32 and m.shape == (ctx.shape[0], 1)
    assert torch.equal(pctx, model.project_ctx(ctx))
    assert model.decode_context(ctx)[1] is None


def test_service_passes_shared_ctx(tmp_path, monkeypatch):
    from nats_amd.data.synthetic import make_toy_corpus
    from nats_amd.engine.checkpoint import save_checkpoint
    import nats_amd.serve.app as app
    from nats_amd.serve import SummarizerService
    d = str(tmp_path)
    make_toy_corpus(d)
    opts = default_options(dim_word=12, dim=16, dim_att=8, n_words=43,
                           maxlen=50)
    saveto = os.path.join(d, "model.npz")
    save_checkpoint(saveto, NatsModel(opts, seed=3).get_params(), [],
                    options=opts)
    seen = []
    real = app.gen_sample_batched

    def spy(*a, **kw):
        seen.append(kw.get("shared_ctx"))
        return real(*a, **kw)

    monkeypatch.setattr(app, "gen_sample_batched", spy)
    dictionary = os.path.join(d, "toy_train_input.txt.pkl")
    assert SummarizerService(saveto, dictionary, device="cpu",
                             k=3).shared_ctx is False
    summaries = []
    for flag in (False, True):
        svc = SummarizerService(
            saveto, dictionary, device="cpu", k=3, maxlen=6, max_wait_ms=1.0,
            shared_ctx=flag)
        try:
            summaries.append(svc.summarize("a b c d")["summary"])
        finally:
            svc.close()
    assert seen == [False, True]
    assert isinstance(summaries[0], str) and summaries[0] == summaries[1]


def test_cli_passes_shared_ctx(monkeypatch):
    """scripts/serve.py --shared-ctx reaches SummarizerService (service and
    server are stand-ins: nothing is loaded or served)."""
    import nats_amd.serve as serve
    path = os.path.join(os.path.dirname(os.path.dirname(
        os.path.abspath(__file__))), "scripts", "serve.py")
    spec = importlib.util.spec_from_file_location("serve_cli", path)
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    seen = []
    monkeypatch.setattr(serve, "SummarizerService",
                        lambda *a, **kw: seen.append(kw) or "service")
    monkeypatch.setattr(serve, "create_app", lambda service: service)
    monkeypatch.setitem(sys.modules, "uvicorn", types.SimpleNamespace(
        run=lambda app, **kw: None))
    for extra in ([], ["--shared-ctx"],
                  ["--shared-ctx", "--fused-select", "--paged-rerank"]):
        monkeypatch.setattr(sys, "argv",
                            ["serve.py", "model.npz", "dict.pkl"] + extra)
        cli.main()
    assert [kw["shared_ctx"] for kw in seen] == [False, True, True]
    assert [kw["paged_rerank"] for kw in seen] == [False, False, True]
    assert [kw["fused_select"] for kw in seen] == [False, False, True]


# -------------------------------------------------------------- GPU tests

@pytest.fixture(scope="module")
def ext():
    m = ops._hip_ext()
    assert m is not None, "HIP extension must build/load on a GPU box"
    return m


def _shared_and_gathered_gpu(case_id):
    """(shared outputs, gathered outputs) of one step on the GPU; asserts
    that the per-source operands come back unchanged."""
    case = _case(case_id)
    P, yg, yc, init, ctx_src, mask_src, pctx_src, row_src, acc_c, acc_a = case
    ctx_b, mask_b, pctx_b = _gathered(case)
    Pg = {k: v.cuda() for k, v in P.items()}
    row = [t.cuda() for t in (init, yg, yc)]

    def acc():
        # fresh device copies per call: the step kernels update fp32
        # contiguous accumulators in place
        return acc_c.cuda(), acc_a.cuda()

    want = ops.cond_gru_step(
        *row, ctx_b.cuda(), None if mask_b is None else mask_b.cuda(),
        pctx_b.cuda(), *acc(), Pg)
    ctx_bf = ctx_src.cuda().bfloat16()
    mask_g = None if mask_src is None else mask_src.cuda()
    pctx_g = pctx_src.cuda()
    keep = [ctx_bf.clone(), pctx_g.clone(),
            None if mask_g is None else mask_g.clone()]
    got = ops.cond_gru_step_shared(*row, ctx_bf, mask_g, pctx_g, row_src,
                                   *acc(), Pg)
    torch.cuda.synchronize()
    assert torch.equal(ctx_bf, keep[0])
    assert torch.equal(pctx_g, keep[1])
    assert mask_g is None or torch.equal(mask_g, keep[2])
    assert torch.equal(ctx_bf.cpu(), ctx_src.bfloat16())
    return got, want


@gpu
@pytest.mark.parametrize("case_id", SHARED_IDS)
def test_shared_step_equals_gathered(ext, case_id):
    """ops.cond_gru_step_shared on the bf16 per-source context against
    ops.cond_gru_step on the gathered fp32 inputs: all five outputs bit
    for bit."""
    got, want = _shared_and_gathered_gpu(case_id)
    assert len(got) == len(want) == 5
    for g, w, n in zip(got, want, STEP_OUT_NAMES):
        assert g.shape == w.shape and g.dtype == w.dtype, n
        assert bool(torch.isfinite(g).all()), n
        assert torch.equal(g, w), "%s: %s differs" % (case_id, n)


@gpu
def test_shared_step_device_table(ext):
    """An int32 device table (taken on trust) gives what the list gives."""
    case = _case("r10_s3")
    P, yg, yc, init, ctx_src, mask_src, pctx_src, row_src, acc_c, acc_a = case
    Pg = {k: v.cuda() for k, v in P.items()}
    args = [t.cuda() for t in (init, yg, yc)] + [
        ctx_src.cuda().bfloat16(), mask_src.cuda(), pctx_src.cuda()]

    def acc():  # fresh copies: the kernels update the accumulators in place
        return acc_c.cuda(), acc_a.cuda()

    want = ops.cond_gru_step_shared(*args, row_src, *acc(), Pg)
    tab = torch.tensor(row_src, dtype=torch.int32, device="cuda")
    got = ops.cond_gru_step_shared(*args, tab, *acc(), Pg)
    for g, w, n in zip(got, want, STEP_OUT_NAMES):
        assert torch.equal(g, w), n
    with pytest.raises(TypeError, match="row_src"):
        ops.cond_gru_step_shared(*args, tab.long(), *acc(), Pg)
    with pytest.raises(ValueError, match="row_src"):
        ops.cond_gru_step_shared(*args, tab[:-1], *acc(), Pg)


@functools.lru_cache(maxsize=None)
def _oracle_ref():
    """fp64 eager step of the first case on the gathered inputs, the alphas
    error of the bf16-operand fp32 eager run against it, and the share of
    unmasked reference alphas >= 1e-6."""
    case = _case("r10_s3")
    P, yg, yc, init, ctx_src, mask_src, pctx_src, row_src, acc_c, acc_a = case
    ctx_b, mask_b, _ = _gathered(case)

    def run_eager(dtype, bf16_operands):
        Pd = {k: v.to(dtype) for k, v in P.items()}
        a = [t.to(dtype) for t in (yg, yc, init, ctx_b, mask_b, acc_c, acc_a)]
        pctx = a[3] @ Pd["decoder_Wc_att"] + Pd["decoder_b_att"]
        if bf16_operands:
            for k in DECODER_BF16_KEYS:
                Pd[k] = round_bf16(Pd[k])
            a[0], a[1], a[3] = (round_bf16(a[0]), round_bf16(a[1]),
                                round_bf16(a[3]))
        with torch.no_grad():
            return eager.cond_gru_step(a[2], a[0], a[1], a[3], a[4], pctx,
                                       a[5], a[6], Pd)

    ref = run_eager(torch.float64, False)
    emu = run_eager(torch.float32, True)
    emu_alpha = alphas_rel_err(emu[2].unsqueeze(0), ref[2].unsqueeze(0),
                               mask_b)
    share = float((ref[2][mask_b.t() > 0] >= 1e-6).double().mean())
    return ref, emu_alpha, share, mask_b


def test_shared_oracle_precondition():
    """The relative alphas check of the oracle test sees most entries."""
    _, emu_alpha, share, _ = _oracle_ref()
    print("shared step: share of unmasked alphas >= 1e-6 %.3f, bf16-operand "
          "alphas rel err %.3e" % (share, emu_alpha))
    assert share >= 0.8, share
    assert emu_alpha > 0


@gpu
def test_shared_step_vs_fp64_oracle(ext):
    """The first case against the fp64 eager step on the gathered inputs,
    with the bounds of test_attn_fused_one_step."""
    ref, emu_alpha, share, mask_b = _oracle_ref()
    keep = mask_b.t()
    got, _ = _shared_and_gathered_gpu("r10_s3")
    out = [o.cpu().float() for o in got]
    for r, o, n in zip(ref, out, STEP_OUT_NAMES):
        assert o.shape == r.shape, n
        if n != "alphas":
            torch.testing.assert_close(o.double(), r, rtol=5e-2, atol=5e-2,
                                       msg=lambda m, n=n: "%s: %s" % (n, m))
    alphas = out[2]
    assert bool((alphas[keep == 0] == 0).all())
    rows = (alphas * keep).sum(-1)
    torch.testing.assert_close(rows, torch.ones_like(rows), rtol=0,
                               atol=1e-3)
    hip_alpha = alphas_rel_err(alphas.unsqueeze(0), ref[2].unsqueeze(0),
                               mask_b)
    print("shared step: alphas rel err vs fp64: bf16-operand eager %.3e, "
          "kernel %.3e (bound %.3e), share >= 1e-6 %.3f"
          % (emu_alpha, hip_alpha, ALPHAS_MARGIN * emu_alpha, share))
    assert hip_alpha <= ALPHAS_MARGIN * emu_alpha, (hip_alpha, emu_alpha)


def _gpu_batch(model, xs, Ts=None):
    """Padded per-sentence context of ``xs`` on the GPU, fp32."""
    lens = [int(x.shape[0]) for x in xs]
    Ts = Ts or max(lens)
    S = len(xs)
    x_pad = torch.zeros(Ts, S, dtype=torch.int64, device="cuda")
    mask = torch.zeros(Ts, S, device="cuda")
    for i, x in enumerate(xs):
        x_pad[:lens[i], i] = x[:, 0].cuda()
        mask[:lens[i], i] = 1.0
    init, ctx = model.f_init(x_pad, mask)
    ctx = (ctx.float() * mask[:, :, None]).contiguous()
    return init.float(), ctx, mask


def _row_state(model, R, Ts, seed):
    H, C = model.options["dim"], 2 * model.options["dim"]
    g = torch.Generator().manual_seed(seed)
    y = torch.randint(2, 80, (R,), generator=g)
    y[0] = -1
    return (y.cuda(), (torch.randn(R, H, generator=g) * 0.1).cuda(),
            (torch.randn(R, C, generator=g) * 0.3).cuda(),
            (torch.rand(R, Ts, generator=g) * 0.2).cuda())


@gpu
def test_f_next_row_src(ext):
    model, xs = _setup()
    model = model.cuda()
    _, ctx, mask = _gpu_batch(model, xs)
    Ts, S = mask.shape
    R = 7
    row_src = [2, 0, 1, 1, 2, 0, 2]
    y, state, acc_c, acc_a = _row_state(model, R, Ts, seed=4)
    idx = torch.tensor(row_src, device="cuda")
    acc_a = acc_a * mask[:, idx].t()
    want = model.f_next(y, ctx[:, idx], mask[:, idx],
                        model.project_ctx(ctx)[:, idx], state, acc_c.clone(),
                        acc_a.clone(), sample_draw=False)
    ctx_dec, m, pctx = model.decode_context(ctx, mask)
    assert ctx_dec.dtype == torch.bfloat16 and ctx_dec.shape == ctx.shape
    assert torch.equal(pctx, model.project_ctx(ctx))
    for tab in (row_src, idx.to(torch.int32)):
        # clones: the step kernels update the accumulators in place
        got = model.f_next(y, ctx_dec, m, pctx, state, acc_c.clone(),
                           acc_a.clone(), sample_draw=False, row_src=tab)
        assert len(got) == len(want) == 7
        for i, (g, w) in enumerate(zip(got, want)):
            assert torch.equal(g, w), i


@gpu
def test_batched_stepper_shared_mode(ext):
    """Two steps with different routing and live row counts replay one
    captured graph and equal the gathered-mode stepper bit for bit."""
    from nats_amd.decode.graph import (BatchedGraphStepper,
                                       get_batched_stepper)
    model, xs = _setup()
    model = model.cuda()
    _, ctx, mask = _gpu_batch(model, xs, Ts=64)
    pctx = model.project_ctx(ctx)
    Ts, S = mask.shape
    R = 9
    plain = BatchedGraphStepper(model, ctx, mask, pctx, R)
    shared = BatchedGraphStepper(model, ctx, mask, pctx, R, shared_ctx=True)
    assert shared.ctx_pad.dtype == torch.bfloat16
    assert shared.ctx_pad.shape == ctx.shape
    assert shared.row_src.dtype == torch.int32
    graphs = []
    for step, routing in enumerate(([0, 0, 1, 1, 1, 2, 2],
                                    [2, 1, 1, 0, 2])):
        live = len(routing)
        sent_idx = torch.tensor(routing, device="cuda")
        y, state, acc_c, acc_a = _row_state(model, live, Ts, seed=20 + step)
        acc_a = acc_a * mask[:, sent_idx].t()
        want = [o[:live].clone() for o in
                plain.step(sent_idx, y, state, acc_c, acc_a)]
        got = [o[:live].clone() for o in
               shared.step(sent_idx, y, state, acc_c, acc_a)]
        graphs.append(shared.graph)
        assert shared.row_src[:live].tolist() == routing
        assert len(got) == len(want) == 6
        for i, (g, w) in enumerate(zip(got, want)):
            assert torch.equal(g, w), (step, i)
    assert graphs[0] is not None and graphs[0] is graphs[1]
    # the mode is part of the cache key; set_context re-rounds the context
    a = get_batched_stepper(model, ctx, mask, pctx, R)
    b = get_batched_stepper(model, ctx, mask, pctx, R, shared_ctx=True)
    assert a is not b and b.shared_ctx and not a.shared_ctx
    assert get_batched_stepper(model, ctx * 0.5, mask, pctx, R,
                               shared_ctx=True) is b
    assert torch.equal(b.ctx_pad, (ctx * 0.5).bfloat16())


GPU_BEAM_MODES = {
    "graph": dict(use_graph=True),
    "nograph": dict(use_graph=False),
    "graph_fused_paged": dict(use_graph=True, fused_select=True,
                              paged_rerank=True, **LAMBDAS),
    "nograph_fused_paged": dict(use_graph=False, fused_select=True,
                                paged_rerank=True, **LAMBDAS),
    "graph_ragged_maxlen": dict(use_graph=True, maxlen=[8, 3, 6]),
}


@gpu
@pytest.mark.parametrize("mode", list(GPU_BEAM_MODES))
def test_batched_shared_ctx_gpu(ext, mode):
    model, xs = _setup()
    model = model.cuda()
    xs = [x.cuda() for x in xs]
    kw = dict(k=3, maxlen=8, use_unk=True)
    kw.update(GPU_BEAM_MODES[mode])
    want = gen_sample_batched(model, xs, shared_ctx=False, **kw)
    got = gen_sample_batched(model, xs, shared_ctx=True, **kw)
    assert sum(len(w[0]) for w in want) > 0
    for g, w in zip(got, want):
        _assert_same_beams(g, w)


@gpu
def test_batched_shared_ctx_gpu_eager(ext, monkeypatch):
    """With the kernels switched off the context is not rounded: the flag
    still changes nothing, bit for bit."""
    monkeypatch.setenv("NATS_AMD_FORCE_EAGER", "1")
    model, xs = _setup()
    model = model.cuda()
    xs = [x.cuda() for x in xs]
    _, ctx = model.f_init(xs[0])
    assert model.decode_context(ctx)[0] is ctx
    kw = dict(k=3, maxlen=8, use_unk=True, use_graph=False)
    want = gen_sample_batched(model, xs, shared_ctx=False, **kw)
    got = gen_sample_batched(model, xs, shared_ctx=True, **kw)
    for g, w in zip(got, want):
        _assert_same_beams(g, w)


@gpu
@pytest.mark.parametrize("use_graph", [True, False])
def test_gen_sample_shared_ctx_gpu(ext, use_graph):
    model, xs = _setup()
    model = model.cuda()
    x = xs[1].cuda()
    kw = dict(k=3, maxlen=8, stochastic=False, use_unk=True,
              use_graph=use_graph)
    want = gen_sample(model, x, shared_ctx=False, **kw)
    got = gen_sample(model, x, shared_ctx=True, **kw)
    assert len(want[0]) > 0
    _assert_same_beams(got, want)
    if use_graph:
        from nats_amd.decode.graph import get_stepper
        _, ctx0 = model.f_init(x)
        st = get_stepper(model, ctx0.float(),
                         model.project_ctx(ctx0).float(), 3, shared_ctx=True)
        assert st.ctx.shape[1] == 1 and st.ctx.dtype == torch.bfloat16
        assert st.row_src.tolist() == [0, 0, 0]
