"""Resident beam rows: ops.beam_reorder (one launch that moves the selected
rows from a decode step's outputs into its input buffers, with the words,
the routing and the padding tail), the steppers' ``replay`` and
gen_sample_batched(resident_state=True).

Nothing on this path is arithmetic: every value it produces is a copy of a
value the default path produces. So every comparison here is ``torch.equal``
/ ``==`` / ``numpy.array_equal``: no tolerance anywhere.

Test model: the inflated-readout tiny model of tests/test_batched_decode.py
with model seed and source seed 4 and the EOS column of ff_logit_W doubled
after the inflation, so that hypotheses finish by EOS before the cap as
well as at it (seed 4, EOS factor 2: the pair every whole-decode test here
uses, on the CPU and on the GPU). Each whole-decode test asserts that on
the flag-off result of its own run.
"""

import functools
import importlib.util
import os
import sys
import types

import numpy
import pytest
import torch

from nats_amd import ops
from nats_amd.decode import graph as graph_mod
from nats_amd.decode.batched import gen_sample_batched
from nats_amd.models.distraction import NatsModel, default_options
from nats_amd.ops import eager

gpu = pytest.mark.gpu

SEED, EOS_FACTOR = 4, 2.0
LENS3, LENS5 = (7, 11, 5), (7, 11, 5, 9, 6)
MAXLEN = 8


# ------------------------------------------------------------ the op: cases

# id -> (n_prev, Rmax, D per buffer, parent, route dtype, table form)
def _perm_parents(n_prev, L):
    """Repeats and a permutation; row 0's parent is not 0."""
    base = [n_prev - 1, 0, n_prev - 1, 2 % n_prev, 1 % n_prev, 0]
    return [base[r % len(base)] if r < len(base) else (3 * r + 1) % n_prev
            for r in range(L)]


OP_CASES = {
    "L3_of_8": (5, 8, (16, 32, 7), _perm_parents(5, 3)),
    "L_eq_Rmax": (5, 8, (16, 32, 7), _perm_parents(5, 8)),
    "L1": (5, 8, (16, 32, 7), [3]),
    "D1": (5, 8, (1,), _perm_parents(5, 3)),
    "D3": (5, 8, (3, 3), _perm_parents(5, 6)),
    "permutation": (6, 6, (16, 7), [4, 0, 5, 1, 3, 2]),
}
ROUTE_DTYPES = {"route64": torch.int64, "route32": torch.int32}


def _op_inputs(n_prev, Rmax, Ds, parent, seed=0, src_rows=None):
    """(table rows, src tuple, word list, sentence list): CPU, fp32."""
    g = torch.Generator().manual_seed(seed)
    src = tuple(torch.randn(src_rows or n_prev, D, generator=g) for D in Ds)
    L = len(parent)
    word = [-1 if r == 1 else int(v) for r, v in enumerate(
        torch.randint(0, 80, (L,), generator=g).tolist())]
    sent = torch.randint(0, 6, (L,), generator=g).tolist()
    return [list(parent), word, sent], src, word, sent


def _expected(table, src, Rmax, route_dtype):
    """The plain index_select expression, with the steppers' padding rule
    (rows past L repeat the new row 0)."""
    parent, word, sent = (torch.tensor(r, dtype=torch.int64) for r in table)
    L = parent.shape[0]
    pad = Rmax - L
    outs = []
    for s in src:
        rows = s.index_select(0, parent)
        outs.append(torch.cat([rows, rows[:1].expand(pad, -1)]))
    y = torch.cat([word, word[:1].expand(pad)])
    route = torch.cat([sent, sent[:1].expand(pad)]).to(route_dtype)
    return outs, y, route


def _fresh_out(Rmax, Ds, route_dtype, device="cpu"):
    """Output buffers filled with values no case produces."""
    dst = tuple(torch.full((Rmax, D), -7.5, device=device) for D in Ds)
    y = torch.full((Rmax,), -9, dtype=torch.int64, device=device)
    route = torch.full((Rmax,), -9, dtype=route_dtype, device=device)
    return dst, y, route


def _assert_buffers(got, want, what):
    (dst, y, route), (w_dst, w_y, w_route) = got, want
    for j, (d, w) in enumerate(zip(dst, w_dst)):
        assert torch.equal(d.cpu(), w), "%s: dst[%d]" % (what, j)
    assert torch.equal(y.cpu(), w_y), "%s: y_out" % what
    assert route.dtype == w_route.dtype
    assert torch.equal(route.cpu(), w_route), "%s: route_out" % what


@pytest.mark.parametrize("route", list(ROUTE_DTYPES))
@pytest.mark.parametrize("form", ["list", "int32", "int64"])
@pytest.mark.parametrize("case_id", list(OP_CASES))
def test_beam_reorder_cpu_equals_index_select(case_id, form, route):
    n_prev, Rmax, Ds, parent = OP_CASES[case_id]
    table, src, _, _ = _op_inputs(n_prev, Rmax, Ds, parent)
    if case_id != "L1":
        assert parent[0] != 0 and len(set(parent)) > 1
    if case_id == "permutation":
        assert sorted(parent) == list(range(n_prev))
    elif len(parent) > 2:
        assert len(set(parent)) < len(parent)      # repeats
    rd = ROUTE_DTYPES[route]
    want = _expected(table, src, Rmax, rd)
    tab = {"list": table, "int32": torch.tensor(table, dtype=torch.int32),
           "int64": torch.tensor(table)}[form]
    dst, y, r = _fresh_out(Rmax, Ds, rd)
    keep = [s.clone() for s in src]
    ret = ops.beam_reorder(tab, src, dst, y, r)
    _assert_buffers((dst, y, r), want, case_id)
    for s, k in zip(src, keep):
        assert torch.equal(s, k)
    # the returned table: int64 on the buffers' device, row 0 the parents
    assert ret.dtype == torch.int64 and ret.shape == (3, len(parent))
    assert ret[0].tolist() == parent and ret[0].is_contiguous()


def test_beam_reorder_cpu_n_prev_of_larger_src():
    """n_prev names the live rows of a larger src buffer (a stepper's
    output buffers): parents are checked against it, not the allocation."""
    table, src, _, _ = _op_inputs(5, 8, (16, 7), [4, 0, 4], src_rows=8)
    dst, y, r = _fresh_out(8, (16, 7), torch.int64)
    ops.beam_reorder(table, src, dst, y, r, n_prev=5)
    _assert_buffers((dst, y, r), _expected(table, src, 8, torch.int64),
                    "n_prev")
    with pytest.raises(ValueError, match="beam_reorder"):
        ops.beam_reorder([[5, 0, 4], table[1], table[2]], src, dst, y, r,
                         n_prev=5)
    with pytest.raises(ValueError, match="beam_reorder"):
        ops.beam_reorder(table, src, dst, y, r, n_prev=9)


def test_beam_reorder_eager_poisons_bad_parent():
    """The eager twin follows the kernel's convention for a table taken on
    trust: a parent outside [0, n_prev) gives a NaN row, y 0, route 0 (and
    so do the padding rows when it is row 0)."""
    g = torch.Generator().manual_seed(1)
    src = (torch.randn(6, 8, generator=g), torch.randn(6, 3, generator=g))
    table = torch.tensor([[2, 4, -1, 1], [7, 8, 9, 10], [1, 2, 3, 4]])
    dst, y, r = _fresh_out(6, (8, 3), torch.int32)
    eager.beam_reorder(table, src, dst, y, r, 4)
    for s, d in zip(src, dst):
        assert torch.equal(d[0], s[2]) and torch.equal(d[3], s[1])
        assert bool(torch.isnan(d[1]).all()) and bool(torch.isnan(d[2]).all())
        assert torch.equal(d[4], s[2]) and torch.equal(d[5], s[2])
    assert y.tolist() == [7, 0, 0, 10, 7, 7]
    assert r.tolist() == [1, 0, 0, 4, 1, 1]


def test_beam_reorder_validation():
    n_prev, Rmax, Ds = 5, 8, (16, 7)
    table, src, word, sent = _op_inputs(n_prev, Rmax, Ds, [4, 0, 2])
    dst, y, r = _fresh_out(Rmax, Ds, torch.int64)

    def call(tab=table, src=src, dst=dst, y=y, r=r, **kw):
        return ops.beam_reorder(tab, src, dst, y, r, **kw)

    call()
    bad = (ValueError, TypeError)
    for parent in ([4, 5, 2], [4, -1, 2]):                # parent range
        with pytest.raises(ValueError, match="parent"):
            call([parent, word, sent])
        with pytest.raises(ValueError, match="parent"):
            call(torch.tensor([parent, word, sent]))
    with pytest.raises(ValueError, match="L=0"):          # L outside [1, Rmax]
        call([[], [], []])
    with pytest.raises(ValueError, match="L=9"):
        call([[0] * 9, [1] * 9, [0] * 9])
    with pytest.raises(ValueError, match="L=9"):
        call(torch.zeros(3, 9, dtype=torch.int64))
    with pytest.raises(ValueError, match="sentence"):     # negative sentence
        call([[4, 0, 2], word, [0, -1, 0]])
    with pytest.raises(ValueError, match="word"):         # word < -1
        call([[4, 0, 2], [3, -2, 3], sent])
    call([[4, 0, 2], [3, -1, 3], sent])                   # BOS is a word
    with pytest.raises(bad, match="table"):
        call([[4, 0, 2], word])                           # two rows
    with pytest.raises(bad, match="table"):
        call(torch.tensor([[4.0, 0, 2], [1, 1, 1], [0, 0, 0]]))
    with pytest.raises(bad, match="table"):
        call([[4, 0, 2.0], word, sent])
    # overlap: dst is (a view of) src, or shares a tail with it
    with pytest.raises(ValueError, match="overlap"):
        call(src=(dst[0][:n_prev], src[1]))
    big = torch.zeros(Rmax + n_prev - 1, 16)
    with pytest.raises(ValueError, match="overlap"):
        call(src=(big[Rmax - 1:], src[1]), dst=(big[:Rmax], dst[1]))
    call(src=(big[Rmax:Rmax + 3], src[1]), dst=(big[:Rmax], dst[1]),
         tab=[[2, 0, 1], word, sent])                     # adjacent is fine
    # non-fp32 buffers
    with pytest.raises(TypeError, match="float32"):
        call(src=(src[0].double(), src[1]))
    with pytest.raises(TypeError, match="float32"):
        call(dst=(dst[0].bfloat16(), dst[1]))
    # mismatched D, row counts, buffer counts, index buffers
    with pytest.raises(ValueError, match="row width"):
        call(src=(src[0][:, :8].contiguous(), src[1]))
    with pytest.raises(ValueError, match="rows"):
        call(dst=(dst[0][:6], dst[1]))
    with pytest.raises(ValueError, match="buffers"):
        call(src=src[:1])
    with pytest.raises(ValueError, match="buffers"):
        call(src=src * 3, dst=dst * 3)
    with pytest.raises(ValueError, match="contiguous"):
        call(src=(torch.zeros(16, n_prev).t(), src[1]))
    with pytest.raises(TypeError, match="y_out"):
        call(y=y.int())
    with pytest.raises(TypeError, match="route_out"):
        call(r=r.float())
    with pytest.raises(ValueError, match="route_out"):
        call(r=r[:-1])


# ------------------------------------------------------- whole decodes: CPU

def _setup(lens=LENS3, seed=SEED, factor=EOS_FACTOR):
    opts = default_options(dim_word=12, dim=16, dim_att=8, n_words=80)
    model = NatsModel(opts, seed=seed).eval()
    with torch.no_grad():
        for key in ("ff_logit_lstm_W", "ff_logit_ctx_W", "ff_logit_prev_W",
                    "ff_logit_W"):
            model.P[key].mul_(50.0)
        model.P["ff_logit_W"][:, 0].mul_(factor)
    g = torch.Generator().manual_seed(seed)
    xs = []
    for n in lens:
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
            g, w = numpy.asarray(g), numpy.asarray(w)
            assert g.dtype == w.dtype and numpy.array_equal(g, w)


def _assert_finish_mix(want, maxlens):
    """Precondition on a flag-off result: hypotheses end by EOS before
    their sentence's cap and others at the cap, so the table shrinks,
    ``want`` shrinks and the padding tail is in use."""
    early = capped = 0
    for (samples, _, _), cap in zip(want, maxlens):
        for s in samples:
            if s[-1] == 0 and len(s) < cap:
                early += 1
            elif len(s) == cap and s[-1] != 0:
                capped += 1
    assert early >= 1 and capped >= 1, (early, capped)


def _maxlens(kw, S):
    m = kw.get("maxlen", MAXLEN)
    return [m] * S if isinstance(m, int) else list(m)


LAMBDAS = dict(kl_factor=0.7, ctx_factor=0.7, state_factor=0.7)
BEAM_MODES = {
    "plain": {},
    "rerank": LAMBDAS,
    "fused": dict(fused_select=True),
    "rerank_fused_paged": dict(fused_select=True, paged_rerank=True,
                               **LAMBDAS),
    "rerank_paged": dict(paged_rerank=True, **LAMBDAS),
    "shared": dict(shared_ctx=True),
    "rerank_fused_paged_shared": dict(fused_select=True, paged_rerank=True,
                                      shared_ctx=True, **LAMBDAS),
    # sentences leave the batch at their own caps: they stop appearing in
    # the table while others go on
    "ragged_maxlen": dict(maxlen=[8, 3, 6]),
    "k7_five_sentences": dict(k=7, lens=LENS5, fused_select=True),
}


def _decode_pair(model, xs, kw):
    want = gen_sample_batched(model, xs, resident_state=False, **kw)
    _assert_finish_mix(want, _maxlens(kw, len(xs)))
    got = gen_sample_batched(model, xs, resident_state=True, **kw)
    assert len(got) == len(want) == len(xs)
    for g, w in zip(got, want):
        _assert_same_beams(g, w)
    return want


def _mode_kw(mode, table=BEAM_MODES):
    kw = dict(k=3, maxlen=MAXLEN, use_unk=True)
    kw.update(table[mode])
    lens = kw.pop("lens", LENS3)
    return kw, lens


@pytest.mark.parametrize("mode", list(BEAM_MODES))
def test_batched_resident_cpu(mode):
    kw, lens = _mode_kw(mode)
    model, xs = _setup(lens)
    want = _decode_pair(model, xs, kw)
    if mode == "k7_five_sentences":
        # 35 rows: past the 32-row chunk of the step kernels
        assert len(xs) * kw["k"] > ops.MAX_KERNEL_BATCH
        assert all(len(w[0]) == 7 for w in want)


def _count_calls(monkeypatch, cls, name, counter):
    real = getattr(cls, name)

    def spy(*a, **k):
        counter[name] = counter.get(name, 0) + 1
        return real(*a, **k)

    monkeypatch.setattr(cls, name, spy)


@pytest.mark.parametrize("mode", ["fused", "rerank_paged", "ragged_maxlen"])
def test_resident_call_counts_cpu(monkeypatch, mode):
    """Per decode of n executed steps: one beam_reorder per step that has
    a successor, one copying fill (step 0), at most one Tensor.cpu per
    step and one at the end."""
    kw, lens = _mode_kw(mode)
    model, xs = _setup(lens)
    counts = {}
    _count_calls(monkeypatch, ops, "beam_reorder", counts)
    _count_calls(monkeypatch, graph_mod.RowStepper, "step", counts)
    _count_calls(monkeypatch, graph_mod.RowStepper, "replay", counts)
    _count_calls(monkeypatch, torch.Tensor, "cpu", counts)
    got = gen_sample_batched(model, xs, resident_state=True, **kw)
    # executed steps: the longest hypothesis (no step runs without adding
    # a word to some hypothesis)
    n = max(len(s) for samples, _, _ in got for s in samples)
    assert n >= 3
    assert counts["step"] == 1
    assert counts["replay"] == n          # one inside step, n-1 direct
    assert counts["beam_reorder"] == n - 1
    assert counts["cpu"] <= n + 1
    print("resident %s: %d steps, %s" % (mode, n, counts))


# ----------------------------------------------------------------- plumbing

def test_service_passes_resident_state(tmp_path, monkeypatch):
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
        seen.append(kw.get("resident_state"))
        return real(*a, **kw)

    monkeypatch.setattr(app, "gen_sample_batched", spy)
    dictionary = os.path.join(d, "toy_train_input.txt.pkl")
    assert SummarizerService(saveto, dictionary, device="cpu",
                             k=3).resident_state is False
    summaries = []
    for flag in (False, True):
        svc = SummarizerService(
            saveto, dictionary, device="cpu", k=3, maxlen=6, max_wait_ms=1.0,
            resident_state=flag)
        try:
            summaries.append(svc.summarize("a b c d")["summary"])
        finally:
            svc.close()
    assert seen == [False, True]
    assert isinstance(summaries[0], str) and summaries[0] == summaries[1]


def test_cli_passes_resident_state(monkeypatch):
    """scripts/serve.py --resident-state reaches SummarizerService (service
    and server are stand-ins: nothing is loaded or served)."""
    import nats_amd.serve as serve
    path = os.path.join(os.path.dirname(os.path.dirname(
        os.path.abspath(__file__))), "scripts", "serve.py")
    spec = importlib.util.spec_from_file_location("serve_cli_resident", path)
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    seen = []
    monkeypatch.setattr(serve, "SummarizerService",
                        lambda *a, **kw: seen.append(kw) or "service")
    monkeypatch.setattr(serve, "create_app", lambda service: service)
    monkeypatch.setitem(sys.modules, "uvicorn", types.SimpleNamespace(
        run=lambda app, **kw: None))
    for extra in ([], ["--resident-state"],
                  ["--resident-state", "--shared-ctx", "--fused-select"]):
        monkeypatch.setattr(sys, "argv",
                            ["serve.py", "model.npz", "dict.pkl"] + extra)
        cli.main()
    assert [kw["resident_state"] for kw in seen] == [False, True, True]
    assert [kw["shared_ctx"] for kw in seen] == [False, False, True]
    assert [kw["fused_select"] for kw in seen] == [False, False, True]


# ---------------------------------------------------------------- GPU tests

@pytest.fixture(scope="module")
def ext():
    m = ops._hip_ext()
    assert m is not None, "HIP extension must build/load on a GPU box"
    return m


# id -> (n_prev, Rmax, D per buffer, L)
GPU_OP_CASES = {
    "unaligned_alpha_rows": (5, 9, (16, 32, 7), 6),   # D 7: odd row bases
    "tiny_D": (5, 8, (3, 1, 2), 5),
    "multi_segment": (60, 60, (1000, 2000, 832), 37),  # 1 + 2 + 1 segments
    "L_eq_Rmax": (5, 8, (16, 32, 7), 8),
}


@functools.lru_cache(maxsize=None)
def _gpu_case(case_id):
    n_prev, Rmax, Ds, L = GPU_OP_CASES[case_id]
    parent = _perm_parents(n_prev, L)
    table, src, _, _ = _op_inputs(n_prev, Rmax, Ds, parent, seed=3)
    return table, src


@gpu
@pytest.mark.parametrize("route", list(ROUTE_DTYPES))
@pytest.mark.parametrize("form", ["host", "device"])
@pytest.mark.parametrize("case_id", list(GPU_OP_CASES))
def test_beam_reorder_kernel_equals_eager(ext, case_id, form, route):
    n_prev, Rmax, Ds, L = GPU_OP_CASES[case_id]
    table, src = _gpu_case(case_id)
    rd = ROUTE_DTYPES[route]
    w_dst, w_y, w_r = _fresh_out(Rmax, Ds, rd)
    eager.beam_reorder(torch.tensor(table), src, w_dst, w_y, w_r, n_prev)
    # the eager twin is itself held to the index_select expression
    _assert_buffers((w_dst, w_y, w_r), _expected(table, src, Rmax, rd),
                    case_id)
    src_g = tuple(s.cuda() for s in src)
    dst, y, r = _fresh_out(Rmax, Ds, rd, device="cuda")
    tab = table if form == "host" else torch.tensor(table, device="cuda")
    ret = ops.beam_reorder(tab, src_g, dst, y, r)
    torch.cuda.synchronize()
    _assert_buffers((dst, y, r), (w_dst, w_y, w_r), case_id)
    for s, k in zip(src_g, src):
        assert torch.equal(s.cpu(), k)
    assert ret.is_cuda and ret.dtype == torch.int64
    assert ret[0].tolist() == table[0]
    if form == "device":
        assert ret.data_ptr() == tab.data_ptr()


@gpu
def test_beam_reorder_kernel_guard(ext):
    """A device table is taken on trust; a parent one past the [:n_prev]
    view, but inside the allocation (a missing guard would read valid
    memory, not fault), must not be read: NaN row, y 0, route 0; every
    other row exact."""
    n_prev, Rmax, Ds = 5, 9, (16, 32, 7)
    g = torch.Generator().manual_seed(9)
    alloc = tuple(torch.randn(n_prev + 3, D, generator=g).cuda() for D in Ds)
    src = tuple(a[:n_prev] for a in alloc)
    parent = [4, 0, n_prev, 2, -1, 1]
    word = [11, 12, 13, 14, 15, 16]
    sent = [1, 2, 3, 4, 5, 0]
    table = torch.tensor([parent, word, sent], device="cuda")
    for rd in ROUTE_DTYPES.values():
        dst, y, r = _fresh_out(Rmax, Ds, rd, device="cuda")
        ops.beam_reorder(table, src, dst, y, r)
        torch.cuda.synchronize()
        for a, d in zip(alloc, dst):
            d, a = d.cpu(), a.cpu()
            for row, p in enumerate(parent):
                if 0 <= p < n_prev:
                    assert torch.equal(d[row], a[p]), row
                else:
                    assert bool(torch.isnan(d[row]).all()), row
            for row in range(len(parent), Rmax):      # padding: new row 0
                assert torch.equal(d[row], a[parent[0]]), row
        assert y.tolist() == [11, 12, 0, 14, 0, 16, 11, 11, 11]
        assert r.tolist() == [1, 2, 0, 4, 0, 0, 1, 1, 1]
    # the same table from the host is refused before any launch
    with pytest.raises(ValueError, match="parent"):
        ops.beam_reorder([parent, word, sent], src, dst, y, r)
    with pytest.raises(ValueError, match="overlap"):
        ops.beam_reorder([[0], [1], [0]], src,
                         tuple(a[1:1 + Rmax - 2] for a in alloc), y[:7],
                         r[:7])


def _gpu_batch(model, xs, Ts):
    """Padded per-sentence context of ``xs`` on the GPU, fp32."""
    lens = [int(x.shape[0]) for x in xs]
    S = len(xs)
    x_pad = torch.zeros(Ts, S, dtype=torch.int64, device="cuda")
    mask = torch.zeros(Ts, S, device="cuda")
    for i, x in enumerate(xs):
        x_pad[:lens[i], i] = x[:, 0].cuda()
        mask[:lens[i], i] = 1.0
    _, ctx = model.f_init(x_pad, mask)
    return (ctx.float() * mask[:, :, None]).contiguous(), mask


@gpu
@pytest.mark.parametrize("shared", [False, True])
def test_stepper_replay_after_reorder(ext, shared):
    """Two consecutive steps with different live counts and routing:
    beam_reorder into the stepper's buffers + replay() gives the six
    outputs of step(...) fed the gathered values, on one captured graph."""
    model, xs = _setup()
    model = model.cuda()
    ctx, mask = _gpu_batch(model, xs, Ts=64)
    pctx = model.project_ctx(ctx)
    Ts, R = 64, 9
    st = graph_mod.BatchedGraphStepper(model, ctx, mask, pctx, R,
                                       shared_ctx=shared)
    dsts, y_buf, route_buf = st.resident_buffers()
    assert route_buf.dtype == (torch.int32 if shared else torch.int64)
    assert route_buf is (st.row_src if shared else st.sent_idx)
    assert y_buf is st.y_in and len(dsts) == 3
    assert [d.data_ptr() for d in dsts] == [
        b.data_ptr() for b in (st.state_in, st.accC_in, st.accA_in)]

    # step 0 through the copying entry: 3 rows, one per sentence
    g = torch.Generator().manual_seed(21)
    H, C = model.options["dim"], 2 * model.options["dim"]
    route0 = torch.tensor([0, 1, 2], device="cuda")
    prev = [o[:3].clone() for o in st.step(
        route0, torch.full((3,), -1, device="cuda"),
        (torch.randn(3, H, generator=g) * 0.1).cuda(),
        torch.zeros(3, C, device="cuda"), torch.zeros(3, Ts, device="cuda"))]
    graphs = [st.graph]
    # (parent, word, sentence) of the next two steps: 7 rows, then 4
    tables = ([[2, 0, 0, 1, 2, 1, 1], [5, 9, 33, 7, 2, 60, 4],
               [2, 0, 0, 1, 2, 1, 1]],
              [[6, 3, 3, 0], [8, 8, 41, 3], [1, 1, 1, 2]])
    for step, table in enumerate(tables):
        live = len(table[0])
        parent = torch.tensor(table[0], device="cuda")
        # prev: (probs, h2, alpha, ctx_t, acc_ctx, acc_alpha)
        gathered = [prev[i].index_select(0, parent) for i in (1, 4, 5)]
        want = [o[:live].clone() for o in st.step(
            torch.tensor(table[2], device="cuda"),
            torch.tensor(table[1], device="cuda"), *gathered)]
        # what step() wrote, by its padding rule (not read back after the
        # replay: the step kernels update the accumulator inputs in place)
        values = [torch.tensor(table[2], device="cuda").to(route_buf.dtype),
                  torch.tensor(table[1], device="cuda")] + gathered
        want_in = [torch.cat([v, v[:1].expand(R - live, *v.shape[1:])])
                   for v in values]
        for b in st.inputs:
            b.fill_(0)
        ops.beam_reorder(table, (prev[1], prev[4], prev[5]), dsts, y_buf,
                         route_buf)
        for b, w in zip(st.inputs, want_in):
            assert torch.equal(b, w), step        # padding tail included
        got = [o[:live].clone() for o in st.replay()]
        graphs.append(st.graph)
        assert len(got) == len(want) == 6
        for i, (a, b) in enumerate(zip(got, want)):
            assert torch.equal(a, b), (step, i)
        prev = got
    assert graphs[0] is not None
    assert graphs[0] is graphs[1] is graphs[2]


GPU_BEAM_MODES = {
    "plain": {},
    "fused_paged_shared": dict(fused_select=True, paged_rerank=True,
                               shared_ctx=True, **LAMBDAS),
    "ragged_maxlen": dict(maxlen=[8, 3, 6]),
}


def _gpu_decode_pair(mode, use_graph, table=GPU_BEAM_MODES, **more):
    kw, lens = _mode_kw(mode, table)
    kw.update(use_graph=use_graph, **more)
    model, xs = _setup(lens)
    model = model.cuda()
    xs = [x.cuda() for x in xs]
    if use_graph:
        # both runs replay one cached stepper: capture it beforehand, so
        # that the capture's warm-up runs fall into neither of them
        gen_sample_batched(model, xs, **dict(kw, maxlen=1))
    return _decode_pair(model, xs, kw), xs, kw


@gpu
@pytest.mark.parametrize("use_graph", [True, False])
@pytest.mark.parametrize("mode", list(GPU_BEAM_MODES))
def test_batched_resident_gpu(ext, mode, use_graph):
    """Seed 4, EOS factor 2 (the CPU pair) gives the EOS / cap mix on the
    GPU too: asserted in _decode_pair."""
    _gpu_decode_pair(mode, use_graph)


@gpu
def test_batched_resident_gpu_k7_graph(ext):
    """Five sentences x beam 7 = 35 rows: the step kernels run two row
    chunks inside the captured graph."""
    want, xs, kw = _gpu_decode_pair(
        "k7_five_sentences", True, table=BEAM_MODES)
    assert len(xs) * kw["k"] > ops.MAX_KERNEL_BATCH
    assert all(len(w[0]) == 7 for w in want)


@gpu
def test_batched_resident_gpu_eager(ext, monkeypatch):
    """With the kernels switched off the eager twin of beam_reorder moves
    the rows on the device: still the same results, bit for bit."""
    monkeypatch.setenv("NATS_AMD_FORCE_EAGER", "1")
    _gpu_decode_pair("fused_paged_shared", False)
