"""Paged distraction-rerank histories (ops.rerank_advance,
ops.rerank_penalties_paged, ops.RerankHistory,
gen_sample_batched(paged_rerank=True)).

The oracle is the reference's own bookkeeping: explicit per-hypothesis
Python lists, copied on every reshuffle of the beam, fed to the numpy fp64
``distraction_penalties``. One seeded random tree (``_tree_case``) is built
once per process and shared by the CPU and GPU tests; nothing mutates it.

Bounds: the eager op (CPU dispatch) against the list reference at rtol
1e-5 / atol 1e-6, the bound test_rerank_reference_precondition uses
between the same two oracles; the kernel against the list reference at
rtol 1e-4 / atol 1e-5, the bound of test_rerank_strided_loops for the same
arithmetic; the kernel against the dense kernel bit for bit, because both
run the same per-step device functions and min/max are exact.
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
from nats_amd.ops import eager

from test_beam_select import _inflate_attention, _setup

gpu = pytest.mark.gpu

STEPS_PER_BLOCK = 8  # history steps per partial-pass block in rerank.hip
FACTORS = (1.3, 0.7, 2.1)
TMAX, RMAX = 20, 12
TS, C, H = 150, 130, 70
# rows of the batch at steps 0..19: grows, shrinks, fills the table
COUNTS = (1, 3, 7, 12, 5, 7, 12, 9, 11, 12, 6, 10, 12, 8, 12, 11, 12, 10, 12,
          9)
N_STEPS = len(COUNTS) - 1   # 19 history steps before the last current step
ZERO_STEP, ZERO_ROW = 4, 2  # final row whose step-4 context is zero-norm


# --------------------------------------------------------------- the tree

@functools.lru_cache(maxsize=None)
def _tree_case():
    """content[t] = (a, c, s) fp32 step outputs of the COUNTS[t] rows of
    step t, built as _rerank_case of test_gpu_kernel_edges.py builds its
    rows (exact zeros in the attention weights, one zero-norm context
    vector); parents[t] (t >= 1) = the row of step t-1 each row continues;
    tables[n] (n >= 1) = the ancestor table after the advance at step n,
    built in plain numpy; refs[n] = fp64 list-reference penalties of step
    n's rows; terms = per-(step, final row) fp64 (kl, cd, sd)."""
    from nats_amd.decode.beam import (_cosine_dist, _kl_div,
                                      distraction_penalties)
    rng = numpy.random.RandomState(0)
    content, parents = [], [None]
    for t, R in enumerate(COUNTS):
        a = rng.rand(R, TS).astype("float32") + 1e-3
        a[:, ::7] = 0
        content.append((a, rng.randn(R, C).astype("float32"),
                        rng.randn(R, H).astype("float32")))
        if t:
            parents.append(rng.randint(0, COUNTS[t - 1], size=R))

    tables = [None]
    anc = numpy.full((TMAX, RMAX), -1, dtype="int32")
    for n in range(1, N_STEPS + 1):
        new = numpy.full((TMAX, RMAX), -1, dtype="int32")
        p = parents[n]
        new[:n - 1, :len(p)] = anc[:n - 1][:, p]
        new[n - 1, :len(p)] = p
        tables.append(new)
        anc = new
    # the zero-norm context vector sits on final row ZERO_ROW's ancestry
    content[ZERO_STEP][1][tables[N_STEPS][ZERO_STEP, ZERO_ROW]] = 0

    # the reference: per-hypothesis lists, copied on every reshuffle
    la, lc, ls = [[]], [[]], [[]]
    refs = [None]
    for n in range(1, N_STEPS + 1):
        pa, pc, ps = content[n - 1]
        la = [list(la[p]) + [pa[p].copy()] for p in parents[n]]
        lc = [list(lc[p]) + [pc[p].copy()] for p in parents[n]]
        ls = [list(ls[p]) + [ps[p].copy()] for p in parents[n]]
        refs.append(sum(distraction_penalties(
            la, lc, ls, *content[n], *FACTORS)).astype("float64"))
    ca, cc, cs = content[N_STEPS]
    R = COUNTS[N_STEPS]
    kl = numpy.array([[_kl_div(la[r][t], ca[r]) for r in range(R)]
                      for t in range(N_STEPS)])
    cd = numpy.array([[_cosine_dist(lc[r][t], cc[r]) for r in range(R)]
                      for t in range(N_STEPS)])
    sd = numpy.array([[_cosine_dist(ls[r][t], cs[r]) for r in range(R)]
                      for t in range(N_STEPS)])
    return dict(content=content, parents=parents, tables=tables, refs=refs,
                terms=(kl, cd, sd))


def _slabs(case, device):
    """Slabs holding every step's rows; unwritten slots are NaN, so a read
    through a wrong slot shows."""
    slabs = [torch.full((TMAX, RMAX, d), float("nan")) for d in (TS, C, H)]
    for t in range(N_STEPS):
        for slab, rows in zip(slabs, case["content"][t]):
            slab[t, :COUNTS[t]] = torch.from_numpy(rows)
    return [s.to(device) for s in slabs]


def _advance_all(case, device, parent_as=list):
    """Tables after each advance, through ops.rerank_advance with ping-pong
    tables as RerankHistory keeps them."""
    anc = [torch.full((TMAX, RMAX), -1, dtype=torch.int32, device=device)
           for _ in range(2)]
    out = [None]
    for n in range(1, N_STEPS + 1):
        got = ops.rerank_advance(anc[0], anc[1],
                                 parent_as(case["parents"][n]), n,
                                 COUNTS[n - 1])
        assert got is anc[1]
        anc.reverse()
        out.append(anc[0].clone())
    return out


def _cur(case, n, device):
    return [torch.from_numpy(x).to(device) for x in case["content"][n]]


# -------------------------------------------------------------- CPU tests

def test_tree_preconditions():
    """The tree exercises what it is meant to: an extremal step of each
    term beyond the first block, a partial last block, a table that is not
    the identity, slots beyond the final step's R (an R-strided read of the
    Rmax-strided table would go wrong), siblings, dropped rows and the
    zero-norm vector on a final row's ancestry. Extremal steps of the 9
    final rows here: KL argmin 6 9 15 4 6 17 5 0 16; context argmax
    10 1 2 3 6 11 10 10 17; state argmax 1 13 8 12 14 0 10 0 9."""
    case = _tree_case()
    kl, cd, sd = case["terms"]
    print("paged rerank extremal steps: kl %s ctx %s state %s" % (
        kl.argmin(0), cd.argmax(0), sd.argmax(0)))
    assert kl.argmin(0).max() >= STEPS_PER_BLOCK
    assert cd.argmax(0).max() >= STEPS_PER_BLOCK
    assert sd.argmax(0).max() >= STEPS_PER_BLOCK
    assert N_STEPS % STEPS_PER_BLOCK != 0
    final = case["tables"][N_STEPS][:N_STEPS, :COUNTS[N_STEPS]]
    assert (final != numpy.arange(COUNTS[N_STEPS])[None, :]).any()
    assert (final >= COUNTS[N_STEPS]).any()
    assert (final >= 0).all() and (final < numpy.array(
        COUNTS[:N_STEPS])[:, None]).all()
    assert cd[ZERO_STEP, ZERO_ROW] == 0.0
    assert (case["content"][3][0] == 0).any()
    for n in range(1, N_STEPS + 1):
        p = case["parents"][n]
        assert len(p) == COUNTS[n]
    assert any(len(set(p)) < len(p) for p in case["parents"][1:])
    assert any(len(set(p)) < COUNTS[n - 1]
               for n, p in enumerate(case["parents"]) if n)
    assert min(TS, C, H) > 64  # every lane-strided loop makes a second trip


def test_advance_matches_numpy_tables():
    case = _tree_case()
    for conv in (list, lambda p: torch.tensor(p, dtype=torch.int32),
                 lambda p: torch.tensor(p, dtype=torch.int64)):
        got = _advance_all(case, "cpu", conv)
        for n in range(1, N_STEPS + 1):
            numpy.testing.assert_array_equal(
                got[n][:n, :COUNTS[n]].numpy(),
                case["tables"][n][:n, :COUNTS[n]])


def test_paged_penalties_match_list_reference():
    """ops.rerank_penalties_paged after ops.rerank_advance, at every step,
    against the per-hypothesis-list reference."""
    case = _tree_case()
    slabs = _slabs(case, "cpu")
    tables = _advance_all(case, "cpu")
    for n in range(1, N_STEPS + 1):
        got = ops.rerank_penalties_paged(
            *slabs, tables[n], n, *_cur(case, n, "cpu"), *FACTORS)
        assert got.shape == (COUNTS[n],) and got.dtype == torch.float32
        numpy.testing.assert_allclose(got.numpy(), case["refs"][n],
                                      rtol=1e-5, atol=1e-6)
    zero = ops.rerank_penalties_paged(
        *slabs, tables[1], 0, *_cur(case, 0, "cpu"), *FACTORS)
    assert zero.tolist() == [0.0]


def test_history_steps_through_the_tree():
    """RerankHistory.step: advance, penalties, append; zeros at step 0."""
    case = _tree_case()
    hist = ops.RerankHistory(TMAX, RMAX, TS, C, H, "cpu")
    for n in range(N_STEPS + 1):
        pen = hist.step(case["parents"][n], *_cur(case, n, "cpu"), FACTORS)
        assert pen.shape == (COUNTS[n],) and hist.n == n + 1
        if n == 0:
            assert pen.tolist() == [0.0]
        else:
            numpy.testing.assert_allclose(pen.numpy(), case["refs"][n],
                                          rtol=1e-5, atol=1e-6)


MAXLENS = {"8": 8, "3_8_6": [3, 8, 6], "14": 14}


@functools.lru_cache(maxsize=None)
def _decode(maxlen_id, fused, paged, lam=0.7, device="cpu",
            dims=(12, 16, 8, 80), use_graph=True):
    from nats_amd.decode.batched import gen_sample_batched
    model, xs = _setup(seed=9, device=device, dims=dims)
    _inflate_attention(model)
    extra = {"paged_rerank": True} if paged else {}
    return gen_sample_batched(
        model, xs, k=3, maxlen=MAXLENS[maxlen_id], use_unk=True,
        kl_factor=lam, ctx_factor=lam, state_factor=lam,
        fused_select=fused, use_graph=use_graph, **extra)


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("maxlen_id", sorted(MAXLENS))
def test_paged_decode_equals_dense_histories(maxlen_id, fused):
    ref = _decode(maxlen_id, fused, False)
    got = _decode(maxlen_id, fused, True)
    assert len(ref) == len(got) == 3
    for (rs, rc, ra), (gs, gc, ga) in zip(ref, got):
        assert gs == rs
        assert gc == rc
        assert len(ga) == len(ra)
        for a_g, a_r in zip(ga, ra):
            assert len(a_g) == len(a_r)
            for v_g, v_r in zip(a_g, a_r):
                numpy.testing.assert_array_equal(v_g, v_r)
    # not vacuous: the rerank decides something here ...
    plain = _decode(maxlen_id, fused, False, lam=0.0)
    assert any(ps != rs for (ps, _, _), (rs, _, _) in zip(plain, ref))
    # ... a sentence retires a hypothesis at length 1 (its want narrows
    # from the second step on) ...
    assert any(s == [0] for s in ref[1][0])
    if maxlen_id == "3_8_6":
        # ... and sentences 0 and 2 are cut off at their caps while
        # sentence 1 decodes on
        for i, cap in ((0, 3), (2, 6)):
            assert any(len(s) == cap and s[-1] != 0 for s in ref[i][0])
        assert max(len(s) for s in ref[1][0]) > 6


def test_paged_flag_without_lambdas_is_a_noop(monkeypatch):
    made = []
    monkeypatch.setattr(ops, "RerankHistory",
                        lambda *a, **kw: made.append(a))
    got = _decode("8", True, True, lam=0.0)
    ref = _decode("8", True, False, lam=0.0)
    assert [g[:2] for g in got] == [r[:2] for r in ref]
    assert made == []


def test_op_validation():
    case = _tree_case()
    slabs = _slabs(case, "cpu")
    anc = torch.from_numpy(case["tables"][3].copy())
    cur = _cur(case, 3, "cpu")
    ok = lambda **kw: ops.rerank_penalties_paged(  # noqa: E731
        kw.get("a", slabs[0]), kw.get("c", slabs[1]), kw.get("s", slabs[2]),
        kw.get("anc", anc), kw.get("n", 3), kw.get("ca", cur[0]),
        kw.get("cc", cur[1]), kw.get("cs", cur[2]), *FACTORS)
    assert ok().shape == (COUNTS[3],)
    name = "rerank_penalties_paged"
    with pytest.raises(TypeError, match=name):
        ok(a=slabs[0].double())
    with pytest.raises(TypeError, match=name):
        ok(cs=cur[2].half())
    with pytest.raises(TypeError, match=name):
        ok(anc=anc.long())
    with pytest.raises(TypeError, match=name):
        ok(c=slabs[1][0])
    with pytest.raises(ValueError, match=name):
        ok(a=torch.cat([slabs[0], slabs[0]], 2)[:, :, ::2])
    with pytest.raises(ValueError, match=name):
        ok(anc=torch.cat([anc, anc], 1)[:, ::2])
    with pytest.raises(ValueError, match="n=21"):
        ok(n=TMAX + 1)
    with pytest.raises(ValueError, match=name):
        ok(s=slabs[2][:, :RMAX - 1].contiguous())
    with pytest.raises(ValueError, match=name):
        ok(cc=cur[1][:-1])
    big = [torch.zeros(RMAX + 1, d) for d in (TS, C, H)]
    with pytest.raises(ValueError, match="R=13"):
        ok(ca=big[0], cc=big[1], cs=big[2])

    new = torch.empty_like(anc)
    adv = lambda **kw: ops.rerank_advance(  # noqa: E731
        kw.get("old", anc), kw.get("new", new),
        kw.get("parent", [0, 2, 11, 5]), kw.get("n", 4),
        kw.get("prev", COUNTS[3]))
    assert adv() is new
    name = "rerank_advance"
    with pytest.raises(ValueError, match=r"parent\[2\]=12"):
        adv(parent=[0, 2, 12, 5])
    with pytest.raises(ValueError, match=r"parent\[1\]=5"):
        adv(parent=torch.tensor([0, 5]), prev=5)
    with pytest.raises(ValueError, match=r"parent\[0\]=-1"):
        adv(parent=[-1])
    with pytest.raises(TypeError, match=name):
        adv(parent=torch.tensor([0.0, 1.0]))
    with pytest.raises(TypeError, match=name):
        adv(new=new.long())
    with pytest.raises(ValueError, match=name):
        adv(new=anc)
    with pytest.raises(ValueError, match=name):
        adv(new=torch.empty(TMAX, RMAX + 1, dtype=torch.int32))
    with pytest.raises(ValueError, match="n=0"):
        adv(n=0)
    with pytest.raises(ValueError, match="n=21"):
        adv(n=TMAX + 1)
    with pytest.raises(ValueError, match="R=13"):
        adv(parent=[0] * (RMAX + 1))
    with pytest.raises(ValueError, match="prev_rows=13"):
        adv(prev=RMAX + 1)


def test_service_passes_paged_rerank(tmp_path, monkeypatch):
    from nats_amd.data.synthetic import make_toy_corpus
    from nats_amd.engine.checkpoint import save_checkpoint
    from nats_amd.models.distraction import NatsModel, default_options
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
        seen.append(kw.get("paged_rerank"))
        return real(*a, **kw)

    monkeypatch.setattr(app, "gen_sample_batched", spy)
    dictionary = os.path.join(d, "toy_train_input.txt.pkl")
    assert SummarizerService(saveto, dictionary, device="cpu",
                             k=3).paged_rerank is False
    for flag in (False, True):
        svc = SummarizerService(
            saveto, dictionary, device="cpu", k=3, maxlen=6, max_wait_ms=1.0,
            kl_factor=0.5, ctx_factor=0.5, state_factor=0.5,
            paged_rerank=flag)
        try:
            assert isinstance(svc.summarize("a b c d")["summary"], str)
        finally:
            svc.close()
    assert seen == [False, True]


def test_cli_passes_paged_rerank(monkeypatch):
    """scripts/serve.py --paged-rerank reaches SummarizerService (service
    and server are stand-ins: nothing is loaded or served)."""
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
    for extra in ([], ["--paged-rerank"]):
        monkeypatch.setattr(sys, "argv",
                            ["serve.py", "model.npz", "dict.pkl"] + extra)
        cli.main()
    assert [kw["paged_rerank"] for kw in seen] == [False, True]
    assert [kw["fused_select"] for kw in seen] == [False, False]


# -------------------------------------------------------------- GPU tests

@pytest.fixture(scope="module")
def ext():
    m = ops._hip_ext()
    assert m is not None, "HIP extension must build/load on a GPU box"
    assert hasattr(m, "rerank_penalties_paged")
    assert hasattr(m, "rerank_advance")
    return m


@pytest.fixture(scope="module")
def dev(ext):
    """Slabs and the per-step tables on the device, advanced there."""
    case = _tree_case()
    return dict(case=case, slabs=_slabs(case, "cuda"),
                tables=_advance_all(case, "cuda"))


def _check_step(ext, dev, n):
    case = dev["case"]
    R = COUNTS[n]
    cur = _cur(case, n, "cuda")
    got = ops.rerank_penalties_paged(*dev["slabs"], dev["tables"][n], n,
                                     *cur, *FACTORS)
    assert got.shape == (R,) and got.dtype == torch.float32
    numpy.testing.assert_allclose(got.cpu().numpy(), case["refs"][n],
                                  rtol=1e-4, atol=1e-5)
    dense = [eager.rerank_gather(s, dev["tables"][n], n, R).contiguous()
             for s in dev["slabs"]]
    old = ext.rerank_penalties(*dense, *cur, *FACTORS)
    numpy.testing.assert_array_equal(got.cpu().numpy(), old.cpu().numpy())


@gpu
def test_device_advance_equals_eager(dev):
    """Integers: exact, over the whole tree, from a host list (checked and
    uploaded) and from a device tensor (taken as is)."""
    case = dev["case"]
    on_dev = _advance_all(
        case, "cuda", lambda p: torch.tensor(p, dtype=torch.int64,
                                             device="cuda"))
    for n in range(1, N_STEPS + 1):
        want = case["tables"][n][:n, :COUNTS[n]]
        for tabs in (dev["tables"], on_dev):
            numpy.testing.assert_array_equal(
                tabs[n][:n, :COUNTS[n]].cpu().numpy(), want)


@gpu
def test_kernel_every_step(ext, dev):
    """Against the fp64 list reference and, bit for bit, against the dense
    kernel on the history gathered through the table."""
    for n in range(1, N_STEPS + 1):
        _check_step(ext, dev, n)


@gpu
@pytest.mark.parametrize("n", [1, STEPS_PER_BLOCK, STEPS_PER_BLOCK + 1,
                               N_STEPS])
def test_kernel_step_counts(ext, dev, n):
    """A single step; exactly one full block; a second block holding one
    step and three idle waves; a partial third block."""
    _check_step(ext, dev, n)


@gpu
def test_kernel_no_history(ext, dev):
    cur = _cur(dev["case"], 0, "cuda")
    got = ops.rerank_penalties_paged(*dev["slabs"], dev["tables"][1], 0,
                                     *cur, *FACTORS)
    assert got.cpu().tolist() == [0.0]


@gpu
def test_kernel_on_leading_rows_of_a_larger_buffer(ext, dev):
    """The graph stepper hands over the first rows of its fixed-size
    output buffers."""
    n = N_STEPS
    R = COUNTS[n]
    cur = _cur(dev["case"], n, "cuda")
    ref = ops.rerank_penalties_paged(*dev["slabs"], dev["tables"][n], n,
                                     *cur, *FACTORS)
    bufs = []
    for c in cur:
        buf = torch.full((RMAX + 4, c.shape[1]), float("nan"), device="cuda")
        buf[:R] = c
        bufs.append(buf[:R])
    got = ops.rerank_penalties_paged(*dev["slabs"], dev["tables"][n], n,
                                     *bufs, *FACTORS)
    numpy.testing.assert_array_equal(got.cpu().numpy(), ref.cpu().numpy())


@gpu
def test_history_on_device(ext, dev):
    case = dev["case"]
    hist = ops.RerankHistory(TMAX, RMAX, TS, C, H, "cuda")
    for n in range(N_STEPS + 1):
        pen = hist.step(case["parents"][n], *_cur(case, n, "cuda"), FACTORS)
        if n:
            numpy.testing.assert_allclose(pen.cpu().numpy(), case["refs"][n],
                                          rtol=1e-4, atol=1e-5)
        else:
            assert pen.cpu().tolist() == [0.0]


@gpu
@pytest.mark.parametrize("fused", [False, True])
def test_paged_decode_on_gpu_with_graph(ext, fused):
    """The decoder step kernels accumulate with float atomics, so two GPU
    decodes are not bit-reproducible: compared as
    test_fused_decode_on_gpu_with_graph compares."""
    kw = dict(device="cuda", dims=(16, 32, 12, 90), use_graph=True)
    ref = _decode("8", fused, False, **kw)
    got = _decode("8", fused, True, **kw)
    for (rs, rc, _), (gs, gc, _) in zip(ref, got):
        assert sorted(map(tuple, gs)) == sorted(map(tuple, rs))
        numpy.testing.assert_allclose(sorted(gc), sorted(rc), rtol=1e-4)
