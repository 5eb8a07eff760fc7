"""Segmented beam candidate selection (ops.beam_select): the eager oracle
against a transcription of the per-sentence decode code, the HIP kernels
against the oracle, and gen_sample_batched(fused_select=True) against the
per-sentence path.

Exact index equality is a fair demand because the winners are PLANTED:
bulk candidates have -log p in [8, 12] and prev_cost in [0, 2] (penalty in
[0, 1]), planted candidates get keys 3 + 0.01*j. Planted keys are 1e-2
apart and more than 4 below every bulk key, while two fp32 log
implementations differ by an ulp or two (~2e-6 at magnitudes below 16), so
no log can reorder them. Deliberate ties use bit-identical p, prev_cost and
penalty, which gives bit-identical keys under any log. Costs are compared
with rtol=atol=1e-5 (one fp32 ulp below 16 is 1.9e-6).
"""

import math

import numpy
import pytest
import torch

from nats_amd import ops
from nats_amd.ops import eager

TILE = 2048  # words per tile-pass block in beam_select.hip
NEG_UNK = math.log(1e-20)


# --------------------------------------------------------------- inputs

def _bulk(rng, lives, V):
    R = sum(lives)
    prev = rng.uniform(0.0, 2.0, size=R).astype("float32")
    nlogp = rng.uniform(8.0, 12.0, size=(R, V))
    return prev, nlogp


def _finish(prev, nlogp, lives, wants, pen=None, use_unk=True):
    probs = torch.from_numpy(numpy.exp(-nlogp).astype("float32"))
    seg = numpy.concatenate([[0], numpy.cumsum(lives)])
    return dict(probs=probs, prev=torch.from_numpy(prev),
                seg=torch.tensor(seg, dtype=torch.int32),
                want=torch.tensor(wants, dtype=torch.int32),
                pen=None if pen is None else torch.from_numpy(pen),
                use_unk=use_unk)


def _planted(seed, V, lives, wants, with_pen=False, use_unk=True,
             positions=None):
    """Bulk + ~2K planted winners per segment. ``positions`` optionally
    fixes each segment's planted (local_row, word) list."""
    rng = numpy.random.RandomState(seed)
    prev, nlogp = _bulk(rng, lives, V)
    pen = (rng.uniform(0.0, 1.0, size=len(prev)).astype("float32")
           if with_pen else None)
    K = max(wants)
    row0 = 0
    for s, live in enumerate(lives):
        if positions is not None:
            pos = positions[s]
        else:
            # word 1 is left to the UNK cases
            cells = [(r, w) for r in range(live) for w in range(V) if w != 1]
            n = min(2 * K, len(cells))
            pick = rng.choice(len(cells), size=n, replace=False)
            pos = [cells[i] for i in pick]
        for j, (r, w) in enumerate(pos):
            target = 3.0 + 0.01 * j
            base = float(prev[row0 + r]) + (float(pen[row0 + r])
                                            if with_pen else 0.0)
            nlogp[row0 + r, w] = target - base
        row0 += live
    return _finish(prev, nlogp, lives, wants, pen, use_unk)


def _tie_case(V):
    """Seven bit-identical keys: inside a row, across rows, and on both
    sides of the first tile boundary; one strictly better key."""
    rng = numpy.random.RandomState(5)
    prev, nlogp = _bulk(rng, [2], V)
    prev[:] = 1.0
    for r, w in ((0, 5), (0, 9), (0, TILE - 1), (0, TILE), (1, 3),
                 (1, TILE - 1), (1, TILE)):
        nlogp[r, w] = 2.0
    nlogp[1, 40] = 1.5
    case = _finish(prev, nlogp, [2], [6])
    case["expect_ranks"] = [V + 40, 5, 9, TILE - 1, TILE, V + 3]
    return case


def _penalty_case():
    """Row 0 holds the better cost, its penalty puts row 1 first; the
    returned costs are the un-reranked ones."""
    V = 50
    rng = numpy.random.RandomState(6)
    prev, nlogp = _bulk(rng, [2], V)
    prev[:] = (0.5, 1.0)
    nlogp[0, 7] = 1.5    # cost 2.0, key 4.0
    nlogp[1, 9] = 2.0    # cost 3.0, key 3.0
    pen = numpy.array([2.0, 0.0], dtype="float32")
    case = _finish(prev, nlogp, [2], [2], pen)
    case["expect_ranks"] = [V + 9, 7]
    case["expect_costs"] = [3.0, 2.0]
    return case


def _unk_case(use_unk):
    """Word 1 planted as the best candidate of every row."""
    V = 60
    case = _planted(7, V, [2], [4], use_unk=use_unk,
                    positions=[[(0, 1), (1, 1), (0, 8), (1, 30), (0, 31),
                                (1, 2)]])
    case["expect_ranks"] = ([1, V + 1, 8, V + 30] if use_unk
                            else [8, V + 30, 31, V + 2])
    return case


def _zero_nan_case():
    """p == 0 costs +inf and sorts last; NaN sorts after +inf."""
    V = 20
    rng = numpy.random.RandomState(8)
    prev, nlogp = _bulk(rng, [1], V)
    case = _finish(prev, nlogp, [1], [V])
    case["probs"][0, 3] = float("nan")
    case["probs"][0, 11] = 0.0
    case["expect_tail"] = [11, 3]
    return case


def _one_per_tile_positions(V, live):
    tiles = (V + TILE - 1) // TILE
    return [(r, min(t * TILE + 17 * (r + 1) + t, V - 1 - r))
            for r in range(live) for t in range(tiles)]


CASES = {
    "single_partial_tile": lambda: _planted(1, 37, [1], [1]),
    "tile_plus_one": lambda: _planted(2, TILE + 1, [2], [5],
                                      positions=[[(0, TILE), (1, TILE),
                                                  (0, 0), (1, TILE - 1),
                                                  (0, 77), (1, 2), (0, 3)]]),
    "two_tiles_minus_one": lambda: _planted(3, 2 * TILE - 1, [2], [5]),
    "odd_stride_three_tiles": lambda: _planted(4, 4099, [3], [10]),
    "uneven_segments": lambda: _planted(9, 2500, [1, 3, 2], [3, 1, 2]),
    "uneven_segments_pen": lambda: _planted(10, 2500, [1, 3, 2], [3, 1, 2],
                                            with_pen=True),
    "k32_want_near_v": lambda: _planted(11, 40, [1], [32]),
    "winners_in_one_tile": lambda: _planted(
        12, 4099, [3], [10],
        positions=[[(1, TILE + 3 * j + 5) for j in range(20)]]),
    "one_winner_per_row_tile": lambda: _planted(
        13, 4099, [3], [9], positions=[_one_per_tile_positions(4099, 3)]),
    "ties": lambda: _tie_case(4099),
    "penalty_reorders": _penalty_case,
    "unk_suppressed": lambda: _unk_case(False),
    "unk_allowed": lambda: _unk_case(True),
    "zero_and_nan": _zero_nan_case,
}


# --------------------------------------------------------------- oracles

def _brute_force(case):
    """The per-sentence phase-1 code of gen_sample_batched, literally."""
    probs, prev = case["probs"], case["prev"]
    seg, wants = case["seg"].tolist(), case["want"].tolist()
    logp = probs.float().log()
    if not case["use_unk"]:
        logp[:, 1] = NEG_UNK
    out = []
    for s, want in enumerate(wants):
        sl = slice(seg[s], seg[s + 1])
        cand = prev[sl][:, None] - logp[sl]
        cand_flat = cand.flatten()
        sel_flat = cand_flat
        if case["pen"] is not None:
            sel_flat = (cand + case["pen"][sl][:, None]).flatten()
        ranks = sel_flat.topk(want, largest=False).indices
        out.append((ranks, cand_flat[ranks]))
    return out


def _run(case, device="cpu", fn=ops.beam_select, **kw):
    dev = {k: (v.to(device) if torch.is_tensor(v) else v)
           for k, v in case.items()}
    return fn(dev["probs"], dev["prev"], dev["seg"], dev["want"],
              penalty=dev["pen"], use_unk=dev["use_unk"], **kw)


def _check_expectations(case, ranks, costs):
    wants = case["want"].tolist()
    K = max(wants)
    assert ranks.shape == costs.shape == (len(wants), K)
    assert ranks.dtype == torch.int64 and costs.dtype == torch.float32
    for s, want in enumerate(wants):
        assert (ranks[s, want:] == -1).all()
        assert torch.isposinf(costs[s, want:]).all()
        assert (ranks[s, :want] >= 0).all()
    if "expect_ranks" in case:
        assert ranks[0, :wants[0]].tolist() == case["expect_ranks"]
    if "expect_costs" in case:
        numpy.testing.assert_allclose(costs[0].cpu().numpy(),
                                      case["expect_costs"], rtol=1e-5,
                                      atol=1e-5)
    if "expect_tail" in case:
        n = len(case["expect_tail"])
        assert ranks[0, wants[0] - n:wants[0]].tolist() == case["expect_tail"]


def _assert_same(got, ref):
    assert torch.equal(got[0].cpu(), ref[0].cpu())
    numpy.testing.assert_allclose(got[1].cpu().numpy(), ref[1].cpu().numpy(),
                                  rtol=1e-5, atol=1e-5, equal_nan=True)


# ------------------------------------------------------------ CPU cases

@pytest.mark.parametrize("use_unk", [True, False])
@pytest.mark.parametrize("with_pen", [False, True])
def test_eager_matches_decode_transcription(with_pen, use_unk):
    case = _planted(20, 300, [1, 3, 2], [3, 1, 2], with_pen=with_pen,
                    use_unk=use_unk)
    ranks, costs = _run(case)
    _check_expectations(case, ranks, costs)
    for s, (r, c) in enumerate(_brute_force(case)):
        want = len(r)
        assert ranks[s, :want].tolist() == r.tolist()
        numpy.testing.assert_allclose(costs[s, :want].numpy(), c.numpy(),
                                      rtol=1e-5, atol=1e-5)


def test_eager_is_the_cpu_dispatch(monkeypatch):
    case = CASES["uneven_segments_pen"]()
    _assert_same(_run(case), _run(case, fn=eager.beam_select))
    monkeypatch.setenv("NATS_AMD_FORCE_EAGER", "1")
    _assert_same(_run(case), _run(case, fn=eager.beam_select))


@pytest.mark.parametrize("name", ["ties", "penalty_reorders",
                                  "unk_suppressed", "unk_allowed",
                                  "zero_and_nan", "k32_want_near_v",
                                  "tile_plus_one"])
def test_eager_rules(name):
    """Tie rule (in a row, across rows, across a tile boundary), padding,
    un-reranked costs, UNK pinning, +inf and NaN ordering."""
    case = CASES[name]()
    ranks, costs = _run(case)
    _check_expectations(case, ranks, costs)
    if name == "zero_and_nan":
        assert torch.isposinf(costs[0, -2]) and torch.isnan(costs[0, -1])
    if name == "unk_suppressed":
        # word 1 still has a (large) cost of its own: prev - log(1e-20)
        full = dict(case, want=torch.tensor([32], dtype=torch.int32))
        r, c = _run(full)
        assert not (r[0] % 60 == 1).any()
        case1 = dict(case, probs=case["probs"][:1, :20].contiguous(),
                     prev=case["prev"][:1],
                     seg=torch.tensor([0, 1], dtype=torch.int32),
                     want=torch.tensor([20], dtype=torch.int32))
        r, c = _run(case1)
        at = r[0].tolist().index(1)
        numpy.testing.assert_allclose(
            float(c[0, at]), float(case["prev"][0]) - NEG_UNK, rtol=1e-6)


def test_lists_and_explicit_k():
    case = CASES["uneven_segments"]()
    ref = _run(case)
    as_lists = dict(case, seg=case["seg"].tolist(), want=case["want"].tolist())
    _assert_same(_run(as_lists), ref)
    wide = _run(case, K=5)
    assert wide[0].shape == (3, 5)
    assert torch.equal(wide[0][:, :3], ref[0])
    assert (wide[0][:, 3:] == -1).all()
    assert torch.isposinf(wide[1][:, 3:]).all()


def test_validation_errors():
    case = _planted(21, 40, [2, 1], [3, 2])
    probs, prev, seg, want = (case[k] for k in ("probs", "prev", "seg",
                                                 "want"))
    i32 = lambda v: torch.tensor(v, dtype=torch.int32)  # noqa: E731
    with pytest.raises(ValueError, match="K=33"):
        ops.beam_select(probs, prev, seg, i32([33, 2]))
    with pytest.raises(ValueError, match="K=40"):
        ops.beam_select(probs, prev, seg, want, K=40)
    with pytest.raises(ValueError, match="exceeds the sentence's 4 cand"):
        ops.beam_select(probs[:, :4].contiguous(), prev, seg, i32([3, 5]))
    with pytest.raises(ValueError, match=r"outside \[1, K"):
        ops.beam_select(probs, prev, seg, i32([0, 2]))
    with pytest.raises(ValueError, match="from 0 to R"):
        ops.beam_select(probs, prev, i32([0, 2, 4]), want)
    # live*V >= 2**31, on a stride-0 view so that nothing is allocated
    huge = torch.zeros(1, 1).expand(2, 2 ** 30)
    with pytest.raises(ValueError, match=r"2\*\*31"):
        ops.beam_select(huge, prev[:2], i32([0, 2]), i32([1]))
    with pytest.raises(TypeError, match="probs"):
        ops.beam_select(probs.double(), prev, seg, want)
    with pytest.raises(TypeError, match="prev_cost"):
        ops.beam_select(probs, prev.double(), seg, want)
    with pytest.raises(TypeError, match="penalty"):
        ops.beam_select(probs, prev, seg, want, penalty=prev.half())
    with pytest.raises(TypeError, match="int32"):
        ops.beam_select(probs, prev, seg.long(), want)
    with pytest.raises(TypeError, match="int32"):
        ops.beam_select(probs, prev, seg, want.long())
    with pytest.raises(ValueError, match="contiguous"):
        ops.beam_select(torch.cat([probs, probs], 1)[:, ::2], prev, seg, want)


# ------------------------------------------------- decode integration

def _setup(seed=3, device="cpu", dims=(12, 16, 8, 80)):
    from nats_amd.models.distraction import NatsModel, default_options
    dim_word, dim, dim_att, n_words = dims
    opts = default_options(dim_word=dim_word, dim=dim, dim_att=dim_att,
                           n_words=n_words)
    model = NatsModel(opts, seed=seed).eval()
    # inflate the readout so the beam's candidates are well separated (a
    # tiny random model is near-uniform and decides on exact ties)
    with torch.no_grad():
        for key in ("ff_logit_lstm_W", "ff_logit_ctx_W", "ff_logit_prev_W",
                    "ff_logit_W"):
            model.P[key].mul_(50.0)
    g = torch.Generator().manual_seed(seed)
    xs = []
    for n in (7, 11, 5):
        x = torch.randint(2, n_words, (n, 1), generator=g)
        x[-1] = 0
        xs.append(x.to(device))
    return model.to(device), xs


def _inflate_attention(model):
    with torch.no_grad():
        for k in ("decoder_W_att", "decoder_Wc_att", "decoder_U_att",
                  "decoder_D_wei"):
            model.P[k].mul_(40.0)


DECODE_MODES = {
    "plain": dict(seed=3, maxlen=9, lam=0.0),
    "rerank": dict(seed=9, maxlen=8, lam=0.7),
    "mixed_maxlen": dict(seed=3, maxlen=[3, 9, 6], lam=0.0),
}


def _decode_pair(mode, device="cpu", dims=(12, 16, 8, 80), **kw):
    from nats_amd.decode.batched import gen_sample_batched
    m = DECODE_MODES[mode]
    model, xs = _setup(seed=m["seed"], device=device, dims=dims)
    if m["lam"]:
        _inflate_attention(model)
    args = dict(k=3, maxlen=m["maxlen"], use_unk=True, kl_factor=m["lam"],
                ctx_factor=m["lam"], state_factor=m["lam"], **kw)
    return (gen_sample_batched(model, xs, fused_select=False, **args),
            gen_sample_batched(model, xs, fused_select=True, **args), xs)


@pytest.mark.parametrize("mode", sorted(DECODE_MODES))
def test_fused_decode_equals_per_sentence_path(mode):
    ref, fused, xs = _decode_pair(mode)
    assert len(ref) == len(fused) == len(xs)
    for (rs, rc, ra), (fs, fc, fa) in zip(ref, fused):
        assert fs == rs
        numpy.testing.assert_allclose(fc, rc, rtol=1e-6)
        assert len(fa) == len(ra)
        for a_f, a_r in zip(fa, ra):
            assert len(a_f) == len(a_r)
            for v_f, v_r in zip(a_f, a_r):
                numpy.testing.assert_array_equal(v_f, v_r)


def test_fused_decode_rejects_wide_beam():
    from nats_amd.decode.batched import gen_sample_batched
    model, xs = _setup()
    with pytest.raises(ValueError, match="K=33"):
        gen_sample_batched(model, xs[:1], k=33, maxlen=3, use_unk=True,
                           fused_select=True)


def test_service_passes_fused_select(tmp_path, monkeypatch):
    import os
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
        seen.append(kw.get("fused_select"))
        return real(*a, **kw)

    monkeypatch.setattr(app, "gen_sample_batched", spy)
    for flag in (False, True):
        svc = SummarizerService(
            saveto, os.path.join(d, "toy_train_input.txt.pkl"), device="cpu",
            k=3, maxlen=6, max_wait_ms=1.0, fused_select=flag)
        try:
            assert isinstance(svc.summarize("a b c d")["summary"], str)
        finally:
            svc.close()
    assert seen == [False, True]


# ------------------------------------------------------------ GPU cases

@pytest.fixture(scope="module")
def ext():
    m = ops._hip_ext()
    assert m is not None, "HIP extension must build/load on a GPU box"
    assert hasattr(m, "beam_select")
    return m


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_kernel_matches_eager(ext, name):
    case = CASES[name]()
    K = int(case["want"].max())
    # device-resident tables (K passed, no sync) and host tables
    got = _run(case, "cuda", K=K)
    ref = _run(case, "cuda", fn=eager.beam_select)
    _assert_same(got, ref)
    _check_expectations(case, got[0].cpu(), got[1].cpu())
    host = dict(case, seg=case["seg"].tolist(), want=case["want"].tolist())
    _assert_same(_run(host, "cuda"), ref)


@pytest.mark.gpu
def test_kernel_on_leading_rows_of_a_larger_buffer(ext):
    """The graph stepper hands over the first rows of its fixed-size
    output buffer."""
    case = CASES["odd_stride_three_tiles"]()
    R, V = case["probs"].shape
    buf = torch.full((R + 5, V), float("nan"), device="cuda")
    buf[:R] = case["probs"].cuda()
    ref = _run(case, "cuda", fn=eager.beam_select)
    case = dict(case, probs=buf[:R])
    _assert_same(_run(case, "cuda", K=10), ref)


@pytest.mark.gpu
def test_kernel_wider_k_pads(ext):
    case = CASES["uneven_segments_pen"]()
    got = _run(case, "cuda", K=32)
    ref = _run(case, "cuda", fn=eager.beam_select, K=32)
    _assert_same(got, ref)
    assert (got[0][:, 3:] == -1).all()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["plain", "rerank"])
def test_fused_decode_on_gpu_with_graph(ext, mode):
    ref, fused, _ = _decode_pair(mode, device="cuda", use_graph=True,
                                 dims=(16, 32, 12, 90))
    for (rs, rc, _), (fs, fc, _) in zip(ref, fused):
        assert sorted(map(tuple, fs)) == sorted(map(tuple, rs))
        numpy.testing.assert_allclose(sorted(fc), sorted(rc), rtol=1e-4)
