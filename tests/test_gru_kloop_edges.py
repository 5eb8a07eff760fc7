"""GRU scan kernels vs the fp64 eager oracle at the hidden sizes where the
MFMA K-loops (NATS_MFMA_KLOOP in common.h, NATS_MFMA_KLOOP_LDSB in
gru_scan.hip) change body: the plain one-fragment loop below a K range of
128, the 4-deep pipelined loop (prologue, steady rotation, drain) from 128
on. Forward scans reduce over Hpad = ceil32(H); backward scans over thirds
of K3pad = ceil32(3H).

The GPU tests carry the ``gpu`` mark one by one; the unmarked
``*_precondition`` tests and the shape table run on the CPU. They show that
the bounds of the GPU tests are outside reference noise and that an oracle
which loses any single 32-wide K slice, in the forward or in the backward
GEMM, falls outside them: a kernel that skips, repeats or misplaces one
fragment of a K-loop does at least that. The one exception found, a
backward-only loss inside the reset-gate columns at H >= 1000, is described
in test_gru_kloop_backward_slice_precondition.

Each reference is computed once per process (lru_cache) and shared.
"""

import functools

import pytest
import torch

from kernel_ref import (GRU_BIDIR_GRAD_NAMES, GRU_GRAD_NAMES,
                        _gru_kloop_inputs, assert_grad_close, grad_err_ratio,
                        run_gru_scan, run_gru_scan_bidir)

gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def ext():
    from nats_amd.ops import _hip_ext
    m = _hip_ext()
    assert m is not None, "HIP extension must build/load on a GPU box"
    return m


# id -> (T, B, H)
SHAPES = {
    "h8": (4, 3, 8),
    "h104": (5, 19, 104),
    "h136": (4, 7, 136),
    "h200": (4, 5, 200),
    "h104_b33": (4, 33, 104),
    "h1000_b20": (3, 20, 1000),
    "h1000_b64": (3, 64, 1000),
    "h1040_b40": (3, 40, 1040),
}
# id -> (Hpad, K3pad, K range of the three backward waves, column tiles)
TILING = {
    # one column tile: a one-block barrier; plain body, two empty thirds (in
    # the persistent backward the third wave has kbeg 64 > kend 32)
    "h8": (32, 32, (32, 0, 0), 1),
    # forward: prologue + drain, no steady trip; backward: pipelined and
    # plain body in one block; 8 valid columns in the last tile, 3 valid
    # rows in the second 16-row tile
    "h104": (128, 320, (128, 128, 64), 7),
    # one steady trip forward and in two backward thirds, plain third
    "h136": (160, 416, (160, 160, 96), 9),
    # three steady trips; all thirds pipelined, of unequal length
    "h200": (224, 608, (224, 224, 160), 13),
    # four persistent jobs, one row each in jobs 2 and 3
    "h104_b33": (128, 320, (128, 128, 64), 7),
    # the benchmark's shape: two jobs of 63 tiles, 4 preferred XCDs per job
    "h1000_b20": (1024, 3008, (1024, 1024, 960), 63),
    # four jobs x 63 tiles = 252 of the 256 blocks, 2 XCDs per job
    "h1000_b64": (1024, 3008, (1024, 1024, 960), 63),
    # too wide for four jobs: 32 + 8 row chunks, each a two-job persistent
    # launch of 65 tiles
    "h1040_b40": (1056, 3136, (1056, 1056, 1024), 65),
}
# id -> (persistent jobs, preferred XCDs per job) of gru_scan_bidir_hip
PERSIST_PLAN = {
    "h8": (2, 2), "h104": (2, 2), "h136": (2, 2), "h200": (2, 2),
    "h104_b33": (4, 2), "h1000_b20": (2, 4), "h1000_b64": (4, 2),
}
EDGE_IDS = ["h8", "h104", "h136", "h200"]
PERSIST_IDS = list(PERSIST_PLAN)
WIDE_ID = "h1040_b40"

# (shape id, scan): "uni" is gru_scan_hip from h0 with a mask, "bidir" both
# directions from a zero state with masks, "bidir_nomask" the same without
SCANS = ([(s, "uni") for s in EDGE_IDS] +
         [(s, "bidir") for s in PERSIST_IDS + [WIDE_ID]] +
         [("h136", "bidir_nomask")])
SCAN_IDS = ["%s-%s" % c for c in SCANS]

GRU_GRAD_REL = 0.06         # the bound of test_gru_scan_backward
BIDIR_GRAD_REL = 0.08       # the bound of test_gru_scan_bidir
H_RTOL, H_ATOL = 0.1, 6e-2  # the bound of test_gru_scan_forward
# Seed of direction 0; direction 1 takes SEED + 1 and the time-flipped mask.
# Seed 7 meets every precondition below, the backward K slices included
# (first measured with it, on the CPU; never chosen by running a kernel).
# What no seed gives at H >= 1000 is said in
# test_gru_kloop_backward_slice_precondition.
SEED = 7


def _ceil(x, m):
    return -(-x // m) * m


def _thirds(K3pad):
    """K ranges of the three waves that share a backward reduction: k_part
    in gru_kernels.h, and the unclamped form in nats_gru_persistent_bwd."""
    chunk = _ceil(K3pad // 3, 32)
    return tuple(max(0, min(K3pad, (i + 1) * chunk) - i * chunk)
                 for i in range(3))


def _kloop_trips(K):
    """(pipelined body taken, trips of its steady loop) for a K range."""
    return K >= 128, max(0, (K - 128) // 32)


@functools.lru_cache(maxsize=None)
def _inputs(shape_id, d):
    T, B, H = SHAPES[shape_id]
    if d == 0:
        return _gru_kloop_inputs(T, B, H, SEED)
    (xg, xc, U, Ux, _), h0 = _gru_kloop_inputs(T, B, H, SEED + 1)
    return (xg, xc, U, Ux, _inputs(shape_id, 0)[0][4].flip(0)), h0


def _bidir_inputs(shape_id, masked=True):
    ins = [_inputs(shape_id, d)[0] for d in (0, 1)]
    if not masked:
        ins = [i[:4] + (None,) for i in ins]
    return ins


def _eager_bidir(*a):
    from nats_amd.ops import eager
    return eager.gru_scan(*a[:5]), eager.gru_scan(*a[5:])


def _run_oracle(scan, ins, fn=None, **kw):
    """One CPU run of a SCANS entry on ``ins`` (uni: ((xg, xc, U, Ux, mask),
    h0); bidir: the two input tuples). Returns (list of h, grads)."""
    from nats_amd.ops import eager
    if scan == "uni":
        h, g = run_gru_scan(fn or eager.gru_scan, ins[0], ins[1], **kw)
        return [h], g
    hs, g = run_gru_scan_bidir(fn or _eager_bidir, ins[0], ins[1], **kw)
    return list(hs), g


def _scan_inputs(shape_id, scan):
    if scan == "uni":
        return _inputs(shape_id, 0)
    return _bidir_inputs(shape_id, masked=scan == "bidir")


@functools.lru_cache(maxsize=None)
def _ref(shape_id, scan):
    """fp64 oracle and the bf16-operand fp32 run of the eager scan."""
    ins = _scan_inputs(shape_id, scan)
    return (_run_oracle(scan, ins, dtype=torch.float64),
            _run_oracle(scan, ins, dtype=torch.float32, bf16_operands=True))


def _rel(scan):
    return GRU_GRAD_REL if scan == "uni" else BIDIR_GRAD_REL


def _input_grad_names(scan):
    """The gradients a lost K slice of the recurrent GEMMs reaches without
    passing through a weight gradient's own sum over (T, B)."""
    return ("xg", "xc", "h0") if scan == "uni" else ("xg0", "xc0", "xg1",
                                                     "xc1")


# --------------------------------------------------------------------------
# host side: every shape selects the bodies its TILING line claims
# --------------------------------------------------------------------------

@pytest.mark.parametrize("shape_id", list(SHAPES))
def test_gru_shape_selects_its_kloop_bodies(shape_id):
    """Hpad, K3pad, the backward thirds and the column tiles of TILING are
    what the tiling rules give, tied to the project's own packers; and the
    K-loop bodies and trip counts that make each shape worth running."""
    from nats_amd.ops.gru import pack_bwd_weights, pack_fwd_weights
    T, B, H = SHAPES[shape_id]
    Hpad, K3pad, thirds, ngrp = TILING[shape_id]
    assert T <= 5
    assert (Hpad, K3pad, ngrp) == (_ceil(H, 32), _ceil(3 * H, 32),
                                   -(-H // 16))
    assert thirds == _thirds(K3pad) and sum(thirds) == K3pad
    (_, _, U, Ux, mask), _ = _inputs(shape_id, 0)
    assert pack_fwd_weights(U, Ux).shape == (ngrp * 3 * 16, Hpad)
    assert pack_bwd_weights(U, Ux).shape == (ngrp * 16, K3pad)
    lens = mask.sum(0)
    assert mask.shape == (T, B) and 2 <= int(lens.min())
    # some row is masked at t = 0 of the reverse direction
    assert int(lens.min()) < T

    fwd = _kloop_trips(Hpad)
    bwd = [_kloop_trips(k) for k in thirds]
    if shape_id == "h8":
        assert ngrp == 1 and thirds == (32, 0, 0)
        assert not fwd[0] and not any(p for p, _ in bwd)
        # persistent backward, third wave: kbeg past kend
        assert 2 * _ceil(K3pad // 3, 32) > K3pad
    if shape_id in ("h104", "h104_b33"):
        assert fwd == (True, 0)
        assert bwd == [(True, 0), (True, 0), (False, 0)]
        assert H - (ngrp - 1) * 16 == 8
    if shape_id == "h104":
        assert B - 16 == 3
    if shape_id == "h136":
        assert fwd == (True, 1)
        assert bwd == [(True, 1), (True, 1), (False, 0)]
    if shape_id == "h200":
        assert fwd == (True, 3)
        assert bwd == [(True, 3), (True, 3), (True, 1)]
    if H >= 1000:
        assert fwd[0] and all(p for p, _ in bwd)
        assert len(set(thirds)) == 2
    if shape_id in PERSIST_PLAN:
        njobs, xpd = PERSIST_PLAN[shape_id]
        assert njobs == 2 * -(-B // 32) and njobs * ngrp <= 256
        assert xpd == (2 if njobs == 4 or ngrp <= 48 else 4)
    if shape_id == "h104_b33":
        assert B - 32 == 1
    if shape_id == "h1000_b64":
        assert PERSIST_PLAN[shape_id][0] * ngrp == 252
    if shape_id == WIDE_ID:
        assert 4 * ngrp > 256 >= 2 * ngrp and (B - 32) == 8


# --------------------------------------------------------------------------
# CPU preconditions
# --------------------------------------------------------------------------

@pytest.mark.parametrize("shape_id,scan", SCANS, ids=SCAN_IDS)
def test_gru_kloop_noise_precondition(shape_id, scan):
    """The bf16-operand eager run stays within HALF the gradient bound of
    the fp64 oracle (floor halved too) and within 0.03 of it in h.
    Measured worst grad err/full bound, max |dh|:
    uni: h8 0.11, 0.0013; h104 0.13, 0.0050; h136 0.27, 0.0045; h200 0.17,
    0.0043. bidir: h8 0.21, 0.0014; h104 0.19, 0.0054; h136 0.14, 0.0067
    (no mask 0.18, 0.0067); h200 0.22, 0.0031; h104_b33 0.17, 0.0042;
    h1000_b20 0.26, 0.0046; h1000_b64 0.17, 0.0057; h1040_b40 0.14, 0.0052.
    """
    (ref_h, ref_g), (emu_h, emu_g) = _ref(shape_id, scan)
    rel = _rel(scan)
    worst = max(grad_err_ratio(ref_g[n], emu_g[n].double(), rel=rel)
                for n in ref_g)
    dh = max(float((r - e.double()).abs().max())
             for r, e in zip(ref_h, emu_h))
    print("%s %s: bf16-operand run, worst grad err/bound %.3f, max |dh| "
          "%.4f" % (shape_id, scan, worst, dh))
    assert set(ref_g) == set(GRU_GRAD_NAMES if scan == "uni"
                             else GRU_BIDIR_GRAD_NAMES)
    assert dh <= 0.03
    for n in ref_g:
        assert float(ref_g[n].abs().max()) > 0
        assert_grad_close(ref_g[n], emu_g[n].double(), n, rel=rel / 2,
                          floor_frac=5e-4)


def _h_fails(ref_h, hs):
    """Per direction: does ``hs`` fail the h comparison of the GPU tests?"""
    out = []
    for r, h in zip(ref_h, hs):
        out.append(bool(((h - r).abs() > H_ATOL + H_RTOL * r.abs()).any()))
    return out


def _dir_ratios(scan, ref_g, g):
    """Per direction: worst err/bound over the input gradients."""
    names = _input_grad_names(scan)
    groups = [names] if scan == "uni" else [names[:2], names[2:]]
    return [max(grad_err_ratio(ref_g[n], g[n], rel=_rel(scan)) for n in grp)
            for grp in groups]


def _fwd_slices(H):
    """First rows of the 32-row slices of U/Ux to ablate: all of them, or at
    the production sizes the first four (the pipelined prologue), one from
    the middle and the last."""
    k0s = list(range(0, H, 32))
    if len(k0s) > 8:
        k0s = k0s[:4] + [k0s[len(k0s) // 2], k0s[-1]]
    return k0s


def _bwd_slices(H):
    """First columns of the 32-column slices of [U|Ux] to ablate: all of
    them, or at the production sizes the first four, the last of the first
    third (its drain), the first of the other two thirds, one from the
    middle and the last."""
    c0s = list(range(0, 3 * H, 32))
    if len(c0s) > 24:
        chunk = _thirds(_ceil(3 * H, 32))[0]
        c0s = c0s[:4] + [chunk - 32, chunk, c0s[len(c0s) // 2], 2 * chunk,
                         c0s[-1]]
    return c0s


def _zero_rows(inp, k0):
    xg, xc, U, Ux, mask = inp
    U, Ux = U.clone(), Ux.clone()
    U[k0:k0 + 32] = 0
    Ux[k0:k0 + 32] = 0
    return xg, xc, U, Ux, mask


def _zero_cols(U, Ux, c0):
    cat = torch.cat([U, Ux], 1).clone()
    cat[:, c0:c0 + 32] = 0
    H = Ux.shape[0]
    return cat[:, :2 * H], cat[:, 2 * H:]


def _ablate(ins, scan, f):
    """``f`` applied to the input tuple of every direction."""
    if scan == "uni":
        return f(ins[0]), ins[1]
    return [f(i) for i in ins]


@pytest.mark.parametrize("shape_id,scan", SCANS, ids=SCAN_IDS)
def test_gru_kloop_forward_slice_precondition(shape_id, scan):
    """An fp64 oracle run with any 32-row slice of U and Ux zeroed (the K
    index of the forward GEMM h @ [U|Ux]) fails the h comparison of the GPU
    tests and exceeds their gradient bound on an input gradient, in each
    direction. Measured least max |dh| and least grad err/bound over the
    slices and directions:
    uni: h8 0.59, 19.7; h104 0.81, 20.7; h136 0.58, 24.9; h200 0.43, 22.3.
    bidir (zero initial state, so one step fewer sees the slice): h8 0.45,
    11.7; h104 0.49, 14.3; h136 0.33, 18.5 (no mask 0.43, 15.6); h200 0.21,
    18.7; h104_b33 0.40, 13.4; h1000_b20 0.14, 10.2; h1000_b64 0.21, 8.6;
    h1040_b40 0.23, 10.0. The h bound at the smallest of these, 0.14, is
    6e-2 + 0.1 |h| <= 0.16 per element and is exceeded where |h| is small."""
    H = SHAPES[shape_id][2]
    ins = _scan_inputs(shape_id, scan)
    ref_h, ref_g = _ref(shape_id, scan)[0]
    low_h, low_g = 1e9, 1e9
    for k0 in _fwd_slices(H):
        abl = _ablate(ins, scan, lambda i: _zero_rows(i, k0))
        hs, g = _run_oracle(scan, abl, dtype=torch.float64)
        dh = [float((h - r).abs().max()) for h, r in zip(hs, ref_h)]
        ratios = _dir_ratios(scan, ref_g, g)
        low_h, low_g = min([low_h] + dh), min([low_g] + ratios)
        assert all(_h_fails(ref_h, hs)), (k0, dh)
        assert min(ratios) > 1, (k0, ratios)
    print("%s %s: forward K slice zeroed, least max |dh| %.3f, least grad "
          "err/bound %.1f" % (shape_id, scan, low_h, low_g))


class _MatmulOtherBwd(torch.autograd.Function):
    """h @ W whose backward takes dh from Wb in place of W: the backward
    GEMM dstep @ [U|Ux]^T on its own, the forward left alone."""

    @staticmethod
    def forward(ctx, h, W, Wb):
        ctx.save_for_backward(h, Wb)
        return h @ W

    @staticmethod
    def backward(ctx, g):
        h, Wb = ctx.saved_tensors
        return g @ Wb.t(), h.t() @ g, None


def _scan_other_bwd(c0):
    """eager.gru_scan with the backward of both recurrent products reading
    [U|Ux] with columns [c0, c0 + 32) zeroed; c0 = None zeroes nothing."""
    def scan(xg, xc, mask, U, Ux, h0=None):
        Ub, Uxb = U.detach(), Ux.detach()
        if c0 is not None:
            Ub, Uxb = _zero_cols(Ub, Uxb, c0)
        H = Ux.shape[1]
        h = h0 if h0 is not None else xg.new_zeros(xg.shape[1], H)
        out = []
        for t in range(xg.shape[0]):
            pre = torch.sigmoid(_MatmulOtherBwd.apply(h, U, Ub) + xg[t])
            r, u = pre[:, :H], pre[:, H:]
            hbar = torch.tanh(_MatmulOtherBwd.apply(h, Ux, Uxb) * r + xc[t])
            h_new = u * h + (1.0 - u) * hbar
            if mask is not None:
                m = mask[t].unsqueeze(1)
                h_new = m * h_new + (1.0 - m) * h
            h = h_new
            out.append(h)
        return torch.stack(out, dim=0)
    return scan


def _other_bwd_fn(scan, c0):
    f = _scan_other_bwd(c0)
    if scan == "uni":
        return f
    return lambda *a: (f(*a[:5]), f(*a[5:]))


@pytest.mark.parametrize("shape_id,scan", SCANS, ids=SCAN_IDS)
def test_gru_kloop_backward_slice_precondition(shape_id, scan):
    """Two ablations of every 32-column slice of cat([U, Ux], 1), the K
    index of the backward GEMM dstep @ [U|Ux]^T; each must exceed the
    gradient bound of the GPU tests on an input gradient in each direction.
      * "cols": the fp64 oracle run with the slice zeroed, forward included;
      * "bwd only": the oracle's forward untouched and only the backward
        products reading the zeroed slice, which is what a backward kernel
        that drops one K fragment computes. _scan_other_bwd(None) is
        checked to reproduce the oracle first.
    "cols" holds for every slice of every shape with seed 7, so the seed the
    forward figures were taken with stays. "bwd only" holds for every slice
    at H <= 200, where every body and trip count of the K-loops is selected,
    and at H >= 1000 for every tested slice that reaches the update-gate or
    candidate columns (>= 1.7x the bound). The slices wholly inside the
    reset-gate columns [0, H) at H >= 1000 are printed, not asserted: dpr
    carries the factor r(1 - r) <= 1/4, one such slice is ~1 % of the K
    range, and over T = 3 its loss lands at 0.8 to 3.0 times the bound
    (seeds 8 and 21 alike: 0.7 to 2.2). A backward kernel that drops one
    reset-gate fragment at the production sizes only is therefore not
    certain to be caught by the GPU tests below; one that drops it at
    H <= 200 is.
    Measured least grad err/bound, cols / bwd only:
    uni: h8 19.7 / 20.9; h104 15.3 / 5.7; h136 16.2 / 6.7; h200 13.8 / 4.8.
    bidir: h8 11.7 / 12.6; h104 10.5 / 2.8; h136 11.4 / 2.2 (no mask 7.8 /
    3.1); h200 7.4 / 1.9; h104_b33 8.3 / 1.7; h1000_b20 6.3 / 1.9 (reset
    gate 0.81 to 1.87); h1000_b64 5.5 / 1.8 (0.86 to 2.99); h1040_b40 7.2 /
    1.8 (0.80 to 1.94)."""
    H = SHAPES[shape_id][2]
    ins = _scan_inputs(shape_id, scan)
    ref_h, ref_g = _ref(shape_id, scan)[0]
    same_h, same_g = _run_oracle(scan, ins, fn=_other_bwd_fn(scan, None),
                                 dtype=torch.float64)
    for h, r in zip(same_h, ref_h):
        assert torch.equal(h, r)
    for n in ref_g:
        torch.testing.assert_close(same_g[n], ref_g[n], rtol=1e-12,
                                   atol=1e-12)
    low_c, low_b, reset_gate = 1e9, 1e9, []
    for c0 in _bwd_slices(H):
        abl = _ablate(ins, scan, lambda i: i[:2] + _zero_cols(
            i[2], i[3], c0) + i[4:])
        _, g = _run_oracle(scan, abl, dtype=torch.float64)
        cols = _dir_ratios(scan, ref_g, g)
        hs, g = _run_oracle(scan, ins, fn=_other_bwd_fn(scan, c0),
                            dtype=torch.float64)
        only = _dir_ratios(scan, ref_g, g)
        low_c = min([low_c] + cols)
        assert all(torch.equal(h, r) for h, r in zip(hs, ref_h))
        assert min(cols) > 1, (c0, cols)
        if H >= 1000 and c0 + 32 <= H:
            reset_gate += only
            continue
        low_b = min([low_b] + only)
        assert min(only) > 1, (c0, only)
    print("%s %s: backward K slice zeroed, least grad err/bound: cols %.2f, "
          "bwd only %.2f%s" % (
              shape_id, scan, low_c, low_b,
              reset_gate and " (reset-gate slices, not asserted: %.2f to "
              "%.2f)" % (min(reset_gate), max(reset_gate)) or ""))


# --------------------------------------------------------------------------
# GPU tests
# --------------------------------------------------------------------------

def _check(label, scan, hs, g, ref):
    """isfinite first (the persistent kernels report a barrier give-up as
    NaN), then h, then every gradient at the project's bound."""
    ref_h, ref_g = ref
    rel = _rel(scan)
    assert set(g) == set(ref_g)
    assert all(bool(torch.isfinite(t).all()) for t in hs)
    assert all(bool(torch.isfinite(t).all()) for t in g.values())
    ratios = {n: grad_err_ratio(ref_g[n], g[n].double(), rel=rel)
              for n in ref_g}
    print("%s: max |dh| %.4f, grad err/bound %s" % (
        label,
        max(float((h.double() - r).abs().max()) for h, r in zip(hs, ref_h)),
        ", ".join("%s %.3f" % kv for kv in ratios.items())))
    for h, r in zip(hs, ref_h):
        assert h.shape == r.shape
        torch.testing.assert_close(h.double(), r, rtol=H_RTOL, atol=H_ATOL)
    for n in ref_g:
        assert_grad_close(ref_g[n], g[n].double(), n, rel=rel)


@gpu
@pytest.mark.parametrize("shape_id", EDGE_IDS)
def test_gru_scan_kloop_edges(ext, shape_id):
    """gru_scan_hip from h0 with a mask: nats_gru_step_fwd over Hpad,
    nats_gru_step_bwd_pointwise + nats_gru_step_bwd_gemm over the thirds of
    K3pad (NATS_MFMA_KLOOP; TILING says which body and how many trips).
    Worst grad err/bound measured on MI355X: h8 0.27 (xg), h104 0.20 (xg),
    h136 0.45 (xg), h200 0.33 (h0); max |dh| 0.0076."""
    from nats_amd.ops.gru import gru_scan_hip
    inputs, h0 = _inputs(shape_id, 0)
    h, g = run_gru_scan(gru_scan_hip, inputs, h0, dev="cuda")
    _check("uni %s" % shape_id, "uni", [h], g, _ref(shape_id, "uni")[0])


def _run_bidir_hip(shape_id, masked=True):
    from nats_amd.ops.gru import gru_scan_bidir_hip
    i0, i1 = _bidir_inputs(shape_id, masked)
    hs, g = run_gru_scan_bidir(gru_scan_bidir_hip, i0, i1, dev="cuda")
    return list(hs), g


@gpu
@pytest.mark.parametrize("shape_id", PERSIST_IDS)
def test_gru_scan_bidir_persistent_kloop_edges(ext, shape_id):
    """nats_gru_persistent_fwd / nats_gru_persistent_bwd
    (NATS_MFMA_KLOOP_LDSB, weights read from swizzled LDS) and the dh0
    launch of nats_gru_step_bwd_gemm, with the job and claim geometry of
    PERSIST_PLAN. Worst grad err/bound measured on MI355X: h8 0.17 (U1),
    h104 0.23, h136 0.24, h200 0.31, h104_b33 0.20, h1000_b20 0.28,
    h1000_b64 0.18 (all xg0 or xg1); max |dh| 0.0069."""
    T, B, H = SHAPES[shape_id]
    assert ext.gru_persistent_ok(H, B)
    hs, g = _run_bidir_hip(shape_id)
    _check("persistent %s" % shape_id, "bidir", hs, g,
           _ref(shape_id, "bidir")[0])


@gpu
def test_gru_scan_bidir_persistent_no_mask(ext):
    """mask0 = mask1 = None through the persistent kernels, at h136.
    Worst grad err/bound measured on MI355X: 0.26 (xg0)."""
    T, B, H = SHAPES["h136"]
    assert ext.gru_persistent_ok(H, B)
    hs, g = _run_bidir_hip("h136", masked=False)
    _check("persistent h136 no mask", "bidir_nomask", hs, g,
           _ref("h136", "bidir_nomask")[0])


@gpu
@pytest.mark.parametrize("shape_id", EDGE_IDS)
def test_gru_scan_bidir_per_step_kloop_edges(ext, shape_id, monkeypatch):
    """The per-step fallback: nats_gru_step_fwd_bidir and
    nats_gru_step_bwd_fused_bidir (NATS_MFMA_KLOOP), otherwise only reached
    for H > 1504. Worst grad err/bound measured on MI355X: h8 0.17, h104
    0.23, h136 0.24, h200 0.31, digit for digit those of the persistent
    kernels, which add the same products in the same order."""
    T, B, H = SHAPES[shape_id]
    # the extension reads the variable on every call
    monkeypatch.setenv("NATS_NO_PERSISTENT", "1")
    assert not ext.gru_persistent_ok(H, B)
    hs, g = _run_bidir_hip(shape_id)
    _check("per-step %s" % shape_id, "bidir", hs, g,
           _ref(shape_id, "bidir")[0])


@gpu
def test_gru_scan_bidir_wide_hidden_large_batch_grads(ext):
    """(3, 40, 1040) through ops.gru_scan_bidir with autograd: four jobs of
    65 tiles exceed the grid, so the dispatcher cuts the batch into 32 + 8
    rows and concatenates; each chunk is a two-job persistent launch
    (Hpad 1056, thirds 1056 / 1056 / 1024, all pipelined), and the weight
    gradients are the sums over both chunks. Worst grad err/bound measured
    on MI355X: 0.27 (xg0, xg1); max |dh| 0.0057."""
    from nats_amd import ops
    T, B, H = SHAPES[WIDE_ID]
    assert not ext.gru_persistent_ok(H, B)
    assert ext.gru_persistent_ok(H, 32) and ext.gru_persistent_ok(H, B - 32)
    i0, i1 = _bidir_inputs(WIDE_ID)
    hs, g = run_gru_scan_bidir(ops.gru_scan_bidir, i0, i1, dev="cuda")
    _check("chunked %s" % WIDE_ID, "bidir", list(hs), g,
           _ref(WIDE_ID, "bidir")[0])
