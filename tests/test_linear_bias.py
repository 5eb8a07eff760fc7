"""GPU tests of the projection glue kernels (ops/hip/io_fusion.hip):
bias_cast_, colsum_bf16, the ops.linear_bias Function built on them, and
the bf16 gradient views the scan Functions hand back for bf16 inputs."""

import pytest
import torch

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16


@pytest.fixture(scope="module")
def ext():
    from nats_amd.ops import _hip_ext
    m = _hip_ext()
    assert m is not None, "HIP extension must build/load on a GPU box"
    return m


def _randn(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (scale * torch.randn(shape, generator=g)).cuda()


# (1,8), (33,104), (5,2000), (3,30000): the 16-byte path (N % 8 == 0), the
# last two with many vectors per row; (7,1) and (37,50) the scalar path
@pytest.mark.parametrize("R,N", [(1, 8), (7, 1), (37, 50), (33, 104),
                                 (5, 2000), (3, 30000)])
def test_bias_cast_matches_fp32_add_then_round(ext, R, N):
    g = _randn((R, N), 1, 4.0).to(BF16)
    b = _randn((N,), 2, 3.0)
    ref = (g.float() + b).to(BF16)
    out = ext.bias_cast_(g.clone(), b)
    assert out.dtype == BF16 and out.shape == (R, N)
    assert torch.equal(out, ref)


def _colsum_check(ext, g):
    R = g.shape[0]
    out = ext.colsum_bf16(g)
    again = ext.colsum_bf16(g)
    assert out.dtype == torch.float32 and out.shape == (g.shape[1],)
    assert torch.equal(out, again)
    ref = g.double().sum(0)
    bound = R * 2.0 ** -24 * g.double().abs().sum(0)
    err = (out.double() - ref).abs()
    print("colsum R=%d N=%d max err/bound %.3e" % (
        R, g.shape[1], float((err / bound.clamp_min(1e-300)).max())))
    assert bool((err <= bound).all())


def _colsum_rows(ext):
    rpb = ext.colsum_rows_per_block()
    return [1, rpb - 1, rpb, rpb + 1]


@pytest.mark.parametrize("which", range(4))
def test_colsum_contiguous(ext, which):
    R = _colsum_rows(ext)[which]
    _colsum_check(ext, _randn((R, 50), 3 + which).to(BF16))


@pytest.mark.parametrize("which", range(4))
def test_colsum_slice_8_byte_aligned(ext, which):
    # the xc gradient of an H=50 scan: columns [2H, 3H) of a [R, 4H] buffer
    R = _colsum_rows(ext)[which]
    full = _randn((R, 4 * 50), 7 + which).to(BF16)
    g = full[:, 100:150]
    assert g.data_ptr() % 16 == 8 and g.stride(0) == 200
    _colsum_check(ext, g)


@pytest.mark.parametrize("N,ld,a", [(48, 192, 96), (300, 300, 0),
                                    (300, 1204, 300)])
def test_colsum_vector_path(ext, N, ld, a):
    # N % 4 == 0 takes the 8-byte loads; 300 columns span two column blocks
    R = ext.colsum_rows_per_block() + 1
    full = _randn((R, ld), 11).to(BF16)
    _colsum_check(ext, full[:, a:a + N])


@pytest.mark.parametrize("chunks", [4, 5, 6, 7])
def test_colsum_final_sum_chains(ext, chunks):
    # the final sum walks the row-chunk partials four at a time: a whole
    # group of four, and one, two and three chunks left over
    R = (chunks - 1) * ext.colsum_rows_per_block() + 3
    _colsum_check(ext, _randn((R, 52), 13 + chunks).to(BF16))


@pytest.mark.parametrize("xshape,N", [((37, 20), 50), ((37, 20), 104),
                                      ((5, 3, 20), 50), ((5, 3, 24), 104)])
@pytest.mark.parametrize("x_grad", [True, False])
def test_linear_bias_function(ext, xshape, N, x_grad):
    from nats_amd import ops
    K = xshape[-1]
    x0 = _randn(xshape, 21)
    W0 = _randn((K, N), 22, 0.3)
    b0 = _randn((N,), 23)
    gy = _randn(xshape[:-1] + (N,), 24).to(BF16)

    def run(fn):
        x = x0.clone().requires_grad_(x_grad)
        W = W0.clone().requires_grad_(True)
        b = b0.clone().requires_grad_(True)
        with torch.autocast("cuda", dtype=BF16):
            y = fn(x, W, b)
        y.backward(gy)
        return y.detach(), x.grad, W.grad, b.grad

    y, dx, dW, db = run(ops.linear_bias)
    yr, dxr, dWr, dbr = run(lambda x, W, b: (x @ W + b).to(BF16))
    assert y.dtype == BF16 and y.shape == yr.shape
    assert torch.equal(y, yr)
    assert dW.dtype == torch.float32 and torch.equal(dW, dWr)
    if x_grad:
        assert dx.dtype == torch.float32 and torch.equal(dx, dxr)
    else:
        assert dx is None
    g2 = gy.reshape(-1, N).double()
    bound = g2.shape[0] * 2.0 ** -24 * g2.abs().sum(0)
    assert db.dtype == torch.float32
    assert bool(((db.double() - g2.sum(0)).abs() <= bound).all())


def test_linear_bias_outside_autocast_is_the_plain_expression(ext):
    from nats_amd import ops
    x, W, b = _randn((6, 20), 31), _randn((20, 12), 32), _randn((12,), 33)
    assert torch.equal(ops.linear_bias(x, W, b), x @ W + b)


def test_bidir_scan_bf16_inputs_get_bf16_grads(ext):
    """bf16 projections in, bf16 gradient views out: no fp32 copy of dpre,
    and the same values the fp32-input call returns."""
    from kernel_ref import _gru_inputs
    from nats_amd.ops.gru import gru_scan_bidir_hip
    T, B, H = 7, 5, 50
    xg, xc, U, Ux, mask = _gru_inputs(T=T, B=B, H=H, seed=4)
    xg1, xc1, U1, Ux1, _ = _gru_inputs(T=T, B=B, H=H, seed=5)
    maskr = mask.flip(0)
    w = _randn((2, T, B, H), 41)

    def run(dtype):
        ins = [t.to(BF16).to(dtype).cuda().requires_grad_(True)
               for t in (xg, xc, xg1, xc1)]
        Ws = [t.cuda().requires_grad_(True) for t in (U, Ux, U1, Ux1)]
        h0, h1 = gru_scan_bidir_hip(
            ins[0], ins[1], mask.cuda(), Ws[0], Ws[1],
            ins[2], ins[3], maskr.cuda(), Ws[2], Ws[3])
        ((h0 * w[0]).sum() + (h1 * w[1]).sum()).backward()
        return [t.grad for t in ins]

    g_bf = run(BF16)
    g_f = run(torch.float32)
    for a, b in zip(g_bf, g_f):
        assert a.dtype == BF16 and b.dtype == torch.float32
        assert torch.equal(a.float(), b)
