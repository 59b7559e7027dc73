"""GPU: the gather-mode fp32 ordered-slab weight gradient (idf_conv_wgrad_f32_gather: stride 2, up-sampling, channel counts
that are not multiples of 4) through ops.conv_wgrad_bias_raw against a float64 convolution's autograd on the host, at the
project's fp32 bound, and bit-identical from call to call."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from infodiffusion_amd import ops  # noqa: E402

CL = torch.channels_last
TOL = 2e-5      # tests/test_gpu_kernels.py TOL[torch.float32]
S1, S2, UP2 = ops.S1, ops.S2, ops.UP2

CASES = [
    # (B, Cin, Hs, Ws, Cout, mode, taps)
    (2, 64, 8, 8, 64, S2, 9),           # smallest output, Wo = 4
    (3, 36, 7, 7, 20, S2, 9),           # odd input: the right / bottom taps leave the image; ragged channels
    (2, 32, 28, 28, 64, S2, 9),         # 14-wide output: K-steps wrap rows, the last row tile masks rows
    (2, 64, 14, 14, 64, S2, 9),         # 7 x 7 output
    (2, 64, 16, 32, 64, S2, 9),         # H != W
    (5, 64, 32, 32, 128, S2, 9),        # splits that begin and end inside an image
    (2, 72, 16, 16, 136, S2, 9),        # a full plus a ragged channel tile on both sides
    (2, 64, 64, 64, 64, S2, 9),         # widest, both parity planes full
    (2, 3, 16, 16, 64, S2, 9),          # few channels and stride together
    (2, 64, 2, 2, 64, UP2, 9),          # 4 x 4 output
    (3, 36, 7, 7, 20, UP2, 9),
    (2, 128, 8, 16, 64, UP2, 9),
    (5, 64, 16, 16, 64, UP2, 9),        # splits
    (2, 64, 32, 32, 64, UP2, 9),        # 64-wide output, one row per tile
    (2, 3, 16, 16, 64, S1, 9), (2, 64, 16, 16, 3, S1, 9), (2, 6, 8, 8, 64, S1, 9),      # few channels, either side
    (3, 3, 64, 64, 64, S1, 9), (3, 64, 64, 64, 3, S1, 9),                              # ... with many slabs
    (2, 3, 8, 8, 5, S1, 1),             # 1x1, slab parts that are no multiple of 4 floats
]


def _rnd(seed, *shape):
    g = torch.Generator(device='cpu')
    g.manual_seed(seed)
    return torch.randn(*shape, generator=g)


def _rel(got, ref):
    return float((got.detach().cpu().double() - ref).abs().max() / ref.abs().max())


def _operands(case):
    B, Cin, Hs, Ws, Cout, mode, taps = case
    Ho, Wo = ((Hs + 1) // 2, (Ws + 1) // 2) if mode == S2 else (2 * Hs, 2 * Ws) if mode == UP2 else (Hs, Ws)
    return _rnd(1, B, Cin, Hs, Ws), _rnd(2, B, Cout, Ho, Wo)


@pytest.mark.parametrize('case', CASES, ids=lambda c: 'x'.join(map(str, c)))
def test_wgrad_f32_gather(case):
    B, Cin, Hs, Ws, Cout, mode, taps = case
    k = 3 if taps == 9 else 1
    a, dy = _operands(case)
    Ho, Wo = dy.shape[2:]
    w = torch.zeros(Cout, Cin, k, k, dtype=torch.float64, requires_grad=True)
    b = torch.zeros(Cout, dtype=torch.float64, requires_grad=True)
    x = F.interpolate(a.double(), scale_factor=2, mode='nearest') if mode == UP2 else a.double()
    y = F.conv2d(x, w, b, stride=2 if mode == S2 else 1, padding=k // 2)
    gw, gb = torch.autograd.grad(y, (w, b), dy.double())

    assert ops.f32_wgrad_gather_ok(B, Hs, Ws, Cin, Ho, Wo, Cout, mode, taps)
    ad, dyd = a.cuda().contiguous(memory_format=CL), dy.cuda().contiguous(memory_format=CL)
    dW, db = ops.conv_wgrad_bias_raw(ad, dyd, mode, taps, True)
    assert dW.shape == gw.shape and db.shape == gb.shape
    rw, rb = _rel(dW, gw), _rel(db, gb)
    print('dW rel', rw, 'db rel', rb)
    assert rw < TOL and rb < TOL
    dW2, db2 = ops.conv_wgrad_bias_raw(ad, dyd, mode, taps, True)
    assert torch.equal(dW2, dW) and torch.equal(db2, db)


def test_wgrad_f32_gather_without_bias():
    case = CASES[5]         # several slabs: the reduce stops in front of db
    ad, dyd = (t.cuda().contiguous(memory_format=CL) for t in _operands(case))
    dW, db = ops.conv_wgrad_bias_raw(ad, dyd, case[5], case[6], False)
    assert db is None and torch.equal(dW, ops.conv_wgrad_bias_raw(ad, dyd, case[5], case[6], True)[0])
