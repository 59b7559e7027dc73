"""GPU: the fused fp32 attention (idf_attn_f32_fwd / idf_attn_f32_bwd) through ops.attention, forward and backward, against a
float64 softmax-attention and its autograd on the host, at the project's fp32 bounds.  Cases are (B, C, H, W); N = H * W."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from infodiffusion_amd import ops  # noqa: E402

CL = torch.channels_last
TOL_O, TOL_DQKV = 2e-5, 1e-4      # tests/test_gpu_kernels.py: TOL[torch.float32], the attention gradient bound

# measured out of the predicate (profiles/f32_attn.txt): 256 tokens x 128 channels below B = 128 -- the parent's
# route keeps them (tests/test_attn_f32_host.py asserts the refusal)
GATED = [(3, 128, 16, 16), (2, 128, 16, 16)]
CASES = [
    (1, 64, 8, 8), (3, 128, 8, 8), (2, 64, 16, 16), (3, 128, 16, 16),
    (2, 64, 4, 16),             # only N matters
    # the planner's one threshold, B * N / 64 >= 512 workgroups of 64 rows: 32-row workgroups below it, 64-row ones from it on
    (127, 64, 16, 16), (128, 64, 16, 16), (128, 128, 16, 16),
    (511, 128, 8, 8), (512, 128, 8, 8), (512, 64, 8, 8),
]
# every scaled score about 100: exp overflows without the max subtraction; (128, 128, 16, 16) stands in for the gated (2, 128, 16, 16)
LARGE = [(2, 128, 16, 16), (2, 64, 8, 8), (128, 128, 16, 16)]
CASES, LARGE = [c for c in CASES if c not in GATED], [c for c in LARGE if c not in GATED]


def _rnd(seed, *shape):
    g = torch.Generator(device='cpu')
    g.manual_seed(seed)
    return torch.randn(*shape, generator=g)


def _host(qkv, do, dtype):
    """(o, dqkv) of softmax(q k^T C^-1/2) v and its autograd in `dtype` on the host."""
    B, C3, H, W = qkv.shape
    C = C3 // 3
    x = qkv.to(dtype).requires_grad_(True)
    q, k, v = x.permute(0, 2, 3, 1).reshape(B, H * W, C3).split(C, dim=2)
    p = torch.softmax(q @ k.transpose(1, 2) * (int(C) ** (-0.5)), dim=-1)
    o = (p @ v).reshape(B, H, W, C).permute(0, 3, 1, 2)
    dqkv, = torch.autograd.grad(o, x, do.to(dtype))
    return o.detach(), dqkv


def _device(qkv, do):
    x = qkv.cuda().contiguous(memory_format=CL).requires_grad_(True)
    o = ops.attention(x)
    dqkv, = torch.autograd.grad(o, x, do.cuda().contiguous(memory_format=CL))
    return o.detach(), dqkv


def _rel(a, ref):
    return float((a.cpu().double() - ref).abs().max() / ref.abs().max())


@pytest.mark.parametrize('case', CASES, ids=lambda c: 'x'.join(map(str, c)))
def test_attention_f32(case):
    B, C, H, W = case
    assert ops.f32_attn_ok(B, H * W, C)
    qkv, do = _rnd(1, B, 3 * C, H, W), _rnd(2, B, C, H, W)
    ro, rd = _host(qkv, do, torch.float64)
    o, dqkv = _device(qkv, do)
    eo, ed = _rel(o, ro), _rel(dqkv, rd)
    print(case, 'o', eo, 'dqkv', ed)
    assert eo < TOL_O and ed < TOL_DQKV
    o2, dqkv2 = _device(qkv, do)
    assert torch.equal(o2, o) and torch.equal(dqkv2, dqkv)


@pytest.mark.parametrize('case', LARGE, ids=lambda c: 'x'.join(map(str, c)))
def test_attention_f32_large_logits(case):
    B, C, H, W = case
    assert ops.f32_attn_ok(B, H * W, C)
    qkv, do = _rnd(3, B, 3 * C, H, W), _rnd(4, B, C, H, W)
    qkv[:, :2 * C] += 10 / C ** 0.25
    ro, rd = _host(qkv, do, torch.float64)
    ho, hd = _host(qkv, do, torch.float32)
    o, dqkv = _device(qkv, do)
    assert bool(torch.isfinite(o).all()) and bool(torch.isfinite(dqkv).all())
    eo, ed, co, cd = _rel(o, ro), _rel(dqkv, rd), _rel(ho, ro), _rel(hd, rd)
    print(case, 'o', eo, 'host fp32', co, 'dqkv', ed, 'host fp32', cd)
    assert eo <= 2 * co and ed <= 2 * cd
