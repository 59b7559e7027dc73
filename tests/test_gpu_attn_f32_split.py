"""GPU: the fused fp32 attention on split-bf16 MFMA operands (idf_attn_f32_split_fwd / _bwd) through ops.attention under
ops.set_f32_mfma('bf16x3' | 'bf16x2'), forward and backward, against a float64 softmax-attention and its autograd on the host.
Cases are (B, C, H, W); N = H * W."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from infodiffusion_amd import ops  # noqa: E402
from tests.test_gpu_attn_f32 import _device, _host, _rel, _rnd  # noqa: E402

TOL_O, TOL_DQKV = 2e-5, 1e-4      # bf16x3: the project's fp32 bounds
U2 = 3 * 2.0 ** -18               # bf16x2: relative error of one product
# bf16x2 dqkv, max |err| / max |ref|: 4 x the worst of CASES measured on the GPU (profiles/f32_attn_split.txt section 5:
# 9.1e-6 .. 1.46e-5, the worst at (2, 64, 16, 16))
TOL_DQKV_X2 = 4 * 1.46e-5

CASES = [
    (1, 64, 8, 8), (3, 128, 8, 8), (2, 64, 16, 16),
    (3, 128, 16, 16),           # the exact kernel refuses it
    (2, 64, 4, 16),             # only N matters; the planner has no threshold: one workgroup shape at every batch size
]
LARGE = [(2, 64, 8, 8), (2, 128, 16, 16)]       # every scaled score about 100
MODES = {'bf16x3': 3, 'bf16x2': 2}
ids = lambda c: 'x'.join(map(str, c))  # noqa: E731


@functools.lru_cache(maxsize=None)
def _problem(case, large):
    """inputs, float64 reference, host fp32 result (large only) and the 'exact' mode result of one case, computed once"""
    B, C, H, W = case
    qkv, do = _rnd(3 if large else 1, B, 3 * C, H, W), _rnd(4 if large else 2, B, C, H, W)
    if large:
        qkv[:, :2 * C] += 10 / C ** 0.25
    return qkv, do, _host(qkv, do, torch.float64), _host(qkv, do, torch.float32) if large else None, _device(qkv, do)


def _x2_fwd_bound(qkv, ro):
    """first-order bound of the bf16x2 forward: the scores carry delta, so the probabilities 2 * delta relative; P V adds u"""
    B, C3, H, W = qkv.shape
    q, k, v = qkv.double().permute(0, 2, 3, 1).reshape(B, H * W, C3).split(C3 // 3, dim=2)
    delta = U2 * (C3 // 3) ** -0.5 * float((q.abs() @ k.abs().transpose(1, 2)).max())
    return (2 * delta + U2) * float(v.abs().max()) + 2e-5 * float(ro.abs().max())


def _split(mode, qkv, do, attn=True):
    ops.set_f32_mfma(mode)
    ops._F32_SPLIT_ATTN = attn
    try:
        return _device(qkv, do)
    finally:
        ops.set_f32_mfma('exact')
        ops._F32_SPLIT_ATTN = True


def _routes(mode, case, qkv, do, o, dqkv, xo, xd):
    B, C, H, W = case
    assert ops.f32_attn_split_ok(B, H * W, C, MODES[mode])
    assert not torch.equal(o, xo) and not torch.equal(dqkv, xd)
    o2, dqkv2 = _split(mode, qkv, do)
    assert torch.equal(o2, o) and torch.equal(dqkv2, dqkv)
    o3, dqkv3 = _split(mode, qkv, do, attn=False)
    assert torch.equal(o3, xo) and torch.equal(dqkv3, xd)


@pytest.mark.parametrize('case', CASES, ids=ids)
@pytest.mark.parametrize('mode', list(MODES))
def test_attention_f32_split(mode, case):
    qkv, do, (ro, rd), _, (xo, xd) = _problem(case, False)
    o, dqkv = _split(mode, qkv, do)
    eo, ed = _rel(o, ro), _rel(dqkv, rd)
    ao, bound = float((o.cpu().double() - ro).abs().max()), _x2_fwd_bound(qkv, ro)
    print(mode, case, 'o', eo, 'dqkv', ed, 'o abs', ao, 'x2 bound', bound)
    if mode == 'bf16x3':
        assert eo < TOL_O and ed < TOL_DQKV
    else:
        assert ao <= bound and ed < TOL_DQKV_X2
    _routes(mode, case, qkv, do, o, dqkv, xo, xd)


@pytest.mark.parametrize('case', LARGE, ids=ids)
@pytest.mark.parametrize('mode', list(MODES))
def test_attention_f32_split_large_logits(mode, case):
    qkv, do, (ro, rd), (ho, hd), (xo, xd) = _problem(case, True)
    o, dqkv = _split(mode, qkv, do)
    assert bool(torch.isfinite(o).all()) and bool(torch.isfinite(dqkv).all())
    eo, ed, co, cd = _rel(o, ro), _rel(dqkv, rd), _rel(ho, ro), _rel(hd, rd)
    ao, bound = float((o.cpu().double() - ro).abs().max()), _x2_fwd_bound(qkv, ro)
    print(mode, case, 'o', eo, 'host fp32', co, 'dqkv', ed, 'host fp32', cd, 'o abs', ao, 'x2 bound', bound)
    if mode == 'bf16x3':
        assert eo <= 2 * co and ed <= 2 * cd
    else:
        assert ao <= bound
    _routes(mode, case, qkv, do, o, dqkv, xo, xd)
