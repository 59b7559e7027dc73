"""GPU: the CelebA B = 2 training step of tests/test_gpu_model_wgrad_split.py in bf16x3 with the attention on split-bf16 operands
too (idf_attn_f32_split_fwd / _bwd): that test's fp32 gradient bounds, and the route is taken from the model."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from infodiffusion_amd import ops  # noqa: E402
from oracle import infodiff_oracle as O  # noqa: E402
from tests.helpers import gold, make_infodiff, rel  # noqa: E402
from tests.test_gpu_model import DEV, _replay  # noqa: E402


def _step(cfg, g, split_attn):
    ops.set_f32_mfma('bf16x3')
    ops._F32_SPLIT_ATTN = split_attn
    try:
        model, args, sd = make_infodiff(cfg, DEV, 'fp32', 'manifest_celeba')
        model.eval()
        _replay(model, cfg, g, 0).backward()
    finally:
        ops.set_f32_mfma('exact')
        ops._F32_SPLIT_ATTN = True
    return {k: p.grad for k, p in model.named_parameters() if p.grad is not None}


def test_train_step_attn_split_vs_reference():
    cfg = O.dataset_cfg('celeba', a_dim=32, mmd_weight=0.1)
    g = gold('model_celeba')
    on, off = _step(cfg, g, True), _step(cfg, g, False)
    gn = sum(float(v.double().pow(2).sum()) for v in on.values()) ** 0.5
    grads = {k[2:]: rel(on[k[2:]], g[k]) for k in g if k.startswith('g.')}
    print('grad-norm rel', abs(gn - float(g['grad_norm'])) / float(g['grad_norm']), 'worst named gradient', max(grads.values()))
    assert abs(gn - float(g['grad_norm'])) / float(g['grad_norm']) < 1e-3
    assert all(e < 2e-3 for e in grads.values()), grads
    qkv = [k for k in on if on[k].dim() == 4 and any(s in k for s in ('proj_q', 'proj_k', 'proj_v'))]
    changed = [k for k in qkv if not torch.equal(on[k], off[k])]
    print('changed qkv weight gradients', changed)
    assert changed, "no attention qkv conv's weight gradient changed with the split attention route"
