"""GPU: the CelebA B = 2 training step of tests/test_gpu_model.py::test_train_step_fp32_vs_reference with the fp32 stride-1 3x3
convs on split-bf16 MFMA operands: bf16x3 inside that test's fp32 tolerances, bf16x2 inside 1e-4 on the loss and north_star's 1e-2
on epsilon-hat."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from infodiffusion_amd import ops  # noqa: E402
from oracle import infodiff_oracle as O  # noqa: E402
from tests.helpers import gold, make_infodiff, rel  # noqa: E402
from tests.test_gpu_model import DEV, _replay  # noqa: E402


@pytest.mark.parametrize('mode', ['bf16x3', 'bf16x2'])
def test_train_step_f32_split_vs_reference(mode):
    cfg = O.dataset_cfg('celeba', a_dim=32, mmd_weight=0.1)
    g = gold('model_celeba')
    ops.set_f32_mfma(mode)
    try:
        model, args, sd = make_infodiff(cfg, DEV, 'fp32', 'manifest_celeba')
        model.eval()
        loss = _replay(model, cfg, g, 0)
        loss.backward()
        with torch.no_grad():
            e17 = model(g['samp_x'].to(DEV), 17, g['samp_a'].to(DEV))
    finally:
        ops.set_f32_mfma('exact')
    named = dict(model.named_parameters())
    gn = sum(float(p.grad.double().pow(2).sum()) for p in named.values() if p.grad is not None) ** 0.5
    grads = {k[2:]: rel(named[k[2:]].grad, g[k]) for k in g if k.startswith('g.')}
    print(mode, 'loss rel', rel(loss, g['loss']), 'grad-norm rel', abs(gn - float(g['grad_norm'])) / float(g['grad_norm']),
          'worst named gradient', max(grads.values()), 'eps-hat max-norm', rel(e17, g['samp_eps17']))
    assert rel(loss, g['loss']) < 1e-4, (float(loss), float(g['loss']))
    assert rel(e17, g['samp_eps17']) <= 1e-2
    if mode == 'bf16x3':
        assert abs(gn - float(g['grad_norm'])) / float(g['grad_norm']) < 1e-3
        assert all(e < 2e-3 for e in grads.values()), grads
        assert rel(e17, g['samp_eps17']) < 1e-4
