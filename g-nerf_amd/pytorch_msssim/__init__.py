"""Overlay stand-in for the pytorch_msssim package: `from pytorch_msssim import ssim, ms_ssim, SSIM, MS_SSIM` (training_loop.py:30)
resolves here when g-nerf_amd is in front of the path, and gets this project's implementation (torch_utils/ops/ssim.py: the gfx950 kernel
for GPU tensors, PyTorch ops for CPU tensors).  Like the other overlay packages it shadows an installed copy by design."""

from torch_utils.ops.ssim import MS_SSIM, SSIM, ms_ssim, ssim

__all__ = ['ssim', 'ms_ssim', 'SSIM', 'MS_SSIM']
