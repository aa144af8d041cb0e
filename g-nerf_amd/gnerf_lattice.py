"""The sample lattice of gen_videos.py's shape extraction (create_samples), for the harness (gen_videos_mi355x.py) and the renderer alike."""

import torch


def voxel_samples(lo, hi, n, cube_length, device):
    """Points lo..hi-1 of gen_videos.py's create_samples(N=n, voxel_origin=[0,0,0], cube_length) (gen_videos.py:33-56), made on
    the device chunk by chunk instead of as one [n^3, 3] host tensor (1.6 GB at n = 512).  The arithmetic is the reference's,
    quirks included: the y and x indices come from FLOAT divisions of the linear index without a floor (a sheared lattice), in
    fp32 (indices above 2^24 are rounded).  lo may also be a tensor of linear indices (hi is not read then): the points of those."""
    idx = lo.to(device=device, dtype=torch.int64).reshape(-1) if isinstance(lo, torch.Tensor) else torch.arange(lo, hi, dtype=torch.int64, device=device)
    origin, size = -cube_length / 2, cube_length / (n - 1)
    f = idx.float()
    s2 = (idx % n).float()
    s1 = (f / n) % n
    s0 = ((f / n) / n) % n
    return torch.stack([s0 * size + origin, s1 * size + origin, s2 * size + origin], dim=-1).unsqueeze(0)
