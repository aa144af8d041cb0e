#!/usr/bin/env python3
"""Fit a camera to an image: render a target at one look-at pose, start from a perturbed pose, and run Adam on (yaw, pitch, radius)
against the L1 distance of the raw renders (gnerf_harness.fit_camera) -- once on the fused renderer's ray gradient
(ImportanceRenderer.fused_ray_grad = True) and once on the PyTorch-op form -- printing both trajectories and the time per step.

  python fit_camera_mi355x.py --random-init --res 32 --steps 30

The generator is frozen and its planes are made once; the rays come from the ray sampler's differentiable form."""

import argparse
import time
import warnings

import torch

import gnerf_harness as H
import gen_videos_mi355x as gv
from training.volumetric_rendering.renderer import ImportanceRenderer


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--network', help='generator pickle (G_ema)')
    ap.add_argument('--random-init', action='store_true', help='seeded random generator instead of a pickle')
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--res', type=int, default=64, help='neural rendering resolution')
    ap.add_argument('--pose', type=float, nargs=3, default=(3.14 / 2, 3.14 / 2 - 0.05, 2.7), metavar=('YAW', 'PITCH', 'RADIUS'), help='the target pose')
    ap.add_argument('--offset', type=float, nargs=3, default=(0.25, -0.12, 0.15), help='start = pose + offset')
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--lr', type=float, default=0.02)
    ap.add_argument('--routes', default='fused,ops', help='comma-separated: fused, ops')
    ap.add_argument('--device', default='cuda' if torch.cuda.is_available() else 'cpu')
    args = ap.parse_args()
    if not (args.network or args.random_init):
        ap.error('give --network or --random-init')
    device = torch.device(args.device)
    G = gv.build_random_generator(args.seed, device) if args.random_init else gv.load_generator(args.network, device)
    z = torch.randn(1, G.z_dim, generator=torch.Generator().manual_seed(args.seed + 1)).to(device)
    target_c = H.camera_label(H.lookat_pose(*args.pose).to(device))
    ws = G.mapping(z, target_c)
    with torch.no_grad():
        target = G.synthesis(ws, target_c, neural_rendering_resolution=args.res, noise_mode='const')['image_raw']
    start = [p + o for p, o in zip(args.pose, args.offset)]
    for route in args.routes.split(','):
        ImportanceRenderer.fused_ray_grad = route == 'fused'
        torch.manual_seed(args.seed + 2)                         # the same renderer draws on either route
        with warnings.catch_warnings():
            warnings.simplefilter('ignore', RuntimeWarning)      # (the op form says that it is the op form)
            t0 = time.perf_counter()
            traj = H.fit_camera(G, ws, target, *start, steps=args.steps, lr=args.lr, resolution=args.res)
            if device.type == 'cuda':
                torch.cuda.synchronize(device)
            dt = time.perf_counter() - t0
        print(f'--- {route}: target yaw {args.pose[0]:.4f} pitch {args.pose[1]:.4f} radius {args.pose[2]:.4f}; {1e3 * dt / (args.steps + 1):.1f} ms per step (host wall clock)')
        for t in traj:
            print(f"step {t['step']:3d}  loss {t['loss']:.5f}  yaw {t['yaw']:.4f}  pitch {t['pitch']:.4f}  radius {t['radius']:.4f}")


if __name__ == '__main__':
    main()
