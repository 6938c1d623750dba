"""Times ln3d_query_points_grad and ln3d_surface_normals at the workload's sizes against what a finite-difference normal costs today
(seven ln3d_query_points calls: the centre and six offsets), and writes profiles/normals_bench.md.

    python tools/normals_bench.py [--out profiles/normals_bench.md] [--iters 20]

Device events around `iters` back-to-back launches after 3 warm-up launches; synthetic 256 x 256 tri-plane (f32 texels) and decoder."""
import argparse
import os
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'normals_bench.md'))
    ap.add_argument('--iters', type=int, default=20)
    args = ap.parse_args()
    from ln3diff_amd import ops, _lib
    from ln3diff_amd.nsr.triplane import Triplane, draw_render_noise
    from ln3diff_amd.synth import orbit_cameras
    dev = 'cuda'
    g = torch.Generator().manual_seed(0)
    tp = Triplane(img_resolution=256)
    tp.decoder.net[2].bias.data[0] += 6.0
    tp = tp.to(dev)
    dec = tp._decoder_dev(torch.device(dev, 0))
    S = 256
    planes = (torch.randn(1, 3, S, S, 32, generator=g) * 2).to(dev)
    scal = torch.empty(_lib.RENDER_SCRATCH_FLOATS, device=dev)
    rows = []
    # ---- mesh vertices: ~1 M points near the surface of a 192^3 grid (here: points of the grid, in grid order, every 7th)
    ax = torch.linspace(-0.45, 0.45, 192)
    pts = torch.stack(torch.meshgrid(ax, ax, ax, indexing='ij'), -1).reshape(-1, 3)[::7].contiguous().to(dev)
    P = pts.shape[0]
    sigma, grad, rgb = torch.empty(P, device=dev), torch.empty(P, 3, device=dev), torch.empty(P, 3, device=dev)
    t_grad = timed(lambda: ops.query_points_grad(planes[0], S, S, pts, dec, 0.9, sigma, grad), args.iters)
    offs = [pts] + [(pts + 1e-3 * torch.eye(3, device=dev)[a] * s).contiguous() for a in range(3) for s in (1, -1)]
    t_fd = timed(lambda: [ops.query_points(planes[0], S, S, q, dec, 0.9, sigma, rgb, scal) for q in offs], args.iters)
    rows.append((f"query_points_grad, {P} points (every 7th of a 192^3 grid)", t_grad, f"7 x query_points: {t_fd:.3f} ms"))
    # ---- normal maps: one view at 256^2 and at 512^2, next to the render of that view
    for res in (256, 512):
        cams = orbit_cameras(1).to(dev)
        j, u = draw_render_noise(1, res * res, 64, device=dev)
        pidx = torch.zeros(1, dtype=torch.int32, device=dev)
        kw = dict(c=cams, planes_channel_last=planes, plane_index=pidx, jitter=j, u_fine=u, views_per_call=1, neural_rendering_resolution=res)
        out = tp(**kw)
        nrm = torch.empty(1, 3, res, res, device=dev)
        t_render = timed(lambda: tp(**kw), args.iters)
        t_n = timed(lambda: ops.surface_normals(planes, S, S, pidx, dec, 0.9, out['image_depth'], out['weights_samples'], nrm, cams=cams, res=res),
                    args.iters)
        cover = float((out['weights_samples'] >= 0.5).float().mean())
        rows.append((f"surface_normals, one {res}^2 view ({100 * cover:.0f} % of the rays on the surface)", t_n,
                     f"Triplane.forward of that view: {t_render:.3f} ms ({100 * t_n / t_render:.1f} % on top)"))
    try:
        smi = subprocess.run(['rocm-smi', '--showclocks', '--showpower'], capture_output=True, text=True, timeout=60).stdout
        clk = '; '.join(l.strip() for l in smi.splitlines() if ('sclk' in l or 'Power' in l) and 'GPU[0]' in l) or 'rocm-smi printed no sclk / power line'
    except Exception as e:                       # noqa: BLE001 - the bench reports, it does not depend on the tool
        clk = f'not measured (rocm-smi: {e})'
    with open(args.out, 'w') as f:
        f.write("# Surface-normal kernels: measured times\n\n")
        f.write(f"`python tools/normals_bench.py --iters {args.iters}` on {torch.cuda.get_device_name(0)}; device events around {args.iters} back-to-back "
                "launches after 3 warm-up launches; 256 x 256 f32 tri-plane, synthetic decoder.\n\n")
        f.write(f"Clock and power while idle after the run: {clk}\n\n")
        f.write("| what | ms per call | compared with |\n|---|---|---|\n")
        for what, t, other in rows:
            f.write(f"| {what} | {t:.3f} | {other} |\n")
        f.write("\nNot measured: f16 texels, the full 1 M welded vertices of a real mesh (their order is the welder's, not the grid's), "
                "kernel-level counters.\n")
    print(open(args.out).read())


if __name__ == "__main__":
    main()
