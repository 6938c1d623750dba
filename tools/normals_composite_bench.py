"""Times the volume-composited normal maps (mode 1 of ln3d_surface_normals) per 256^2 and 512^2 view: the composited launch, the second
(generic-kernel) render that feeds it, the whole overhead inside Triplane.forward, and the honest alternative on the same operands -
ln3d_query_points_grad over all M * T coordinates plus the element-wise composite in torch.  Writes profiles/normals_composited.md.

    python tools/normals_composite_bench.py [--out profiles/normals_composited.md] [--iters 5] [--rounds 5]

One process; the variants take turns in `rounds` alternating windows of `iters` back-to-back calls between device events (after one
warm-up call each), and the median window is reported with the spread, so a clock drift hits every variant alike.  Clock and power are
read (rocm-smi, read-only) while a queue of the measured launches is still running on the device, once per resolution.  Synthetic
256 x 256 f32 tri-plane and decoder, 64 + 64 samples per ray."""
import argparse
import os
import statistics
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def window(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def alternate(variants, iters, rounds):
    """{name: fn} -> {name: (median ms, min ms, max ms)} over `rounds` windows taken in turn"""
    for fn in variants.values():
        fn()
    torch.cuda.synchronize()
    t = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            t[k].append(window(fn, iters))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in t.items()}


def clocks():
    try:
        smi = subprocess.run(['rocm-smi', '--showclocks', '--showpower'], capture_output=True, text=True, timeout=60).stdout
        return '; '.join(l.strip() for l in smi.splitlines() if ('sclk' in l or 'Power' in l) and 'GPU[0]' in l) or 'rocm-smi printed no sclk / power line'
    except Exception as e:                       # noqa: BLE001 - the bench reports, it does not depend on the tool
        return f'not measured (rocm-smi: {e})'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'normals_composited.md'))
    ap.add_argument('--iters', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=5)
    args = ap.parse_args()
    from ln3diff_amd import ops, _lib
    from ln3diff_amd.nsr.triplane import Triplane, draw_render_noise, render_call_kwargs, unit_outward
    from ln3diff_amd.synth import orbit_cameras
    dev = 'cuda'
    g = torch.Generator().manual_seed(0)
    tp = Triplane(img_resolution=256)
    tp.decoder.net[2].bias.data[0] += 6.0
    tp = tp.to(dev)
    dec = tp._decoder_dev(torch.device(dev, 0))
    S, T = 256, 128
    planes = (torch.randn(1, 3, S, S, 32, generator=g) * 2).to(dev)
    rk = tp.rendering_kwargs
    lines, loads = [], []
    for res in (256, 512):
        M = res * res
        cams = orbit_cameras(1).to(dev)
        j, u = draw_render_noise(1, M, 64, device=dev)
        pidx = torch.zeros(1, dtype=torch.int32, device=dev)
        kw = dict(c=cams, planes_channel_last=planes, plane_index=pidx, jitter=j, u_fine=u, views_per_call=1, neural_rendering_resolution=res)
        out = tp(**kw)
        wsum = out['weights_samples']
        wts, crd = torch.empty(1, M, T - 1, device=dev), torch.empty(1, M, T, 3, device=dev)
        rgb, dep, ws, lim = torch.empty(1, 3, M, device=dev), torch.empty(1, M, device=dev), torch.empty(1, M, device=dev), torch.empty(2 * M, device=dev)
        scal = torch.empty(_lib.RENDER_SCRATCH_FLOATS, device=dev)
        nrm, acc = torch.empty(1, 3, M, device=dev), torch.empty(1, 3, M, device=dev)
        jj, uu = j.to(dev).reshape(1, M, 64).contiguous(), u.to(dev).reshape(M, 64).contiguous()

        def second_render():
            ops.render_triplane(planes, S, S, pidx, cams, res, dec, jj, uu, rgb, dep, ws, lim, scal, views_per_call=1, weights=wts, all_coords=crd,
                                **render_call_kwargs(rk))

        def composite():
            ops.surface_normals(planes, S, S, pidx, dec, rk['box_warp'], None, wsum, nrm, cams=cams, res=res, mode='composited', weights=wts,
                                coords=crd, accum=acc)

        sig, grad = torch.empty(M * T, device=dev), torch.empty(M * T, 3, device=dev)
        om_buf = torch.empty(M, T, device=dev)                                      # allocated outside the timed windows

        def alternative():
            ops.query_points_grad(planes[0], S, S, crd.reshape(M * T, 3), dec, rk['box_warp'], sig, grad)
            w = wts[0]
            om_buf.zero_()
            om_buf[:, :-1] += w
            om_buf[:, 1:] += w
            om_buf.mul_(0.5)
            return (om_buf[..., None] * unit_outward(grad).reshape(M, T, 3)).sum(1)

        second_render()
        composite()
        torch.cuda.synchronize()
        om = torch.zeros(M, T, device=dev)
        om[:, :-1] += wts[0]
        om[:, 1:] += wts[0]
        share = float((om > 0).float().mean())
        agree = float((alternative() - acc[0].t()).abs().max())
        r = alternate({'plain': lambda: tp(**kw), 'surface': lambda: tp(return_normals=True, **kw),
                       'composited': lambda: tp(return_normals=True, normal_mode='composited', **kw),
                       'second_render': second_render, 'launch': composite, 'alternative': alternative}, args.iters, args.rounds)
        for _ in range(40 if res == 256 else 12):                                   # a queue of the measured launches, still running while
            second_render()                                                         # rocm-smi reads the clock and the power
            composite()
            alternative()
        busy = clocks()
        torch.cuda.synchronize()
        loads.append(f"{res}^2: {busy}")
        f = lambda k: "%.3f (%.3f - %.3f)" % r[k]                                   # noqa: E731
        lines += [f"| {res}^2 | Triplane.forward, no normals | {f('plain')} |",
                  f"| {res}^2 | Triplane.forward, return_normals (surface mode) | {f('surface')} |",
                  f"| {res}^2 | Triplane.forward, normal_mode='composited' | {f('composited')} |",
                  f"| {res}^2 | of that: the second render (generic kernel, writes weights + all_coords) | {f('second_render')} |",
                  f"| {res}^2 | of that: the composited launch ({100 * share:.1f} % of the {M * T} samples carry omega > 0) | {f('launch')} |",
                  f"| {res}^2 | alternative: query_points_grad over all {M * T} samples + torch composite (max abs difference of N: {agree:.2e}) | {f('alternative')} |"]
    clk = clocks()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        fh.write("# Volume-composited normal maps: measured times\n\n")
        fh.write(f"`python tools/normals_composite_bench.py --iters {args.iters} --rounds {args.rounds}` on {torch.cuda.get_device_name(0)}: one process, "
                 f"the variants in turn in {args.rounds} alternating windows of {args.iters} back-to-back calls between device events after one warm-up "
                 "call each; median window (fastest - slowest).  One view, 256 x 256 f32 tri-plane of random texels, synthetic decoder, 64 + 64 "
                 "samples per ray, weight_floor 0.\n\n")
        fh.write("Clock and power read while a queue of the measured launches (second render, composited launch, alternative) was running: "
                 + " | ".join(loads) + f".  Idle after the run: {clk}\n\n")
        fh.write("| view | what | ms per call |\n|---|---|---|\n")
        fh.write("\n".join(lines) + "\n")
        fh.write("\nThe alternative's torch part (unit_outward, the product and the sum over the samples) allocates its temporaries inside the "
                 "timed window, as a caller's would; its omega buffer does not.  One wavefront serves one ray, so a ray with few weighted samples "
                 "leaves most lanes idle through the gradient: the launch row is the price of that layout on this scene.\n")
        fh.write("\nThe Triplane.forward rows include the allocation of the per-sample scratch (133 MB per 256^2 view).  Not measured: f16 texels, a "
                 "weight_floor above 0, more than one view per call, a trained tri-plane (a random one is dense everywhere in the box, so the share "
                 "of samples that carry weight is that of this scene only), kernel-level counters.\n")
    print(open(args.out).read())


if __name__ == "__main__":
    main()
