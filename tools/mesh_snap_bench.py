"""Times the level-set snapping of include/ln3d_meshsnap.h on the level set of a 192^3 grid and writes profiles/mesh_snap.md.

    python tools/mesh_snap_bench.py [--out profiles/mesh_snap.md] [--reps 7] [--calls 10] [--grid 192] [--commit SHA]

Snapping needs a field, not just a mesh, so the bench field is a tri-plane's own: production-sized planes [3, 256, 256, 32] with smooth
content (seeded noise at 32 x 32, bilinearly enlarged), the seeded decoder of tests/render_refs.make_decoder with a sigma bias of 10, at the level of
the median of its own density grid - the family of the scenes the tests use.  Its 192^3 density grid is extracted at full density and with simplify_cell 3, each with and
without 10 iterations of smooth_mesh, and the box-space vertices are snapped with the defaults of mesh_from_grid (tol 1e-3 max(1, |thr|),
max move max(1, simplify_cell) cells, max step half of it) at 4 and 8 iterations.

Two things are timed on the same operands in the same process, with device events around `calls` back-to-back calls after 3 warm-up
calls, `reps` times each, alternating, and the medians are reported with the spread:
  fused     one ln3d_snap_points launch;
  composed  what it replaces: iters + 1 full-width calls of ln3d_query_points_grad and the loop's update as torch element-wise operations
            (masked, because there is no early exit without a read-back).
Before anything is timed the composed loop's states and evaluation counts are compared with the kernel's (they implement one definition;
a few points may decide a close comparison differently), and the kernel's residual is checked against ln3d_query_points_grad bit for bit."""
import argparse
import os
import statistics
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))


def composed(query, pts, level, iters, tol, max_step, max_dist):
    """the loop of the header as iters + 1 full-width field queries and torch element-wise updates -> (points, residual, state, evals)"""
    p = pts.clone()
    s, g = query(p)
    r = s - level
    f = torch.ones_like(r)
    evals = torch.ones_like(r, dtype=torch.int32)
    stalled = torch.zeros_like(r, dtype=torch.bool)
    active = torch.ones_like(r, dtype=torch.bool)
    for _ in range(iters):
        g2 = (g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2]
        stall = active & ~(torch.isfinite(pts).all(-1) & torch.isfinite(r) & torch.isfinite(g2) & (g2 != 0))
        stalled |= stall
        active = active & ~stall & ~(r.abs() <= tol)
        ln = r.abs() / torch.sqrt(g2)
        t = (f * torch.clamp(max_step / ln, max=1.0)) * r / g2
        c = torch.where(active[:, None], p - t[:, None] * g, p)
        d = c - pts
        far = active & ~(torch.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]) <= max_dist)
        ev = active & ~far
        sc, gc = query(torch.where(ev[:, None], c, p))
        rc = sc - level
        better = ev & (rc.abs() < r.abs())
        evals += ev.int()
        p, g = torch.where(better[:, None], c, p), torch.where(better[:, None], gc, g)
        r = torch.where(better, rc, r)
        f = torch.where(active & ~better, f * 0.5, torch.where(better, torch.ones_like(f), f))
    state = torch.where(r.abs() <= tol, 0, torch.where(stalled, 2, 1)).int()
    return p, r, state, evals


def quantiles(x):
    q = torch.quantile(x.double().cpu(), torch.tensor([0.5, 0.9, 0.99], dtype=torch.float64))
    return "%.2e / %.2e / %.2e / %.2e" % (float(q[0]), float(q[1]), float(q[2]), float(x.max()))


def face_normals(v, f):
    a, b, c = v[f[:, 0]].double(), v[f[:, 1]].double(), v[f[:, 2]].double()
    return torch.cross(b - a, c - a, dim=-1)


def clock_mhz():
    """the shader clock right after the timed window, read (never set) through torch's device query; 'not read' where that is unavailable"""
    try:
        return "%d MHz" % torch.cuda.clock_rate()
    except Exception:                            # noqa: BLE001
        return "not read"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'mesh_snap.md'))
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--calls', type=int, default=10)
    ap.add_argument('--grid', type=int, default=192)
    ap.add_argument('--commit', default=None, help="the commit the measured tree sits on (default: git rev-parse HEAD)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mesh_snap_bench measures on the GPU; there is none here")
    from mesh_clean_bench import events
    from render_refs import make_decoder
    from ln3diff_amd import ops
    from ln3diff_amd.mesh import extract_isosurface, smooth_mesh
    from ln3diff_amd.nsr.triplane import Triplane
    dev, G = 'cuda', args.grid
    H = W = 256
    gen = torch.Generator().manual_seed(91)
    low = torch.randn(3, 32, 32, 32, generator=gen) * 2                                     # [plane, channel, h, w]
    planes = torch.nn.functional.interpolate(low, size=(H, W), mode='bilinear', align_corners=False).permute(0, 2, 3, 1).contiguous().to(dev)
    tp = Triplane(img_resolution=8)
    weights = make_decoder(91, 10.0, 1.0)
    for layer, w, b in ((tp.decoder.net[0], weights[0], weights[1]), (tp.decoder.net[2], weights[2], weights[3])):
        layer.weight.data.copy_(w)
        layer.bias.data.copy_(b)
    tp = tp.to(dev)
    dec, bw = tp._decoder_dev(torch.device(dev, 0)), tp.rendering_kwargs['box_warp']
    ax = torch.linspace(-0.45, 0.45, G, device=dev)
    grid_pts = torch.stack(torch.meshgrid(ax, ax, ax, indexing='ij'), dim=-1).reshape(-1, 3)
    sigma = torch.cat([tp.query_points(planes, grid_pts[i:i + 2 ** 20])['sigma'] for i in range(0, grid_pts.shape[0], 2 ** 20)]).reshape(G, G, G)
    del grid_pts
    thr = round(float(sigma.float().median()), 2)                                           # a level inside the field's own densities

    def query(p):
        s, g = torch.empty(p.shape[0], device=dev), torch.empty(p.shape[0], 3, device=dev)
        ops.query_points_grad(planes, H, W, p.contiguous(), dec, bw, s, g)
        return s, g

    rows, dist_rows = [], []
    for cell in (0.0, 3.0):
        for smooth in (0, 10):
            verts, faces = extract_isosurface(sigma, thr, simplify_cell=cell)
            verts, faces = smooth_mesh(verts, faces, smooth, check=False)
            pts = ((verts / (G - 1) * 2 - 1) * 0.45).contiguous()
            nv, nf = pts.shape[0], faces.shape[0]
            move = max(1.0, cell) * 0.9 / (G - 1)
            tol = 1e-3 * max(1.0, abs(thr))
            n0 = face_normals(pts, faces)
            for iters in (4, 8):
                out = {'points': torch.empty_like(pts), 'residual': torch.empty(nv, device=dev),
                       'state': torch.empty(nv, dtype=torch.int32, device=dev), 'evals': torch.empty(nv, dtype=torch.int32, device=dev)}
                fused = lambda: ops.snap_points(planes, H, W, pts, dec, bw, thr, iters, tol, move / 2, move, out['points'], out['residual'],   # noqa: E731
                                                out['state'], out['evals'])
                comp = lambda: composed(query, pts, thr, iters, tol, move / 2, move)        # noqa: E731
                fused()
                cp, cr, cs, ce = comp()
                torch.cuda.synchronize()
                if not torch.equal(query(out['points'])[0] - thr, out['residual']):
                    raise SystemExit("the kernel's residual is not ln3d_query_points_grad's sigma at its points minus the level: nothing is reported")
                differ = int(((cs != out['state']) | (ce != out['evals'])).sum())
                if differ > 0.01 * nv:
                    raise SystemExit(f"the composed loop and the kernel disagree on {differ} of {nv} points: nothing is reported")
                tf, tc = [], []
                for _ in range(args.reps):                                                  # alternating
                    tf.append(events(fused, args.calls))
                    tc.append(events(comp, args.calls))
                before = (query(pts)[0] - thr).abs()
                after = out['residual'].abs()
                flipped = int(((face_normals(out['points'], faces) * n0).sum(-1) < 0).sum())
                st = [float((out['state'] == k).float().mean()) for k in range(3)]
                rows.append((cell, smooth, iters, nv, nf, statistics.median(tf), min(tf), max(tf), statistics.median(tc), min(tc), max(tc),
                             statistics.median(tc) / statistics.median(tf), differ))
                dist_rows.append((cell, smooth, iters, quantiles(before), quantiles(after), float(out['evals'].float().mean()), st, flipped, nf))
    clock = clock_mhz()

    commit = args.commit
    if commit is None:
        try:
            commit = subprocess.run(['git', 'rev-parse', '--short', 'HEAD'], cwd=ROOT, capture_output=True, text=True, timeout=60).stdout.strip()
        except Exception:                        # noqa: BLE001
            commit = ''
        commit = commit or 'an unknown commit (no git checkout here)'
    with open(args.out, 'w') as f:
        f.write("# Level-set snapping: measured times and residuals\n\n")
        f.write(f"`python tools/mesh_snap_bench.py --reps {args.reps} --calls {args.calls} --grid {G}` on {torch.cuda.get_device_name(0)}, "
                f"{time.strftime('%Y-%m-%d')}, on top of commit {commit}; shader clock right after the timed windows: {clock}.  Every time is "
                f"device events around {args.calls} back-to-back calls after 3 warm-up calls; fused and composed windows alternate, {args.reps} of "
                "each, and the table gives the median with the smallest and the largest window.\n\n")
        f.write(f"Field: a tri-plane [3, 256, 256, 32] of seeded noise at 32 x 32 enlarged bilinearly (times 2), the seeded decoder of the tests "
                f"with a sigma bias of 10, level {thr:g} (the median of its {G}^3 density grid); that grid, marching cubes, no clean-up, at full density and simplified to "
                "cell 3, without and with 10 iterations of smooth_mesh.  Snapping with mesh_from_grid's defaults: tol 1e-3 max(1, |thr|), max "
                "move max(1, simplify_cell) grid cells, max step half of it.\n\n")
        f.write("fused: one ln3d_snap_points launch.  composed: iters + 1 full-width ln3d_query_points_grad calls plus the loop's update as torch "
                "element-wise operations, on the same operands in the same process.  Before timing, the kernel's residual equalled "
                "ln3d_query_points_grad's sigma at its points minus the level bit for bit, and the two loops' state and evals were compared "
                "(last column: points on which they differ - close comparisons decided the other way by torch's differently rounded update).\n\n")
        f.write("| simplify_cell | smoothing iterations | snap iters | vertices | faces | fused ms (min - max) | composed ms (min - max) | composed / fused | "
                "points the two loops disagree on |\n|---|---|---|---|---|---|---|---|---|\n")
        for cell, smooth, iters, nv, nf, mf, lf, hf, mc, lc, hc, ratio, differ in rows:
            f.write(f"| {cell:g} | {smooth} | {iters} | {nv} | {nf} | {mf:.3f} ({lf:.3f} - {hf:.3f}) | {mc:.3f} ({lc:.3f} - {hc:.3f}) | {ratio:.2f} | {differ} |\n")
        f.write("\n|sigma - thr| at the vertices as the kernel's own field evaluates it (median / 90 % / 99 % / max), the mean number of field "
                "evaluations per vertex, the share per state (0 converged, 1 out of iterations, 2 stalled) and the faces whose normal reverses "
                "(dot product of the face normal before and after below 0):\n\n")
        f.write("| simplify_cell | smoothing iterations | snap iters | before | after | mean evals | state 0 / 1 / 2 | reversed faces |\n|---|---|---|---|---|---|---|---|\n")
        for cell, smooth, iters, before, after, ev, st, flipped, nf in dist_rows:
            f.write(f"| {cell:g} | {smooth} | {iters} | {before} | {after} | {ev:.2f} | {st[0]:.4f} / {st[1]:.4f} / {st[2]:.4f} | {flipped} of {nf} |\n")
        f.write("\nNot measured: kernel-level counters, the kernel's own time apart from these windows, a sampled latent's own planes (these are "
                "synthetic and smooth), other tolerances and reaches, power during the run.  Nothing is gated on these numbers.\n")
    print(open(args.out).read())


if __name__ == "__main__":
    main()
