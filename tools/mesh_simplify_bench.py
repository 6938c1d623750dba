"""Times the mesh simplification of include/ln3d_meshsimplify.h on a 192^3 grid and writes profiles/mesh_simplify.md.

    python tools/mesh_simplify_bench.py [--out profiles/mesh_simplify.md] [--iters 20] [--grid 192] [--commit SHA] [--placement quadric]

The field is the one of tools/mesh_clean_bench.py (the five-blob field of tests/mesh_clean_refs.py rescaled to the grid, seeded noise, seeded
specks).  Per cell size: the five entry points and ln3d_mesh_gather, and torch's unique / sorts / prefix sums between them, are timed with
device events around `iters` back-to-back calls after 3 warm-up calls.  For kernels this short that is the rate at which back-to-back
launches drain (launch throughput), an upper bound on the kernel's own time, not that time.  simplify_mesh as a whole and mesh_from_grid
with and without simplification (without an .obj, and once with one) are timed with a host clock around calls that end in a device
synchronise, because they contain read-backs.  The device result is compared with the numpy reference of tests/mesh_simplify_refs.py at a
small grid before anything is reported.
--placement quadric measures the opt-in quadric-error placement (include/ln3d_meshquadric.h) INSTEAD: per cell size simplify_mesh as a
whole with placement='mean' and with placement='quadric' in alternating windows of `iters` calls in this one process (host clock, median and
range over the windows), and the steps the option adds (the two kernels, the pair-key sort and searchsorted) with device events; nothing of
the default report is measured or written, and --out then defaults to profiles/mesh_quadric_times.md."""
import argparse
import os
import subprocess
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--grid', type=int, default=192)
    ap.add_argument('--commit', default=None, help="the commit the measured tree sits on (default: git rev-parse HEAD)")
    ap.add_argument('--placement', choices=('mean', 'quadric'), default='mean', help="quadric: time placement='quadric' against 'mean' instead")
    ap.add_argument('--windows', type=int, default=7, help="alternating windows per placement (--placement quadric)")
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, 'profiles', 'mesh_simplify.md' if args.placement == 'mean' else 'mesh_quadric_times.md')
    if not torch.cuda.is_available():
        raise SystemExit("mesh_simplify_bench measures on the GPU; there is none here")
    import numpy as np
    import mesh_simplify_refs as S
    from mesh_clean_bench import events, clocked, field
    from ln3diff_amd import ops
    from ln3diff_amd.mesh import extract_isosurface, simplify_mesh, mesh_from_grid
    from ln3diff_amd.nsr.triplane import Triplane
    from ln3diff_amd.vit.vit_triplane import _RendererSeams
    dev, G, thr, it = 'cuda', args.grid, 10.0, args.iters
    zero = (0.0, 0.0, 0.0)

    # ---- the same code on a grid small enough for the numpy reference
    sv, sf = extract_isosurface(torch.from_numpy(field(32)).to(dev), thr)
    for cell in (2.0, 3.0):
        gv, gf = simplify_mesh(sv, sf, cell, zero)
        rv, rf = S.simplify(sv.cpu().numpy(), sf.cpu().numpy(), cell, zero)
        if not (np.array_equal(S.bits(gv.cpu().numpy()), S.bits(rv)) and np.array_equal(gf.cpu().numpy(), rf)):
            raise SystemExit("the device result differs from the reference's: nothing is reported")

    sigma = torch.from_numpy(field(G)).to(dev)
    verts, faces = extract_isosurface(sigma, thr)
    nv, nf = verts.shape[0], faces.shape[0]
    if args.placement == 'quadric':
        return placement_report(args, verts, faces, events, clocked)
    tables = []
    for cell in (2.0, 3.0):
        key = torch.empty(nv, dtype=torch.int64, device=dev)
        ops.simplify_keys(verts, zero, cell, key)
        uniq, cluster, members = torch.unique(key, return_inverse=True, return_counts=True)
        nc = uniq.shape[0]
        order = torch.sort(cluster, stable=True)[1]
        start = torch.zeros(nc + 1, dtype=torch.int64, device=dev)
        start[1:] = torch.cumsum(members, 0)
        rep = torch.empty(nc, 3, device=dev)
        cfaces, fkey = torch.empty(nf, 3, dtype=torch.int64, device=dev), torch.empty(nf, dtype=torch.int64, device=dev)
        ops.simplify_faces(faces, cluster, nc, cfaces, fkey)
        sorted_key, perm = torch.sort(fkey, stable=True)
        keep_f, keep_v = torch.empty(nf, dtype=torch.int32, device=dev), torch.empty(nc, dtype=torch.int32, device=dev)
        ops.simplify_first(sorted_key, perm, keep_f)
        ops.simplify_used(cfaces, keep_f, keep_v)
        vpre, fpre = torch.cumsum(keep_v.long(), 0), torch.cumsum(keep_f.long(), 0)
        nvo, nfo = int(vpre[-1]), int(fpre[-1])
        vout, fout = torch.empty(nvo, 3, device=dev), torch.empty(nfo, 3, dtype=torch.int64, device=dev)
        rows = [
            ("ln3d_simplify_keys", events(lambda: ops.simplify_keys(verts, zero, cell, key), it), "kernel, launch throughput"),
            ("torch.unique(key, return_inverse, return_counts) (contains a size read-back)", clocked(lambda: torch.unique(key, return_inverse=True, return_counts=True), it), "torch, host clock"),
            ("torch.sort(cluster, stable) + cumsum of the counts", events(lambda: (torch.sort(cluster, stable=True), torch.cumsum(members, 0)), it), "torch"),
            ("ln3d_simplify_mean", events(lambda: ops.simplify_mean(verts, order, start, rep, check=False), it), "kernel, launch throughput"),
            ("ln3d_simplify_faces", events(lambda: ops.simplify_faces(faces, cluster, nc, cfaces, fkey, check=False), it), "kernel, launch throughput"),
            ("torch.sort(fkey, stable)", events(lambda: torch.sort(fkey, stable=True), it), "torch"),
            ("ln3d_simplify_first", events(lambda: ops.simplify_first(sorted_key, perm, keep_f, check=False), it), "kernel, launch throughput"),
            ("ln3d_simplify_used (2 launches)", events(lambda: ops.simplify_used(cfaces, keep_f, keep_v, check=False), it), "kernel, launch throughput"),
            ("two cumsum (keep_v, keep_f) with their int64 casts", events(lambda: (torch.cumsum(keep_v.long(), 0), torch.cumsum(keep_f.long(), 0)), it), "torch"),
            ("ln3d_mesh_gather", events(lambda: ops.mesh_gather(rep, cfaces, keep_v, vpre, keep_f, fpre, vout, fout, check=False), it), "kernel, launch throughput"),
        ]
        kernels = sum(t for _, t, how in rows if how == "kernel, launch throughput")
        torch_ms = sum(t for _, t, how in rows if how.startswith("torch"))
        whole = clocked(lambda: simplify_mesh(verts, faces, cell, zero), it)
        members_max = int(members.max())
        tables.append((cell, nc, nvo, nfo, int((fkey == -1).sum()), int((fkey != -1).sum()) - nfo, members_max, rows, kernels, torch_ms, whole))

    # ---- mesh_from_grid with and without, in this process: extraction, (simplification,) the colour and normal query, the copies to the host
    class D(_RendererSeams):
        pass
    dec = D()
    dec.triplane_decoder = Triplane(img_resolution=256).to(dev)
    dec.rendering_kwargs = dec.triplane_decoder.rendering_kwargs
    planes = (torch.randn(1, 3, 256, 256, 32, generator=torch.Generator().manual_seed(0)) * 2).to(dev)
    d = {'planes_channel_last': planes}
    grid_rows = []
    for what, kw in (("no simplification", {}), ("simplify_cell=2", dict(simplify_cell=2.0)), ("simplify_cell=3", dict(simplify_cell=3.0))):
        for normals in (False, True):
            t = clocked(lambda: mesh_from_grid(dec, d, sigma, G, thr, normals=normals, **kw), max(3, it // 4))
            out = mesh_from_grid(dec, d, sigma, G, thr, normals=normals, **kw)
            with tempfile.TemporaryDirectory() as tmp:                     # the same call writing its .obj: once, the file loop dominates
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                mesh_from_grid(dec, d, sigma, G, thr, normals=normals, path=os.path.join(tmp, 'm.obj'), **kw)
                t_obj = (time.perf_counter() - t0) * 1e3
            grid_rows.append((what, normals, out[0].shape[0], out[1].shape[0], t, t_obj))

    commit = args.commit
    if commit is None:
        try:
            commit = subprocess.run(['git', 'rev-parse', '--short', 'HEAD'], cwd=ROOT, capture_output=True, text=True, timeout=60).stdout.strip()
        except Exception:                        # noqa: BLE001
            commit = ''
        commit = commit or 'an unknown commit (no git checkout here)'
    with open(args.out, 'w') as f:
        f.write("# Mesh simplification: measured times\n\n")
        f.write(f"`python tools/mesh_simplify_bench.py --iters {it} --grid {G}` on {torch.cuda.get_device_name(0)}, {time.strftime('%Y-%m-%d')}, "
                f"on top of commit {commit}.  Kernels and torch steps: device events around {it} back-to-back calls after 3 warm-up calls "
                "(torch.unique, which reads a size back, and the composite calls: a host clock around calls that end in a device synchronise).  "
                "The kernel rows are therefore launch throughput - how fast back-to-back launches of a kernel this short drain - and an upper "
                "bound on the kernel's own time, not that time; so is their sum.\n\n")
        f.write(f"Field: the five-blob field rescaled to {G}^3 plus Gaussian noise (sigma 2) and 2000 single-node specks, level {thr:g}, marching "
                f"cubes, no clean-up: {nv} vertices, {nf} faces.  Cells in grid units, origin (0, 0, 0).  At grid 32 the device result equals "
                "the numpy reference's bit for bit (checked by this run).\n\n")
        for cell, nc, nvo, nfo, ndeg, ndup, mmax, rows, kernels, torch_ms, whole in tables:
            f.write(f"## cell {cell:g}\n\n{nv} / {nf} -> {nvo} / {nfo} vertices / faces ({nf / max(nfo, 1):.1f}x fewer faces); {nc} clusters, the largest with "
                    f"{mmax} members; {ndeg} faces collapse, {ndup} are duplicates.\n\n")
            f.write("| step | ms per call | what |\n|---|---|---|\n")
            for what, t, how in rows:
                f.write(f"| {what} | {t:.3f} | {how} |\n")
            f.write(f"| sum of the kernels | {kernels:.3f} | |\n| sum of the torch steps | {torch_ms:.3f} | |\n")
            f.write(f"| simplify_mesh as a whole (index check, bounds read-back, all of the above, counts read-back, allocations) | {whole:.3f} | host clock |\n\n")
        f.write("## mesh_from_grid (extraction, clean-up off, colour query, copies to the host), without and with its .obj\n\n")
        f.write("| call | normals | vertices | faces | ms per call (host clock) | ms with the .obj written (host clock, once) |\n|---|---|---|---|---|---|\n")
        for what, normals, a, b, t, t_obj in grid_rows:
            f.write(f"| {what} | {'yes' if normals else 'no'} | {a} | {b} | {t:.3f} | {t_obj:.1f} |\n")
        f.write("\nNot measured: kernel-level counters, a sampled latent's own level set, clock and power during the run.\n")
    print(open(args.out).read())


def placement_report(args, verts, faces, events, clocked):
    """--placement quadric: 'mean' against 'quadric' on the same mesh, alternating, and the steps that 'quadric' adds"""
    import statistics
    import numpy as np
    import mesh_quadric_refs as R
    import mesh_simplify_refs as S
    from ln3diff_amd import ops
    from ln3diff_amd.mesh import extract_isosurface, simplify_mesh, simplify_placement
    from mesh_clean_bench import field
    dev, it, zero = 'cuda', args.iters, (0.0, 0.0, 0.0)
    nv, nf = verts.shape[0], faces.shape[0]
    # ---- the same code on a grid small enough for the float64 reference
    sv, sf = extract_isosurface(torch.from_numpy(field(32)).to(dev), 10.0)
    for cell in (2.0, 3.0):
        st = S.stages(sv.cpu().numpy(), sf.cpu().numpy(), cell, zero)
        st['key_unique'] = np.unique(st['key'])
        case = dict(st=st, cell=cell, ref=R.place64(sv.cpu().numpy(), sf.cpu().numpy(), st, cell))
        _, quad, placed, _ = simplify_placement(sv, sf, cell, zero)
        fails, fig = R.check_placement(case, quad.cpu().numpy(), placed.cpu().numpy())
        # a marching-cubes vertex has two integer coordinates, so at an integer cell many solutions lie ON a face of their cell: those
        # clusters' flags are not compared (their share is no failure here), every other cluster's flag and position is
        fails = [x for x in fails if 'are doubtful' not in x]
        if fails:
            raise SystemExit(f"the device placement differs from the float64 reference's at cell {cell:g} ({fails}): nothing is reported")
    out = []
    for cell in (2.0, 3.0):
        mean = lambda: simplify_mesh(verts, faces, cell, zero)                               # noqa: E731
        quad = lambda: simplify_mesh(verts, faces, cell, zero, placement='quadric')          # noqa: E731
        t = {'mean': [], 'quadric': []}
        for _ in range(args.windows):                                                        # alternating windows, one process
            t['mean'].append(clocked(mean, it))
            t['quadric'].append(clocked(quad, it))
        rep_mean, _, placed, uniq = simplify_placement(verts, faces, cell, zero)
        nc = rep_mean.shape[0]
        key = torch.empty(nv, dtype=torch.int64, device=dev)
        ops.simplify_keys(verts, zero, cell, key)
        cluster = torch.unique(key, return_inverse=True)[1]
        cfaces, fkey = torch.empty(nf, 3, dtype=torch.int64, device=dev), torch.empty(nf, dtype=torch.int64, device=dev)
        ops.simplify_faces(faces, cluster, nc, cfaces, fkey)
        pair = torch.empty(3 * nf, dtype=torch.int64, device=dev)
        ops.quadric_pairs(cfaces, nc, pair, check=False)
        skey = torch.sort(pair)[0]
        start = torch.searchsorted(skey >> 31, torch.arange(nc + 1, device=dev))
        rows_per = (start[1:] - start[:-1])
        rep, pl = torch.empty(nc, 3, device=dev), torch.empty(nc, dtype=torch.int32, device=dev)
        steps = [
            ("ln3d_quadric_pairs", events(lambda: ops.quadric_pairs(cfaces, nc, pair, check=False), it), "kernel, launch throughput"),
            ("torch.sort(pair_key) + searchsorted of nc + 1 row pointers", events(lambda: torch.searchsorted(torch.sort(pair)[0] >> 31, torch.arange(nc + 1, device=dev)), it), "torch"),
            ("ln3d_quadric_place", events(lambda: ops.quadric_place(verts, faces, skey, start, rep_mean, zero, cell, uniq, 1e-3, rep, pl, check=False), it), "kernel, launch throughput"),
        ]
        out.append((cell, nc, int(placed.sum()), float(rows_per.float().mean()), int(rows_per.max()), t, steps))
    with open(args.out, 'w') as f:
        f.write("# Quadric-error placement: measured times\n\n")
        f.write(f"`python tools/mesh_simplify_bench.py --placement quadric --iters {it} --windows {args.windows} --grid {args.grid}` on "
                f"{torch.cuda.get_device_name(0)}, {time.strftime('%Y-%m-%d')}.  simplify_mesh as a whole: a host clock around {it} calls that end in "
                f"a device synchronise, after 3 warm-up calls, {args.windows} windows per placement, alternating in one process; median (smallest - "
                "largest window).  The added steps: device events around back-to-back calls, so the kernel rows are launch throughput, an upper "
                "bound on the kernel's own time.  At grid 32 the device placement passes the checks of tests/mesh_quadric_refs.py against the "
                "float64 reference (checked by this run).\n\n")
        f.write(f"Field: that of profiles/mesh_simplify.md at {args.grid}^3: {nv} vertices, {nf} faces.\n\n")
        for cell, nc, npl, avg, mx, t, steps in out:
            med = {k: statistics.median(v) for k, v in t.items()}
            f.write(f"## cell {cell:g}\n\n{nc} clusters, {npl} placed ({100.0 * npl / nc:.1f} %), {avg:.1f} faces per cluster on average, {mx} at most.\n\n")
            f.write("| call | ms per call (host clock) |\n|---|---|\n")
            for k in ('mean', 'quadric'):
                f.write(f"| simplify_mesh(placement='{k}') | {med[k]:.3f} ({min(t[k]):.3f} - {max(t[k]):.3f}) |\n")
            f.write(f"| difference of the medians | {med['quadric'] - med['mean']:.3f} |\n\n")
            f.write("| added step | ms per call | what |\n|---|---|---|\n")
            for what, ms, how in steps:
                f.write(f"| {what} | {ms:.3f} | {how} |\n")
            f.write("\n")
        f.write("Not measured: kernel-level counters, a sampled latent's own level set, clock and power during the run.\n")
    print(open(args.out).read())


if __name__ == "__main__":
    main()
