"""Times the mesh export - the .obj text, and the binary PLY and GLB of include/ln3d_meshpack.h - and writes profiles/mesh_export.md.

    python tools/mesh_export_bench.py [--out profiles/mesh_export.md] [--windows 5] [--calls 3] [--grid 192] [--dir DIR] [--commit SHA]
    python tools/mesh_export_bench.py --obj-only --tree PATH        # the .obj rows alone, with the package of another checkout (the parent)

Two fields: the 192^3 bench level set of tools/mesh_clean_bench.py (profiles/mesh_simplify.md) with the seeded random tri-plane of
tools/mesh_simplify_bench.py as its colour field, and the smooth tri-plane field of tools/mesh_snap_bench.py at the median of its own
density grid.  Each at full density and at simplify_cell 3.

What is timed, all with a host clock around calls that end with the file closed (they contain read-backs, so a device synchronise too), in
ONE process, the variants alternating window by window, median over the windows with the smallest and largest:
  mesh_from_grid as a whole: without a file, with its .obj, with mesh_format='ply' and 'glb'; textured_mesh_from_grid at T = 2048 on the
    bench level set at cell 3, as .obj + .mtl + .png and as one .glb;
  the export step alone, on what mesh_from_grid has at that point: write_ply / write_glb on the device tensors, against the honest
    alternative - packing the same records on the host with numpy structured arrays from the arrays mesh_from_grid already returns
    (numpy_ply / numpy_glb below, which write the same bytes: compared before anything is timed);
  the parts of a binary export: the pack launches (device events around back-to-back calls: launch throughput, an upper bound on the
    kernels' own time), the copies of the packed sections to the host, and the writes of those host buffers.
Files go to --dir (default: a fresh temporary directory); the report says what file system that is."""
import argparse
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def med(ts):
    return "%.2f (%.2f - %.2f)" % (statistics.median(ts), min(ts), max(ts))


def window(fn, calls):
    """ms per call of `calls` calls, each of which ends with its file closed; the device is idle before and after"""
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3 / calls


def alternating(variants, windows, calls):
    """{name: fn} -> {name: [ms per call of every window]}: one warm-up call each, then the variants alternate window by window"""
    for fn in variants.values():
        fn()
    out = {k: [] for k in variants}
    for _ in range(windows):
        for k, fn in variants.items():
            out[k].append(window(fn, calls))
    return out


def numpy_ply(path, v, f, colors, vn=None):
    """write_ply's bytes from mesh_from_grid's returned arrays: structured arrays filled on the host"""
    nv, nf = len(v), len(f)
    vd = np.dtype([('p', '<f4', 3)] + ([('n', '<f4', 3)] if vn is not None else []) + [('c', 'u1', 3)])
    rec = np.empty(nv, vd)
    rec['p'], rec['c'] = v, colors
    if vn is not None:
        rec['n'] = vn
    fr = np.empty(nf, np.dtype([('k', 'u1'), ('i', '<i4', 3)]))
    fr['k'], fr['i'] = 3, f
    from ln3diff_amd.mesh import _ply_header
    with open(path, 'wb') as fh:
        fh.write(_ply_header(nv, nf, vn is not None))
        fh.write(rec.data)
        fh.write(fr.data)


def numpy_glb(path, v, f, colors, vn=None):
    """write_glb's untextured bytes from mesh_from_grid's returned arrays"""
    from ln3diff_amd.mesh import _glb_json, _write_glb_file
    rgba = np.empty((len(v), 4), np.uint8)
    rgba[:, :3], rgba[:, 3] = colors, 255
    named = [('POSITION', v)] + ([('NORMAL', vn)] if vn is not None else []) + [('COLOR_0', rgba), ('indices', f.astype(np.uint32).reshape(-1))]
    sections = [(k, memoryview(np.ascontiguousarray(a)).cast('B')) for k, a in named]
    bounds = np.concatenate([v.min(0), v.max(0)])
    doc, n = _glb_json([(k, len(d)) for k, d in sections], len(v), bounds, False, 3 * len(f))
    _write_glb_file(path, doc, [d for _, d in sections], n)


def fields(G, dev):
    """-> [(name, decoder, dec_out, sigma [G,G,G], thr)]"""
    from mesh_clean_bench import field
    from render_refs import make_decoder
    from ln3diff_amd.nsr.triplane import Triplane
    from ln3diff_amd.vit.vit_triplane import _RendererSeams

    class D(_RendererSeams):
        pass
    out = []
    dec = D()
    dec.triplane_decoder = Triplane(img_resolution=256).to(dev)
    dec.rendering_kwargs = dec.triplane_decoder.rendering_kwargs
    planes = (torch.randn(1, 3, 256, 256, 32, generator=torch.Generator().manual_seed(0)) * 2).to(dev)
    out.append(("bench level set (five blobs, noise, specks)", dec, {'planes_channel_last': planes}, torch.from_numpy(field(G)).to(dev), 10.0))
    gen = torch.Generator().manual_seed(91)
    low = torch.randn(3, 32, 32, 32, generator=gen) * 2
    planes = torch.nn.functional.interpolate(low, size=(256, 256), mode='bilinear', align_corners=False).permute(0, 2, 3, 1).contiguous().to(dev)
    tp = Triplane(img_resolution=8)
    w = make_decoder(91, 10.0, 1.0)
    for layer, a, b in ((tp.decoder.net[0], w[0], w[1]), (tp.decoder.net[2], w[2], w[3])):
        layer.weight.data.copy_(a)
        layer.bias.data.copy_(b)
    tp = tp.to(dev)
    ax = torch.linspace(-0.45, 0.45, G, device=dev)
    pts = torch.stack(torch.meshgrid(ax, ax, ax, indexing='ij'), dim=-1).reshape(-1, 3)
    sigma = torch.cat([tp.query_points(planes, pts[i:i + 2 ** 20])['sigma'] for i in range(0, pts.shape[0], 2 ** 20)]).reshape(G, G, G)
    dec2 = D()
    dec2.triplane_decoder = tp
    dec2.rendering_kwargs = tp.rendering_kwargs
    out.append(("smooth tri-plane field", dec2, {'planes_channel_last': planes[None]}, sigma.float(), round(float(sigma.float().median()), 2)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--windows', type=int, default=5)
    ap.add_argument('--calls', type=int, default=3)
    ap.add_argument('--grid', type=int, default=192)
    ap.add_argument('--dir', default=None, help="where the files are written (default: a fresh temporary directory)")
    ap.add_argument('--commit', default=None, help="the commit the measured tree sits on (default: git rev-parse HEAD)")
    ap.add_argument('--tree', default=ROOT, help="the checkout whose ln3diff_amd is measured (default: this one)")
    ap.add_argument('--obj-only', action='store_true', help="the .obj rows alone: for a checkout without the binary formats")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mesh_export_bench measures on the GPU; there is none here")
    tree = os.path.abspath(args.tree)
    for p in (os.path.join(ROOT, 'tools'), os.path.join(ROOT, 'tests'), tree):
        sys.path.insert(0, p)
    from ln3diff_amd import mesh                                                           # first: the helpers below put this checkout in front
    assert os.path.dirname(os.path.dirname(os.path.abspath(mesh.__file__))) == tree, mesh.__file__
    from mesh_clean_bench import events
    dev, G = 'cuda', args.grid
    out_path = args.out or os.path.join(ROOT, 'profiles', 'mesh_export_obj_only.md' if args.obj_only else 'mesh_export.md')
    tmp = args.dir or tempfile.mkdtemp(prefix='mesh_export_')
    os.makedirs(tmp, exist_ok=True)
    fs = subprocess.run(['df', '-PT', tmp], capture_output=True, text=True).stdout.strip().splitlines()[-1].split()
    where = "%s (file system type %s)" % (tmp, fs[1] if len(fs) > 1 else 'unknown')
    path = lambda name: os.path.join(tmp, name)                                             # noqa: E731
    size = lambda name: os.path.getsize(path(name))                                         # noqa: E731

    whole_rows, step_rows, part_rows, tex_rows = [], [], [], []
    for fname, dec, d, sigma, thr in fields(G, dev):
        for cell in (0.0, 3.0):
            big = cell == 0.0 and fname.startswith('smooth')
            windows, calls = (2, 1) if big else (args.windows, args.calls)                 # a .obj of 1.4 M vertices takes seconds
            kw = dict(simplify_cell=cell)
            make = lambda **k: mesh.mesh_from_grid(dec, d, sigma, G, thr, **kw, **k)        # noqa: E731
            v, f, colors = make()
            variants = {'none': lambda: make(), 'obj': lambda: make(path=path('m.obj'))}
            if not args.obj_only:
                variants.update(ply=lambda: make(path=path('m.ply'), mesh_format='ply'), glb=lambda: make(path=path('m.glb'), mesh_format='glb'))
            t = alternating(variants, windows, calls)
            sizes = {k: size('m.' + k) for k in variants if k != 'none'}
            whole_rows.append((fname, cell, len(v), len(f), t, sizes))
            if args.obj_only:
                continue
            # ---- the export step alone: the device tensors mesh_from_grid holds at that point, and the arrays it returns
            _, vtx, faces, v2, f2, c2, _, q = mesh._coloured_mesh(dec, d, sigma, G, thr, 0, 'cubes', mesh.MeshPost(simplify_cell=cell))
            rgb = q['rgb'][0]
            mesh.write_ply(path('dev.ply'), vtx, faces, rgb, check=False)
            numpy_ply(path('np.ply'), v2, f2, c2)
            mesh.write_glb(path('dev.glb'), vtx, faces, rgb, check=False)
            numpy_glb(path('np.glb'), v2, f2, c2)
            same = [open(path('dev.' + e), 'rb').read() == open(path('np.' + e), 'rb').read() for e in ('ply', 'glb')]
            if not all(same):                                                               # numpy's matmul and the kernel round differently somewhere
                print("note: device and numpy files differ (ply, glb equal: %s) on %s cell %g" % (same, fname, cell))
            ts = alternating({'device ply': lambda: mesh.write_ply(path('dev.ply'), vtx, faces, rgb, check=False),
                              'numpy ply': lambda: numpy_ply(path('np.ply'), v2, f2, c2),
                              'device glb': lambda: mesh.write_glb(path('dev.glb'), vtx, faces, rgb, check=False),
                              'numpy glb': lambda: numpy_glb(path('np.glb'), v2, f2, c2)}, args.windows, args.calls)
            step_rows.append((fname, cell, len(v2), len(f2), ts, same))
            # ---- the parts of the device exports
            from ln3diff_amd import ops
            nv, nf = vtx.shape[0], faces.shape[0]
            rot9 = torch.from_numpy(mesh.rotation_matrix_x(-90).reshape(-1)).to(dev)
            rgbf = rgb.float().contiguous()
            vbuf = torch.empty((nv * 15 + 3) // 4 * 4, dtype=torch.uint8, device=dev)
            fbuf = torch.empty((nf * 13 + 3) // 4 * 4, dtype=torch.uint8, device=dev)
            pos, rgba = torch.empty(nv, 3, device=dev), torch.empty(nv, 4, dtype=torch.uint8, device=dev)
            idx, b6 = torch.empty(3 * nf, dtype=torch.int32, device=dev), torch.empty(6, device=dev)
            k_ply = events(lambda: (ops.pack_ply_vertices(vtx, None, rgbf, rot9, vbuf), ops.pack_ply_faces(faces, fbuf)), 20)
            k_glb = events(lambda: (ops.pack_gltf_vertices(vtx, None, rgbf, rot9, pos, None, rgba), ops.pack_gltf_indices(faces, idx),
                                    ops.position_bounds(pos, b6)), 20)
            host = {}

            def copy(bufs, key):
                host[key] = [b.cpu().numpy() for b in bufs]

            def write(key, name):
                with open(path(name), 'wb') as fh:
                    for a in host[key]:
                        fh.write(a.data)
            tc = alternating({'ply': lambda: copy((vbuf, fbuf), 'ply'), 'glb': lambda: copy((pos, rgba, idx), 'glb')}, args.windows, args.calls)
            tw = alternating({'ply': lambda: write('ply', 'parts.ply'), 'glb': lambda: write('glb', 'parts.glb')}, args.windows, args.calls)
            part_rows.append((fname, cell, k_ply, k_glb, tc, tw, vbuf.numel() + fbuf.numel(), pos.numel() * 4 + rgba.numel() + idx.numel() * 4))
            if cell == 3.0 and fname.startswith('bench'):
                T = 2048
                tex = lambda **k: mesh.textured_mesh_from_grid(dec, d, sigma, G, thr, texture_size=T, **kw, **k)     # noqa: E731
                tt = alternating({'none': lambda: tex(), 'obj + mtl + png': lambda: tex(path=path('t.obj')),
                                  'glb': lambda: tex(path=path('t.glb'), mesh_format='glb')}, 3, 1)
                out5 = tex()
                t0 = time.perf_counter()
                png = mesh.png_bytes(out5[4])
                t_png = (time.perf_counter() - t0) * 1e3
                tex_rows.append((fname, cell, T, len(out5[1]), tt, size('t.obj') + size('t.mtl') + size('t.png'), size('t.glb'), t_png, len(png)))

    commit = args.commit
    if commit is None:
        try:
            commit = subprocess.run(['git', 'rev-parse', '--short', 'HEAD'], cwd=tree, capture_output=True, text=True, timeout=60).stdout.strip()
        except Exception:                        # noqa: BLE001
            commit = ''
        commit = commit or 'an unknown commit (no git checkout here)'
    with open(out_path, 'w') as fh:
        fh.write("# Mesh export: the .obj text against the binary PLY and GLB, measured times\n\n")
        fh.write(f"`python tools/mesh_export_bench.py --windows {args.windows} --calls {args.calls} --grid {G}"
                 f"{' --obj-only' if args.obj_only else ''}` on {torch.cuda.get_device_name(0)}, {time.strftime('%Y-%m-%d')}, on top of commit {commit}.  "
                 f"Every time is a host clock around {args.calls} calls that end with the file closed and the device idle (1 call, 2 windows, for the "
                 f"full-density smooth field), after one warm-up call per variant; the variants of a table row alternate window by window in this one "
                 f"process, {args.windows} windows each; median (smallest - largest window), in ms per call.  Files were written to {where}.\n\n")
        fh.write("## mesh_from_grid as a whole (extraction, colour query, copies of the returned arrays, the file)\n\n")
        fh.write("| field | simplify_cell | vertices | faces | no file | .obj | ply | glb | file sizes (bytes) |\n|---|---|---|---|---|---|---|---|---|\n")
        for fname, cell, nv, nf, t, sizes in whole_rows:
            fh.write(f"| {fname} | {cell:g} | {nv} | {nf} | {med(t['none'])} | {med(t['obj'])} | {med(t['ply']) if 'ply' in t else '-'} | "
                     f"{med(t['glb']) if 'glb' in t else '-'} | {', '.join('%s %d' % kv for kv in sizes.items())} |\n")
        if step_rows:
            fh.write("\n## The export step alone: packed on the device against packed on the host with numpy\n\n")
            fh.write("device: write_ply / write_glb on the device tensors (pack launches, one copy per section, the writes).  numpy: structured arrays "
                     "filled from the arrays mesh_from_grid has already returned, then the same writes; it needs no launch and no copy, but the "
                     "returned arrays exist only because mesh_from_grid copied them to the host for its return value.\n\n")
            fh.write("| field | simplify_cell | vertices | faces | device ply | numpy ply | device glb | numpy glb | same bytes (ply, glb) |\n|---|---|---|---|---|---|---|---|---|\n")
            for fname, cell, nv, nf, ts, same in step_rows:
                fh.write(f"| {fname} | {cell:g} | {nv} | {nf} | {med(ts['device ply'])} | {med(ts['numpy ply'])} | {med(ts['device glb'])} | "
                         f"{med(ts['numpy glb'])} | {same[0]}, {same[1]} |\n")
            fh.write("\n## The parts of a device export\n\n")
            fh.write("kernels: device events around 20 back-to-back rounds of the format's launches (ply: 2; glb: 2 and the 3 of the bounds) - launch "
                     "throughput, an upper bound on the kernels' own time.  copies: `.cpu().numpy()` of every packed section.  write: the host buffers "
                     "into one file.\n\n")
            fh.write("| field | simplify_cell | ply kernels | ply copies | ply write | ply bytes | glb kernels | glb copies | glb write | glb bytes |\n"
                     "|---|---|---|---|---|---|---|---|---|---|\n")
            for fname, cell, k_ply, k_glb, tc, tw, b_ply, b_glb in part_rows:
                fh.write(f"| {fname} | {cell:g} | {k_ply:.3f} | {med(tc['ply'])} | {med(tw['ply'])} | {b_ply} | {k_glb:.3f} | {med(tc['glb'])} | "
                         f"{med(tw['glb'])} | {b_glb} |\n")
        if tex_rows:
            fh.write("\n## textured_mesh_from_grid (3 windows of 1 call)\n\n")
            fh.write("| field | simplify_cell | T | faces | no file | .obj + .mtl + .png | one .glb | bytes of the three files | bytes of the .glb | png_bytes alone (once) |\n"
                     "|---|---|---|---|---|---|---|---|---|---|\n")
            for fname, cell, T, nf, tt, b_obj, b_glb, t_png, n_png in tex_rows:
                fh.write(f"| {fname} | {cell:g} | {T} | {nf} | {med(tt['none'])} | {med(tt['obj + mtl + png'])} | {med(tt['glb'])} | {b_obj} | {b_glb} | "
                         f"{t_png:.1f} ms for {n_png} bytes |\n")
        fh.write("\nNot measured: kernel-level counters and the kernels' own times apart from the launch-throughput windows, a sampled latent's own "
                 "level set, a cold page cache or a slow disk, clock and power during the run.  Nothing is gated on these numbers.\n")
    print(open(out_path).read())


if __name__ == "__main__":
    main()
