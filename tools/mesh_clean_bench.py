"""Times the mesh clean-up of include/ln3d_meshclean.h on a 192^3 grid against what a user does today (download the faces, label them on the
CPU), and writes profiles/mesh_clean.md.

    python tools/mesh_clean_bench.py [--out profiles/mesh_clean.md] [--iters 20] [--grid 192] [--commit SHA]

The field is the five-blob field of tests/mesh_clean_refs.py rescaled to the grid, plus seeded Gaussian noise (a rough surface with specks
next to it) and seeded single-node specks.  The four entry points are timed with device events around `iters` back-to-back calls after 3
warm-up calls; the composite steps (extraction, clean_mesh, the colour query) with a host clock around work that ends in a device
synchronise, because they contain read-backs.  The device labels are compared with the CPU's before anything is reported."""
import argparse
import os
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def events(fn, iters):
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


def clocked(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3 / iters


def field(G, seed=0):
    import mesh_clean_refs as M
    rng = np.random.default_rng(seed)
    s = M.blob_field(G).astype(np.float64) + 2.0 * rng.standard_normal((G, G, G))
    i = rng.integers(1, G - 1, (2000, 3))
    s[i[:, 0], i[:, 1], i[:, 2]] = 20.0
    return s.astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'mesh_clean.md'))
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--grid', type=int, default=192)
    ap.add_argument('--commit', default=None, help="the commit the measured tree sits on (default: git rev-parse HEAD)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mesh_clean_bench measures on the GPU; there is none here")
    import mesh_clean_refs as M
    from ln3diff_amd import ops, _lib
    from ln3diff_amd.mesh import extract_isosurface, clean_mesh
    from ln3diff_amd.nsr.triplane import Triplane
    dev, G, thr = 'cuda', args.grid, 10.0
    sigma = torch.from_numpy(field(G)).to(dev)
    verts, faces = extract_isosurface(sigma, thr)
    nv, nf = verts.shape[0], faces.shape[0]
    label, nvert, nface, keep_v = (torch.empty(nv, dtype=torch.int32, device=dev) for _ in range(4))
    keep_f = torch.empty(nf, dtype=torch.int32, device=dev)
    best = torch.empty(1, dtype=torch.int64, device=dev)
    ops.mesh_components(faces, nv, label)
    ops.mesh_component_counts(faces, label, nvert, nface, best, check=False)
    ops.mesh_mark(faces, label, nface, 0, True, best, keep_v, keep_f, check=False)
    vpre, fpre = torch.cumsum(keep_v.long(), 0), torch.cumsum(keep_f.long(), 0)
    vout, fout = torch.empty(int(vpre[-1]), 3, device=dev), torch.empty(int(fpre[-1]), 3, dtype=torch.int64, device=dev)
    ncomp = int((label == torch.arange(nv, dtype=torch.int32, device=dev)).sum())
    ncomp_faces = int((nface > 0).sum())

    # ---- what a user does today: faces to the host, components on the CPU
    torch.cuda.synchronize()
    t = time.perf_counter()
    f_host = faces.cpu().numpy()
    t_down = (time.perf_counter() - t) * 1e3
    try:
        import scipy  # noqa: F401
        t = time.perf_counter()
        cpu_label = M.scipy_labels(f_host, nv)
        t_cpu, cpu_what = (time.perf_counter() - t) * 1e3, f"scipy {scipy.__version__} csgraph.connected_components"
    except ImportError:
        t = time.perf_counter()
        cpu_label = M.labels(f_host, nv)
        t_cpu, cpu_what = (time.perf_counter() - t) * 1e3, "the numpy / Python union-find of tests/mesh_clean_refs.py (scipy is not installed here)"
    if not np.array_equal(cpu_label, label.cpu().numpy()):
        raise SystemExit("the device labels differ from the CPU's: nothing is reported")

    rows = [("extract_isosurface (count, scan, emit, weld; two read-backs)", clocked(lambda: extract_isosurface(sigma, thr), args.iters), "host clock"),
            ("ln3d_mesh_components (3 launches)", events(lambda: ops.mesh_components(faces, nv, label, check=False), args.iters), "events"),
            ("ln3d_mesh_component_counts (3 launches)", events(lambda: ops.mesh_component_counts(faces, label, nvert, nface, best, check=False), args.iters), "events"),
            ("ln3d_mesh_mark, largest only", events(lambda: ops.mesh_mark(faces, label, nface, 0, True, best, keep_v, keep_f, check=False), args.iters), "events"),
            ("ln3d_mesh_gather, largest only", events(lambda: ops.mesh_gather(verts, faces, keep_v, vpre, keep_f, fpre, vout, fout, check=False), args.iters), "events"),
            ("clean_mesh(keep='largest'): index check, the four calls, two scans, one read-back", clocked(lambda: clean_mesh(verts, faces, 'largest'), args.iters), "host clock")]

    # ---- the colour query, over every vertex and over the survivors
    S = 256
    tp = Triplane(img_resolution=256).to(dev)
    dec = tp._decoder_dev(torch.device(dev, 0))
    planes = (torch.randn(3, S, S, 32, generator=torch.Generator().manual_seed(0)) * 2).to(dev)
    scal = torch.empty(_lib.RENDER_SCRATCH_FLOATS, device=dev)
    for what, v in (("colour query (ln3d_query_points) without cleaning", verts), ("colour query with cleaning (keep='largest')", vout)):
        pts = ((v / (G - 1) * 2 - 1) * 0.45).contiguous()
        sg, rgb = torch.empty(pts.shape[0], device=dev), torch.empty(pts.shape[0], 3, device=dev)
        rows.append((f"{what}: {pts.shape[0]} points", events(lambda: ops.query_points(planes, S, S, pts, dec, 0.9, sg, rgb, scal), args.iters), "events"))
    rows.append((f"today: faces to the host ({f_host.nbytes / 1e6:.1f} MB)", t_down, "host clock, once"))
    rows.append((f"today: {cpu_what}", t_cpu, "host clock, once"))

    try:
        smi = subprocess.run(['rocm-smi', '--showclocks', '--showpower'], capture_output=True, text=True, timeout=60).stdout
        clk = '; '.join(l.strip() for l in smi.splitlines() if ('sclk' in l or 'Power' in l) and 'GPU[0]' in l) or 'rocm-smi printed no sclk / power line'
    except Exception as e:                       # noqa: BLE001 - the bench reports, it does not depend on the tool
        clk = f'not measured (rocm-smi: {e})'
    commit = args.commit
    if commit is None:
        try:
            commit = subprocess.run(['git', 'rev-parse', '--short', 'HEAD'], cwd=ROOT, capture_output=True, text=True, timeout=60).stdout.strip()
        except Exception:                        # noqa: BLE001
            commit = ''
        commit = commit or 'an unknown commit (no git checkout here)'
    with open(args.out, 'w') as f:
        f.write("# Mesh clean-up: measured times\n\n")
        f.write(f"`python tools/mesh_clean_bench.py --iters {args.iters} --grid {G}` on {torch.cuda.get_device_name(0)}, {time.strftime('%Y-%m-%d')}, "
                f"on top of commit {commit}.  Entry points: device events around {args.iters} back-to-back calls after 3 warm-up calls; composite "
                "steps: a host clock around calls that end in a device synchronise.\n\n")
        f.write(f"Clock and power while idle after the run: {clk}\n\n")
        f.write(f"Field: the five-blob field rescaled to {G}^3 plus Gaussian noise (sigma 2) and 2000 single-node specks, level {thr:g}, marching cubes: "
                f"{nv} vertices, {nf} faces, {ncomp} components ({ncomp_faces} with a face), the largest with {int(best.item()) >> 32} faces "
                f"and {int(vpre[-1])} vertices.  The device labels equal the CPU's.\n\n")
        f.write("| what | ms per call | how |\n|---|---|---|\n")
        for what, t, how in rows:
            f.write(f"| {what} | {t:.3f} | {how} |\n")
        f.write("\nNot measured: kernel-level counters, marching tetrahedra, a sampled latent's own level set.\n")
    print(open(args.out).read())


if __name__ == "__main__":
    main()
