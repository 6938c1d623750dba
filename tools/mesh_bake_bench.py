"""Times the texture bake of include/ln3d_meshbake.h on the level set of a 192^3 grid and writes profiles/mesh_bake.md.

    python tools/mesh_bake_bench.py [--out profiles/mesh_bake.md] [--iters 10] [--grid 192] [--commit SHA]

The field is the one of tools/mesh_clean_bench.py; the tri-plane is random (the cost of the point query does not depend on its values).  Per
simplify_cell 0 / 2 / 3 and texture size 1024 / 2048 / 4096: ln3d_bake_points, forward_points on all T^2 points and ln3d_bake_pack are timed
with device events around `iters` back-to-back calls after 3 warm-up calls (for the two bake kernels that is launch throughput at the small
sizes, an upper bound on the kernel's own time); bake_texture as a whole, which ends in the copy of the texture to the host, with a host
clock.  A size too small for the face count is reported as such.  Before anything is reported the device's points and owner are compared
with the numpy reference of tests/mesh_bake_refs.py on a small mesh."""
import argparse
import os
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'mesh_bake.md'))
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--grid', type=int, default=192)
    ap.add_argument('--commit', default=None, help="the commit the measured tree sits on (default: git rev-parse HEAD)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mesh_bake_bench measures on the GPU; there is none here")
    import numpy as np
    import mesh_bake_refs as R
    from mesh_clean_bench import events, clocked, field
    from ln3diff_amd import ops
    from ln3diff_amd.mesh import atlas_layout, bake_points, bake_texture, extract_isosurface
    from ln3diff_amd.nsr.triplane import Triplane
    from ln3diff_amd.vit.vit_triplane import _RendererSeams
    dev, G, thr, it = 'cuda', args.grid, 10.0, args.iters

    def box(v, g):
        return (v / (g - 1) * 2 - 1) * 0.45

    # ---- the same code on a mesh small enough for the numpy reference
    sv, sf = extract_isosurface(torch.from_numpy(field(16)).to(dev), thr, simplify_cell=2.0)
    sv = box(sv, 16)
    size = 4 * atlas_layout(sf.shape[0], 8192)[0] + 3
    gp, go = bake_points(sv, sf, size)
    rp, ro = R.points(sv.cpu().numpy(), sf.cpu().numpy(), size)
    if not (np.array_equal(gp.cpu().numpy().view(np.int32), rp.view(np.int32)) and np.array_equal(go.cpu().numpy(), ro)):
        raise SystemExit("the device result differs from the reference's: nothing is reported")

    class D(_RendererSeams):
        pass
    dec = D()
    dec.triplane_decoder = Triplane(img_resolution=256).to(dev)
    dec.rendering_kwargs = dec.triplane_decoder.rendering_kwargs
    planes = (torch.randn(1, 3, 256, 256, 32, generator=torch.Generator().manual_seed(0)) * 2).to(dev)
    sigma = torch.from_numpy(field(G)).to(dev)
    rows = []
    for cell in (0.0, 2.0, 3.0):
        verts, faces = extract_isosurface(sigma, thr, simplify_cell=cell)
        verts = box(verts, G)
        nv, nf = verts.shape[0], faces.shape[0]
        for T in (1024, 2048, 4096):
            try:
                n, c = atlas_layout(nf, T)
            except ValueError as e:
                rows.append((cell, nv, nf, T, str(e).split(';')[0]))
                continue
            points, owner = torch.empty(T * T, 3, device=dev), torch.empty(T * T, dtype=torch.int32, device=dev)
            tex = torch.empty(T * T, 3, dtype=torch.uint8, device=dev)
            ops.bake_points(verts, faces, T, n, c, points, owner)
            rgb = dec.forward_points(planes, points[None])['rgb'][0].contiguous()
            owned = int((owner >= 0).sum())
            t_pts = events(lambda: ops.bake_points(verts, faces, T, n, c, points, owner, check=False), it)
            t_query = events(lambda: dec.forward_points(planes, points[None]), it)
            t_pack = events(lambda: ops.bake_pack(rgb, owner, 0, tex), it)
            t_copy = clocked(lambda: tex.cpu(), it)
            t_all = clocked(lambda: bake_texture(dec, planes, verts, faces, T), max(3, it // 2))
            rows.append((cell, nv, nf, T, (n, c, owned, t_pts, t_query, t_pack, t_copy, t_all)))
            del points, owner, tex, rgb
            torch.cuda.empty_cache()

    commit = args.commit
    if commit is None:
        try:
            commit = subprocess.run(['git', 'rev-parse', '--short', 'HEAD'], cwd=ROOT, capture_output=True, text=True, timeout=60).stdout.strip()
        except Exception:                        # noqa: BLE001
            commit = ''
        commit = commit or 'an unknown commit (no git checkout here)'
    with open(args.out, 'w') as f:
        f.write("# Texture baking: measured times\n\n")
        f.write(f"`python tools/mesh_bake_bench.py --iters {it} --grid {G}` on {torch.cuda.get_device_name(0)}, {time.strftime('%Y-%m-%d')}, "
                f"on top of commit {commit}.  The three device steps: device events around {it} back-to-back calls after 3 warm-up calls (for the "
                "two bake kernels at the small sizes that is launch throughput, an upper bound on the kernel's own time); the copy of the texture "
                "to the host and bake_texture as a whole (face-index check with its read-back, allocations, the three steps, the copy, the UVs "
                "on the host): a host clock around calls that end synchronised.\n\n")
        f.write(f"Field: the five-blob field rescaled to {G}^3 plus Gaussian noise (sigma 2) and 2000 single-node specks, level {thr:g}, marching "
                "cubes, no clean-up; a random 3 x 256 x 256 x 32 f32 tri-plane.  The query runs on all T^2 texels, the unowned ones included.  On "
                "a small mesh the device's points and owner equal the numpy reference's bit for bit (checked by this run).\n\n")
        f.write("| simplify_cell | vertices | faces | T | n | c | owned texels | ln3d_bake_points ms | forward_points ms | ln3d_bake_pack ms | "
                "tex to host ms | bake_texture ms |\n|---|---|---|---|---|---|---|---|---|---|---|---|\n")
        for cell, nv, nf, T, r in rows:
            if isinstance(r, str):
                f.write(f"| {cell:g} | {nv} | {nf} | {T} | - | - | - | - | - | - | - | {r} |\n")
            else:
                n, c, owned, t_pts, t_query, t_pack, t_copy, t_all = r
                f.write(f"| {cell:g} | {nv} | {nf} | {T} | {n} | {c} | {owned} ({100.0 * owned / (T * T):.0f} %) | {t_pts:.3f} | {t_query:.3f} | {t_pack:.3f} | "
                        f"{t_copy:.3f} | {t_all:.3f} |\n")
        f.write("\nNot measured: the .obj / .png writers (Python loops and zlib on the host), kernel-level counters, f16 texels, a sampled "
                "latent's own level set, clock and power during the run.  Nothing is gated on these numbers.\n")
    print(open(args.out).read())


if __name__ == "__main__":
    main()
